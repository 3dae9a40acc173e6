// sdfr_query.h -- questions put to the loaded scene instead of rendering it (device code, host-compilable): the scene
// distance and normal at points, the first hit along rays, the first hit under pixels of the current camera (sdfr_query_distance,
// sdfr_query_rays, sdfr_pick in include/sdfr.h).  Each answer is a value the reference's driver computes, made from the
// stages of sdfr_pixel.h as the pixel pipeline calls them (sdfr_render_pixel.h); the kernels that run them one lane per item
// are in sdfr_query_kernel.h, and tests/cpp/query_host.cpp compiles these functions for the CPU to compare them with the oracle.
#pragma once
#include "sdfr_pixel.h"

namespace sdfr {

// One query launch (sdfr_kernels.h: launch_query).  Points: `pos` [n][3] -> `distance` [n], `normals` [n][3] or null.  Rays:
// `pos` = origins [n][3], `dir` [n][3] -> `hits` [n][12].  Picks: `pixels` [n][2] of a width x height frame -> `hits` [n][12].
// With `surfaces` [n][32] (sdfr_surface.h) the surface kernel answers, `hits` may be null, and two more kinds of items exist.
// Frame: every pixel of the width x height frame, item y * width + x, n = width * height, nothing read.  Mesh: `pos` = vertex
// positions, `dir` = vertex normals, the ray towards each vertex from `reach` outside it (query_mesh_ray).
// The occlusion kernel (sdfr_occlusion.h) answers the last two kinds into `occlusion` [n][4]: items that are `pos` = points and
// `dir` = normals, or the pos and normal of the hit records `hit_items` [n][12]; `dist_max` is the radius.
enum { QUERY_POINTS = 0, QUERY_RAYS = 1, QUERY_PICK = 2, QUERY_FRAME = 3, QUERY_MESH = 4, QUERY_OCCLUSION = 5, QUERY_HIT_OCCLUSION = 6 };
struct QueryArgs
{
	int kind;  // QUERY_*
	int n;
	const float *pos, *dir;
	const int32_t *pixels;
	float dist_max; // rays: march_ray's dist_max (picks and frames: the range; meshes: 2 * reach)
	float reach;    // meshes
	float *distance, *normals;
	uint32_t *hits;     // 12 words per item: the layout of sdfr_hit
	uint32_t *surfaces; // 32 words per item: the layout of sdfr_surface
	// the occlusion kinds (appended: the other kernels' argument offsets stay)
	const uint32_t *hit_items; // 12 words per item, read
	uint32_t *occlusion;       // 4 words per item: the layout of sdfr_occlusion
	float bias;
};
enum { QUERY_HIT_WORDS = 12, QUERY_SURFACE_WORDS = 32, QUERY_OCCLUSION_WORDS = 4 };
// what a query kernel takes: one argument, as the pixel kernels (PixelKernelArgs)
struct QueryKernelArgs
{
	FrameU U;
	QueryArgs q;
};

// One lattice launch (sdfr_kernels.h: launch_query_lattice; sdfr_mesh_extract): the distance query at the points of a regular lattice,
// computed from their indices -- point (i, j, k) is origin + (float)index * cell per axis, one multiply then one add -- into
// out[i + px * (j + py * k)].  px * py * pz <= 2^30.
struct LatticeArgs
{
	float origin[3];
	float cell;
	int32_t px, py, pz; // lattice points per axis
	int32_t rows;       // 0: a wave owns a 4 x 4 x 4 brick of points; 1: 64 consecutive points of a row (the A/B of DESIGN.md 4.6)
	float *out;
};
struct LatticeKernelArgs
{
	FrameU U;
	LatticeArgs g;
};

// map_geometry at the sample of a query: a scene that reads the march state (GeoStep) gets the running camera_distance and
// the ray's offsets, every other scene (p, dir) as in the pixel pipeline
template <class Scene, bool DBG>
SDF_HD float query_geometry(const FrameU &U, const DebugFlags &F, const typename Scene::RayInv &R, vec3 p, vec3 dir, bool fast, float camera_distance,
	vec3 right_off, vec3 bottom_off)
{
	if constexpr (SceneReadsMarchState<Scene>::value)
	{
		GeoStep gs;
		gs.camera_distance = camera_distance;
		gs.right_off = right_off;
		gs.bottom_off = bottom_off;
		return map_geometry_at<Scene, DBG>(U, F, R, p, dir, fast, gs);
	}
	else
		return map_geometry<Scene, DBG>(U, F, R, p, dir, fast);
}

// the driver's normal at pos (pshader_sdf.hlsl:164-177, 320-330): map_normal with the NormalOutput preloaded {grad_eps, 0, false};
// its normal if it sets use_normal, else the three forward differences against `baseline`, normalised
template <class Scene, bool DBG>
SDF_HD vec3 query_normal(const FrameU &U, const DebugFlags &F, const typename Scene::RayInv &R, vec3 pos, vec3 dir, float camera_distance,
	vec3 right_off, vec3 bottom_off, float baseline)
{
	const NormalOut no = scene_normal<Scene>(U, pos, dir, camera_distance, right_off, bottom_off);
	if (no.use_normal) return no.normal;
	const float g0 = query_geometry<Scene, DBG>(U, F, R, grad_sample_pos(pos, 0, no.sample_dist), dir, false, camera_distance, right_off, bottom_off) - baseline;
	const float g1 = query_geometry<Scene, DBG>(U, F, R, grad_sample_pos(pos, 1, no.sample_dist), dir, false, camera_distance, right_off, bottom_off) - baseline;
	const float g2 = query_geometry<Scene, DBG>(U, F, R, grad_sample_pos(pos, 2, no.sample_dist), dir, false, camera_distance, right_off, bottom_off) - baseline;
	return normalize(V3(g0, g1, g2));
}

SDF_HD RayFlags query_ray_flags()
{
	RayFlags f; // the default MarchingInput: outside, no transparency, not a shadow pass
	f.has_transparent = false;
	f.is_shadow = false;
	f.last_transparent_pos = V3s(0.f);
	return f;
}

// Distance query: map_geometry (pshader_sdf.hlsl:111-135) at GeometryInput{pos = p, dir = (0, 0, 0, 0), camera_distance = 0,
// offsets 0} -- dir.w = 0 selects the direction-free ("slow") methods --, and, when `normal` is given, the normal there with
// baseline = that distance
template <class Scene, bool DBG>
SDF_HD float query_point(const FrameU &U, vec3 p, vec3 *normal)
{
	const DebugFlags F = debug_flags(U);
	const vec3 zero = V3s(0.f);
	const typename Scene::RayInv R = Scene::ray_setup(U, zero, query_ray_flags());
	const float d = query_geometry<Scene, DBG>(U, F, R, p, zero, false, 0.f, zero, zero);
	if (normal) *normal = query_normal<Scene, DBG>(U, F, R, p, zero, 0.f, zero, zero, d);
	return d;
}

// Ray query: what the driver does with a primary ray up to its material (pshader_sdf.hlsl:299-353): march_ray with dir.w = 1,
// inside_sign +1, the default MarchingInput, camera_distance from 0 and the given offsets; on a hit the normal and map_material.
// With FrameU::step_shortcuts a miss may end early, as in the pixel pipeline (render_pixel): hits are unchanged.
// rec: the 12 words of sdfr_hit.  Returns whether the ray hit; of a hit, `at` is the surface point and the material map_material
// made of it, for whoever goes on where the driver does (sdfr_surface.h).
// MARCH_ONLY: the march alone -- whether the ray hit is all that is returned, the normal and map_material of a hit are not computed,
// `rec` and `at` are not touched (query_ray_hits; the occlusion query, sdfr_occlusion.h).  One copy of the march for both; a
// template parameter and not a function of its own, because the existing kernels' code stays the same, instruction for instruction,
// only if the body they instantiate does.
struct QueryHit
{
	SurfacePoint sp;
	Material mat;
};
template <class Scene, bool DBG, bool MARCH_ONLY = false>
SDF_HD bool query_ray_at(const FrameU &U, vec3 origin, vec3 dir, float dist_max, vec3 right_off, vec3 bottom_off, uint32_t rec[QUERY_HIT_WORDS],
	QueryHit &at)
{
	const DebugFlags F = debug_flags(U);
	const typename Scene::RayInv R = Scene::ray_setup(U, dir, query_ray_flags());
	March m = march_begin(origin, dir);
	int status;
	const bool shortcuts = !DBG && (RayEscapes<Scene>::available || EscapesFrom<Scene>::available) && U.step_shortcuts != 0;
	float clear_from = 3e38f;
	if constexpr (EscapesFrom<Scene>::available)
		if (shortcuts) clear_from = EscapesFrom<Scene>::get(U, origin, dir, dist_max);
	do
	{
		march_pre(m);
		// the step shortcut of render_pixel: only a sample the march will not take back may end the ray
		bool escaped = shortcuts && RayEscapes<Scene>::test(U, R, march_pos(m), dir);
		if constexpr (EscapesFrom<Scene>::available) escaped = escaped || m.t >= clear_from;
		if (escaped && m.factor == 1.f)
		{
			status = MARCH_MISS;
			break;
		}
		const float d = query_geometry<Scene, DBG>(U, F, R, march_pos(m), dir, true, m.t, right_off, bottom_off);
		if (escaped && !((m.last_d + d) < m.last_d * m.factor))
		{
			status = MARCH_MISS;
			break;
		}
		status = march_advance(m, d, dist_max, (uint32_t)U.iter_count, U.dist_eps);
	} while (status == MARCH_CONTINUE);
	if constexpr (MARCH_ONLY) return status == MARCH_HIT;

	const vec3 pos = march_pos(m);
	vec3 n = V3s(0.f);
	uint32_t material = 0u;
	if (status == MARCH_HIT)
	{
		n = query_normal<Scene, DBG>(U, F, R, pos, dir, m.t, right_off, bottom_off, m.d);
		SurfacePoint &sp = at.sp;
		sp.pos = pos;
		sp.dir = dir;
		sp.camera_distance = m.t;
		sp.right_off = right_off;
		sp.bottom_off = bottom_off;
		sp.normal = n;
		sp.iteration_count = m.iter;
		sp.scene_distance = m.d;
		at.mat = default_material(U, pos);
		map_material<Scene, DBG>(U, F, sp, at.mat);
		material = at.mat.id;
	}
	rec[0] = f32_bits(m.t);
	rec[1] = f32_bits(m.d);
	rec[2] = f32_bits(pos.x);
	rec[3] = f32_bits(pos.y);
	rec[4] = f32_bits(pos.z);
	rec[5] = f32_bits(n.x);
	rec[6] = f32_bits(n.y);
	rec[7] = f32_bits(n.z);
	rec[8] = m.iter;
	rec[9] = material;
	rec[10] = status == MARCH_HIT ? 1u : 0u;
	rec[11] = 0u;
	return status == MARCH_HIT;
}
template <class Scene, bool DBG>
SDF_HD void query_ray(const FrameU &U, vec3 origin, vec3 dir, float dist_max, vec3 right_off, vec3 bottom_off, uint32_t rec[QUERY_HIT_WORDS])
{
	QueryHit at;
	query_ray_at<Scene, DBG>(U, origin, dir, dist_max, right_off, bottom_off, rec, at);
}

// whether the ray hits: query_ray's march and its `hit`, nothing else
template <class Scene, bool DBG>
SDF_HD bool query_ray_hits(const FrameU &U, vec3 origin, vec3 dir, float dist_max, vec3 right_off, vec3 bottom_off)
{
	uint32_t rec[QUERY_HIT_WORDS];
	QueryHit at;
	return query_ray_at<Scene, DBG, true>(U, origin, dir, dist_max, right_off, bottom_off, rec, at);
}

// Pick: pixel (px, py)'s primary ray of the frame U describes (pshader_sdf.hlsl:263-267), marched to limits.range; a pixel
// outside the frame is an invalid item (hit = -1, every other word 0)
template <class Scene, bool DBG>
SDF_HD void query_pick(const FrameU &U, int px, int py, uint32_t rec[QUERY_HIT_WORDS])
{
	if (px < 0 || py < 0 || px >= U.width || py >= U.height)
	{
		for (int k = 0; k < QUERY_HIT_WORDS; ++k) rec[k] = 0u;
		rec[10] = 0xffffffffu;
		return;
	}
	const PixelRay pr = pixel_ray(U, px, py);
	query_ray<Scene, DBG>(U, U.eye, pr.dir, U.range, pr.right_ray, pr.bottom_ray, rec);
}

} // namespace sdfr

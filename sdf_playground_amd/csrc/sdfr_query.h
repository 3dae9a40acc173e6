// sdfr_query.h -- questions put to the loaded scene instead of rendering it (device code, host-compilable): the scene
// distance and normal at points, the first hit along rays, the first hit under pixels of the current camera (sdfr_query_distance,
// sdfr_query_rays, sdfr_pick in include/sdfr.h).  Each answer is a value the reference's driver computes, made from the
// stages of sdfr_pixel.h as the pixel pipeline calls them (sdfr_render_pixel.h); the kernels that run them one lane per item
// are in sdfr_query_kernel.h, and tests/cpp/query_host.cpp compiles these functions for the CPU to compare them with the oracle.
#pragma once
#include "sdfr_render_pixel.h"
#include "sdfr_query_args.h"

namespace sdfr {

// QueryArgs, what one query launch reads and writes: sdfr_query_args.h; which of its arrays each kind of item takes, and how the
// kinds are launched: the table of sdfr_query_plan.h.  What a query kernel takes is one argument, as the pixel kernels:
// SceneKernelArgs<the kind's arguments> (sdfr_frame.h)

// the driver's normal at pos (pshader_sdf.hlsl:164-177, 320-330): map_normal with the NormalOutput preloaded {grad_eps, 0, false};
// its normal if it sets use_normal, else the three forward differences against `baseline`, normalised
template <class Scene, bool DBG>
SDF_HD vec3 query_normal(const FrameU &U, const DebugFlags &F, const typename Scene::RayInv &R, vec3 pos, vec3 dir, float camera_distance,
	vec3 right_off, vec3 bottom_off, float baseline)
{
	const NormalOut no = scene_normal<Scene>(U, pos, dir, camera_distance, right_off, bottom_off);
	if (no.use_normal) return no.normal;
	const float g0 = scene_distance<Scene, DBG>(U, F, R, grad_sample_pos(pos, 0, no.sample_dist), dir, false, camera_distance, right_off, bottom_off) - baseline;
	const float g1 = scene_distance<Scene, DBG>(U, F, R, grad_sample_pos(pos, 1, no.sample_dist), dir, false, camera_distance, right_off, bottom_off) - baseline;
	const float g2 = scene_distance<Scene, DBG>(U, F, R, grad_sample_pos(pos, 2, no.sample_dist), dir, false, camera_distance, right_off, bottom_off) - baseline;
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
	const float d = scene_distance<Scene, DBG>(U, F, R, p, zero, false, 0.f, zero, zero);
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
// SHADOW: one segment of a shadow ray (sdfr_lighting.h), the driver's turn for a ray with is_shadow_ray set (pshader_sdf.hlsl:299-353 again):
// the march is made with *shadow_flags as the MarchingInput -- is_shadow_pass, and the has_transparent / last_transparent_pos of the
// chain so far -- and a scene whose materials do not read the normal of a shadow hit (ShadowHitsNeedNormal) is not asked for it, as in
// the pixel pipeline; everything else is the same body, for the same reason as above.
struct QueryHit
{
	SurfacePoint sp;
	Material mat;
};
template <class Scene, bool DBG, bool MARCH_ONLY = false, bool SHADOW = false>
SDF_HD bool query_ray_at(const FrameU &U, vec3 origin, vec3 dir, float dist_max, vec3 right_off, vec3 bottom_off, uint32_t rec[QUERY_HIT_WORDS],
	QueryHit &at, const RayFlags *shadow_flags = nullptr)
{
	const DebugFlags F = debug_flags(U);
	RayFlags flags = query_ray_flags();
	if constexpr (SHADOW) flags = *shadow_flags;
	const typename Scene::RayInv R = Scene::ray_setup(U, dir, flags);
	March m = march_begin(origin, dir);
	int status;
	const bool shortcuts = !DBG && (RayEscapes<Scene>::value || EscapesFrom<Scene>::value) && U.step_shortcuts != 0;
	float clear_from = 3e38f;
	if constexpr (EscapesFrom<Scene>::value)
		if (shortcuts) clear_from = EscapesFrom<Scene>::get(U, origin, dir, dist_max);
	do
	{
		march_pre(m);
		// the step shortcut of render_pixel: only a sample the march will not take back may end the ray
		bool escaped = shortcuts && RayEscapes<Scene>::test(U, R, march_pos(m), dir);
		if constexpr (EscapesFrom<Scene>::value) escaped = escaped || m.t >= clear_from;
		if (escaped && m.factor == 1.f)
		{
			status = MARCH_MISS;
			break;
		}
		const float d = scene_distance<Scene, DBG>(U, F, R, march_pos(m), dir, true, m.t, right_off, bottom_off);
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
		if constexpr (!SHADOW || ShadowHitsNeedNormal<Scene>::value) n = query_normal<Scene, DBG>(U, F, R, pos, dir, m.t, right_off, bottom_off, m.d);
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

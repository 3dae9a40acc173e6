// sdfr_surface.h -- what the loaded scene's surface looks like where a ray first meets it (device code, host-compilable): the record
// of sdfr_query_ray_surfaces, sdfr_pick_surfaces and sdfr_mesh_surfaces (sdfr_surface in include/sdfr.h).  It is the driver's lines
// between the hit and the light loop (pshader_sdf.hlsl:333-481) restated once, after the ray query's march, normal and map_material
// (sdfr_query.h: query_ray_at): the marble extension, the shading normal, and the material switch with the procedural wood, marble and
// fire and the debug views.  shade_hit (sdfr_pixel.h) runs the same lines inside the bounce loop, between the rays it spawns; here
// nothing is spawned and no light is looked at.  The kernel that runs it one lane per item is in sdfr_query_kernel.h, and
// tests/cpp/surface_host.cpp compiles these functions for the CPU to compare them with the oracle.
#pragma once
#include "sdfr_query.h"

namespace sdfr {

enum { SURFACE_USE_HDR = 1u, SURFACE_LIT = 2u }; // sdfr_surface::flags

// The 32 words of sdfr_surface for a hit: `sp` and `m` as query_ray leaves them (map_material done), view direction sp.dir.
SDF_HD void surface_record(const FrameU &U, const SurfacePoint &sp, Material m, uint32_t rec[QUERY_SURFACE_WORDS])
{
	// extension, off by default: reflective marble (sdfr_limits::extension_marble_reflection)
	if (U.extension_marble_reflection != 0.f && (m.id == MAT_MARBLE_DARK || m.id == MAT_MARBLE_LIGHT)) m.reflection = V3s(U.extension_marble_reflection);
	const vec3 n = lerp(sp.normal, V3(m.normal.x, m.normal.y, m.normal.z), m.normal.w);

	vec3 diffuse = V3(m.diffuse.x, m.diffuse.y, m.diffuse.z);
	vec3 color = V3s(0.f);
	float alpha = m.diffuse.w;
	bool use_light = true;
	switch (m.id)
	{
	case MAT_ITER:
		color = color + mat_iter_heat(sp.iteration_count, (uint32_t)(U.iter_count - 1));
		use_light = false;
		break;
	case MAT_PLAIN:
		color = color + diffuse;
		use_light = false;
		break;
	case MAT_NORMAL1:
	{
		vec3 nc = max(n, 0.01f);
		nc = nc / max1(max1(nc.x, nc.y), nc.z);
		color = color + nc;
		use_light = false;
		break;
	}
	case MAT_NORMAL2:
		color = color + abs(n);
		use_light = false;
		break;
	case MAT_DISTANCE_PLANE:
		color = color + mat_debug_plane(m.prop_x);
		use_light = false;
		break;
	case MAT_WOOD:
		diffuse = diffuse + mat_wood(m.mpos);
		break;
	case MAT_MARBLE_DARK:
		diffuse = diffuse + mat_marble(m.mpos, V3(0.556f, 0.478f, 0.541f));
		break;
	case MAT_MARBLE_LIGHT:
		diffuse = diffuse + mat_marble(m.mpos, V3(0.7f, 0.7f, 0.7f));
		break;
	case MAT_FIRE:
	{
		const float fadeout = sat1(dot(-sp.dir, n));
		const vec4 fc = mat_fire(m.mpos, 1.f - fadeout);
		color = color + V3(fc.x, fc.y, fc.z);
		alpha = sat1(fc.w);
		break;
	}
	default:
		break;
	}

	rec[0] = m.id;
	rec[1] = (m.use_hdr ? (uint32_t)SURFACE_USE_HDR : 0u) | (use_light ? (uint32_t)SURFACE_LIT : 0u);
	rec[2] = m.max_cost;
	rec[3] = 1u;
	rec[4] = f32_bits(diffuse.x);
	rec[5] = f32_bits(diffuse.y);
	rec[6] = f32_bits(diffuse.z);
	rec[7] = f32_bits(alpha);
	rec[8] = f32_bits(m.specular.x);
	rec[9] = f32_bits(m.specular.y);
	rec[10] = f32_bits(m.specular.z);
	rec[11] = f32_bits(m.specular.w);
	rec[12] = f32_bits(m.emissive.x);
	rec[13] = f32_bits(m.emissive.y);
	rec[14] = f32_bits(m.emissive.z);
	rec[15] = f32_bits(m.ior);
	rec[16] = f32_bits(color.x);
	rec[17] = f32_bits(color.y);
	rec[18] = f32_bits(color.z);
	rec[19] = 0u;
	rec[20] = f32_bits(m.reflection.x);
	rec[21] = f32_bits(m.reflection.y);
	rec[22] = f32_bits(m.reflection.z);
	rec[23] = 0u;
	rec[24] = f32_bits(m.refraction.x);
	rec[25] = f32_bits(m.refraction.y);
	rec[26] = f32_bits(m.refraction.z);
	rec[27] = 0u;
	rec[28] = f32_bits(n.x);
	rec[29] = f32_bits(n.y);
	rec[30] = f32_bits(n.z);
	rec[31] = 0u;
}

// a miss (valid 0) or an invalid item (valid -1): every other word 0
SDF_HD void surface_none(uint32_t valid, uint32_t rec[QUERY_SURFACE_WORDS])
{
	for (int k = 0; k < QUERY_SURFACE_WORDS; ++k) rec[k] = 0u;
	rec[3] = valid;
}

// One item of a surface query as a ray: where it starts, its direction as given, its offsets, how far it is marched.
struct QueryRay
{
	vec3 origin, dir, right_off, bottom_off;
	float dist_max;
};
// a caller's ray: no offsets
SDF_HD QueryRay query_plain_ray(vec3 origin, vec3 dir, float dist_max)
{
	QueryRay r;
	r.origin = origin;
	r.dir = dir;
	r.right_off = r.bottom_off = V3s(0.f);
	r.dist_max = dist_max;
	return r;
}
// pixel (px, py)'s primary ray of the frame U describes, marched to limits.range, as query_pick's; false: the pixel is outside the frame
SDF_HD bool query_pixel_ray(const FrameU &U, int px, int py, QueryRay &r)
{
	r = query_plain_ray(U.eye, V3s(0.f), U.range);
	if (px < 0 || py < 0 || px >= U.width || py >= U.height) return false;
	const PixelRay pr = pixel_ray(U, px, py);
	r.dir = pr.dir;
	r.right_off = pr.right_ray;
	r.bottom_off = pr.bottom_ray;
	return true;
}
// The ray that looks at a mesh vertex from outside (sdfr_mesh_surfaces): from position + reach * normal -- one multiply, then one add
// per component -- along -normal, used as given, marched to 2 * reach.  A scene picks its material where |distance| < dist_eps
// (the scenes' material_hit), and a surface-nets vertex lies a fraction of a cell off the surface: the material is taken where a
// march ends, as the driver takes it.
SDF_HD QueryRay query_mesh_ray(vec3 position, vec3 normal, float reach)
{
	const vec3 off = reach * normal;
	return query_plain_ray(position + off, -normal, 2.f * reach);
}

// The ray query (query_ray_at: `hit` is query_ray's record, bit for bit) and the surface at its hit; an item that is no ray (in_frame false: a
// pixel outside the frame) gets hit = -1 and valid = -1.  The one place a surface kernel marches from, whatever its items are.
template <class Scene, bool DBG>
SDF_HD void query_surface(const FrameU &U, const QueryRay &ray, bool in_frame, uint32_t hit[QUERY_HIT_WORDS], uint32_t rec[QUERY_SURFACE_WORDS])
{
	if (!in_frame)
	{
		for (int k = 0; k < QUERY_HIT_WORDS; ++k) hit[k] = 0u;
		hit[10] = 0xffffffffu;
		surface_none(0xffffffffu, rec);
		return;
	}
	QueryHit at;
	if (query_ray_at<Scene, DBG>(U, ray.origin, ray.dir, ray.dist_max, ray.right_off, ray.bottom_off, hit, at)) surface_record(U, at.sp, at.mat, rec);
	else surface_none(0u, rec);
}

} // namespace sdfr

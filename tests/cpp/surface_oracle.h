// tests/cpp/surface_oracle.h -- TEST-ONLY: the surface record of include/sdfr.h (sdfr_surface: sdfr_query_ray_surfaces,
// sdfr_pick_surfaces, sdfr_mesh_surfaces) defined with the CPU oracle's own restatement of the reference's driver (oracle/driver.h),
// by calling its steps: ray_turn for the ray, then second_normal and material_switch.  The surface tests compare the library (on the
// GPU) and its CPU build (surface_host.cpp) with these, bit for bit.  Part of record_oracle.cpp; the product never loads it.
#pragma once
#include "record_oracle.h"

namespace {

enum { SURFACE_WORDS = 32 };

void surface_none(uint32_t valid, uint32_t *rec)
{
	for (int k = 0; k < SURFACE_WORDS; ++k) rec[k] = 0u;
	rec[3] = valid;
}

// pshader_sdf.hlsl:299-481 for one primary-shaped ray, without the rays it would spawn: `hit` as ray_query's record, `rec` the
// 32 words of sdfr_surface
template <class Scene>
void surface_query(const Frame &F, float3 origin, float3 dir, real dist_max, float3 right_off, float3 bottom_off, uint32_t *hit, uint32_t *rec)
{
	Turn turn;
	surface_none(0u, rec);
	if (!primary_turn<Scene>(F, camera_ray(origin, dir), dist_max, right_off, bottom_off, turn, hit)) return;

	MaterialOutput &material_output = turn.material_output;
	float3 new_normal = second_normal(turn);
	float3 diffuse_color = material_output.diffuse_color.xyz();
	float3 color = float3(real(0.f));
	real hdr_output = 0.f; // not part of the record
	const bool use_light = material_switch(F, new_normal, turn.iter_count, turn.geometry_input.dir.xyz(), material_output, diffuse_color, color, hdr_output);

	rec[0] = material_output.material_id;
	rec[1] = (material_output.use_hdr ? 1u : 0u) | (use_light ? 2u : 0u);
	rec[2] = material_output.max_cost;
	rec[3] = 1u;
	put3(rec + 4, diffuse_color);
	rec[7] = bits(val(material_output.diffuse_color.w));
	put3(rec + 8, material_output.specular_color.xyz());
	rec[11] = bits(val(material_output.specular_color.w));
	put3(rec + 12, material_output.emissive_color);
	rec[15] = bits(val(material_output.optical_index));
	put3(rec + 16, color);
	put3(rec + 20, material_output.reflection_color);
	put3(rec + 24, material_output.refraction_color);
	put3(rec + 28, new_normal);
}

template <class Scene>
void surface_pick(const Frame &F, int px, int py, uint32_t *hit, uint32_t *rec)
{
	if (outside_frame(F, px, py, hit))
	{
		surface_none(0xffffffffu, rec);
		return;
	}
	const PrimaryRay primary = primary_ray(F, px, py);
	surface_query<Scene>(F, F.eye, primary.dir, F.range, primary.right_ray_vec, primary.bottom_ray_vec, hit, rec);
}

} // namespace

extern "C" {

int so_rays(const char *scene, const orc_frame *f, int n, const float *origins, const float *dirs, float max_distance, uint32_t *hits, uint32_t *surfaces)
{
	const Entry *e = find(scene);
	if (!e) return -1;
	const Frame F = enter_frame(*f);
	const real dist_max = ray_range(F, max_distance);
	each_ray(n, origins, dirs, [&](int i, float3 o, float3 d) {
		e->surface_rays(F, o, d, dist_max, no_offset, no_offset, hits + HIT_WORDS * i, surfaces + SURFACE_WORDS * i);
	});
	return 0;
}

int so_pick(const char *scene, const orc_frame *f, int n, const int32_t *pixels, uint32_t *hits, uint32_t *surfaces)
{
	const Entry *e = find(scene);
	if (!e) return -1;
	const Frame F = enter_frame(*f);
	parallel_items(n, [&](int a, int b) {
		for (int i = a; i < b; ++i) e->surface_pick(F, pixels[2 * i], pixels[2 * i + 1], hits + HIT_WORDS * i, surfaces + SURFACE_WORDS * i);
	});
	return 0;
}

} // extern "C"

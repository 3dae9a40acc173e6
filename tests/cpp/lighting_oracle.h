// tests/cpp/lighting_oracle.h -- TEST-ONLY: the lighting records of include/sdfr.h (sdfr_lighting, sdfr_light_sample:
// sdfr_query_ray_lighting, sdfr_pick_lighting, sdfr_mesh_lighting) defined with the CPU oracle's own restatement of the reference's
// driver (oracle/driver.h), by calling the steps of ps_main for a primary ray -- ray_turn, second_normal, material_switch,
// scene_lights, shadow_ray_start, light_term, shadow_ray -- and, in place of the ray queue, each shadow ray's turns of the bounce loop
// one after the other (ray_turn, see_through_ray).  What is stated here is the chain loop, the masks, the sums and the records.  The
// lighting tests compare the library (on the GPU) and its CPU build (lighting_host.cpp) with these, bit for bit.  Part of
// record_oracle.cpp; the product never loads it.
#pragma once
#include "record_oracle.h"

namespace {

enum { LIGHTING_WORDS = 16, SAMPLE_WORDS = 20, SLOTS = 8, CHAIN_SEGMENTS = 64 };

// hit: the 12 words of sdfr_hit; rec: the 16 of sdfr_lighting; samples: 8 x 20 words of sdfr_light_sample, or null
template <class Scene>
void lighting_query(const Frame &F, float3 origin, float3 dir, real dist_max, float3 right_off, float3 bottom_off, uint32_t *hit, uint32_t *rec,
	uint32_t *samples)
{
	const int LIGHT_COUNT = F.light_count;
	for (int k = 0; k < LIGHTING_WORDS; ++k) rec[k] = 0u;
	if (samples)
		for (int k = 0; k < SLOTS * SAMPLE_WORDS; ++k) samples[k] = 0u;

	// the primary ray: depth 0, contribution (1, 1, 1), outside
	const Ray primary = camera_ray(origin, dir);
	Turn turn;
	if (!primary_turn<Scene>(F, primary, dist_max, right_off, bottom_off, turn, hit)) return;

	MaterialOutput &material_output = turn.material_output;
	float3 new_normal = second_normal(turn);
	float3 diffuse_color = material_output.diffuse_color.xyz();
	float3 color = float3(real(0.f));
	real hdr_output = 0.f; // not part of the records
	const bool use_light = material_switch(F, new_normal, turn.iter_count, turn.geometry_input.dir.xyz(), material_output, diffuse_color, color, hdr_output);

	uint32_t used_mask = 0, traced_mask = 0, visible_mask = 0, segments = 0;
	real ambient_lighting_factor = 0.f;
	float3 delivered[SLOTS];
	for (int i = 0; i < SLOTS; ++i) delivered[i] = float3(real(0.f));
	if (use_light)
	{
		LightOutput light_output[MAX_LIGHT_COUNT];
		scene_lights<Scene>(F, turn.geometry_input, light_output, ambient_lighting_factor);

		float3 view_dir = turn.geometry_input.dir.xyz();
		float3 scene_pos = shadow_ray_start(turn, new_normal);

		// :524-587
		for (int i2 = 0; i2 < LIGHT_COUNT && i2 < SLOTS; ++i2)
		{
			if (!light_output[i2].used) continue;
			used_mask |= 1u << i2;
			const LightTerm term = light_term(F, light_output[i2], scene_pos, view_dir, new_normal, diffuse_color, material_output);
			// ambient (:550)
			color = color + diffuse_color * term.light_color * ambient_lighting_factor;

			uint32_t state = 1, chain_segments = 0;
			// the shadow ray, and its turns of the bounce loop (:299-353, :598-632) in place of the queue
			if (sends_shadow_ray(primary, material_output, term))
			{
				traced_mask |= 1u << i2;
				Ray ray = shadow_ray(primary, scene_pos, material_output, term);
				state = 2;
				while (chain_segments < CHAIN_SEGMENTS)
				{
					++chain_segments;
					const real max_range = ray.shadow_range;
					Turn shadow_turn;
					PixelStats st = {0, 0, 0};
					if (!ray_turn<Scene>(F, ray, right_off, bottom_off, max_range, shadow_turn, st))
					{
						state = 3; // (:621-626) output_color += contribution
						delivered[i2] = ray.contribution;
						break;
					}
					if (!passes_see_through(ray, shadow_turn.material_output)) break;
					ray = see_through_ray(ray, shadow_turn, max_range);
				}
				segments += chain_segments;
				if (state == 3) visible_mask |= 1u << i2;
			}
			if (samples)
			{
				uint32_t *s = samples + SAMPLE_WORDS * i2;
				s[0] = state;
				s[1] = term.directional ? 1u : 0u;
				s[2] = chain_segments;
				put3(s + 4, term.lighting_dir);
				s[7] = bits(val(term.distance_to_trace));
				put3(s + 8, term.light_color);
				s[11] = bits(val(term.light_dot));
				put3(s + 12, term.light_influenced_color);
				s[15] = bits(val(term.specular_factor));
				put3(s + 16, delivered[i2]);
			}
		}
		// emissive + alpha (:590-593)
		color = color + material_output.emissive_color;
		color = color * r_saturate(material_output.diffuse_color.w);
	}

	// the driver's sums: out_color += (0 + color * contribution) for the primary ray's turn, then += (0 + contribution) for each
	// escaped shadow ray, popped in slot order when every chain is one segment long
	float3 direct = float3(real(0.f)), lit = float3(real(0.f));
	{
		float3 output_color = float3(real(0.f));
		output_color = output_color + color * primary.contribution;
		lit = lit + output_color;
	}
	for (int i = 0; i < SLOTS; ++i)
		if (visible_mask & (1u << i))
		{
			float3 output_color = float3(real(0.f));
			output_color = output_color + delivered[i];
			direct = direct + output_color;
			lit = lit + output_color;
		}

	rec[0] = 1u;
	rec[1] = used_mask;
	rec[2] = traced_mask;
	rec[3] = visible_mask;
	put3(rec + 4, color);
	rec[7] = bits(val(ambient_lighting_factor));
	put3(rec + 8, direct);
	rec[11] = segments;
	put3(rec + 12, lit);
}

template <class Scene>
void lighting_pick(const Frame &F, int px, int py, uint32_t *hit, uint32_t *rec, uint32_t *samples)
{
	if (outside_frame(F, px, py, hit))
	{
		for (int k = 0; k < LIGHTING_WORDS; ++k) rec[k] = 0u;
		rec[0] = 0xffffffffu;
		if (samples)
			for (int k = 0; k < SLOTS * SAMPLE_WORDS; ++k) samples[k] = 0u;
		return;
	}
	const PrimaryRay primary = primary_ray(F, px, py);
	lighting_query<Scene>(F, F.eye, primary.dir, F.range, primary.right_ray_vec, primary.bottom_ray_vec, hit, rec, samples);
}

uint32_t *samples_of(uint32_t *lights, int i) { return lights ? lights + (size_t)SLOTS * SAMPLE_WORDS * i : nullptr; }

} // namespace

extern "C" {

// lights may be null
int lo_rays(const char *scene, const orc_frame *f, int n, const float *origins, const float *dirs, float max_distance, uint32_t *hits, uint32_t *lighting,
	uint32_t *lights)
{
	const Entry *e = find(scene);
	if (!e) return -1;
	const Frame F = enter_frame(*f);
	const real dist_max = ray_range(F, max_distance);
	each_ray(n, origins, dirs, [&](int i, float3 o, float3 d) {
		e->lighting_rays(F, o, d, dist_max, no_offset, no_offset, hits + HIT_WORDS * i, lighting + LIGHTING_WORDS * i, samples_of(lights, i));
	});
	return 0;
}

int lo_pick(const char *scene, const orc_frame *f, int n, const int32_t *pixels, uint32_t *hits, uint32_t *lighting, uint32_t *lights)
{
	const Entry *e = find(scene);
	if (!e) return -1;
	const Frame F = enter_frame(*f);
	parallel_items(n, [&](int a, int b) {
		for (int i = a; i < b; ++i)
			e->lighting_pick(F, pixels[2 * i], pixels[2 * i + 1], hits + HIT_WORDS * i, lighting + LIGHTING_WORDS * i, samples_of(lights, i));
	});
	return 0;
}

} // extern "C"

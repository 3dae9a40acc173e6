// sdfr_lighting.h -- how the scene's lights fall on the surface where a ray first meets it (device code, host-compilable): the records
// of sdfr_query_ray_lighting, sdfr_pick_lighting and sdfr_mesh_lighting (sdfr_lighting, sdfr_light_sample in include/sdfr.h).  It goes
// on where sdfr_surface.h stops: the driver's light loop (pshader_sdf.hlsl:505-593) for a primary ray's hit -- depth 0, contribution
// (1, 1, 1), outside --, and the life of each shadow ray that loop starts (:598-632) followed to its end in place, segment by segment
// through see-through surfaces, instead of through the pixel's ray queue.  shade_hit (sdfr_pixel.h) runs the same lines inside the
// bounce loop; here nothing else is spawned: no reflection, no refraction, no continuation through a see-through primary hit, no
// background.  The kernel that runs it one lane per item is in sdfr_query_kernel.h, and tests/cpp/lighting_host.cpp compiles these
// functions for the CPU to compare them with the oracle.
#pragma once
#include "sdfr_surface.h"

namespace sdfr {

enum { LIGHT_DIRECTIONAL = 1u };                                                               // sdfr_light_sample::flags
enum { LIGHT_UNUSED = 0u, LIGHT_NO_CHAIN = 1u, LIGHT_BLOCKED = 2u, LIGHT_ESCAPED = 3u };     // sdfr_light_sample::state
// A shadow chain ends blocked after this many segments.  The driver bounds a chain by the hit materials' max_cost alone (each
// segment costs 2), the renderer also by bounce_count; a query lane must end whatever a run-time scene's max_cost says.
enum { LIGHT_CHAIN_SEGMENTS = 64 };

// a miss (valid 0) or an invalid item (valid -1): every other word 0
SDF_HD void lighting_none(uint32_t valid, uint32_t rec[QUERY_LIGHTING_WORDS])
{
	for (int k = 0; k < QUERY_LIGHTING_WORDS; ++k) rec[k] = 0u;
	rec[0] = valid;
}

// One shadow chain (pshader_sdf.hlsl:598-632 over the turns of one light's shadow ray): from `pos` along `dir` for `range`, carrying
// `carried`.  Each segment is query_ray_at's march as a shadow pass with the chain's transparency state, the item's ray offsets and
// camera_distance from 0.  A miss: the chain escapes and delivers what it carries.  A hit on a see-through material that can still
// afford it (diffuse.w < 1 && depth + 2 < max_cost, the HIT's max_cost): tinted, it goes on from the hit with what is left of the
// range.  Any other hit: blocked, nothing delivered.  The material switch is not applied to a shadow hit.  Returns whether it escaped.
template <class Scene, bool DBG>
SDF_HD bool shadow_chain(const FrameU &U, vec3 pos, vec3 dir, float range, vec3 right_off, vec3 bottom_off, vec3 &carried, uint32_t &segments)
{
	RayFlags flags;
	flags.has_transparent = false;
	flags.is_shadow = true;
	flags.last_transparent_pos = V3s(0.f);
	uint32_t depth = 2u;
	segments = 0u;
	while (segments < (uint32_t)LIGHT_CHAIN_SEGMENTS)
	{
		++segments;
		uint32_t hit[QUERY_HIT_WORDS];
		QueryHit at;
		if (!query_ray_at<Scene, DBG, false, true>(U, pos, dir, range, right_off, bottom_off, hit, at, &flags)) return true;
		const Material &m = at.mat;
		if (!(m.diffuse.w < 1.f && depth + 2u < m.max_cost)) break;
		carried = ((1.f - m.diffuse.w) * V3(m.diffuse.x, m.diffuse.y, m.diffuse.z)) * carried;
		pos = at.sp.pos;
		range = range - at.sp.camera_distance;
		flags.has_transparent = true;
		flags.last_transparent_pos = pos;
		depth += 2u;
	}
	carried = V3s(0.f);
	return false;
}

// The 16 words of sdfr_lighting for a hit: `sp` and `m` as query_ray_at leaves them (map_material done), view direction sp.dir.
// samples(slot, words): takes the 20 words of sdfr_light_sample of every slot 0 .. 7 in turn where samples.wanted(), else nothing.
template <class Scene, bool DBG, class Samples>
SDF_HD void lighting_record(const FrameU &U, const SurfacePoint &sp, const Material &m, uint32_t rec[QUERY_LIGHTING_WORDS], const Samples &samples)
{
	// the hit up to the light loop: the marble extension, the shading normal, the material switch (sdfr_surface.h)
	uint32_t srf[QUERY_SURFACE_WORDS];
	surface_record(U, sp, m, srf);
	const bool use_light = (srf[1] & (uint32_t)SURFACE_LIT) != 0u;
	const uint32_t max_cost = srf[2];
	const vec3 diffuse = V3(bits_f32(srf[4]), bits_f32(srf[5]), bits_f32(srf[6]));
	const float alpha = sat1(bits_f32(srf[7]));
	const vec3 specular = V3(bits_f32(srf[8]), bits_f32(srf[9]), bits_f32(srf[10]));
	const float specular_power = bits_f32(srf[11]);
	const vec3 emissive = V3(bits_f32(srf[12]), bits_f32(srf[13]), bits_f32(srf[14]));
	vec3 color = V3(bits_f32(srf[16]), bits_f32(srf[17]), bits_f32(srf[18]));
	const vec3 n = V3(bits_f32(srf[28]), bits_f32(srf[29]), bits_f32(srf[30]));
	const vec3 view_dir = sp.dir;

	uint32_t sample[QUERY_LIGHT_SAMPLE_WORDS];
	uint32_t used_mask = 0u, traced_mask = 0u, visible_mask = 0u, segments = 0u;
	float ambient = 0.f;
	vec3 direct = V3s(0.f), lit = V3s(0.f) + color;
	if (use_light)
	{
		ambient = SceneAmbient<Scene>::get(); // map_light may override the default 0.075
		// a scene in the reference's own shape fills the whole light table in one call (SceneLights); every other scene answers slot by slot
			Light table[SceneLights<Scene>::value ? SDFR_MAX_LIGHTS : 1];
		bool table_used[SceneLights<Scene>::value ? SDFR_MAX_LIGHTS : 1];
		if constexpr (SceneLights<Scene>::value) scene_light_table<Scene>(U, sp, table, table_used, ambient);
		const float sample_dist = scene_normal<Scene>(U, sp.pos, sp.dir, sp.camera_distance, sp.right_off, sp.bottom_off).sample_dist;
		const float move = max1(U.shadow_eps, sample_dist) + max1(0.f, -sp.scene_distance);
		const vec3 lit_pos = mad(n, move, sp.pos);

		// The hit's own colour first -- every light's ambient line, in slot order, then emissive and alpha -- because the driver adds it to
		// the pixel before any light a shadow ray delivers (shade_hit's INL branch does the same); then the loop again for the rest
		for (int i = 0; i < U.light_count; ++i)
		{
			Light L;
			if (!light_in_slot<Scene>(U, i, table, table_used, L)) continue;
			color = color + diffuse * light_colour(L) * ambient;
		}
		color = color + emissive;
		color = color * alpha;
		lit = V3s(0.f) + color;
		for (int i = 0; i < SDFR_MAX_LIGHTS; ++i)
		{
			Light L;
			if (!(i < U.light_count && light_in_slot<Scene>(U, i, table, table_used, L)))
			{
				if (samples.wanted())
				{
					for (int k = 0; k < QUERY_LIGHT_SAMPLE_WORDS; ++k) sample[k] = 0u;
					samples(i, sample);
				}
				continue;
			}
			used_mask |= 1u << i;
			vec3 ldir;
			float trace_dist;
			if (L.directional)
			{
				ldir = L.pos / (length(L.pos) + U.dist_eps);
				trace_dist = U.range;
			}
			else
			{
				ldir = lit_pos - L.pos;
				trace_dist = length(ldir);
				ldir = ldir / trace_dist;
				trace_dist = trace_dist - L.extend;
			}
			const vec3 lcol = light_colour(L);
			const float ndl = sat1(dot(-n, ldir));
			vec3 influenced = V3s(0.f) + diffuse * lcol * ndl;
			const vec3 half_vec = -normalize(view_dir + ldir);
			const float spec = pow1(sat1(dot(n, half_vec)), specular_power);
			influenced = influenced + specular * lcol * spec;

			uint32_t state = LIGHT_NO_CHAIN, chain_segments = 0u;
			vec3 delivered = V3s(0.f);
			// the driver's condition for a primary ray (depth 0); its queue and bounce budgets are not the query's
			if (0u + 2u < max_cost && ndl > 0.f)
			{
				traced_mask |= 1u << i;
				vec3 carried = influenced * V3s(1.f) * alpha;
				const bool escaped = shadow_chain<Scene, DBG>(U, lit_pos, -ldir, trace_dist, sp.right_off, sp.bottom_off, carried, chain_segments);
				segments += chain_segments;
				state = escaped ? LIGHT_ESCAPED : LIGHT_BLOCKED;
				if (escaped)
				{
					visible_mask |= 1u << i;
					delivered = carried;
					direct = direct + carried;
					lit = lit + carried;
				}
			}
			if (samples.wanted())
			{
				sample[0] = state;
				sample[1] = L.directional ? (uint32_t)LIGHT_DIRECTIONAL : 0u;
				sample[2] = chain_segments;
				sample[3] = 0u;
				sample[4] = f32_bits(ldir.x);
				sample[5] = f32_bits(ldir.y);
				sample[6] = f32_bits(ldir.z);
				sample[7] = f32_bits(trace_dist);
				sample[8] = f32_bits(lcol.x);
				sample[9] = f32_bits(lcol.y);
				sample[10] = f32_bits(lcol.z);
				sample[11] = f32_bits(ndl);
				sample[12] = f32_bits(influenced.x);
				sample[13] = f32_bits(influenced.y);
				sample[14] = f32_bits(influenced.z);
				sample[15] = f32_bits(spec);
				sample[16] = f32_bits(delivered.x);
				sample[17] = f32_bits(delivered.y);
				sample[18] = f32_bits(delivered.z);
				sample[19] = 0u;
				samples(i, sample);
			}
		}
	}
	else if (samples.wanted())
	{
		for (int k = 0; k < QUERY_LIGHT_SAMPLE_WORDS; ++k) sample[k] = 0u;
		for (int i = 0; i < SDFR_MAX_LIGHTS; ++i) samples(i, sample);
	}

	rec[0] = 1u;
	rec[1] = used_mask;
	rec[2] = traced_mask;
	rec[3] = visible_mask;
	rec[4] = f32_bits(color.x);
	rec[5] = f32_bits(color.y);
	rec[6] = f32_bits(color.z);
	rec[7] = f32_bits(ambient);
	rec[8] = f32_bits(direct.x);
	rec[9] = f32_bits(direct.y);
	rec[10] = f32_bits(direct.z);
	rec[11] = segments;
	rec[12] = f32_bits(lit.x);
	rec[13] = f32_bits(lit.y);
	rec[14] = f32_bits(lit.z);
	rec[15] = 0u;
}

// The ray query (query_ray_at: `hit` is query_ray's record, bit for bit) and the lighting at its hit; an item that is no ray (in_frame
// false: a pixel outside the frame) gets hit = -1 and valid = -1.  The one place a lighting kernel marches from, whatever its items are.
template <class Scene, bool DBG, class Samples>
SDF_HD void query_lighting(const FrameU &U, const QueryRay &ray, bool in_frame, uint32_t hit[QUERY_HIT_WORDS], uint32_t rec[QUERY_LIGHTING_WORDS],
	const Samples &samples)
{
	QueryHit at;
	bool lit = false;
	if (!in_frame)
	{
		for (int k = 0; k < QUERY_HIT_WORDS; ++k) hit[k] = 0u;
		hit[10] = 0xffffffffu;
		lighting_none(0xffffffffu, rec);
	}
	else if (query_ray_at<Scene, DBG>(U, ray.origin, ray.dir, ray.dist_max, ray.right_off, ray.bottom_off, hit, at))
		lit = true;
	else
		lighting_none(0u, rec);
	if (lit)
		lighting_record<Scene, DBG>(U, at.sp, at.mat, rec, samples);
	else if (samples.wanted())
	{
		uint32_t sample[QUERY_LIGHT_SAMPLE_WORDS];
		for (int k = 0; k < QUERY_LIGHT_SAMPLE_WORDS; ++k) sample[k] = 0u;
		for (int i = 0; i < SDFR_MAX_LIGHTS; ++i) samples(i, sample);
	}
}

} // namespace sdfr

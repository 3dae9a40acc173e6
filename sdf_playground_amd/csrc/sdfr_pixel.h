// sdfr_pixel.h -- the stages of the per-pixel raymarch pipeline (device code,
// host-compilable): primary-ray generation, the 8-slot cost-ordered ray queue, one
// sphere-tracing step, the forward-difference normal, hit shading with secondary-ray
// spawning, and miss shading.
//
// Behavioural contract = the reference's ps_main (Engine/shader/pshader_sdf.hlsl:260-639)
// with its helpers map_geometry (:111-135), map_material (:137-162), grad (:164-177),
// march_ray (:179-220), find_next_ray / find_free_ray (:222-246).  The kernels
// (sdfr_kernels.hip) decide how these stages are scheduled on the machine.
#pragma once
#include "sdfr_frame.h"
#include "sdfr_lib.h"
#include "sdfr_scene_traits.h"

namespace sdfr {

// ---- pixel -> primary ray (pshader_sdf.hlsl:263-267; pixel centres as D3D rasterises the
// full-screen quad of FullscreenQuad.cpp:52-58, row 0 = top) -------------------------------
struct PixelRay
{
	vec3 dir;
	vec3 right_ray, bottom_ray; // footprint of one pixel per unit distance
};
SDF_HD PixelRay pixel_ray(const FrameU &U, int px, int py)
{
	float sx = ((float)px + 0.5f) / U.widthf * 2.f - 1.f;
	float sy = 1.f - ((float)py + 0.5f) / U.heightf * 2.f;
	vec3 d = U.front + sx * U.right + sy * U.top;
	float invlen = rcp1(length(d));
	PixelRay r;
	r.dir = d * invlen;
	r.right_ray = U.ddx * U.right * invlen;
	r.bottom_ray = U.ddy * U.top * invlen;
	return r;
}
SDF_HD RayRec primary_ray(const FrameU &U, const PixelRay &pr)
{
	RayRec r;
	r.pos = U.eye;
	r.dir = pr.dir;
	r.contrib = V3(1.f, 1.f, 1.f);
	r.shadow_range = 0.f;
	r.bits = 0; // depth 0, outside, no transparency, not a shadow ray
	return r;
}
SDF_HD RayFlags ray_flags(const RayRec &r)
{
	RayFlags f;
	f.has_transparent = ray_has_transparent(r);
	f.is_shadow = ray_is_shadow(r);
	f.last_transparent_pos = f.has_transparent ? r.pos : V3s(0.f);
	return f;
}

// ---- cost-ordered ray queue: depths packed one byte per slot ---------------------------------
// find_next_ray (pshader_sdf.hlsl:222-233): smallest depth, lowest slot wins ties.
SDF_HD int queue_next(uint64_t depths, int slots)
{
	int best = 0;
	uint32_t best_depth = (uint32_t)(depths & 0xffu);
	for (int i = 1; i < slots; ++i)
	{
		uint32_t d = (uint32_t)((depths >> (8 * i)) & 0xffu);
		if (d < best_depth) { best = i; best_depth = d; }
	}
	return best;
}
// find_free_ray (pshader_sdf.hlsl:235-246): first invalid slot
SDF_HD int queue_free(uint64_t depths, int slots)
{
	int i = 0;
	for (; i < slots; ++i)
		if (((depths >> (8 * i)) & 0xffu) == RAY_DEPTH_INVALID) break;
	return i;
}
SDF_HD uint64_t queue_set_depth(uint64_t depths, int slot, uint32_t d)
{
	return (depths & ~(0xffull << (8 * slot))) | ((uint64_t)d << (8 * slot));
}
#define SDFR_QUEUE_EMPTY 0xffffffffffffffffull

// ---- the driver's debug switches (pshader_sdf.hlsl:86-109) -----------------------------------
// The kernels are specialised at compile time on DBG = "debug plane on or objects hidden";
// the common case (DBG = false) carries no trace of them.  In the DBG = true build the two
// wave-uniform switches are deliberately held in VGPRs (debug_flags), so every branch on them
// is an ordinary exec-masked branch.  Reason (found on gfx950 / ROCm 7.2, see DESIGN.md
// "Compiler hazard"): hipcc may materialise a wave-uniform bool through VALU under a partial
// exec mask inside the divergent march loop and test it again after the loop under a wider
// mask, where the lanes that left the loop early read stale zero bits.
struct DebugFlags
{
	int plane_on; // any(debug normal)
	int show_on;  // any(show_objects)
};
SDF_HD DebugFlags debug_flags(const FrameU &U)
{
	DebugFlags f;
	f.plane_on = U.debug_plane_on;
	f.show_on = U.show_on;
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("" : "+v"(f.plane_on), "+v"(f.show_on));
#endif
	return f;
}
SDF_HD bool frame_needs_debug(const FrameU &U) { return U.debug_plane_on != 0 || U.show_on == 0; }

// ---- scene distance with the driver's debug plane (pshader_sdf.hlsl:111-135) ---------------
// Step: nothing, or the GeoStep of a scene that reads the march state (scene_distance, below, makes it).  Called without one by the
// wavefront march (k_march), where no scene that reads the march state runs.
template <class Scene, bool DBG, class... Step>
SDF_HD float map_geometry(const FrameU &U, const DebugFlags &F, const typename Scene::RayInv &R, vec3 p, vec3 dir, bool fast, const Step &...gs)
{
	if (!DBG)
		return Scene::dist(U, R, p, dir, fast, gs...);
	float d = 3e38f;
	if (F.show_on)
		d = Scene::dist(U, R, p, dir, fast, gs...);
	if (F.plane_on)
	{
		float plane = sd_plane_fast(p - V3(U.debug_x, U.debug_y, U.debug_z), dir, fast, U.debug_normal);
		return min1(d, plane);
	}
	return d;
}

// The one call for a scene's distance at a sample: its camera_distance and the pixel's ray offsets go along, and a scene that reads the
// march state (geometry_reads_march_state, sdfr_scene_traits.h) gets them as a GeoStep -- formed here and nowhere else; every other
// scene gets (p, dir), and the three arguments leave no trace in its code.
template <class Scene, bool DBG>
SDF_HD float scene_distance(const FrameU &U, const DebugFlags &F, const typename Scene::RayInv &R, vec3 p, vec3 dir, bool fast, float camera_distance,
	vec3 right_off, vec3 bottom_off)
{
	if constexpr (SceneReadsMarchState<Scene>::value)
	{
		GeoStep gs;
		gs.camera_distance = camera_distance;
		gs.right_off = right_off;
		gs.bottom_off = bottom_off;
		return map_geometry<Scene, DBG>(U, F, R, p, dir, fast, gs);
	}
	else
		return map_geometry<Scene, DBG>(U, F, R, p, dir, fast);
}

// ---- sphere tracing with over-relaxation (pshader_sdf.hlsl:179-220) as a resumable state ----
struct March
{
	vec3 start, dir;
	float t;          // camera_distance
	float last_d;     // last_scene_distance
	float last_safe;  // last_safe_camera_distance
	float factor;     // step_factor
	float d;          // scene_distance of the last evaluation (already * inside_sign)
	uint32_t iter;
};
enum { MARCH_CONTINUE = 0, MARCH_HIT = 1, MARCH_MISS = 2 };

SDF_HD March march_begin(vec3 start, vec3 dir)
{
	March m;
	m.start = start;
	m.dir = dir;
	m.t = 0.f;
	m.last_d = 0.f;
	m.last_safe = 0.f;
	m.factor = 1.f;
	m.d = 0.f;
	m.iter = 0;
	return m;
}
SDF_HD vec3 march_pos(const March &m) { return mad(m.dir, m.t, m.start); }

// consume one scene-distance sample `d` taken at march_pos(m); requires m.iter < iter_count
SDF_HD int march_advance(March &m, float d, float dist_max, uint32_t iter_count, float dist_eps)
{
	// written with selects instead of branches: the loop body is short and every lane of the wave
	// takes one of the three ways each iteration
	m.d = d;
	// over-stepped: rewind to the last safe point and continue without relaxation
	const bool over = (m.factor > 1.f) & ((m.last_d + d) < m.last_d * m.factor);
	const bool out_of_range = m.t > dist_max;
	const bool stop = !over & (out_of_range | (d < dist_eps));
	const float t_fwd = m.t + d * m.factor;
	const float safe_fwd = m.t + d;
	m.last_d = over ? m.last_d : d;
	m.t = stop ? m.t : (over ? m.last_safe : t_fwd);
	m.last_safe = (over | stop) ? m.last_safe : safe_fwd;
	m.factor = over ? 1.f : m.factor;
	if (stop) return out_of_range ? MARCH_MISS : MARCH_HIT;
	m.iter++;
	return m.iter < iter_count ? MARCH_CONTINUE : MARCH_MISS;
}
// relaxation starts at the fourth sample (pshader_sdf.hlsl:189-192)
SDF_HD void march_pre(March &m) { if (m.iter == 3) m.factor = 1.5f; }
// march_advance for one of a ray's first three samples, where m.factor is 1 (requires m.iter < 3 and m.iter < iter_count; no march_pre
// before it): no over-step, d * 1 is d, so the step forward and the last safe point are the one sum, and m.factor stays.  Every field
// of the state and the status come out as march_pre + march_advance leave them, bit for bit (tests/test_march_peel_cpu.py).
SDF_HD int march_advance_unrelaxed(March &m, float d, float dist_max, uint32_t iter_count, float dist_eps)
{
	m.d = d;
	const bool out_of_range = m.t > dist_max;
	const bool stop = out_of_range | (d < dist_eps);
	const float fwd = m.t + d;
	m.last_d = d;
	m.t = stop ? m.t : fwd;
	m.last_safe = stop ? m.last_safe : fwd;
	if (stop) return out_of_range ? MARCH_MISS : MARCH_HIT;
	m.iter++;
	return m.iter < iter_count ? MARCH_CONTINUE : MARCH_MISS;
}

// ---- forward-difference normal (pshader_sdf.hlsl:164-177, Q10) --------------------------------
SDF_HD vec3 grad_sample_pos(vec3 p, int axis, float eps)
{
	if (axis == 0) return p + V3(eps, 0.f, 0.f);
	if (axis == 1) return p + V3(0.f, eps, 0.f);
	return p + V3(0.f, 0.f, eps);
}

// normal_output as the driver preloads it, then the scene's say
template <class Scene>
SDF_HD NormalOut scene_normal(const FrameU &U, vec3 hit_pos, vec3 dir, float camera_distance, vec3 right_ray, vec3 bottom_ray)
{
	NormalOut no;
	no.sample_dist = U.grad_eps;
	no.normal = V3s(0.f);
	no.use_normal = false;
	if (SceneNormal<Scene>::value)
	{
		SurfacePoint sp;
		sp.pos = hit_pos;
		sp.dir = dir;
		sp.camera_distance = camera_distance;
		sp.right_off = right_ray;
		sp.bottom_off = bottom_ray;
		sp.normal = V3s(0.f);
		sp.iteration_count = 0u;
		sp.scene_distance = 0.f;
		SceneNormal<Scene>::call(U, sp, no);
	}
	return no;
}

// ---- results handed from marching to shading ---------------------------------------------------
struct HitInfo
{
	vec3 pos;         // geometry_input.pos at the hit
	float t;          // camera_distance
	float d;          // scene_distance (* inside_sign)
	uint32_t iter;
	vec3 normal;      // normal_output.normal
	float sample_dist; // normal_output.normal_sample_dist: grad_eps unless the scene's map_normal changed it (pshader_sdf.hlsl:323,520)
};

// the queue storage is supplied by the caller (registers/scratch in the per-pixel kernel,
// HBM arrays in the wavefront kernels)
template <class Store>
struct Spawner
{
	Store &store;
	uint64_t depths;
	int count;
	int slots;
	SDF_HD Spawner(Store &s, uint64_t d, int c, int n) : store(s), depths(d), count(c), slots(n) {}
	// `if (ray_count < RAY_COUNT) { find_free_ray; fill; ++ray_count; }`
	SDF_HD void push(const RayRec &r)
	{
		if (count < slots)
		{
			int slot = queue_free(depths, slots);
			store.put(slot, r);
			depths = queue_set_depth(depths, slot, ray_depth(r));
			++count;
		}
	}
};

SDF_HD Material default_material(const FrameU &U, vec3 hit_pos)
{
	Material m;
	m.id = MAT_NONE;
	m.mpos = hit_pos;
	m.prop_x = 0.f;
	m.diffuse = V4(0.f, 0.f, 0.f, 1.f);
	m.specular = V4(0.f, 0.f, 0.f, 60.f);
	m.emissive = V3s(0.f);
	m.reflection = V3s(0.f);
	m.refraction = V3s(0.f);
	m.ior = 1.4f;
	m.normal = V4(0.f, 0.f, 0.f, 0.f);
	m.max_cost = U.max_cost_default;
	m.use_hdr = true;
	return m;
}

// map_material (pshader_sdf.hlsl:137-162)
template <class Scene, bool DBG>
SDF_HD void map_material(const FrameU &U, const DebugFlags &F, const SurfacePoint &sp, Material &m)
{
	if (!DBG)
	{
		Scene::material(U, sp, m);
		return;
	}
	bool on_debug_plane = false;
	if (F.plane_on)
	{
		float plane = sd_plane(sp.pos - V3(U.debug_x, U.debug_y, U.debug_z), U.debug_normal);
		on_debug_plane = on_surface(U, plane);
	}
	if (on_debug_plane)
	{
		RayFlags nf;
		nf.has_transparent = false;
		nf.is_shadow = false;
		nf.last_transparent_pos = V3s(0.f);
		typename Scene::RayInv R0 = Scene::ray_setup(U, sp.dir, nf);
		const float d = scene_distance<Scene, false>(U, F, R0, sp.pos, sp.dir, false, sp.camera_distance, sp.right_off, sp.bottom_off); // the scene's alone
		m.id = MAT_DISTANCE_PLANE;
		m.prop_x = d / U.debug_scale;
	}
	else
	{
		Scene::material(U, sp, m);
	}
}

// the direction in which directional light i shines
template <class Scene>
SDF_HD vec3 directional_light_dir(const FrameU &U, int i, const Light &L)
{
	if (FrameSunDir<Scene>::value && i == 0) return FrameSunDir<Scene>::get(U);
	return L.pos / (length(L.pos) + U.dist_eps);
}
struct InlineShadows
{
	vec3 acc;   // the pixel's sum; shade_hit adds the hit's colour and the delivered light to it, in the order the bounce loop would
	int budget; // turns of the bounce loop left after this ray's
	int taken;  // shadow rays delivered here: each counts as a ray and a turn
};

// map_light for a scene in the reference's own shape (lights(), sdfr_scene_traits.h): the table as the driver hands it over -- no slot used, every
// light zero --, then the scene's one call, which may also change `ambient`.  Called under `if constexpr (SceneLights<Scene>::value)`:
// handing the one-entry tables of a scene that answers slot by slot to a function, even an empty one, changed every scene's query kernels.
template <class Scene>
SDF_HD void scene_light_table(const FrameU &U, const SurfacePoint &sp, Light *table, bool *table_used, float &ambient)
{
	for (int i = 0; i < SDFR_MAX_LIGHTS; ++i)
	{
		table_used[i] = false;
		table[i].pos = V3s(0.f);
		table[i].directional = false;
		table[i].extend = 0.f;
		table[i].color = V3s(0.f);
		table[i].falloff = 0.f;
	}
	Scene::lights(U, sp, table, table_used, ambient);
}
// light i of the frame: the scene's (its own slot function or the table a scene in the reference's shape filled), or an extension light
template <class Scene, class Table, class Used>
SDF_HD bool light_in_slot(const FrameU &U, int i, const Table &table, const Used &table_used, Light &L)
{
	bool used = SceneLightSlot<Scene>::get(U, i, L);
	if (SceneLights<Scene>::value)
	{
		L = table[i];
		used = table_used[i];
	}
	if (i >= 1 && i <= U.extension_lights) // extension: orbiting point lights (sdfr_frame.h)
	{
		const float *E = U.ext_light[i - 1];
		L.pos = V3(E[0], E[1], E[2]);
		L.directional = false;
		L.extend = 0.25f;
		L.falloff = 0.25f;
		L.color = V3(E[3], E[4], E[5]);
		used = true;
	}
	return used;
}
SDF_HD vec3 light_colour(const Light &L)
{
	float falloff = 1.f;
	if (!L.directional) falloff = pow1(0.1f, L.falloff); // distance-independent (Q3)
	return L.color * falloff;
}

// Shade a ray that hit the scene (pshader_sdf.hlsl:317-620).  Returns the colour this ray
// adds to the pixel (already multiplied by the ray's contribution); updates `hdr`; pushes
// secondary rays.
// NG: where the noise of the procedural materials gets its gradients (sdfr_noise.h)
template <class Scene, bool DBG, class Store, bool INL = false, class NG = NoiseGradFormula>
SDF_HD vec3 shade_hit(const FrameU &U, const DebugFlags &F, const RayRec &ray, const PixelRay &px, const HitInfo &hit, float max_range,
	float &hdr, Spawner<Store> &q, InlineShadows *inl = nullptr)
{
	bool added = false; // INL: the returned colour is in inl->acc already
	const uint32_t depth = ray_depth(ray);
	const float inside_sign = ray_inside_sign(ray);
	const vec3 view_dir = ray.dir;

	SurfacePoint sp;
	sp.pos = hit.pos;
	sp.dir = ray.dir;
	sp.camera_distance = hit.t;
	sp.right_off = px.right_ray;
	sp.bottom_off = px.bottom_ray;
	sp.normal = hit.normal;
	sp.iteration_count = hit.iter;
	sp.scene_distance = hit.d;

	Material m = default_material(U, hit.pos);
	map_material<Scene, DBG>(U, F, sp, m);
	// extension, off by default: reflective marble (sdfr_limits::extension_marble_reflection)
	if (U.extension_marble_reflection != 0.f && (m.id == MAT_MARBLE_DARK || m.id == MAT_MARBLE_LIGHT)) m.reflection = V3s(U.extension_marble_reflection);

	vec3 out = V3s(0.f);
	if (!ray_is_shadow(ray))
	{
		// the first surface decides whether the pixel is tone-mapped (Q2)
		float new_hdr = m.use_hdr ? 1.f : 0.f;
		hdr = lerp1(hdr, new_hdr, step1(hdr, 0.f));

		vec3 n = lerp(hit.normal, V3(m.normal.x, m.normal.y, m.normal.z), m.normal.w);

		// reflection: cost 3, outside rays only
		if (any3(m.reflection) && inside_sign > 0.f && depth + 3 < m.max_cost)
		{
			vec3 rv = reflect(view_dir, n);
			RayRec c;
			c.pos = mad(rv, U.reflect_eps, hit.pos);
			c.dir = rv;
			c.contrib = m.reflection * ray.contrib;
			c.shadow_range = 0.f;
			c.bits = depth + 3;
			q.push(c);
		}
		// refraction: admitted at cost 4, queued at cost 2 (pshader_sdf.hlsl:387,405)
		if (any3(m.refraction) && depth + 4 < m.max_cost)
		{
			RayRec c;
			vec3 rv;
			if (inside_sign > 0.f)
			{
				rv = refract(view_dir, n, 1.f / m.ior);
				c.bits = (depth + 2) | RAY_INSIDE;
			}
			else
			{
				rv = refract(view_dir, -n, m.ior);
				c.bits = depth + 2;
			}
			c.pos = mad(rv, U.refract_eps, hit.pos);
			c.dir = rv;
			c.contrib = m.refraction * ray.contrib;
			c.shadow_range = 0.f;
			q.push(c);
		}

		vec3 diffuse = V3(m.diffuse.x, m.diffuse.y, m.diffuse.z);
		vec3 color = V3s(0.f);
		bool use_light = true;
		switch (m.id)
		{
		case MAT_ITER:
			color = color + mat_iter_heat(hit.iter, (uint32_t)(U.iter_count - 1));
			use_light = false;
			hdr = 0.f;
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
			hdr = 0.f;
			break;
		}
		case MAT_NORMAL2:
			color = color + abs(n);
			use_light = false;
			hdr = 0.f;
			break;
		case MAT_DISTANCE_PLANE:
			color = color + mat_debug_plane(m.prop_x);
			use_light = false;
			hdr = 0.f;
			break;
		case MAT_WOOD:
			diffuse = diffuse + mat_wood<NG>(m.mpos);
			break;
		case MAT_MARBLE_DARK:
			diffuse = diffuse + mat_marble<NG>(m.mpos, V3(0.556f, 0.478f, 0.541f));
			break;
		case MAT_MARBLE_LIGHT:
			diffuse = diffuse + mat_marble<NG>(m.mpos, V3(0.7f, 0.7f, 0.7f));
			break;
		case MAT_FIRE:
		{
			float fadeout = sat1(dot(-view_dir, n));
			vec4 fc = mat_fire<NG>(m.mpos, 1.f - fadeout);
			color = color + V3(fc.x, fc.y, fc.z);
			m.diffuse = V4(1.f, 1.f, 1.f, sat1(fc.w));
			break;
		}
		default:
			break;
		}

		// see-through surface: continue the same ray from the hit point (Q8)
		if (m.diffuse.w < 1.f && depth + 2 < m.max_cost)
		{
			RayRec c;
			c.pos = hit.pos;
			c.dir = view_dir;
			c.contrib = (1.f - m.diffuse.w) * V3(m.diffuse.x, m.diffuse.y, m.diffuse.z) * ray.contrib;
			c.shadow_range = 0.f;
			c.bits = (depth + 2) | RAY_TRANSPARENT;
			q.push(c);
		}

		if (use_light)
		{
			float ambient = SceneAmbient<Scene>::get(); // map_light may override the default 0.075
			// a scene in the reference's own shape fills the whole light table in one call (SceneLights)
			Light table[SceneLights<Scene>::value ? SDFR_MAX_LIGHTS : 1];
			bool table_used[SceneLights<Scene>::value ? SDFR_MAX_LIGHTS : 1];
			if constexpr (SceneLights<Scene>::value) scene_light_table<Scene>(U, sp, table, table_used, ambient);
			float move = max1(U.shadow_eps, hit.sample_dist) + max1(0.f, -hit.d);
			vec3 lit_pos = mad(n, move, hit.pos);
			const float alpha = sat1(m.diffuse.w);

			if constexpr (INL)
			{
				// The hit's own colour first -- every light's ambient share, in the lights' order -- so that it is in the pixel's sum
				// before any light a shadow ray delivers; then the loop as below, the ambient line left out.
				for (int i = 0; i < U.light_count; ++i)
				{
					Light L;
					if (!light_in_slot<Scene>(U, i, table, table_used, L)) continue;
					color = color + diffuse * light_colour(L) * ambient;
				}
				color = color + m.emissive;
				color = color * alpha;
				out = out + color * ray.contrib;
				inl->acc = inl->acc + out;
				added = true;
				for (int i = 0; i < U.light_count; ++i)
				{
					Light L;
					if (!light_in_slot<Scene>(U, i, table, table_used, L)) continue;
					vec3 ldir;
					float trace_dist;
					if (L.directional)
					{
						ldir = directional_light_dir<Scene>(U, i, L);
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
					float ndl = sat1(dot(-n, ldir));
					vec3 direct = V3s(0.f) + diffuse * lcol * ndl;
					vec3 half_vec = -normalize(view_dir + ldir);
					float spec = pow1(sat1(dot(n, half_vec)), m.specular.w);
					direct = direct + V3(m.specular.x, m.specular.y, m.specular.z) * lcol * spec;
					if (depth + 2 < m.max_cost && ndl > 0.f)
					{
						RayRec c;
						c.pos = lit_pos;
						c.dir = -ldir;
						c.contrib = direct * ray.contrib * alpha;
						c.shadow_range = trace_dist;
						c.bits = (depth + 2) | RAY_SHADOW;
						// the reference's queue holds the rays delivered so far as well: it has a slot for this one only if all of them fit
						if (inl->taken + q.count >= q.slots) continue;
						if (U.step_shortcuts != 0 && q.count == 0 && inl->taken < inl->budget)
						{
							// the first turn of the march loop (render_pixel): an unrelaxed sample at the ray's start
							const typename Scene::RayInv R = Scene::ray_setup(U, c.dir, ray_flags(c));
							March sm = march_begin(c.pos, c.dir);
							march_pre(sm);
							if (sm.factor == 1.f && RayEscapes<Scene>::test(U, R, march_pos(sm), c.dir))
							{
								inl->acc = inl->acc + (V3s(0.f) + c.contrib); // shade_miss of a shadow ray
								inl->taken++;
								q.store.ray_marched(c, 0u, MARCH_MISS);
								continue;
							}
						}
						q.push(c);
					}
				}
			}
			else // the reference's one loop: every light's ambient share and its shadow ray (body not re-indented: the headline kernel's code;
			// light_in_slot and light_colour in its place were tried and changed every scene's code)
			for (int i = 0; i < U.light_count; ++i)
			{
				Light L;
				bool used = SceneLightSlot<Scene>::get(U, i, L);
				if (SceneLights<Scene>::value)
				{
					L = table[i];
					used = table_used[i];
				}
				if (i >= 1 && i <= U.extension_lights) // extension: orbiting point lights (sdfr_frame.h)
				{
					const float *E = U.ext_light[i - 1];
					L.pos = V3(E[0], E[1], E[2]);
					L.directional = false;
					L.extend = 0.25f;
					L.falloff = 0.25f;
					L.color = V3(E[3], E[4], E[5]);
					used = true;
				}
				if (!used) continue;
				vec3 ldir;
				float trace_dist;
				float falloff = 1.f;
				if (L.directional)
				{
					ldir = directional_light_dir<Scene>(U, i, L);
					trace_dist = U.range;
				}
				else
				{
					ldir = lit_pos - L.pos;
					trace_dist = length(ldir);
					ldir = ldir / trace_dist;
					trace_dist = trace_dist - L.extend;
					falloff = pow1(0.1f, L.falloff); // distance-independent (Q3)
				}
				vec3 lcol = L.color * falloff;

				color = color + diffuse * lcol * ambient;

				// diffuse + Blinn specular are delivered by the shadow ray if it escapes (F6)
				float ndl = sat1(dot(-n, ldir));
				vec3 direct = V3s(0.f) + diffuse * lcol * ndl;
				vec3 half_vec = -normalize(view_dir + ldir);
				float spec = pow1(sat1(dot(n, half_vec)), m.specular.w);
				direct = direct + V3(m.specular.x, m.specular.y, m.specular.z) * lcol * spec;

				if (depth + 2 < m.max_cost && ndl > 0.f)
				{
					RayRec c;
					c.pos = lit_pos;
					c.dir = -ldir;
					c.contrib = direct * ray.contrib * alpha;
					c.shadow_range = trace_dist;
					c.bits = (depth + 2) | RAY_SHADOW;
					q.push(c);
				}
			}
			if (!added)
			{
				color = color + m.emissive;
				color = color * alpha;
			}
		}
		if (!added) out = out + color * ray.contrib;
	}
	else
	{
		// a shadow ray stopped by a see-through surface continues, tinted (pshader_sdf.hlsl:598-619)
		if (m.diffuse.w < 1.f && depth + 2 < m.max_cost)
		{
			RayRec c;
			c.pos = hit.pos;
			c.dir = view_dir;
			c.contrib = (1.f - m.diffuse.w) * V3(m.diffuse.x, m.diffuse.y, m.diffuse.z) * ray.contrib;
			c.shadow_range = max_range - hit.t;
			c.bits = (depth + 2) | RAY_TRANSPARENT | RAY_SHADOW;
			q.push(c);
		}
	}
	if constexpr (INL)
		if (!added) inl->acc = inl->acc + out;
	return out;
}

// A ray that left the scene (pshader_sdf.hlsl:621-632): an escaped shadow ray delivers the
// light it carries, any other ray sees the background.
template <class Scene, class NG = NoiseGradFormula>
SDF_HD vec3 shade_miss(const FrameU &U, const RayRec &ray, uint32_t iter)
{
	if (ray_is_shadow(ray))
		return V3s(0.f) + ray.contrib;
	return V3s(0.f) + SceneBackground<Scene, NG>::get(U, ray.dir, iter) * ray.contrib;
}

} // namespace sdfr

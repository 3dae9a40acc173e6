// sdfr_render_pixel.h -- the whole pipeline for ONE pixel, start to finish, on one lane.
//
// Used by the "pixel" kernel (one lane per pixel, sdfr_pixel_kernel.h), by scenes compiled at
// run time (sdfr_jit.cpp) and by tests/hostsim, which compiles it for the CPU to bit-compare the
// pipeline stages with the oracle where no GPU is available.  The schedule follows the
// reference's bounce loop (pshader_sdf.hlsl:286-634) literally.
#pragma once
#include "sdfr_pixel.h"

namespace sdfr {


struct LocalRayStore
{
	RayRec slot[SDFR_MAX_RAYS];
	SDF_HD void put(int i, const RayRec &r) { slot[i] = r; }
	SDF_HD RayRec get(int i) const { return slot[i]; }
	SDF_HD void ray_marched(const RayRec &, uint32_t, int) {}
};

// Write-behind cache of depth one in front of a ray store: the most recently pushed ray stays
// in registers and reaches the backing store only when another push follows.  Most pixels
// spawn a single child (the shadow ray) that is popped right away, so its 44-byte record never
// travels to HBM and back.
//
// A store also keeps the pixel's ray footprint (PixelRay) between the prologue and the hit
// shading that needs it for the checker filter: keep_pixel_ray / pixel_ray_kept; and the pixel's
// tone-map flag, which only hit shading touches: keep_hdr / hdr_kept.
template <class Backing>
struct CachedRayStore
{
	Backing &backing;
	RayRec cached;
	int cached_slot;
	PixelRay kept;
	float hdr;
	SDF_HD explicit CachedRayStore(Backing &b) : backing(b), cached_slot(-1) {}
	SDF_HD void keep_pixel_ray(const PixelRay &pr) { kept = pr; }
	SDF_HD PixelRay pixel_ray_kept() const { return kept; }
	SDF_HD void keep_hdr(float h) { hdr = h; }
	SDF_HD float hdr_kept() const { return hdr; }
	SDF_HD void ray_marched(const RayRec &r, uint32_t iter, int status) { backing.ray_marched(r, iter, status); }
	SDF_HD void put(int i, const RayRec &r)
	{
		if (cached_slot >= 0) backing.put(cached_slot, cached);
		cached = r;
		cached_slot = i;
	}
	SDF_HD RayRec get(int i)
	{
		if (i == cached_slot)
		{
			cached_slot = -1;
			return cached;
		}
		return backing.get(i);
	}
};

// which sample of a ray a pass of the peeled march takes (render_pixel): one of the first three, whose m.factor is 1, or a later one
template <bool FirstThree>
struct MarchSample { static constexpr bool value = FirstThree; };

struct PixelCounters
{
	uint32_t rays, march_evals, hits;
#ifdef SDFR_PHASE_CLOCKS
	// developer build (tools/phase_clocks.py): wave clock spent marching / taking normals / shading
	uint64_t clk_march, clk_grad, clk_shade, clk_miss, clk_total;
#endif
};
#ifdef SDFR_PHASE_CLOCKS
#define SDFR_CLK(var) const uint64_t var = __builtin_readcyclecounter()
#define SDFR_CLK_ADD(field, t0, t1) cnt.field += (t1) - (t0)
#else
#define SDFR_CLK(var)
#define SDFR_CLK_ADD(field, t0, t1)
#endif

// `store` holds the pixel's pending rays (put/get by slot).  The primary ray never enters
// it: the reference pops it from slot 0 before anything is pushed (pshader_sdf.hlsl:289-294),
// so the queue is empty -- and slot 0 free again -- when the first hit is shaded.  NG: the gradient source of the shading's
// noise (sdfr_noise.h).
template <class Scene, bool DBG, class Store, class NG = NoiseGradFormula>
SDF_HD vec4 render_pixel(const FrameU &U, int px, int py, PixelCounters &cnt, Store &store)
{
	SDFR_CLK(c_begin);
	constexpr bool INL = !DBG && InlineEscapedShadows<Scene>::value;
	const DebugFlags F = debug_flags(U);
	RayRec ray;
	{
		const PixelRay pr = pixel_ray(U, px, py);
		ray = primary_ray(U, pr);
		store.keep_pixel_ray(pr);
	}
	uint64_t depths = SDFR_QUEUE_EMPTY;
	int count = 0; // rays waiting in the store

	store.keep_hdr(-1.f); // hdr_output "not set" (pshader_sdf.hlsl:284)
	vec3 acc = V3s(0.f);
	for (int bounce = 0; bounce < U.bounce_count; ++bounce)
	{
		if (bounce > 0)
		{
			if (count == 0) break;
			const int idx = queue_next(depths, U.ray_count);
			ray = store.get(idx);
			depths = queue_set_depth(depths, idx, RAY_DEPTH_INVALID);
			--count;
		}
		cnt.rays++;

		typename Scene::RayInv R = Scene::ray_setup(U, ray.dir, ray_flags(ray));
		const float inside_sign = ray_inside_sign(ray);
		const float max_range = ray_is_shadow(ray) ? ray.shadow_range : U.range;

		SDFR_CLK(c0);
		March m = march_begin(ray.pos, ray.dir);
		int status;
		const uint32_t evals_before = cnt.march_evals;
		const bool shortcuts = !DBG && (RayEscapes<Scene>::value || EscapesFrom<Scene>::value) && U.step_shortcuts != 0 && inside_sign > 0.f;
		if constexpr (RayBounds<Scene>::value)
			if (shortcuts) RayBounds<Scene>::apply(U, R, ray.pos, ray.dir, max_range); // what the start and the range fix for the whole ray
		float clear_from = 3e38f;
		if constexpr (EscapesFrom<Scene>::value)
			if (shortcuts) clear_from = EscapesFrom<Scene>::get(U, ray.pos, ray.dir, max_range); // (a ray inside a refracting body ends on its surface)
		if constexpr (!DBG && PeelUnrelaxedSamples<Scene>::value)
		{
			// The loop below with the ray's first three samples in front of it as straight-line code (PeelUnrelaxedSamples, sdfr_scene_traits.h): one
			// pass, `first_three` a MarchSample: with m.factor 1 for certain an escaped sample ends the ray before its evaluation and nothing
			// is rewound (march_advance_unrelaxed).  Then the factor once, then the passes that may rewind, without march_pre.
			auto march_step = [&](auto first_three) -> int
			{
				constexpr bool UNRELAXED = decltype(first_three)::value;
				bool escaped = shortcuts && RayEscapes<Scene>::test(U, R, march_pos(m), ray.dir);
				if constexpr (EscapesFrom<Scene>::value) escaped = escaped || m.t >= clear_from;
				if (escaped && (UNRELAXED || m.factor == 1.f)) return MARCH_MISS;
				const PixelRay pr = store.pixel_ray_kept(); // (read by a scene that reads the march state alone)
				const float d = scene_distance<Scene, DBG>(U, F, R, march_pos(m), ray.dir, true, m.t, pr.right_ray, pr.bottom_ray) * inside_sign;
				cnt.march_evals++;
				if constexpr (UNRELAXED)
					return march_advance_unrelaxed(m, d, max_range, (uint32_t)U.iter_count, U.dist_eps);
				else
				{
					if (escaped && !((m.last_d + d) < m.last_d * m.factor)) return MARCH_MISS;
					return march_advance(m, d, max_range, (uint32_t)U.iter_count, U.dist_eps);
				}
			};
			// (a ray goes on more often than not: said, because a comparison with 0 counts as unlikely and the compiler laid the passes out backwards)
			status = march_step(MarchSample<true>());
			if (__builtin_expect(status == MARCH_CONTINUE, 1)) status = march_step(MarchSample<true>());
			if (__builtin_expect(status == MARCH_CONTINUE, 1)) status = march_step(MarchSample<true>());
			if (__builtin_expect(status == MARCH_CONTINUE, 1))
			{
				m.factor = 1.5f;
				do
					status = march_step(MarchSample<false>());
				while (status == MARCH_CONTINUE);
			}
		}
		else // the march as every other scene's kernel has it (body not re-indented: their code stays what it was; one step body shared with the
		// passes above was tried and changed every scene's code)
		do
		{
			march_pre(m);
			// Step shortcut.  Only a sample the march will not take back may end the ray: an unrelaxed one (factor 1: the
			// first three samples and everything after a rewind) is final as it stands, a relaxed one once its own distance
			// shows that it did not over-step (march_advance's test) -- an over-stepped sample can lie beyond an obstacle
			// that the rewound march then hits.
			bool escaped = shortcuts && RayEscapes<Scene>::test(U, R, march_pos(m), ray.dir);
			if constexpr (EscapesFrom<Scene>::value) escaped = escaped || m.t >= clear_from;
			if (escaped && m.factor == 1.f)
			{
				status = MARCH_MISS; // what the remaining steps would come to
				break;
			}
			float d;
			if constexpr (SceneReadsMarchState<Scene>::value)
			{
				const PixelRay pr = store.pixel_ray_kept();
				d = scene_distance<Scene, DBG>(U, F, R, march_pos(m), ray.dir, true, m.t, pr.right_ray, pr.bottom_ray) * inside_sign;
			}
			else // (through scene_distance as well, this call changed the code of the tree's kernel)
				d = map_geometry<Scene, DBG>(U, F, R, march_pos(m), ray.dir, true) * inside_sign;
			cnt.march_evals++;
			if (escaped && !((m.last_d + d) < m.last_d * m.factor))
			{
				status = MARCH_MISS;
				break;
			}
			status = march_advance(m, d, max_range, (uint32_t)U.iter_count, U.dist_eps);
		} while (status == MARCH_CONTINUE);
		SDFR_CLK(c1);
		SDFR_CLK_ADD(clk_march, c0, c1);
		store.ray_marched(ray, cnt.march_evals - evals_before, status); // a hook for analysis builds (tests/hostsim); empty in the kernels

		// A shadow ray stopped by a surface whose material nobody needs (ShadowHitsNeedMaterial, sdfr_scene_traits.h): the hit is counted, and what
		// shade_hit would come to -- add 0, push nothing, leave the tone-map flag alone -- is what a miss does with a ray that carries no
		// light: shade_miss of a shadow ray is 0 + contrib, +0 in every component, as V3s(0) is.  Written as a change of the ray and not as a
		// third branch beside hit and miss: the branch cost the march loop a one-bank fma or the kernel 4 bytes of scratch, wherever it stood.
		if (!DBG && !ShadowHitsNeedMaterial<Scene>::value && ray_is_shadow(ray) && status == MARCH_HIT)
		{
			cnt.hits++;
			ray.contrib = V3s(0.f);
			status = MARCH_MISS;
		}
		vec3 out;
		if (status == MARCH_HIT)
		{
			cnt.hits++;
			HitInfo hit;
			hit.pos = march_pos(m);
			hit.t = m.t;
			hit.d = m.d;
			hit.iter = m.iter;
			hit.normal = V3s(0.f);
			hit.sample_dist = U.grad_eps;
			if (ShadowHitsNeedNormal<Scene>::value || !ray_is_shadow(ray))
			{
				// map_normal, then the sampled normal unless the scene supplied one (pshader_sdf.hlsl:318-330)
				NormalOut no;
				if (SceneNormal<Scene>::value)
				{
					const PixelRay pr = store.pixel_ray_kept();
					no = scene_normal<Scene>(U, hit.pos, ray.dir, hit.t, pr.right_ray, pr.bottom_ray);
				}
				else
					no = scene_normal<Scene>(U, hit.pos, ray.dir, hit.t, V3s(0.f), V3s(0.f));
				hit.sample_dist = no.sample_dist;
				hit.normal = no.normal;
				if (!no.use_normal)
				{
					const float baseline = m.d * inside_sign;
					float g0, g1, g2;
					if constexpr (SceneReadsMarchState<Scene>::value)
					{
						// grad() works on the hit's GeometryInput: its camera_distance and offsets stay (pshader_sdf.hlsl:164-177)
						const PixelRay pr = store.pixel_ray_kept();
						g0 = scene_distance<Scene, DBG>(U, F, R, grad_sample_pos(hit.pos, 0, no.sample_dist), ray.dir, false, hit.t, pr.right_ray, pr.bottom_ray) - baseline;
						g1 = scene_distance<Scene, DBG>(U, F, R, grad_sample_pos(hit.pos, 1, no.sample_dist), ray.dir, false, hit.t, pr.right_ray, pr.bottom_ray) - baseline;
						g2 = scene_distance<Scene, DBG>(U, F, R, grad_sample_pos(hit.pos, 2, no.sample_dist), ray.dir, false, hit.t, pr.right_ray, pr.bottom_ray) - baseline;
					}
					else // (through scene_distance as well, these calls changed the code of every built-in scene's kernels but normal_test's)
					{
						g0 = map_geometry<Scene, DBG>(U, F, R, grad_sample_pos(hit.pos, 0, no.sample_dist), ray.dir, false) - baseline;
						g1 = map_geometry<Scene, DBG>(U, F, R, grad_sample_pos(hit.pos, 1, no.sample_dist), ray.dir, false) - baseline;
						g2 = map_geometry<Scene, DBG>(U, F, R, grad_sample_pos(hit.pos, 2, no.sample_dist), ray.dir, false) - baseline;
					}
					hit.normal = normalize(V3(g0, g1, g2));
				}
			}
#ifdef SDFR_PHASE_CLOCKS
			asm volatile("" : "+v"(hit.normal.x), "+v"(hit.normal.y), "+v"(hit.normal.z));
#endif
			SDFR_CLK(c2);
			SDFR_CLK_ADD(clk_grad, c1, c2);

			Spawner<Store> q(store, depths, count, U.ray_count);
			float hdr = store.hdr_kept();
			if constexpr (INL)
			{
				// escaped shadow rays deliver their light from the light loop (InlineEscapedShadows, sdfr_scene_traits.h): each is a ray and a turn of this loop
				InlineShadows inl;
				inl.acc = acc;
				inl.budget = U.bounce_count - 1 - bounce;
				inl.taken = 0;
				out = shade_hit<Scene, DBG, Store, true, NG>(U, F, ray, store.pixel_ray_kept(), hit, max_range, hdr, q, &inl);
				acc = inl.acc;
				bounce += inl.taken;
				cnt.rays += (uint32_t)inl.taken;
			}
			else
				out = shade_hit<Scene, DBG, Store, false, NG>(U, F, ray, store.pixel_ray_kept(), hit, max_range, hdr, q);
			store.keep_hdr(hdr);
			depths = q.depths;
			count = q.count;
#ifdef SDFR_PHASE_CLOCKS
			asm volatile("" : "+v"(out.x), "+v"(out.y), "+v"(out.z));
#endif
			SDFR_CLK(c3);
			SDFR_CLK_ADD(clk_shade, c2, c3);
			if constexpr (!INL) acc = acc + out;
		}
		else
		{
			out = shade_miss<Scene, NG>(U, ray, m.iter);
#ifdef SDFR_PHASE_CLOCKS
			asm volatile("" : "+v"(out.x), "+v"(out.y), "+v"(out.z));
#endif
			SDFR_CLK(c4);
			SDFR_CLK_ADD(clk_miss, c1, c4);
			acc = acc + out;
		}
	}
	SDFR_CLK(c_end);
	SDFR_CLK_ADD(clk_total, c_begin, c_end);
	return V4(acc.x, acc.y, acc.z, abs1(store.hdr_kept()));
}

} // namespace sdfr

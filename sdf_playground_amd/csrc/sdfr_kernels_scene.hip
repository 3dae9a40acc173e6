// sdfr_kernels_scene.hip -- the per-scene kernels of the renderer (k_pixel, k_march, k_shade; see
// sdfr_kernels.hip for the two schedules and everything that launches them), instantiated for ONE scene.  The build compiles this file
// once per scene of the registry (sdfr_perpixel.h) with -DSDFR_SCENE=<index> (sdf_playground_amd/buildlib.py),
// in parallel: 23 scenes x 2 debug variants x 3 kernels in one translation unit took a minute to compile,
// nothing in one scene's kernels depends on another's, and a scene can be built with options of its own
// (buildlib.SCENE_FLAGS).
#include "sdfr_kernels.h"
#include "sdfr_perpixel.h"
#include "sdfr_pixel_kernel.h"

#ifndef SDFR_SCENE
#error "compile with -DSDFR_SCENE=<scene index, sdfr_perpixel.h>"
#endif

namespace sdfr {

// refill a march wave once this many lanes are idle (or when all are); a wave claims SDFR_GRAB list entries per atomic (sdfr_kernels.h)
#define SDFR_REFILL_THRESHOLD 16

// =================================================================================================
// PIXEL schedule (body: sdfr_pixel_kernel.h)
// =================================================================================================
// the shading's noise reads its gradients from LDS where the scene asks for it (PixelNoiseGrads, sdfr_scene_traits.h); the debug variants keep the formula
template <class Scene, bool DBG>
__global__ SDFR_PIXEL_KERNEL_ATTRS(Scene) void k_pixel(PixelKernelArgs args)
{
	pixel_kernel<Scene, DBG, typename PickNoiseGrads<!DBG && PixelNoiseGrads<Scene>::value>::type>(args);
}

// =================================================================================================
// WAVEFRONT schedule (k_init lives in sdfr_kernels.hip)
// =================================================================================================
// march result fields
enum { RS_STATUS = 0, RS_T, RS_D, RS_NX, RS_NY, RS_NZ, RS_SAMPLE_DIST, RS_COUNT };

// ---- k_march ----------------------------------------------------------------------------------------
enum { LANE_IDLE = 0, LANE_MARCH = 1, LANE_GRAD0 = 2, LANE_GRAD1 = 3, LANE_GRAD2 = 4 };

template <class Scene, bool DBG>
__global__ __launch_bounds__(SDFR_BLOCK) void k_march(FrameU U, RowMap rm, WavefrontWorkspace ws, const uint32_t *__restrict__ list,
	const uint32_t *__restrict__ n_ptr, uint32_t *cursor, uint32_t *pixel_stats, RenderTotals *totals)
{
	const uint32_t n = *n_ptr;
	const size_t cap = ws.capacity;
	const DebugFlags F = debug_flags(U);
	const uint32_t lane = threadIdx.x & 63u;
	// [next, end) = unconsumed part of the list range this wave currently owns (wave-uniform).
	// Ranges of SDFR_GRAB entries are claimed from a per-round cursor with one atomic each, so
	// the load balances itself whatever the grid size and residency are.
	uint32_t next = 0, end = 0;
	bool exhausted = n == 0;

	int state = LANE_IDLE;
	uint32_t pid = 0;
	March m = march_begin(V3s(0.f), V3s(0.f));
	typename Scene::RayInv R = {};
	float inside_sign = 1.f, max_range = 0.f, baseline = 0.f, g0 = 0.f, g1 = 0.f;
	float sample_dist = U.grad_eps; // of the hit whose normal is being sampled (the scene's map_normal may widen it)
	uint32_t evals = 0;       // of the current ray
	uint32_t tot_evals = 0, tot_hits = 0;

	for (;;)
	{
		const unsigned long long idle = __ballot(state == LANE_IDLE);
		if (idle)
		{
			if (next == end && !exhausted)
			{
				uint32_t base = 0;
				if (lane == 0) base = atomicAdd(cursor, (uint32_t)SDFR_GRAB);
				base = __builtin_amdgcn_readfirstlane(base);
				if (base >= n)
					exhausted = true;
				else
				{
					next = base;
					end = base + SDFR_GRAB < n ? base + SDFR_GRAB : n;
				}
			}
			const uint32_t n_idle = (uint32_t)__popcll(idle);
			if (next == end)
			{
				if (n_idle == 64u) break; // list drained and every lane finished
			}
			else if (n_idle >= SDFR_REFILL_THRESHOLD || n_idle == 64u)
			{
				// hand the next list entries to the idle lanes, in lane order
				const uint32_t avail = end - next;
				if (state == LANE_IDLE)
				{
					const uint32_t rank = (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
					if (rank < avail)
					{
						const uint32_t p = list[next + rank];
						if (p != SDFR_INVALID_PIXEL)
						{
							pid = p;
							const RayRec ray = load_ray(ws.ray_cur, cap, pid);
							R = Scene::ray_setup(U, ray.dir, ray_flags(ray));
							inside_sign = ray_inside_sign(ray);
							max_range = ray_is_shadow(ray) ? ray.shadow_range : U.range;
							m = march_begin(ray.pos, ray.dir);
							evals = 0;
							state = LANE_MARCH;
						}
					}
				}
				next += n_idle < avail ? n_idle : avail;
			}
		}

		if (state != LANE_IDLE)
		{
			// one scene-distance evaluation per lane: a march sample or a normal sample
			const bool marching = state == LANE_MARCH;
			if (marching) march_pre(m);
			const vec3 hp = march_pos(m);
			vec3 p = hp;
			if (state == LANE_GRAD0) p = grad_sample_pos(hp, 0, sample_dist);
			if (state == LANE_GRAD1) p = grad_sample_pos(hp, 1, sample_dist);
			if (state == LANE_GRAD2) p = grad_sample_pos(hp, 2, sample_dist);
			const float dist = map_geometry<Scene, DBG>(U, F, R, p, m.dir, marching);

			if (marching)
			{
				evals++;
				const int status = march_advance(m, dist * inside_sign, max_range, (uint32_t)U.iter_count, U.dist_eps);
				if (status == MARCH_HIT)
				{
					baseline = m.d * inside_sign;
					state = LANE_GRAD0;
					sample_dist = U.grad_eps;
					if (SceneNormal<Scene>::value)
					{
						// map_normal (pshader_sdf.hlsl:318-330): the scene's own normal ends the ray here, a changed spacing feeds the samples
						int px, py;
						pid_to_pixel(U, rm, pid, px, py);
						const PixelRay pr = pixel_ray(U, px, py);
						const NormalOut no = scene_normal<Scene>(U, march_pos(m), m.dir, m.t, pr.right_ray, pr.bottom_ray);
						sample_dist = no.sample_dist;
						if (no.use_normal)
						{
							ws.result[RS_STATUS * cap + pid] = __uint_as_float((uint32_t)MARCH_HIT << 24 | m.iter);
							ws.result[RS_T * cap + pid] = m.t;
							ws.result[RS_D * cap + pid] = m.d;
							ws.result[RS_NX * cap + pid] = no.normal.x;
							ws.result[RS_NY * cap + pid] = no.normal.y;
							ws.result[RS_NZ * cap + pid] = no.normal.z;
							ws.result[RS_SAMPLE_DIST * cap + pid] = sample_dist;
							tot_evals += evals;
							tot_hits += 1;
							if (pixel_stats) pixel_stats[3 * (size_t)pid + 1] += evals;
							state = LANE_IDLE;
						}
					}
				}
				else if (status == MARCH_MISS)
				{
					ws.result[RS_STATUS * cap + pid] = __uint_as_float((uint32_t)MARCH_MISS << 24 | m.iter);
					tot_evals += evals;
					if (pixel_stats) pixel_stats[3 * (size_t)pid + 1] += evals;
					state = LANE_IDLE;
				}
			}
			else if (state == LANE_GRAD0)
			{
				g0 = dist - baseline;
				state = LANE_GRAD1;
			}
			else if (state == LANE_GRAD1)
			{
				g1 = dist - baseline;
				state = LANE_GRAD2;
			}
			else
			{
				const vec3 nrm = normalize(V3(g0, g1, dist - baseline));
				ws.result[RS_STATUS * cap + pid] = __uint_as_float((uint32_t)MARCH_HIT << 24 | m.iter);
				ws.result[RS_T * cap + pid] = m.t;
				ws.result[RS_D * cap + pid] = m.d;
				ws.result[RS_NX * cap + pid] = nrm.x;
				ws.result[RS_NY * cap + pid] = nrm.y;
				ws.result[RS_NZ * cap + pid] = nrm.z;
				ws.result[RS_SAMPLE_DIST * cap + pid] = sample_dist;
				tot_evals += evals;
				tot_hits += 1;
				if (pixel_stats) pixel_stats[3 * (size_t)pid + 1] += evals;
				state = LANE_IDLE;
			}
		}
	}
	block_add_totals(totals, 0, 0, tot_evals, tot_hits);
}

// ---- k_shade -----------------------------------------------------------------------------------------
template <class Scene, bool DBG>
__global__ __launch_bounds__(SDFR_BLOCK) void k_shade(FrameU U, RowMap rm, WavefrontWorkspace ws, const uint32_t *__restrict__ list,
	const uint32_t *__restrict__ n_ptr, uint32_t *__restrict__ next_list, uint32_t *next_n, int round, void *out, int format,
	uint32_t *pixel_stats, RenderTotals *totals)
{
	const uint32_t n = *n_ptr;
	const size_t cap = ws.capacity;
	const DebugFlags F = debug_flags(U);
	__shared__ uint32_t s_count, s_base;
	uint32_t n_rays = 0, n_done = 0;

	for (uint32_t base = blockIdx.x * SDFR_BLOCK; base < n; base += gridDim.x * SDFR_BLOCK)
	{
		if (threadIdx.x == 0) s_count = 0;
		__syncthreads();
		const uint32_t i = base + threadIdx.x;
		uint32_t pid = SDFR_INVALID_PIXEL;
		if (i < n) pid = list[i];
		bool alive = false;
		if (pid != SDFR_INVALID_PIXEL)
		{
			n_rays++;
			const RayRec ray = load_ray(ws.ray_cur, cap, pid);
			int px, py;
			pid_to_pixel(U, rm, pid, px, py);
			const PixelRay pr = pixel_ray(U, px, py);
			const uint32_t status_iter = __float_as_uint(ws.result[RS_STATUS * cap + pid]);
			const uint32_t status = status_iter >> 24, iter = status_iter & 0xffffffu;

			uint64_t depths = (uint64_t)ws.qdepth_lo[pid] | ((uint64_t)ws.qdepth_hi[pid] << 32);
			int count = 0;
			for (int s = 0; s < SDFR_MAX_RAYS; ++s)
				count += (((depths >> (8 * s)) & 0xffu) != RAY_DEPTH_INVALID) ? 1 : 0;
			float hdr = ws.accum[3 * cap + pid];

			vec3 add;
			GlobalRayStore store = {ws.ray_queue, cap, pid}; // the pixel's pending rays (48-byte records)
			if (status == MARCH_HIT)
			{
				HitInfo hit;
				hit.t = ws.result[RS_T * cap + pid];
				hit.d = ws.result[RS_D * cap + pid];
				hit.iter = iter;
				hit.normal = V3(ws.result[RS_NX * cap + pid], ws.result[RS_NY * cap + pid], ws.result[RS_NZ * cap + pid]);
				hit.sample_dist = ws.result[RS_SAMPLE_DIST * cap + pid];
				hit.pos = mad(ray.dir, hit.t, ray.pos);
				const float max_range = ray_is_shadow(ray) ? ray.shadow_range : U.range;
				Spawner<GlobalRayStore> q(store, depths, count, U.ray_count);
				add = shade_hit<Scene, DBG, GlobalRayStore>(U, F, ray, pr, hit, max_range, hdr, q);
				depths = q.depths;
				count = q.count;
				if (pixel_stats) pixel_stats[3 * (size_t)pid + 2] += 1;
			}
			else
			{
				add = shade_miss<Scene>(U, ray, iter);
			}
			const vec3 acc = V3(ws.accum[0 * cap + pid], ws.accum[1 * cap + pid], ws.accum[2 * cap + pid]) + add;
			if (pixel_stats) pixel_stats[3 * (size_t)pid + 0] += 1;

			if (count > 0 && round + 1 < U.bounce_count)
			{
				// pop the pixel's next ray: it is traced in the next round
				const int slot = queue_next(depths, U.ray_count);
				const RayRec nr = store.get(slot);
				store_ray(ws.ray_cur, cap, pid, nr);
				depths = queue_set_depth(depths, slot, RAY_DEPTH_INVALID);
				ws.qdepth_lo[pid] = (uint32_t)depths;
				ws.qdepth_hi[pid] = (uint32_t)(depths >> 32);
				ws.accum[0 * cap + pid] = acc.x;
				ws.accum[1 * cap + pid] = acc.y;
				ws.accum[2 * cap + pid] = acc.z;
				ws.accum[3 * cap + pid] = hdr;
				alive = true;
			}
			else
			{
				store_pixel(out, format, pid, V4(acc.x, acc.y, acc.z, abs1(hdr)), (uint32_t)rm.local_rows * (uint32_t)U.width);
				n_done++;
			}
		}
		// append the surviving pixels to the next round's list: one atomic per block
		uint32_t my_off = 0;
		if (alive) my_off = atomicAdd(&s_count, 1u);
		__syncthreads();
		if (threadIdx.x == 0 && s_count) s_base = atomicAdd(next_n, s_count);
		__syncthreads();
		if (alive) next_list[s_base + my_off] = pid;
		__syncthreads();
	}
	block_add_totals(totals, n_done, n_rays, 0, 0);
}

// =================================================================================================
// what this unit exports: the scene's kernels and launch traits, under a name made of the scene's index (scene_kernels, sdfr_kernels.hip)
// =================================================================================================
using UnitScene = SceneAt<SDFR_SCENE>::type;

const SceneKernels *SDFR_CAT(scene_kernels_, SDFR_SCENE)()
{
	// (named in the order pixel, march, shade with the debug variant first: a unit's code object holds its kernels in the order they are
	// first named in, and this keeps the order, and with it every byte of the object's code, that the launchers which lived here gave it)
	static const SceneKernels k = [] {
		SceneKernels k;
		k.pixel[1] = (const void *)k_pixel<UnitScene, true>;
		k.pixel[0] = (const void *)k_pixel<UnitScene, false>;
		k.march[1] = (const void *)k_march<UnitScene, true>;
		k.shade[1] = (const void *)k_shade<UnitScene, true>;
		k.march[0] = (const void *)k_march<UnitScene, false>;
		k.shade[0] = (const void *)k_shade<UnitScene, false>;
		k.persistent_tiles = PersistentTiles<UnitScene>::value;
		k.square_units = SquareUnits<UnitScene>::value;
		k.retire_after = RetireAfter<UnitScene>::value;
		k.tile_w_log2 = SceneTileShape<UnitScene>::value;
		return k;
	}();
	return &k;
}

} // namespace sdfr

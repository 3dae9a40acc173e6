// sdfr_components.hip -- the scene-independent kernels of sdfr_components_label (the rules: sdfr_components.h; the plan:
// sdfr_components_plan.h).  The distances they read are the scene's lattice kernel's (query_lattice_kernel) or the caller's.
//
//   bricks   a block owns 8 x 8 x 8 points: their inside bits, the brick's inner edges united in LDS with LDS atomics, then
//            parent[x] = the global index of the local root.  The local index orders the brick's points as the global one does (i
//            fastest), so the local minimum is the global minimum of that piece and parent[x] <= x holds globally.
//   seams    the edges that cross brick faces, united with global atomicMin at agent scope (HIP's default)
//   flatten  parent[x] = root(x)
//   number   flag parent[x] == x, the mesh's exclusive prefix sum over the flags; its last element, the number of components, is read
//            back and the table cut; then label[x] = scan[parent[x]] -- in place, and into the caller's labels --, a root starting its
//            component's record
//   tally    per point: a 64-bit atomicAdd of 1, atomicMin / atomicMax of the six bounds, an atomicOr of the face bits -- aggregated in
//            the wave first: when every live lane of a run of 64 points has one label, the common case, the wave's popcount and bounds
//            go on in registers to the next run, and one lane issues them at the end (k_components_tally)
//   pack     the records in component order into the caller's array, the counts by integer reductions in the wave, one atomic per wave
//            and word; the words lie COMPONENT_WORD_STRIDE apart while they are counted
//
// No kernel waits for another lane or workgroup: the stages are separate launches of one stream, and the union (components_union) acts
// only on what its atomics returned.  Every result is an integer and every atomic an integer one: the order of arrival changes nothing.
#include "sdfr_kernels.h"
#include "sdfr_components.h"
#include "sdfr_components_plan.h"

namespace sdfr {

static_assert(COMPONENTS_BLOCK % 64 == 0 && COMPONENTS_BLOCK == SDFR_MESH_BLOCK, "whole waves, and the scan's block");
static_assert(sizeof(Component) == 40 && offsetof(Component, points) == 8 && offsetof(Component, lo) == 16 && offsetof(Component, hi) == 28, "the tally's words");
static_assert(sizeof(ComponentCounts) == 64 && (1 + COMPONENT_COUNT_WORDS) * COMPONENT_WORD_STRIDE <= COMPONENT_RESULT_BYTES && sizeof(ComponentCounts) <= COMPONENT_WORD_STRIDE,
	"the packed counts lie before the words they are counted in");

struct AtomicMinExchange
{
	__device__ __forceinline__ uint32_t operator()(uint32_t *word, uint32_t value) const { return atomicMin(word, value); }
};

// lattice point x -> (i, j, k); x < 2^30
__device__ __forceinline__ void component_coords(const MeshGrid &g, uint32_t x, int &i, int &j, int &k)
{
	const uint32_t px = (uint32_t)(g.n[0] + 1), py = (uint32_t)(g.n[1] + 1);
	const uint32_t row = x / px;
	i = (int)(x - row * px);
	k = (int)(row / py);
	j = (int)(row - (uint32_t)k * py);
}

#if SDFR_COMPONENTS_BRICK
// One block per brick, one lane per point of it.  A lane past the lattice holds kind 2, which joins nothing, and writes nothing.
__global__ __launch_bounds__(COMPONENTS_BRICK_POINTS) void k_components_bricks(MeshGrid g, const float *__restrict__ lattice, uint32_t *__restrict__ parent)
{
	constexpr uint32_t B = SDFR_COMPONENTS_BRICK;
	static_assert(B * B * B == COMPONENTS_BRICK_POINTS, "a lane per point of the brick");
	__shared__ uint32_t local_parent[B * B * B];
	__shared__ uint8_t local_kind[B * B * B];
	const uint32_t px = (uint32_t)(g.n[0] + 1), py = (uint32_t)(g.n[1] + 1), pz = (uint32_t)(g.n[2] + 1);
	const uint32_t bx = (px + B - 1u) / B, by = (py + B - 1u) / B;
	const uint32_t brick_row = blockIdx.x / bx, brick_k = brick_row / by;
	const uint32_t i0 = (blockIdx.x - brick_row * bx) * B, j0 = (brick_row - brick_k * by) * B, k0 = brick_k * B;
	const uint32_t l = threadIdx.x, li = l % B, lj = (l / B) % B, lk = l / (B * B);
	const uint32_t i = i0 + li, j = j0 + lj, k = k0 + lk;
	const bool live = i < px && j < py && k < pz;
	const uint32_t x = i + px * (j + py * k); // (read only if live)
	const uint32_t kind = live ? component_kind(g, lattice[x]) : 2u;
	local_parent[l] = l;
	local_kind[l] = (uint8_t)kind;
	__syncthreads();
	if (live)
	{
		if (li + 1u < B && component_joined(kind, local_kind[l + 1u])) components_union(local_parent, l, l + 1u, AtomicMinExchange());
		if (lj + 1u < B && component_joined(kind, local_kind[l + B])) components_union(local_parent, l, l + B, AtomicMinExchange());
		if (lk + 1u < B && component_joined(kind, local_kind[l + B * B])) components_union(local_parent, l, l + B * B, AtomicMinExchange());
	}
	__syncthreads();
	if (!live) return;
	const uint32_t root = components_find(local_parent, l); // (every union of the brick is done: the chain ends at the piece's minimum)
	parent[x] = (i0 + root % B) + px * ((j0 + (root / B) % B) + py * (k0 + root / (B * B)));
}
#else
__global__ __launch_bounds__(COMPONENTS_BLOCK) void k_components_identity(uint32_t points, uint32_t *__restrict__ parent)
{
	const uint32_t x = blockIdx.x * (uint32_t)COMPONENTS_BLOCK + threadIdx.x;
	if (x < points) parent[x] = x;
}
#endif

// One lane per point: its edges to the next point along each axis, those that cross a brick's face (without the brick stage: all).
// The finds are the shortcut; the union acts on what its atomics return.
__global__ __launch_bounds__(COMPONENTS_BLOCK) void k_components_seams(MeshGrid g, const float *__restrict__ lattice, uint32_t *parent)
{
	const uint32_t x = blockIdx.x * (uint32_t)COMPONENTS_BLOCK + threadIdx.x;
	if (x >= mesh_point_count(g)) return;
	int c[3];
	component_coords(g, x, c[0], c[1], c[2]);
	const uint32_t px = (uint32_t)(g.n[0] + 1), py = (uint32_t)(g.n[1] + 1);
	const uint32_t step[3] = {1u, px, px * py};
	uint32_t kind = 3u; // (not read yet: most points have no seam edge)
	for (int a = 0; a < 3; ++a)
	{
		if (c[a] >= g.n[a]) continue;
#if SDFR_COMPONENTS_BRICK
		if (((uint32_t)c[a] % SDFR_COMPONENTS_BRICK) != SDFR_COMPONENTS_BRICK - 1u) continue;
#endif
		if (kind == 3u) kind = component_kind(g, lattice[x]);
		const uint32_t y = x + step[a];
		if (!component_joined(kind, component_kind(g, lattice[y]))) continue;
		components_union(parent, components_find(parent, x), components_find(parent, y), AtomicMinExchange());
	}
}

__global__ __launch_bounds__(COMPONENTS_BLOCK) void k_components_flatten(uint32_t points, uint32_t *parent)
{
	const uint32_t x = blockIdx.x * (uint32_t)COMPONENTS_BLOCK + threadIdx.x;
	if (x >= points) return;
	// (another lane may be writing a word of the chain: it holds a point of the set or, already, the root)
	parent[x] = components_find(parent, x);
}

// the root flags; the element after the last is the 0 whose prefix sum is the number of components
__global__ __launch_bounds__(COMPONENTS_BLOCK) void k_components_roots(uint32_t points, const uint32_t *__restrict__ parent, uint32_t *__restrict__ flags)
{
	const uint32_t x = blockIdx.x * (uint32_t)COMPONENTS_BLOCK + threadIdx.x;
	if (x > points) return;
	flags[x] = x < points && parent[x] == x ? 1u : 0u;
}

// label[x] = scan[root(x)], in place of parent[x] -- which this lane alone reads -- and into `labels` unless null; a root starts its record
__global__ __launch_bounds__(COMPONENTS_BLOCK) void k_components_number(MeshGrid g, const float *__restrict__ lattice, uint32_t *parent, const uint32_t *__restrict__ scan,
	uint32_t *__restrict__ labels, Component *__restrict__ table)
{
	const uint32_t x = blockIdx.x * (uint32_t)COMPONENTS_BLOCK + threadIdx.x;
	if (x >= mesh_point_count(g)) return;
	const uint32_t root = parent[x], label = scan[root];
	parent[x] = label;
	if (labels) labels[x] = label;
	if (root == x) table[label] = component_empty(g, x, component_kind(g, lattice[x]));
}

__device__ __forceinline__ int components_wave_min(int v)
{
	for (int d = 32; d >= 1; d >>= 1)
	{
		const int o = __shfl_xor(v, d, 64);
		v = o < v ? o : v;
	}
	return v;
}
__device__ __forceinline__ int components_wave_max(int v)
{
	for (int d = 32; d >= 1; d >>= 1)
	{
		const int o = __shfl_xor(v, d, 64);
		v = o > v ? o : v;
	}
	return v;
}
__device__ __forceinline__ uint32_t components_wave_or(uint32_t v)
{
	for (int d = 32; d >= 1; d >>= 1) v |= (uint32_t)__shfl_xor((int)v, d, 64);
	return v;
}
__device__ __forceinline__ long long components_wave_sum(long long v)
{
	for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
	return v;
}
__device__ __forceinline__ long long components_wave_max(long long v)
{
	for (int d = 32; d >= 1; d >>= 1)
	{
		const long long o = __shfl_xor(v, d, 64);
		v = o > v ? o : v;
	}
	return v;
}

// What a wave adds to one component's record, issued by one lane: the points by a 64-bit atomicAdd; a bound or a face bit only where it
// would move the word.  The words are read first through an agent-scope load (past the L1, which would go on serving the initial value): a
// bound only ever falls (lo) or rises (hi) and a flag bit is only ever set, so a stale word can make the lane issue an atomic it did not
// need, never skip one it needed.  A component's bounds and faces settle after its first few waves; what is left for the one record every
// wave of a large component adds to is the add.
__device__ __forceinline__ void component_tally(Component *c, uint32_t points, const int lo[3], const int hi[3], uint32_t faces)
{
	atomicAdd(reinterpret_cast<unsigned long long *>(&c->points), (unsigned long long)points);
	for (int a = 0; a < 3; ++a)
	{
		if (lo[a] < __hip_atomic_load(&c->lo[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&c->lo[a], lo[a]);
		if (hi[a] > __hip_atomic_load(&c->hi[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&c->hi[a], hi[a]);
	}
	if (faces & ~__hip_atomic_load(&c->flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&c->flags, faces);
}

// A wave tallies COMPONENTS_TALLY_RUNS runs of 64 consecutive points (no early return inside a run: every lane of the wave takes part in
// the ballots and the shuffles).  Per run the lanes are grouped by label -- one group in the common case, up to COMPONENTS_TALLY_GROUPS
// before the lanes left over issue their own atomics --, a group reduced in the wave to its popcount, bounds and face bits.  The wave keeps
// one group's sums in registers from run to run (all wave-uniform): a group of the same label is merged into them, a run of one other
// label replaces them, any other group is issued at once, by one lane; what is kept is issued at the end.  So the one record that most
// waves of a large component add to takes one add per wave, not eight atomics per run or per lane: 16 384 tiles queuing behind one word
// cost 170 us in the measure, and a lane per point of a 256^3 lattice's outside is a thousand times that.
__global__ __launch_bounds__(COMPONENTS_BLOCK) void k_components_tally(MeshGrid g, const uint32_t *__restrict__ label_of, Component *table)
{
	const uint32_t points = mesh_point_count(g), lane = threadIdx.x & 63u;
	const uint32_t wave = blockIdx.x * (uint32_t)(COMPONENTS_BLOCK / 64) + (threadIdx.x >> 6);
	const uint32_t base = wave * (uint32_t)COMPONENTS_TALLY_POINTS; // (< 2^30 + 2^14: the grid covers the points and no more)
	uint32_t kept_label = 0u, kept_points = 0u, kept_faces = 0u; // kept_points == 0: nothing kept
	int kept_lo[3] = {0, 0, 0}, kept_hi[3] = {0, 0, 0};
	for (uint32_t run = 0; run < (uint32_t)COMPONENTS_TALLY_RUNS; ++run)
	{
		const uint32_t first = base + run * 64u;
		if (first >= points) break; // (wave-uniform)
		const uint32_t x = first + lane;
		const bool live = x < points;
		int c[3] = {0, 0, 0};
		uint32_t label = 0u, faces = 0u;
		if (live)
		{
			component_coords(g, x, c[0], c[1], c[2]);
			label = label_of[x];
			faces = component_point_faces(g, c[0], c[1], c[2]);
		}
		const unsigned long long lives = __ballot(live);
		unsigned long long left = lives;
		for (int group = 0; group < COMPONENTS_TALLY_GROUPS && left; ++group)
		{
			const uint32_t of = (uint32_t)__shfl((int)label, __ffsll((long long)left) - 1, 64);
			const bool in = live && label == of;
			const unsigned long long members = __ballot(in) & left;
			int lo[3], hi[3];
			for (int a = 0; a < 3; ++a)
			{
				lo[a] = components_wave_min(in ? c[a] : g.n[a] + 1);
				hi[a] = components_wave_max(in ? c[a] : -1);
			}
			const uint32_t all_faces = components_wave_or(in ? faces : 0u), n = (uint32_t)__popcll(members);
			if (kept_points && kept_label == of)
			{
				kept_points += n;
				kept_faces |= all_faces;
				for (int a = 0; a < 3; ++a)
				{
					kept_lo[a] = lo[a] < kept_lo[a] ? lo[a] : kept_lo[a];
					kept_hi[a] = hi[a] > kept_hi[a] ? hi[a] : kept_hi[a];
				}
			}
			else if (!kept_points || members == lives)
			{
				if (kept_points && lane == 0u) component_tally(table + kept_label, kept_points, kept_lo, kept_hi, kept_faces);
				kept_label = of;
				kept_points = n;
				kept_faces = all_faces;
				for (int a = 0; a < 3; ++a)
				{
					kept_lo[a] = lo[a];
					kept_hi[a] = hi[a];
				}
			}
			else if (lane == 0u) component_tally(table + of, n, lo, hi, all_faces);
			left &= ~members;
		}
		if (live && ((left >> lane) & 1ull)) component_tally(table + label, 1u, c, c, faces); // more labels in the run than groups: a lane each
	}
	if (kept_points && lane == 0u) component_tally(table + kept_label, kept_points, kept_lo, kept_hi, kept_faces);
}

// word t of the counts while they are counted (t = 0 .. COMPONENT_COUNT_WORDS - 1: ComponentCounts after `components`)
__device__ __forceinline__ unsigned long long *component_word(void *result, int t)
{
	return reinterpret_cast<unsigned long long *>(static_cast<char *>(result) + (size_t)COMPONENT_WORD_STRIDE * (size_t)(1 + t));
}
__global__ __launch_bounds__(64) void k_components_init(void *result)
{
	if (blockIdx.x == 0 && threadIdx.x < COMPONENT_COUNT_WORDS) *component_word(result, (int)threadIdx.x) = 0ull;
}

// One lane per component: its record into `records` unless null, and what it adds to the counts
__global__ __launch_bounds__(COMPONENTS_BLOCK) void k_components_pack(uint32_t components, const Component *__restrict__ table, Component *__restrict__ records, void *result)
{
	const uint32_t n = blockIdx.x * (uint32_t)COMPONENTS_BLOCK + threadIdx.x;
	const bool live = n < components;
	Component c = {};
	if (live)
	{
		c = table[n];
		if (records) records[n] = c;
	}
	const bool solid = live && (c.flags & COMPONENT_INSIDE) != 0u, hollow = live && !solid, closed = (c.flags & COMPONENT_FACES) == 0u;
	long long words[COMPONENT_COUNT_WORDS];
	words[0] = __popcll(__ballot(solid));
	words[1] = __popcll(__ballot(hollow));
	words[2] = __popcll(__ballot(solid && closed));
	words[3] = __popcll(__ballot(hollow && closed));
	words[4] = components_wave_sum(solid ? (long long)c.points : 0ll);
	words[5] = components_wave_max(solid ? (long long)c.points : 0ll);
	words[6] = components_wave_max(hollow ? (long long)c.points : 0ll);
	if ((threadIdx.x & 63u) != 0u) return;
	for (int t = 0; t < COMPONENT_COUNT_WORDS; ++t)
	{
		if (!words[t]) continue;
		if (t < 5) atomicAdd(component_word(result, t), (unsigned long long)words[t]);
		else atomicMax(component_word(result, t), (unsigned long long)words[t]);
	}
}
__global__ __launch_bounds__(64) void k_components_finish(uint32_t components, void *result)
{
	if (blockIdx.x != 0) return;
	int64_t *out = static_cast<int64_t *>(result);
	if (threadIdx.x == 0) out[0] = (int64_t)components;
	else if (threadIdx.x <= COMPONENT_COUNT_WORDS) out[threadIdx.x] = (int64_t)*component_word(result, (int)threadIdx.x - 1);
}

hipError_t launch_components_union(const ComponentsPlan &p, const float *lattice, uint32_t *parent, uint32_t *scan, uint32_t *sums, hipStream_t stream)
{
	const uint32_t points = (uint32_t)p.points;
#if SDFR_COMPONENTS_BRICK
	hipLaunchKernelGGL(k_components_bricks, dim3(p.brick_blocks), dim3(COMPONENTS_BRICK_POINTS), 0, stream, p.g, lattice, parent);
#else
	hipLaunchKernelGGL(k_components_identity, dim3(p.point_blocks), dim3(COMPONENTS_BLOCK), 0, stream, points, parent);
#endif
	hipLaunchKernelGGL(k_components_seams, dim3(p.point_blocks), dim3(COMPONENTS_BLOCK), 0, stream, p.g, lattice, parent);
	hipLaunchKernelGGL(k_components_flatten, dim3(p.point_blocks), dim3(COMPONENTS_BLOCK), 0, stream, points, parent);
	hipLaunchKernelGGL(k_components_roots, dim3(p.root_blocks), dim3(COMPONENTS_BLOCK), 0, stream, points, (const uint32_t *)parent, scan);
	launch_mesh_scan(scan, points + 1u, sums, stream);
	return hipGetLastError();
}

hipError_t launch_components_tally(const ComponentsPlan &p, const ComponentsFill &f, const float *lattice, uint32_t *parent, const uint32_t *scan, uint32_t *labels,
	Component *table, Component *records, void *result, hipStream_t stream)
{
	const uint32_t components = (uint32_t)f.components;
	hipLaunchKernelGGL(k_components_init, dim3(1), dim3(64), 0, stream, result);
	hipLaunchKernelGGL(k_components_number, dim3(p.point_blocks), dim3(COMPONENTS_BLOCK), 0, stream, p.g, lattice, parent, scan, labels, table);
	hipLaunchKernelGGL(k_components_tally, dim3(p.tally_blocks), dim3(COMPONENTS_BLOCK), 0, stream, p.g, (const uint32_t *)parent, table);
	hipLaunchKernelGGL(k_components_pack, dim3(f.component_blocks), dim3(COMPONENTS_BLOCK), 0, stream, components, (const Component *)table, f.fill ? records : nullptr, result);
	hipLaunchKernelGGL(k_components_finish, dim3(1), dim3(64), 0, stream, components, result);
	return hipGetLastError();
}

} // namespace sdfr

// sdfr_mesh.hip -- the scene-independent kernels of sdfr_mesh_extract (stage functions: sdfr_mesh.h) and of the mesh's texture atlas
// (k_atlas_texels, at the end; sdfr_atlas.h): classify cells and lattice
// points, exclusive prefix sums of the two flag arrays, emit vertices, emit indices.  The distances they read come from the
// scene's lattice kernel (sdfr_query_kernel.h: query_lattice_kernel).  For sdfr_mesh_extract_sharp the vertex pass leaves each
// vertex's cell index instead (k_mesh_emit_cells), and the scene's sharp-vertex kernel makes the vertices (mesh_sharp_kernel).
//
// The prefix sum is the plain three-phase one -- per-block totals, their scan (the same three phases again while they are more
// than one block), then every block scans its own elements on top of its offset -- so no kernel ever waits for another workgroup:
// the phases are separate launches of one stream.  The output order (cells and lattice points by linear index) is the scan's.
#include "sdfr_kernels.h"
#include "sdfr_mesh.h"
#include "sdfr_mesh_survey.h"
#include "sdfr_measure.h"
#define SDFR_ATLAS_GEOMETRY_ONLY // the texel map alone: no scene is looked at here
#include "sdfr_atlas.h"

namespace sdfr {

static_assert(SDFR_MESH_BLOCK % 64 == 0 && SDFR_MESH_BLOCK <= 1024, "whole waves");

// exclusive prefix sum of `v` over the block's threads and the block's total: wave64 shuffles inside a wave, LDS across the waves
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t &total)
{
	__shared__ uint32_t wave_sum[SDFR_MESH_BLOCK / 64];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t incl = v;
	for (int d = 1; d < 64; d <<= 1)
	{
		const uint32_t up = __shfl_up(incl, d, 64);
		if (lane >= (uint32_t)d) incl += up;
	}
	if (lane == 63u) wave_sum[wave] = incl;
	__syncthreads();
	uint32_t before = 0u, all = 0u;
	for (uint32_t w = 0; w < SDFR_MESH_BLOCK / 64; ++w)
	{
		const uint32_t s = wave_sum[w];
		if (w < wave) before += s;
		all += s;
	}
	total = all;
	return before + incl - v;
}

// phase 1: sums[b] = total of block b's elements
__global__ __launch_bounds__(SDFR_MESH_BLOCK) void k_mesh_scan_reduce(const uint32_t *__restrict__ data, uint32_t n, uint32_t *__restrict__ sums)
{
	const uint32_t i = blockIdx.x * (uint32_t)SDFR_MESH_BLOCK + threadIdx.x;
	uint32_t total;
	(void)block_exclusive_scan(i < n ? data[i] : 0u, total);
	if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// phase 3 (offsets: the scanned block totals), and the whole scan of n <= SDFR_MESH_BLOCK elements (offsets null)
__global__ __launch_bounds__(SDFR_MESH_BLOCK) void k_mesh_scan_down(uint32_t *__restrict__ data, uint32_t n, const uint32_t *__restrict__ offsets)
{
	const uint32_t i = blockIdx.x * (uint32_t)SDFR_MESH_BLOCK + threadIdx.x;
	uint32_t total;
	const uint32_t ex = block_exclusive_scan(i < n ? data[i] : 0u, total);
	if (i < n) data[i] = ex + (offsets ? offsets[blockIdx.x] : 0u);
}

// data [n] -> its exclusive prefix sum, in place; sums: mesh_scan_sum_words(n) words (sdfr_mesh.h)
static void scan_exclusive(uint32_t *data, uint32_t n, uint32_t *sums, hipStream_t stream)
{
	if (n <= SDFR_MESH_BLOCK)
	{
		hipLaunchKernelGGL(k_mesh_scan_down, dim3(1), dim3(SDFR_MESH_BLOCK), 0, stream, data, n, (const uint32_t *)nullptr);
		return;
	}
	const uint32_t blocks = (n + SDFR_MESH_BLOCK - 1u) / SDFR_MESH_BLOCK;
	hipLaunchKernelGGL(k_mesh_scan_reduce, dim3(blocks), dim3(SDFR_MESH_BLOCK), 0, stream, (const uint32_t *)data, n, sums);
	scan_exclusive(sums, blocks, sums + blocks, stream);
	hipLaunchKernelGGL(k_mesh_scan_down, dim3(blocks), dim3(SDFR_MESH_BLOCK), 0, stream, data, n, (const uint32_t *)sums);
}

// lattice point p -> (i, j, k); p < 2^30
__device__ __forceinline__ void point_coords(const MeshGrid &g, uint32_t p, int &i, int &j, int &k)
{
	const uint32_t px = (uint32_t)(g.n[0] + 1), py = (uint32_t)(g.n[1] + 1);
	const uint32_t row = p / px;
	i = (int)(p - row * px);
	k = (int)(row / py);
	j = (int)(row - (uint32_t)k * py);
}

// one lane per lattice point: its quad count, and the vertex flag of the cell whose lowest corner it is; the element after the
// last of each array is the 0 whose prefix sum is the total
__global__ __launch_bounds__(SDFR_MESH_BLOCK) void k_mesh_classify(MeshGrid g, const float *__restrict__ lattice, uint32_t *__restrict__ cell_vertex,
	uint32_t *__restrict__ point_quad)
{
	const uint32_t p = blockIdx.x * (uint32_t)SDFR_MESH_BLOCK + threadIdx.x;
	const uint32_t points = mesh_point_count(g);
	if (p > points) return;
	if (p == points)
	{
		point_quad[points] = 0u;
		cell_vertex[mesh_cell_count(g)] = 0u;
		return;
	}
	int i, j, k;
	point_coords(g, p, i, j, k);
	point_quad[p] = mesh_point_quads(g, lattice, i, j, k);
	if (i < g.n[0] && j < g.n[1] && k < g.n[2]) cell_vertex[mesh_cell_index(g, i, j, k)] = mesh_cell_active(g, lattice, i, j, k);
}

// one lane per cell: an active cell (its scanned index differs from the next cell's) writes its vertex
__global__ __launch_bounds__(SDFR_MESH_BLOCK) void k_mesh_emit_vertices(MeshGrid g, const float *__restrict__ lattice, const uint32_t *__restrict__ cell_vertex,
	float *__restrict__ positions)
{
	const uint32_t c = blockIdx.x * (uint32_t)SDFR_MESH_BLOCK + threadIdx.x;
	if (c >= mesh_cell_count(g)) return;
	const uint32_t v = cell_vertex[c];
	if (cell_vertex[c + 1u] == v) return;
	const uint32_t nx = (uint32_t)g.n[0], ny = (uint32_t)g.n[1];
	const uint32_t row = c / nx, k = row / ny;
	float pos[3];
	mesh_cell_vertex(g, lattice, (int)(c - row * nx), (int)(row - k * ny), (int)k, pos);
	float *o = positions + (size_t)3 * v;
	o[0] = pos[0];
	o[1] = pos[1];
	o[2] = pos[2];
}

// one lane per cell, for the sharp vertices (sdfr_mesh_sharp.h): an active cell writes its own linear index (< 2^30) as the bits of its
// vertex's first word, where the scene's sharp-vertex kernel (sdfr_query_kernel.h: mesh_sharp_kernel) finds it and writes the vertex
__global__ __launch_bounds__(SDFR_MESH_BLOCK) void k_mesh_emit_cells(MeshGrid g, const uint32_t *__restrict__ cell_vertex, float *__restrict__ positions)
{
	const uint32_t c = blockIdx.x * (uint32_t)SDFR_MESH_BLOCK + threadIdx.x;
	if (c >= mesh_cell_count(g)) return;
	const uint32_t v = cell_vertex[c];
	if (cell_vertex[c + 1u] == v) return;
	positions[(size_t)3 * v] = bits_f32(c);
}

// one lane per lattice point: a point with quads writes their triangles
__global__ __launch_bounds__(SDFR_MESH_BLOCK) void k_mesh_emit_indices(MeshGrid g, const float *__restrict__ lattice, const uint32_t *__restrict__ cell_vertex,
	const uint32_t *__restrict__ point_quad, uint32_t *__restrict__ indices)
{
	const uint32_t p = blockIdx.x * (uint32_t)SDFR_MESH_BLOCK + threadIdx.x;
	if (p >= mesh_point_count(g)) return;
	const uint32_t q = point_quad[p];
	if (point_quad[p + 1u] == q) return;
	int i, j, k;
	point_coords(g, p, i, j, k);
	mesh_point_emit(g, lattice, cell_vertex, i, j, k, q, indices);
}

// the same prefix sum for the other extractions of this family (sdfr_slice.hip)
void launch_mesh_scan(uint32_t *data, uint32_t n, uint32_t *sums, hipStream_t stream) { scan_exclusive(data, n, sums, stream); }

hipError_t launch_mesh_count(const MeshGrid &g, const float *lattice, uint32_t *cell_vertex, uint32_t *point_quad, uint32_t *sums, hipStream_t stream)
{
	const uint32_t points = mesh_point_count(g), cells = mesh_cell_count(g);
	hipLaunchKernelGGL(k_mesh_classify, dim3(points / SDFR_MESH_BLOCK + 1u), dim3(SDFR_MESH_BLOCK), 0, stream, g, lattice, cell_vertex, point_quad);
	scan_exclusive(cell_vertex, cells + 1u, sums, stream);
	scan_exclusive(point_quad, points + 1u, sums + mesh_scan_sum_words((size_t)cells + 1), stream);
	return hipGetLastError();
}

hipError_t launch_mesh_emit(const MeshGrid &g, const float *lattice, const uint32_t *cell_vertex, const uint32_t *point_quad, float *positions,
	uint32_t *indices, bool cells_only, hipStream_t stream)
{
	const uint32_t points = mesh_point_count(g), cells = mesh_cell_count(g);
	if (cells_only)
		hipLaunchKernelGGL(k_mesh_emit_cells, dim3((cells + SDFR_MESH_BLOCK - 1u) / SDFR_MESH_BLOCK), dim3(SDFR_MESH_BLOCK), 0, stream, g, cell_vertex, positions);
	else
		hipLaunchKernelGGL(k_mesh_emit_vertices, dim3((cells + SDFR_MESH_BLOCK - 1u) / SDFR_MESH_BLOCK), dim3(SDFR_MESH_BLOCK), 0, stream, g, lattice, cell_vertex,
			positions);
	if (indices)
		hipLaunchKernelGGL(k_mesh_emit_indices, dim3((points + SDFR_MESH_BLOCK - 1u) / SDFR_MESH_BLOCK), dim3(SDFR_MESH_BLOCK), 0, stream, g, lattice,
			cell_vertex, point_quad, indices);
	return hipGetLastError();
}

// ---- what a lattice holds (sdfr_mesh_survey; the predicates: sdfr_mesh_survey.h) ----
// One lane per lattice point, as k_mesh_classify: the point's quads, its inside flag, and the cell whose lowest corner it is.  Every
// result is an integer.  A wave counts by ballot and popcount and takes the bounds of its cells by shuffles -- only a wave that holds a
// near cell, an active one: most hold none --; its first lane leaves the wave's 10 counts and 12 bounds in LDS; then lane t of the block
// adds up word t of the four waves and, if the block saw anything for that word, issues the one atomic: a 64-bit atomicAdd for a count,
// atomicMin / atomicMax on 32 bits for a bound (agent scope, HIP's default).  Integer atomics: the order of arrival changes nothing.
// While they are counted the 22 words lie MESH_SURVEY_WORD_STRIDE bytes apart, after the packed result they are gathered into at the
// end (k_mesh_survey_pack): packed into the result's one 128-byte line, the atomics of all words and all blocks queued up behind each
// other and the kernel took 2.5 times as long (profiles/mesh_survey_timing.txt).  k_mesh_survey_init sets them: lo = n, hi = -1.
static_assert(offsetof(MeshSurvey, quads) == 8 && offsetof(MeshSurvey, near_cells) == 16 && offsetof(MeshSurvey, inside_points) == 24 &&
		offsetof(MeshSurvey, active_lo) == 32 && offsetof(MeshSurvey, active_hi) == 44 && offsetof(MeshSurvey, near_lo) == 56 &&
		offsetof(MeshSurvey, near_hi) == 68 && offsetof(MeshSurvey, face_active) == 80 && sizeof(MeshSurvey) == 128,
	"the packed words: counts 0..3, bounds 0..11, counts 4..9");

// word t of the survey while it is counted: 0 .. 9 the counts (64 bits), 10 .. 21 the bounds (32 bits), each in a page of its own
// after the packed result at `out` (MESH_SURVEY_WORK_BYTES in all)
__device__ __forceinline__ char *survey_word(MeshSurvey *out, int t) { return reinterpret_cast<char *>(out) + (size_t)MESH_SURVEY_WORD_STRIDE * (size_t)(1 + t); }

__global__ void k_mesh_survey_init(MeshSurvey *__restrict__ out, MeshGrid g)
{
	const int t = (int)threadIdx.x;
	if (blockIdx.x != 0) return;
	if (t < MESH_SURVEY_COUNTS) *reinterpret_cast<int64_t *>(survey_word(out, t)) = 0;
	else if (t < MESH_SURVEY_COUNTS + MESH_SURVEY_BOUNDS)
	{
		const int b = t - MESH_SURVEY_COUNTS;
		*reinterpret_cast<int32_t *>(survey_word(out, t)) = (b / 3) % 2 == 0 ? g.n[b % 3] : -1;
	}
}
__global__ void k_mesh_survey_pack(MeshSurvey *__restrict__ out)
{
	const int t = (int)threadIdx.x;
	if (blockIdx.x != 0) return;
	if (t < MESH_SURVEY_COUNTS) *(t < 4 ? &out->active_cells + t : &out->face_active[t - 4]) = *reinterpret_cast<const int64_t *>(survey_word(out, t));
	else if (t < MESH_SURVEY_COUNTS + MESH_SURVEY_BOUNDS) out->active_lo[t - MESH_SURVEY_COUNTS] = *reinterpret_cast<const int32_t *>(survey_word(out, t));
}

__device__ __forceinline__ int wave_min(int v)
{
	for (int d = 32; d >= 1; d >>= 1)
	{
		const int o = __shfl_xor(v, d, 64);
		v = o < v ? o : v;
	}
	return v;
}
__device__ __forceinline__ int wave_max(int v)
{
	for (int d = 32; d >= 1; d >>= 1)
	{
		const int o = __shfl_xor(v, d, 64);
		v = o > v ? o : v;
	}
	return v;
}

__global__ __launch_bounds__(SDFR_MESH_BLOCK) void k_mesh_survey(MeshGrid g, const float *__restrict__ lattice, float band, MeshSurvey *__restrict__ out)
{
	constexpr int WAVES = SDFR_MESH_BLOCK / 64;
	__shared__ uint32_t wave_count[WAVES][MESH_SURVEY_COUNTS];
	__shared__ int32_t wave_bound[WAVES][MESH_SURVEY_BOUNDS];
	const uint32_t p = blockIdx.x * (uint32_t)SDFR_MESH_BLOCK + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	// (no early return: every lane of the block takes part in the ballots, the shuffles and the barrier)
	MeshSurveyPoint c = {};
	int cell[3] = {0, 0, 0};
	if (p < mesh_point_count(g))
	{
		point_coords(g, p, cell[0], cell[1], cell[2]);
		c = mesh_survey_point(g, lattice, band, cell[0], cell[1], cell[2]);
	}
	const unsigned long long active = __ballot(c.active != 0u), near = __ballot(c.near != 0u);
	uint32_t counts[MESH_SURVEY_COUNTS];
	counts[0] = (uint32_t)__popcll(active);
	counts[1] = (uint32_t)__popcll(__ballot((c.quads & 1u) != 0u)) + 2u * (uint32_t)__popcll(__ballot((c.quads & 2u) != 0u));
	counts[2] = (uint32_t)__popcll(near);
	counts[3] = (uint32_t)__popcll(__ballot(c.inside != 0u));
	for (int f = 0; f < 6; ++f) counts[4 + f] = active ? (uint32_t)__popcll(__ballot(((c.faces >> f) & 1u) != 0u)) : 0u;
	int32_t bounds[MESH_SURVEY_BOUNDS];
	for (int a = 0; a < 3; ++a)
	{
		// (wave-uniform branches: `active` and `near` are the whole wave's)
		bounds[a] = active ? wave_min(c.active ? cell[a] : g.n[a]) : g.n[a];
		bounds[3 + a] = active ? wave_max(c.active ? cell[a] : -1) : -1;
		bounds[6 + a] = near ? wave_min(c.near ? cell[a] : g.n[a]) : g.n[a];
		bounds[9 + a] = near ? wave_max(c.near ? cell[a] : -1) : -1;
	}
	if (lane == 0u)
	{
		for (int t = 0; t < MESH_SURVEY_COUNTS; ++t) wave_count[wave][t] = counts[t];
		for (int t = 0; t < MESH_SURVEY_BOUNDS; ++t) wave_bound[wave][t] = bounds[t];
	}
	__syncthreads();
	const int t = (int)threadIdx.x;
	if (t < MESH_SURVEY_COUNTS)
	{
		uint32_t sum = 0u;
		for (int w = 0; w < WAVES; ++w) sum += wave_count[w][t];
		if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(survey_word(out, t)), (unsigned long long)sum);
	}
	else if (t < MESH_SURVEY_COUNTS + MESH_SURVEY_BOUNDS)
	{
		const int b = t - MESH_SURVEY_COUNTS, a = b % 3;
		const bool is_min = (b / 3) % 2 == 0;
		int32_t v = wave_bound[0][b];
		for (int w = 1; w < WAVES; ++w)
		{
			const int32_t o = wave_bound[w][b];
			v = (is_min ? o < v : o > v) ? o : v;
		}
		int32_t *word = reinterpret_cast<int32_t *>(survey_word(out, t));
		// (reading the word first, to send only a bound that would move it, was measured with the packed words and was slower: every
		// block then reads the result, also those that saw nothing -- profiles/mesh_survey_timing.txt)
		if (is_min ? v < g.n[a] : v >= 0) is_min ? atomicMin(word, v) : atomicMax(word, v);
	}
}

hipError_t launch_mesh_survey(const MeshGrid &g, const float *lattice, float band, MeshSurvey *out, hipStream_t stream)
{
	const uint32_t points = mesh_point_count(g);
	hipLaunchKernelGGL(k_mesh_survey_init, dim3(1), dim3(64), 0, stream, out, g);
	hipLaunchKernelGGL(k_mesh_survey, dim3((points + SDFR_MESH_BLOCK - 1u) / SDFR_MESH_BLOCK), dim3(SDFR_MESH_BLOCK), 0, stream, g, lattice, band, out);
	hipLaunchKernelGGL(k_mesh_survey_pack, dim3(1), dim3(64), 0, stream, out);
	return hipGetLastError();
}

// ---- the tiles of a measure, reduced (sdfr_measure; the definition and its host restatement: sdfr_measure.h) ----
// k_measure_reduce: one wave per block turns a run of 64 consecutive records of one component (blockIdx.y) into one, by the six
// xor-butterflies of the scene's measure kernel -- the pairwise tree x[m] = x[2m] + x[2m + 1], whichever lane is asked --, the lanes past
// the last record carrying +0.0.  Launched in passes that ping-pong between two buffers until one record is left: the order of the sum is
// the launches', never the arrival's.  k_measure_init sets the tally's words before the scene's kernel counts into them with integer
// atomics (hit_lo = n, hit_hi = -1, the keys of +inf and -inf), sixteen copies of each; k_measure_pack gathers them and the last record
// into the result.
static_assert(sizeof(MeasureResult) == 160 && offsetof(MeasureResult, columns_hit) == 80 && offsetof(MeasureResult, steps) == 112 && offsetof(MeasureResult, hit_lo) == 136 &&
		offsetof(MeasureResult, t_lo) == 152 && sizeof(MeasureResult) <= MEASURE_TALLY_STRIDE * MEASURE_TALLY_FIRST, "the packed result lies before the tally's words");
static_assert((MEASURE_TALLY_COPIES & (MEASURE_TALLY_COPIES - 1)) == 0 && MEASURE_TALLY_WORDS * MEASURE_TALLY_COPIES <= 256 &&
		MEASURE_TALLY_BYTES == MEASURE_TALLY_STRIDE * (MEASURE_TALLY_FIRST + MEASURE_TALLY_WORDS * MEASURE_TALLY_COPIES), "a thread per copy of a word in k_measure_init");
// copy k of word t
__device__ __forceinline__ char *measure_word(void *tally, int t, int k)
{
	return static_cast<char *>(tally) + (size_t)MEASURE_TALLY_STRIDE * (size_t)(MEASURE_TALLY_FIRST + MEASURE_TALLY_COPIES * t + k);
}

__global__ __launch_bounds__(256) void k_measure_init(void *tally, int32_t nu, int32_t nv)
{
	const int t = (int)threadIdx.x / MEASURE_TALLY_COPIES, k = (int)threadIdx.x % MEASURE_TALLY_COPIES;
	if (blockIdx.x != 0) return;
	if (t < MEASURE_TALLY_COUNTS) *reinterpret_cast<int64_t *>(measure_word(tally, t, k)) = 0;
	else if (t < 11) *reinterpret_cast<int32_t *>(measure_word(tally, t, k)) = t == 7 ? nu : t == 8 ? nv : -1;
	else if (t < MEASURE_TALLY_WORDS) *reinterpret_cast<uint32_t *>(measure_word(tally, t, k)) = measure_order_key(measure_inf(t == 12));
}
__global__ __launch_bounds__(64) void k_measure_pack(void *tally, const double *__restrict__ record)
{
	const int t = (int)threadIdx.x;
	if (blockIdx.x != 0) return;
	MeasureResult *out = static_cast<MeasureResult *>(tally);
	if (t < MEASURE_TALLY_COUNTS)
	{
		int64_t sum = 0;
		for (int k = 0; k < MEASURE_TALLY_COPIES; ++k) sum += *reinterpret_cast<const int64_t *>(measure_word(tally, t, k));
		(&out->columns_hit)[t] = sum;
	}
	else if (t < 11)
	{
		int32_t v = *reinterpret_cast<const int32_t *>(measure_word(tally, t, 0));
		for (int k = 1; k < MEASURE_TALLY_COPIES; ++k)
		{
			const int32_t o = *reinterpret_cast<const int32_t *>(measure_word(tally, t, k));
			v = (t < 9 ? o < v : o > v) ? o : v;
		}
		out->hit_lo[t - 7] = v; // (hit_hi follows hit_lo)
	}
	else if (t < MEASURE_TALLY_WORDS)
	{
		uint32_t v = *reinterpret_cast<const uint32_t *>(measure_word(tally, t, 0));
		for (int k = 1; k < MEASURE_TALLY_COPIES; ++k)
		{
			const uint32_t o = *reinterpret_cast<const uint32_t *>(measure_word(tally, t, k));
			v = (t == 11 ? o < v : o > v) ? o : v;
		}
		(&out->t_lo)[t - 11] = measure_order_value(v);
	}
	else if (t < MEASURE_TALLY_WORDS + MEASURE_MOMENTS) out->moments[t - MEASURE_TALLY_WORDS] = record[t - MEASURE_TALLY_WORDS];
}
__global__ __launch_bounds__(64) void k_measure_reduce(const double *__restrict__ in, uint32_t n, double *__restrict__ out)
{
	const uint32_t run = blockIdx.x, c = blockIdx.y, i = run * (uint32_t)MEASURE_RUN + threadIdx.x;
	// (no early return: every lane takes part in the shuffles)
	double v = i < n ? in[(size_t)i * MEASURE_MOMENTS + c] : 0.0;
	for (int d = 1; d < 64; d <<= 1) v = v + __shfl_xor(v, d, 64);
	if (threadIdx.x == 0) out[(size_t)run * MEASURE_MOMENTS + c] = v;
}

hipError_t launch_measure_init(void *tally, int32_t nu, int32_t nv, hipStream_t stream)
{
	hipLaunchKernelGGL(k_measure_init, dim3(1), dim3(256), 0, stream, tally, nu, nv);
	return hipGetLastError();
}
hipError_t launch_measure_reduce(double *const partials[2], const uint32_t *pass_records, int passes, void *tally, hipStream_t stream)
{
	for (int k = 0; k < passes; ++k)
	{
		const uint32_t n = pass_records[k], runs = (n + (uint32_t)MEASURE_RUN - 1u) / (uint32_t)MEASURE_RUN;
		hipLaunchKernelGGL(k_measure_reduce, dim3(runs, MEASURE_MOMENTS), dim3(64), 0, stream, partials[k % 2], n, partials[(k + 1) % 2]);
	}
	hipLaunchKernelGGL(k_measure_pack, dim3(1), dim3(64), 0, stream, tally, partials[passes % 2]);
	return hipGetLastError();
}

// ---- the texels of a mesh's texture atlas (sdfr_atlas_texels; the map: sdfr_atlas.h) ----
// One wave per block and one texel per lane, an 8 x 8 square of the image per wave as in the bake kernel (sdfr_query_kernel.h): the
// quad of a tile of 8 texels and more is addressed by the block index alone and read once for the wave.  Every texel of the image is
// written: state 1 with its point and unit normal, 0 (degenerate) or -1 (no well-formed quad) with zeros.  With the planes of a bake
// instead of the two texel arrays (a bake of a mesh without quads, which needs no scene): -1 and zeros.
__global__ __launch_bounds__(64) void k_atlas_texels(AtlasArgs g)
{
	const uint32_t lane = threadIdx.x;
	const uint32_t blocks_x = (uint32_t)g.width >> 3;
	const uint32_t by = blockIdx.x / blocks_x, bx = blockIdx.x - by * blocks_x;
	const uint32_t x = bx * 8u + (lane & 7u), y = by * 8u + (lane >> 3);
	if (x >= (uint32_t)g.width || y >= (uint32_t)g.height) return; // (never: both are multiples of 8 and the grid covers them exactly)
	const uint32_t T = 1u << g.tile_log2;
	AtlasQuad Q;
	if (g.tile_log2 >= 3) Q = atlas_load_quad(g, atlas_tile_of(g, bx * 8u, by * 8u)); // wave-uniform
	else Q = atlas_load_quad(g, atlas_tile_of(g, x, y));
	vec3 P, N;
	const int state = atlas_texel(Q, x & (T - 1u), y & (T - 1u), T, P, N);
	const size_t i = (size_t)y * (uint32_t)g.width + x;
	g.valid[i] = state;
	if (g.texel_positions)
	{
		float *p = g.texel_positions + 3 * i, *n = g.texel_normals + 3 * i;
		p[0] = P.x;
		p[1] = P.y;
		p[2] = P.z;
		n[0] = N.x;
		n[1] = N.y;
		n[2] = N.z;
	}
	for (float *plane : {g.albedo, g.normal, g.lit})
		if (plane)
		{
			float *o = plane + 4 * i;
			o[0] = o[1] = o[2] = o[3] = 0.f;
		}
}

hipError_t launch_atlas_texels(const AtlasArgs &g, uint32_t blocks, hipStream_t stream)
{
	hipLaunchKernelGGL(k_atlas_texels, dim3(blocks), dim3(64), 0, stream, g);
	return hipGetLastError();
}

} // namespace sdfr

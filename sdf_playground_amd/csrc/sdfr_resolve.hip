// sdfr_resolve.hip -- the resolve kernel of sdfr_render_aa (stage functions: sdfr_resolve.h): one launch per pass
// turns the pass's compact strips of the supersampled frame S into the rows of the image they cover, all pyramid levels at once.
//
// One lane per sub-sample column of a strip.  A lane loads its column's 8 rows as eight 16-byte loads -- a wave reads 1 KiB of
// each row, contiguous, and every load is issued before the first add -- and keeps them in registers.  Per level the horizontal
// partner is the lane whose column differs in that level's bit, reached through a DPP move (K <= 8: never further than 4 lanes),
// the vertical partner is the lane's own next row.  After log2 K levels the K lanes of a group hold the same 8 / K pixels; the
// first of them stores.  No LDS, no atomics; the kernel is bound by its 16 * K^2 bytes read per pixel written.
#include "sdfr_kernels.h"
#include "sdfr_resolve.h"

namespace sdfr {

#define SDFR_RESOLVE_BLOCK 256 // lanes = sub-sample columns of a block; whole waves, so a group of K lanes never straddles two
static_assert(SDFR_RESOLVE_BLOCK % 64 == 0, "whole waves");

// the value the lane whose index differs in bit log2(M) holds.  M = 1, 2: a quad permutation.  M = 4: the lanes of a group of four
// hold the same value by then, so ANY lane of the other four of the eight will do: the mirror of the half row (lane i <-> 7 - i).
template <int M>
__device__ __forceinline__ float lane_partner(float v)
{
	constexpr int ctrl = M == 1 ? 0xB1 /* quad_perm [1,0,3,2] */ : M == 2 ? 0x4E /* quad_perm [2,3,0,1] */ : 0x141 /* row_half_mirror */;
	return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xf, 0xf, false));
}
template <int M>
__device__ __forceinline__ uint32_t lane_partner(uint32_t v)
{
	constexpr int ctrl = M == 1 ? 0xB1 : M == 2 ? 0x4E : 0x141;
	return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, 0xf, 0xf, false);
}
template <int M>
__device__ __forceinline__ vec4 lane_partner(const vec4 &v)
{
	return V4(lane_partner<M>(v.x), lane_partner<M>(v.y), lane_partner<M>(v.z), lane_partner<M>(v.w));
}

// one level of the pyramid over the lane's rows: ROWS rows in, ROWS / 2 out
template <int M, int ROWS>
__device__ __forceinline__ void resolve_level(vec4 (&row)[8], bool right)
{
#pragma unroll
	for (int r = 0; r < ROWS; r += 2)
	{
		const vec4 p0 = lane_partner<M>(row[r]), p1 = lane_partner<M>(row[r + 1]);
		// both lanes of a pair add left + right, in that order
		const vec4 top = right ? aa_pair(p0, row[r]) : aa_pair(row[r], p0);
		const vec4 bottom = right ? aa_pair(p1, row[r + 1]) : aa_pair(row[r + 1], p1);
		row[r / 2] = aa_rows(top, bottom);
	}
}

template <int LOG2K>
__global__ __launch_bounds__(SDFR_RESOLVE_BLOCK) void k_resolve(ResolveArgs A)
{
	constexpr int K = 1 << LOG2K, OUT_ROWS = 8 >> LOG2K;
	// the frame's counters: this pass's are added by one lane of the launch (stream order: its render launch has ended)
	if (blockIdx.x == 0 && threadIdx.x == 0)
	{
		RenderTotals t = *A.pass_totals;
		if (!A.first_pass)
		{
			const RenderTotals f = *A.frame_totals;
			t.pixels += f.pixels;
			t.rays += f.rays;
			t.march_evals += f.march_evals;
			t.hits += f.hits;
		}
		*A.frame_totals = t;
	}
	// the grid is one-dimensional (a tall frame has more strips than a grid has rows): blocks_x blocks per strip
	const uint32_t ls = blockIdx.x / A.blocks_x;                                                             // strip of the compact buffer
	const uint32_t x = (blockIdx.x - ls * A.blocks_x) * (uint32_t)SDFR_RESOLVE_BLOCK + threadIdx.x; // column of S
	// (lanes past the row leave in whole groups of K: K divides s_width, and no lane that stays reads from one that left)
	if (x >= (uint32_t)A.s_width) return;
	const int row0 = (int)(strip_local_to_global(A.rm, ls) * (uint32_t)OUT_ROWS); // first row of the image this strip covers
	// rows of the image this strip has: a strip of S cut short by the frame's end has fewer, and its rows past the frame are not read
	const int out_rows = A.height - row0 < OUT_ROWS ? A.height - row0 : OUT_ROWS;
	if (out_rows <= 0) return;
	const size_t first = (size_t)ls * 8u * (size_t)A.s_width + x; // the lane's sub-sample of the strip's row 0

	vec4 row[8];
	const float4 *src = reinterpret_cast<const float4 *>(A.color) + first;
#pragma unroll
	for (int r = 0; r < 8; ++r)
	{
		float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
		if ((r >> LOG2K) < out_rows) v = src[(size_t)r * (size_t)A.s_width];
		row[r] = V4(v.x, v.y, v.z, v.w);
	}
	AaCounters cnt[OUT_ROWS] = {};
	if (A.stats)
	{
		// the counters need no order: each lane sums the K rows of an image row first, the lanes of a group then add up
		const uint32_t *st = A.stats + 3u * first;
#pragma unroll
		for (int o = 0; o < OUT_ROWS; ++o)
		{
			AaCounters s = {0u, 0u, 0u};
#pragma unroll
			for (int k = 0; k < K; ++k)
				if (o < out_rows)
				{
					const uint32_t *p = st + 3u * (size_t)(o * K + k) * (size_t)A.s_width;
					const AaCounters c = {p[0], p[1], p[2]};
					s = aa_add(s, c);
				}
			cnt[o] = s;
		}
	}

	if (LOG2K >= 1) resolve_level<1, 8>(row, (x & 1u) != 0u);
	if (LOG2K >= 2) resolve_level<2, 4>(row, (x & 2u) != 0u);
	if (LOG2K >= 3) resolve_level<4, 2>(row, (x & 4u) != 0u);
	if (A.stats)
	{
#pragma unroll
		for (int o = 0; o < OUT_ROWS; ++o)
		{
			AaCounters s = cnt[o];
			if (LOG2K >= 1) s = aa_add(s, AaCounters{lane_partner<1>(s.rays), lane_partner<1>(s.evals), lane_partner<1>(s.hits)});
			if (LOG2K >= 2) s = aa_add(s, AaCounters{lane_partner<2>(s.rays), lane_partner<2>(s.evals), lane_partner<2>(s.hits)});
			if (LOG2K >= 3) s = aa_add(s, AaCounters{lane_partner<4>(s.rays), lane_partner<4>(s.evals), lane_partner<4>(s.hits)});
			cnt[o] = s;
		}
	}

	if ((x & (uint32_t)(K - 1)) != 0u) return; // one lane in K stores
	const uint32_t ox = x >> LOG2K;
#pragma unroll
	for (int o = 0; o < OUT_ROWS; ++o)
	{
		if (o >= out_rows) break;
		const size_t pix = (size_t)(row0 + o) * (size_t)A.width + ox;
		const vec4 c = row[o];
		if (A.format == FORMAT_RGBA32F)
			reinterpret_cast<float4 *>(A.out)[pix] = make_float4(c.x, c.y, c.z, c.w);
		else
		{
			uint2 h;
			aa_half_pixel(c, h.x, h.y);
			reinterpret_cast<uint2 *>(A.out)[pix] = h;
		}
		if (A.stats)
		{
			uint32_t *p = A.out_stats + 3u * pix;
			p[0] = cnt[o].rays;
			p[1] = cnt[o].evals;
			p[2] = cnt[o].hits;
		}
	}
}

// a.local_strips >= 1 strips of a.s_width >= 1 columns; a.factor_log2 0 .. 3
hipError_t launch_resolve(ResolveArgs a, hipStream_t stream)
{
	a.blocks_x = ((uint32_t)a.s_width + SDFR_RESOLVE_BLOCK - 1u) / SDFR_RESOLVE_BLOCK;
	// (S has at most 2^30 pixels, a pass at most 2^28: the block count fits a grid's first dimension)
	const dim3 grid(a.blocks_x * a.local_strips), block(SDFR_RESOLVE_BLOCK);
	switch (a.factor_log2)
	{
	case 0: hipLaunchKernelGGL(k_resolve<0>, grid, block, 0, stream, a); break;
	case 1: hipLaunchKernelGGL(k_resolve<1>, grid, block, 0, stream, a); break;
	case 2: hipLaunchKernelGGL(k_resolve<2>, grid, block, 0, stream, a); break;
	case 3: hipLaunchKernelGGL(k_resolve<3>, grid, block, 0, stream, a); break;
	default: return hipErrorInvalidValue;
	}
	return hipGetLastError();
}

} // namespace sdfr

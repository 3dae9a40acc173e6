// sdfr_resolve.h -- the resolve of sdfr_render_aa (include/sdfr.h, where the definition stands in full): the
// arithmetic of box2, the half conversion and the counter sums as functions of a few values, host-compilable.  sdfr_resolve.hip runs
// them one lane per sub-sample column of a strip; tests/cpp/resolve_host.cpp runs the same text sequentially on the CPU.  All
// arithmetic is fp32 in source order (-ffp-contract=off), so both give the same bits.
//
// box2(A)[y][x] = ((A[2y][2x] + A[2y][2x+1]) + (A[2y+1][2x] + A[2y+1][2x+1])) * 0.25f.  The kernel makes the two inner sums with the
// neighbouring lane (aa_pair: left + right, in that order on both lanes) and the outer one from its own registers (aa_rows).
#pragma once
#include "sdfr_frame.h"

namespace sdfr {

// one row's share of box2: the left sample plus the right one
SDF_HD vec4 aa_pair(const vec4 &left, const vec4 &right) { return V4(left.x + right.x, left.y + right.y, left.z + right.z, left.w + right.w); }
// the upper row's share plus the lower row's, times a quarter
SDF_HD vec4 aa_rows(const vec4 &top, const vec4 &bottom)
{
	return V4((top.x + bottom.x) * 0.25f, (top.y + bottom.y) * 0.25f, (top.z + bottom.z) * 0.25f, (top.w + bottom.w) * 0.25f);
}
SDF_HD vec4 aa_box2(const vec4 &a00, const vec4 &a01, const vec4 &a10, const vec4 &a11) { return aa_rows(aa_pair(a00, a01), aa_pair(a10, a11)); }

// fp32 -> the bits of the nearest half, ties to even: what a direct SDFR_RGBA16F render stores (store_pixel, sdfr_pixel_kernel.h).
// On the device this is the conversion instruction; a host compiler without a half type gets the same rounding spelt out.
SDF_HD uint32_t aa_half_bits(float f)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __builtin_bit_cast(unsigned short, (_Float16)f);
#else
	const uint32_t u = f32_bits(f), sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
	if (a > 0x7f800000u) return sign | 0x7e00u | ((a >> 13) & 0x3ffu); // NaN: quiet, the payload's upper bits kept
	if (a >= 0x477ff000u) return sign | 0x7c00u;                        // infinity, and what rounds to it (>= 65520)
	if (a < 0x33000001u) return sign;                                   // <= 2^-25 rounds to zero
	// the 24-bit significand in units of the half's last place: normal halves keep 11 bits, subnormal ones what lies above 2^-24
	const uint32_t exponent = a >> 23, significand = (a & 0x7fffffu) | 0x800000u;
	const uint32_t shift = exponent >= 113u ? 13u : 126u - exponent;
	uint32_t q = significand >> shift;
	const uint32_t rest = significand & ((1u << shift) - 1u), tie = 1u << (shift - 1u);
	if (rest > tie || (rest == tie && (q & 1u))) ++q;
	// (a normal half's q carries its hidden bit: adding the exponent field below it accounts for it, and for a carry out of the rounding)
	return sign | (exponent >= 113u ? ((exponent - 113u) << 10) + q : q);
#endif
}
// an RGBA16F pixel as two words
SDF_HD void aa_half_pixel(const vec4 &c, uint32_t &lo, uint32_t &hi)
{
	lo = aa_half_bits(c.x) | (aa_half_bits(c.y) << 16);
	hi = aa_half_bits(c.z) | (aa_half_bits(c.w) << 16);
}

// {rays, march evaluations, hits} of one sub-sample, and their sums
struct AaCounters { uint32_t rays, evals, hits; };
SDF_HD AaCounters aa_add(const AaCounters &a, const AaCounters &b)
{
	AaCounters r;
	r.rays = a.rays + b.rays;
	r.evals = a.evals + b.evals;
	r.hits = a.hits + b.hits;
	return r;
}

// One resolve launch: the compact buffers of pass rm.rank of rm.world passes -> the rows of the image that pass's strips cover.
struct ResolveArgs
{
	const float *color;     // [rm.local_rows][s_width] RGBA32F
	const uint32_t *stats;  // [rm.local_rows][s_width][3], or null
	void *out;              // [height][width] RGBA32F / RGBA16F
	uint32_t *out_stats;    // [height][width][3], or null
	RowMap rm;              // the pass's row map: strip_local_to_global
	int s_width;            // K * width
	int width, height;      // of the image
	int factor_log2;
	int format;             // FORMAT_RGBA32F or FORMAT_RGBA16F
	uint32_t local_strips;  // strips of the pass that lie inside S
	uint32_t blocks_x;      // blocks per strip (set by the launcher)
	// the counters of this pass's render launch are added to the frame's (set by the first pass)
	const RenderTotals *pass_totals;
	RenderTotals *frame_totals;
	int first_pass;
};

} // namespace sdfr

// sdfr_aa_plan.h -- how sdfr_render_aa (include/sdfr.h) cuts the supersampled frame S (K * W x K * H) into passes.
// Plain host arithmetic over sdfr_launch_plan.h: no HIP call, no environment -- the entry point reads the byte budget
// (SDFR_AA_BUDGET_BYTES) and passes it in as a value, so the plan can be checked on a machine without a GPU (tests/test_aa_cpu.py).
//
// A pass is a RENDER_STRIPS launch of S with world = passes, rank = pass, no strip split: pass p renders the strips p, p + passes,
// p + 2 * passes ... of S into one compact buffer.  K divides SDFR_STRIP_ROWS, so the 8 rows of a strip of S are 8 / K complete rows
// of the image: strip g of S is the image's rows g * 8 / K ... (g + 1) * 8 / K - 1, cut at H when K * H is no multiple of 8.
#pragma once
#include "sdfr_launch_plan.h"

namespace sdfr {

enum { SDFR_AA_MAX_FACTOR = SDFR_STRIP_ROWS };
static const unsigned long long SDFR_AA_DEFAULT_BUDGET = 1ull << 30; // bytes of one pass's compact colour buffer: the best of the three measured
// most pixels a pass may hold whatever the budget says: the pixel kernel indexes a launch's pending rays with 32 bits
// (ensure_workspace: pixels * SDFR_MAX_RAYS < 2^32)
static const unsigned long long SDFR_AA_MAX_PASS_PIXELS = 1ull << 28;

// log2 of a factor of {1, 2, 4, 8}; -1: not one of them
inline int aa_factor_log2(int factor) { return factor == 1 ? 0 : factor == 2 ? 1 : factor == 4 ? 2 : factor == 8 ? 3 : -1; }

struct AaPlan
{
	int factor, factor_log2;
	int s_width, s_height;    // S: K * W x K * H
	int rows_per_strip;       // image rows a whole strip of S resolves to: 8 / K
	uint32_t strips;          // strips of S
	uint32_t passes;          // P
	uint32_t strips_per_pass; // strips the compact buffer holds: ceil(strips / P); the last passes may fill one fewer
	size_t pass_pixels;       // pixels of the compact buffer (whole strips)
};

// width, height >= 1, factor one of 1, 2, 4, 8, K^2 * W * H <= 2^30 (the caller checks).  P is the smallest count for which one pass's
// compact RGBA32F buffer -- ceil(strips / P) strips of 8 * K * W pixels of 16 bytes -- fits budget_bytes, with at least one strip per pass.
inline AaPlan plan_aa(int width, int height, int factor, unsigned long long budget_bytes)
{
	AaPlan p;
	p.factor = factor;
	p.factor_log2 = aa_factor_log2(factor);
	p.s_width = width * factor;
	p.s_height = height * factor;
	p.rows_per_strip = SDFR_STRIP_ROWS / factor;
	p.strips = (uint32_t)(((int64_t)p.s_height + SDFR_STRIP_ROWS - 1) / SDFR_STRIP_ROWS);
	const unsigned long long strip_pixels = (unsigned long long)SDFR_STRIP_ROWS * (unsigned long long)p.s_width;
	unsigned long long fit = budget_bytes / (strip_pixels * 16ull); // strips of S the budget holds
	const unsigned long long cap = SDFR_AA_MAX_PASS_PIXELS / strip_pixels;
	if (fit > cap) fit = cap;
	if (fit < 1ull) fit = 1ull;
	p.passes = (uint32_t)((p.strips + fit - 1ull) / fit);
	p.strips_per_pass = (p.strips + p.passes - 1u) / p.passes;
	p.pass_pixels = (size_t)strip_buffer_pixels(p.s_width, p.s_height, (int)p.passes, 0, 1); // = strips_per_pass * 8 * s_width
	return p;
}

// the row map of pass `pass` as the launchers and the resolve kernel see it (strip_local_to_global: local strip -> strip of S)
inline RowMap aa_pass_row_map(const AaPlan &p, uint32_t pass, int tile_w_log2)
{
	return frame_rows(RENDER_STRIPS, p.s_width, p.s_height, (int)pass, (int)p.passes, tile_w_log2, 0, 1).rm;
}
// strips of S that pass `pass` renders: its local strips 0 .. n - 1 exist, the compact buffer's later ones lie past the frame
inline uint32_t aa_pass_strips(const AaPlan &p, uint32_t pass) { return pass < p.strips ? (p.strips - pass + p.passes - 1u) / p.passes : 0u; }
// local strip `ls` of pass `pass` -> the image rows [row0, row0 + rows) it resolves to; rows = 0: the strip lies past the frame
inline void aa_strip_rows(const AaPlan &p, int height, uint32_t pass, uint32_t ls, int &row0, int &rows)
{
	const long long first = ((long long)ls * p.passes + pass) * p.rows_per_strip;
	row0 = first < height ? (int)first : height;
	rows = first >= height ? 0 : first + p.rows_per_strip <= height ? p.rows_per_strip : (int)(height - first);
}

} // namespace sdfr

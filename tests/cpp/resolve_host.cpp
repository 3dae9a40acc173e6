// tests/cpp/resolve_host.cpp -- TEST-ONLY: the stage functions of sdfr_render_aa's resolve (sdf_playground_amd/csrc/sdfr_resolve.h) and
// its pass planner (sdfr_aa_plan.h) compiled for the CPU.  rh_resolve runs the stage functions sequentially over one pass's compact
// strip buffer, the way sdfr_resolve.hip runs them one lane per sub-sample column, so that the CPU test tier can compare them with the
// definition restated in numpy (tests/aa_util.py) bit for bit without a GPU.  Built with -ffp-contract=off, as the library.  The
// product never loads this.
#include "sdfr_aa_plan.h"
#include "sdfr_resolve.h"

using namespace sdfr;

namespace {

struct Strip
{
	const float *color;    // the strip's 8 rows of the compact buffer
	const uint32_t *stats; // or null
	int s_width;
};
// pixel (y, x) of level `level` of the pyramid over a strip: level 0 is S, level l is box2 of level l - 1
vec4 pyramid(const Strip &s, int level, int y, int x)
{
	if (level == 0)
	{
		const float *p = s.color + 4 * ((size_t)y * s.s_width + x);
		return V4(p[0], p[1], p[2], p[3]);
	}
	return aa_box2(pyramid(s, level - 1, 2 * y, 2 * x), pyramid(s, level - 1, 2 * y, 2 * x + 1), pyramid(s, level - 1, 2 * y + 1, 2 * x),
		pyramid(s, level - 1, 2 * y + 1, 2 * x + 1));
}

} // namespace

extern "C" {

// out[0..7]: factor_log2, s_width, s_height, rows_per_strip, strips, passes, strips_per_pass, pass_pixels
void rh_plan(int width, int height, int factor, unsigned long long budget, long long *out)
{
	const AaPlan p = plan_aa(width, height, factor, budget);
	const long long v[8] = {p.factor_log2, p.s_width, p.s_height, p.rows_per_strip, p.strips, p.passes, p.strips_per_pass, (long long)p.pass_pixels};
	for (int i = 0; i < 8; ++i) out[i] = v[i];
}
// strips pass `pass` renders; for each of its local strips the rows [row0, row0 + rows) of the image: rows_out [2 * strips_per_pass]
int rh_pass_rows(int width, int height, int factor, unsigned long long budget, unsigned pass, int *rows_out)
{
	const AaPlan p = plan_aa(width, height, factor, budget);
	for (uint32_t ls = 0; ls < p.strips_per_pass; ++ls) aa_strip_rows(p, height, pass, ls, rows_out[2 * ls], rows_out[2 * ls + 1]);
	return (int)aa_pass_strips(p, pass);
}
// half[i] = the half nearest to in[i]
void rh_half(const float *in, unsigned short *half, long long n)
{
	for (long long i = 0; i < n; ++i) half[i] = (unsigned short)aa_half_bits(in[i]);
}

// One pass: color [pass_pixels][4] (stats [pass_pixels][3] or null), the compact buffers of pass `pass` of the plan for `budget`, into
// the rows of out ([height][width] RGBA32F, format 0, or RGBA16F, format 1) and out_stats that the pass covers.  Nothing else is written.
void rh_resolve(int width, int height, int factor, unsigned long long budget, unsigned pass, const float *color, const uint32_t *stats, int format,
	void *out, uint32_t *out_stats)
{
	const AaPlan p = plan_aa(width, height, factor, budget);
	const RowMap rm = aa_pass_row_map(p, pass, 3);
	const uint32_t strips = aa_pass_strips(p, pass);
	for (uint32_t ls = 0; ls < strips; ++ls)
	{
		int row0, rows;
		aa_strip_rows(p, height, pass, ls, row0, rows);
		if (rows > 0 && (int)(strip_local_to_global(rm, ls) * (uint32_t)p.rows_per_strip) != row0) __builtin_trap(); // the kernel's row and the plan's agree
		const size_t first = (size_t)ls * SDFR_STRIP_ROWS * (size_t)p.s_width;
		const Strip s = {color + 4 * first, stats ? stats + 3 * first : nullptr, p.s_width};
		for (int o = 0; o < rows; ++o)
			for (int ox = 0; ox < width; ++ox)
			{
				const vec4 c = pyramid(s, p.factor_log2, o, ox);
				const size_t pix = (size_t)(row0 + o) * width + ox;
				if (format == FORMAT_RGBA32F)
				{
					float *q = static_cast<float *>(out) + 4 * pix;
					q[0] = c.x, q[1] = c.y, q[2] = c.z, q[3] = c.w;
				}
				else
				{
					uint32_t *q = static_cast<uint32_t *>(out) + 2 * pix;
					aa_half_pixel(c, q[0], q[1]);
				}
				if (!stats) continue;
				AaCounters sum = {0u, 0u, 0u};
				for (int dy = 0; dy < factor; ++dy)
					for (int dx = 0; dx < factor; ++dx)
					{
						const uint32_t *q = s.stats + 3 * ((size_t)(o * factor + dy) * p.s_width + (size_t)ox * factor + dx);
						const AaCounters one = {q[0], q[1], q[2]};
						sum = aa_add(sum, one);
					}
				uint32_t *q = out_stats + 3 * pix;
				q[0] = sum.rays, q[1] = sum.evals, q[2] = sum.hits;
			}
	}
}

} // extern "C"

// sdfr_measure.h -- the moments of the solid over a bundle of parallel columns: the stage functions of sdfr_measure (include/sdfr.h, where
// the definition stands in full), scene-independent and host-compilable like sdfr_span.h.  measure_column is the march of
// span_item (sdfr_span.h) with another sink: where a span closes, the integrals of 1, t and t^2 over it are added up in fp64 instead of
// the span being stored.  The lines of the march are repeated, not shared, as the lighting kernel repeats the surface kernel's: span_item's
// zero-fill loop and max_spans gate have no place here, and k_query_spans keeps its code.  k_query_measure (sdfr_query_kernel.h) runs it
// one lane per column and reduces a tile in the wave; k_measure_reduce (sdfr_mesh.hip) reduces the tiles.  measure_reduce_host restates
// both reductions sequentially; tests/cpp/measure_host.cpp runs the same text over analytic fields on the CPU.  The march is fp32 and the
// moments fp64, every operation separate and in source order (-ffp-contract=off), so both give the same bits.
#pragma once
#include "sdfr_span.h"

namespace sdfr {

enum { MEASURE_MOMENTS = 10, MEASURE_TILE = 8, MEASURE_RUN = 64, MEASURE_COLUMN_WORDS = 10, MEASURE_MAX_AXIS = 8192, MEASURE_MAX_COLUMNS = 1 << 24 };

struct MeasureGrid // sdfr_measure_grid
{
	float origin[3];
	float du[3], dv[3], dw[3];
	int32_t nu, nv;
};
struct MeasureColumn // sdfr_measure_column
{
	double m0, m1, m2;
	uint32_t spans, steps, flags;
	int32_t valid;
};
struct MeasureResult // sdfr_measure_result
{
	double moments[MEASURE_MOMENTS];
	int64_t columns_hit, columns_open, columns_out_of_steps, columns_invalid;
	int64_t steps, spans, crossings;
	int32_t hit_lo[2], hit_hi[2];
	float t_lo, t_hi;
};
// what a lane knows of its column: the record, and what only the totals keep
struct MeasureLane
{
	MeasureColumn c;
	uint32_t crossings;
	float t_lo, t_hi; // over the column's spans; +inf and -inf without one
};

SDF_HD float measure_inf(bool negative) { return bits_f32(negative ? 0xff800000u : 0x7f800000u); }
// a lane without a column, or a column without an answer: all zero, and no span
SDF_HD MeasureLane measure_no_column()
{
	MeasureLane l;
	l.c.m0 = l.c.m1 = l.c.m2 = 0.0;
	l.c.spans = l.c.steps = l.c.flags = 0u;
	l.c.valid = 0;
	l.crossings = 0u;
	l.t_lo = measure_inf(false);
	l.t_hi = measure_inf(true);
	return l;
}

// component c of the origin of column (i, j): slice_coord's form with layer 0
SDF_HD float measure_origin(const float origin[3], const float du[3], const float dv[3], int c, int i, int j)
{
	return (origin[c] + (float)i * du[c]) + (float)j * dv[c];
}

// a span [t_in, t_out] closes: the integrals of 1, t and t^2 over it
SDF_HD void measure_close(MeasureLane &l, float t_in, float t_out)
{
	const double a = (double)t_in, b = (double)t_out;
	l.c.m0 = l.c.m0 + (b - a);
	l.c.m1 = l.c.m1 + 0.5 * (b * b - a * a);
	l.c.m2 = l.c.m2 + ((b * b) * b - (a * a) * a) / 3.0;
	l.t_lo = t_in < l.t_lo ? t_in : l.t_lo;
	l.t_hi = t_out > l.t_hi ? t_out : l.t_hi;
}

// One column: the march of span_item from o along d, line for line, with measure_close where a span closes.  A column whose origin or
// direction is not span_item_ok: valid = 0, no evaluation, all zero.  distance(p) is D at p.
template <class Distance>
SDF_HD MeasureLane measure_column(const Distance &distance, vec3 o, vec3 d, float t_max, float min_step, float iso, int32_t max_steps)
{
	MeasureLane l = measure_no_column();
	if (!span_item_ok(o, d)) return l;
	l.c.valid = 1;
	uint32_t crossings = 0u, spans = 0u, steps = 0u, flags = 0u;
	float t = 0.f, t_prev = 0.f, s_prev = 0.f, t_in = 0.f;
	bool inside_prev = false, open = false;
	for (;;)
	{
		const vec3 p = V3(o.x + t * d.x, o.y + t * d.y, o.z + t * d.z); // one multiply, then one add
		const float s = distance(p) - iso;
		const bool inside = s < 0.f; // NaN is outside
		if (steps != 0u ? inside != inside_prev : inside)
		{
			float tc = 0.f;
			if (steps != 0u)
			{
				float u = s_prev / (s_prev - s);
				if (!(u >= 0.f && u <= 1.f)) u = 0.5f;
				tc = t_prev + u * (t - t_prev);
				++crossings;
			}
			else
				flags |= (uint32_t)SPAN_STARTS_INSIDE;
			if (inside)
			{
				open = true;
				t_in = tc;
				++spans;
			}
			else
			{
				open = false;
				measure_close(l, t_in, tc);
			}
		}
		++steps;
		if (!(t < t_max)) break; // that was the sample at t_max
		if (steps == (uint32_t)max_steps)
		{
			flags |= (uint32_t)SPAN_OUT_OF_STEPS;
			break;
		}
		const float a = abs1(s);
		const float h = a > min_step ? a : min_step; // NaN steps by min_step
		const float t_next = t + h;
		t_prev = t;
		s_prev = s;
		inside_prev = inside;
		t = t_next < t_max ? t_next : t_max;
	}
	if (open)
	{
		flags |= (uint32_t)SPAN_ENDS_INSIDE;
		measure_close(l, t_in, t);
	}
	l.c.spans = spans;
	l.c.steps = steps;
	l.c.flags = flags;
	l.crossings = crossings;
	return l;
}

// the ten contributions of column (i, j) in the order of sdfr_measure_result.moments; a column without an answer has m0 = m1 = m2 = +0.0
// and contributes +0.0 (i, j >= 0)
SDF_HD void measure_contributions(const MeasureColumn &c, int i, int j, double v[MEASURE_MOMENTS])
{
	const double u = (double)i, w = (double)j;
	v[0] = c.m0;
	v[1] = u * c.m0;
	v[2] = w * c.m0;
	v[3] = c.m1;
	v[4] = (u * u) * c.m0;
	v[5] = (w * w) * c.m0;
	v[6] = c.m2;
	v[7] = (u * w) * c.m0;
	v[8] = w * c.m1;
	v[9] = u * c.m1;
}

// fp32 bounds through integer atomics: a map of the bits that keeps the order of the numbers (no NaN comes here)
SDF_HD uint32_t measure_order_key(float f)
{
	const uint32_t b = f32_bits(f);
	return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
SDF_HD float measure_order_value(uint32_t k) { return bits_f32((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

SDF_HD uint32_t measure_tiles(int32_t n) { return ((uint32_t)n + (uint32_t)MEASURE_TILE - 1u) / (uint32_t)MEASURE_TILE; }

#if !defined(__HIPCC_RTC__)
// The pairwise tree over 64 values, level by level x[m] = x[2m] + x[2m + 1]: what six xor-butterflies leave in every lane
inline double measure_tree64(double x[MEASURE_RUN])
{
	for (int n = MEASURE_RUN / 2; n >= 1; n /= 2)
		for (int m = 0; m < n; ++m) x[m] = x[2 * m] + x[2 * m + 1];
	return x[0];
}
// `n` records of MEASURE_MOMENTS doubles, in place: runs of 64 records by index, the last padded with +0.0, each replaced by its tree
// sum per component, until one record is left (in the first ten doubles).  A single record is its own result.  -> the passes made
inline int measure_reduce_records(double *records, size_t n)
{
	int passes = 0;
	while (n > 1)
	{
		const size_t runs = (n + MEASURE_RUN - 1) / MEASURE_RUN;
		for (size_t r = 0; r < runs; ++r)
		{
			double out[MEASURE_MOMENTS];
			for (int c = 0; c < MEASURE_MOMENTS; ++c)
			{
				double x[MEASURE_RUN];
				for (size_t l = 0; l < MEASURE_RUN; ++l) x[l] = MEASURE_RUN * r + l < n ? records[(MEASURE_RUN * r + l) * MEASURE_MOMENTS + c] : 0.0;
				out[c] = measure_tree64(x);
			}
			for (int c = 0; c < MEASURE_MOMENTS; ++c) records[r * MEASURE_MOMENTS + c] = out[c]; // (run r's records lie at or after record r)
		}
		n = runs;
		++passes;
	}
	return passes;
}
// The whole reduction restated on the host: lanes [nu * nv], row-major i + nu * j, -> the result; tiles: scratch of
// measure_tiles(nu) * measure_tiles(nv) * MEASURE_MOMENTS doubles.
inline void measure_reduce_host(const MeasureLane *lanes, int32_t nu, int32_t nv, double *tiles, MeasureResult &out)
{
	const uint32_t tu = measure_tiles(nu), tv = measure_tiles(nv);
	MeasureResult r = {};
	r.hit_lo[0] = nu, r.hit_lo[1] = nv, r.hit_hi[0] = r.hit_hi[1] = -1;
	r.t_lo = measure_inf(false), r.t_hi = measure_inf(true);
	for (uint32_t tj = 0; tj < tv; ++tj)
		for (uint32_t ti = 0; ti < tu; ++ti)
		{
			double x[MEASURE_MOMENTS][MEASURE_RUN];
			for (int l = 0; l < MEASURE_RUN; ++l)
			{
				const int i = (int)(ti * 8u) + (l & 7), j = (int)(tj * 8u) + (l >> 3);
				double v[MEASURE_MOMENTS];
				for (int c = 0; c < MEASURE_MOMENTS; ++c) v[c] = 0.0;
				if (i < nu && j < nv)
				{
					const MeasureLane &lane = lanes[(size_t)i + (size_t)nu * (size_t)j];
					if (lane.c.valid == 1) measure_contributions(lane.c, i, j, v);
					else ++r.columns_invalid;
					if (lane.c.spans >= 1u)
					{
						++r.columns_hit;
						r.hit_lo[0] = i < r.hit_lo[0] ? i : r.hit_lo[0], r.hit_hi[0] = i > r.hit_hi[0] ? i : r.hit_hi[0];
						r.hit_lo[1] = j < r.hit_lo[1] ? j : r.hit_lo[1], r.hit_hi[1] = j > r.hit_hi[1] ? j : r.hit_hi[1];
					}
					if (lane.c.flags & (uint32_t)(SPAN_STARTS_INSIDE | SPAN_ENDS_INSIDE)) ++r.columns_open;
					if (lane.c.flags & (uint32_t)SPAN_OUT_OF_STEPS) ++r.columns_out_of_steps;
					r.steps += lane.c.steps, r.spans += lane.c.spans, r.crossings += lane.crossings;
					r.t_lo = lane.t_lo < r.t_lo ? lane.t_lo : r.t_lo;
					r.t_hi = lane.t_hi > r.t_hi ? lane.t_hi : r.t_hi;
				}
				for (int c = 0; c < MEASURE_MOMENTS; ++c) x[c][l] = v[c];
			}
			for (int c = 0; c < MEASURE_MOMENTS; ++c) tiles[((size_t)ti + (size_t)tu * tj) * MEASURE_MOMENTS + c] = measure_tree64(x[c]);
		}
	(void)measure_reduce_records(tiles, (size_t)tu * tv);
	for (int c = 0; c < MEASURE_MOMENTS; ++c) r.moments[c] = tiles[c];
	out = r;
}
#endif

} // namespace sdfr

// tests/cpp/span_host.cpp -- TEST-ONLY: the stage function of the span queries (sdf_playground_amd/csrc/sdfr_span.h) compiled for the CPU and
// run ray by ray over two analytic fields, the way k_query_spans runs it one lane per ray over a scene, so that the CPU test tier can
// compare it with the definition restated in numpy (tests/span_util.py) word for word without a GPU.  Built with -ffp-contract=off, as
// the library.  The product never loads this.
#include "sdfr_span.h"

#include <cmath>
#include <limits>

using namespace sdfr;

namespace {

// D = min_k(|x - c_k| - r_k), the minimum taken in the order of k by `v < D ? v : D` from +inf; NaN where nan_lo <= x <= nan_hi
struct SlabLadder
{
	int n;
	const float *c, *r;
	float nan_lo, nan_hi;
	float operator()(vec3 p) const
	{
		float D = std::numeric_limits<float>::infinity();
		for (int k = 0; k < n; ++k)
		{
			const float v = fabsf(p.x - c[k]) - r[k];
			D = v < D ? v : D;
		}
		return p.x >= nan_lo && p.x <= nan_hi ? std::numeric_limits<float>::quiet_NaN() : D;
	}
};

// a sphere's exact distance (compared with analytic chords, not bit for bit)
struct Sphere
{
	float c[3], radius;
	float operator()(vec3 p) const
	{
		const float x = p.x - c[0], y = p.y - c[1], z = p.z - c[2];
		return sqrtf(x * x + y * y + z * z) - radius;
	}
};

struct ItemSpans
{
	float *item; // [max_spans][2]
	void operator()(int k, float t_in, float t_out) const
	{
		item[2 * k] = t_in;
		item[2 * k + 1] = t_out;
	}
};

template <class Field>
int march_all(int64_t n, const float *origins, const float *dirs, const SpanParams &p, const Field &field, uint32_t *summaries, float *spans)
{
	for (int64_t i = 0; i < n; ++i)
	{
		const float *o = origins + 3 * i, *d = dirs + 3 * i;
		const ItemSpans store = {spans ? spans + (size_t)2 * p.max_spans * i : nullptr};
		span_item(field, store, true, V3(o[0], o[1], o[2]), V3(d[0], d[1], d[2]), p.t_max, p.min_step, p.iso, p.max_steps, p.max_spans,
			summaries + (size_t)SPAN_SUMMARY_WORDS * i);
	}
	return 0;
}

} // namespace

extern "C" {

int sph_march_slabs(int64_t n, const float *origins, const float *dirs, const SpanParams *p, int slabs, const float *c, const float *r, float nan_lo, float nan_hi,
	uint32_t *summaries, float *spans)
{
	const SlabLadder field = {slabs, c, r, nan_lo, nan_hi};
	return march_all(n, origins, dirs, *p, field, summaries, spans);
}
int sph_march_sphere(int64_t n, const float *origins, const float *dirs, const SpanParams *p, const float *centre, float radius, uint32_t *summaries, float *spans)
{
	const Sphere field = {{centre[0], centre[1], centre[2]}, radius};
	return march_all(n, origins, dirs, *p, field, summaries, spans);
}
int sph_params_size() { return (int)sizeof(SpanParams); }
int sph_summary_words() { return (int)SPAN_SUMMARY_WORDS; }

} // extern "C"

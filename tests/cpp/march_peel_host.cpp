// tests/cpp/march_peel_host.cpp -- TEST-ONLY host build of the march's step for a ray's first three samples (march_advance_unrelaxed,
// sdf_playground_amd/csrc/sdfr_pixel.h) beside the general step it stands for there, march_pre + march_advance, on the same states.
// Loaded by tests/test_march_peel_cpu.py, which makes the states and compares every word.  A state travels as twelve 32-bit words:
// start (3), dir (3), t, last_d, last_safe, factor, d, iter.
#include "sdfr_pixel.h"

#include <stdint.h>
#include <string.h>

using namespace sdfr;

namespace {

constexpr int WORDS = 12;

March load(const uint32_t *w)
{
	March m;
	float f[11];
	memcpy(f, w, sizeof f);
	m.start = V3(f[0], f[1], f[2]);
	m.dir = V3(f[3], f[4], f[5]);
	m.t = f[6], m.last_d = f[7], m.last_safe = f[8], m.factor = f[9], m.d = f[10];
	m.iter = w[11];
	return m;
}

void store(const March &m, uint32_t *w)
{
	const float f[11] = {m.start.x, m.start.y, m.start.z, m.dir.x, m.dir.y, m.dir.z, m.t, m.last_d, m.last_safe, m.factor, m.d};
	memcpy(w, f, sizeof f);
	w[11] = m.iter;
}

} // namespace

// n states with factor 1 and iter below 3 and below iter_count[i], one distance sample each: the general pass and the specialised one
extern "C" void peel_one(int64_t n, const uint32_t *state, const float *d, const float *dist_max, const uint32_t *iter_count, float dist_eps,
                         uint32_t *general, int32_t *general_status, uint32_t *special, int32_t *special_status)
{
	for (int64_t i = 0; i < n; ++i)
	{
		March g = load(state + WORDS * i), s = g;
		march_pre(g);
		general_status[i] = march_advance(g, d[i], dist_max[i], iter_count[i], dist_eps);
		special_status[i] = march_advance_unrelaxed(s, d[i], dist_max[i], iter_count[i], dist_eps);
		store(g, general + WORDS * i);
		store(s, special + WORDS * i);
	}
}

// n rays from their start (march_begin) with `samples` distance samples each (d[samples * i + k] is what the k-th evaluation returns):
// every pass through march_pre + march_advance, against the peeled schedule -- `peeled` specialised passes, the factor, the general pass
// without march_pre for the rest.  peeled = 3 is the pixel kernel's; 2 sets the factor one sample early and has to show.  Both stop with
// the ray; `passes` says how many samples the general schedule took.
extern "C" void peel_ray(int64_t n, int samples, int peeled, const float *start_dir, const float *d, const float *dist_max, const uint32_t *iter_count,
                         float dist_eps, uint32_t *general, int32_t *general_status, uint32_t *special, int32_t *special_status, int32_t *passes)
{
	for (int64_t i = 0; i < n; ++i)
	{
		const float *sd = start_dir + 6 * i;
		March g = march_begin(V3(sd[0], sd[1], sd[2]), V3(sd[3], sd[4], sd[5])), s = g;
		int gs = MARCH_CONTINUE, ss = MARCH_CONTINUE, k = 0;
		for (; k < samples && gs == MARCH_CONTINUE; ++k)
		{
			march_pre(g);
			gs = march_advance(g, d[samples * i + k], dist_max[i], iter_count[i], dist_eps);
		}
		passes[i] = k;
		// the general schedule's state where the test reads it: before the next pass, that is after its march_pre
		if (gs == MARCH_CONTINUE) march_pre(g);
		k = 0;
		for (; k < samples && k < peeled && ss == MARCH_CONTINUE; ++k)
			ss = march_advance_unrelaxed(s, d[samples * i + k], dist_max[i], iter_count[i], dist_eps);
		if (ss == MARCH_CONTINUE && k == peeled) s.factor = 1.5f;
		for (; k < samples && ss == MARCH_CONTINUE; ++k)
			ss = march_advance(s, d[samples * i + k], dist_max[i], iter_count[i], dist_eps);
		general_status[i] = gs, special_status[i] = ss;
		store(g, general + WORDS * i);
		store(s, special + WORDS * i);
	}
}

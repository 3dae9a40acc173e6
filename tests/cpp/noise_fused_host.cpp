// tests/cpp/noise_fused_host.cpp -- TEST-ONLY host build of the table path of snoise3 / turbulence3 with its fused hash
// (NoiseHashExact, sdf_playground_amd/csrc/sdfr_noise.h) beside the plain text it replaces (NoiseHashPlain, noise_mod289,
// noise_permute).  Loaded by tests/test_noise_fused_cpu.py.
#include "sdfr_noise.h"

#include <stdint.h>

using namespace sdfr;

namespace {

struct HostTab
{
	static float t[3][SDFR_NOISE_GRADS];
	static float at(int c, uint32_t k) { return t[c][k]; }
};
float HostTab::t[3][SDFR_NOISE_GRADS];
typedef NoiseGradTable<HostTab> HostGrads;

} // namespace

extern "C" void nf_fill()
{
	for (int k = 0; k < SDFR_NOISE_GRADS; ++k)
	{
		const vec3 g = simplex_grad((float)k);
		HostTab::t[0][k] = g.x; HostTab::t[1][k] = g.y; HostTab::t[2][k] = g.z;
	}
}

// what = 0: snoise3, 1: turbulence3.  out: n x 2 (formula with the plain hash, table with the fused hash); fell[k] = 1 where the
// table path cleared `ok` and the value is the recomputation's.  Returns how many did.
extern "C" long long nf_noise(int what, const float *in, float *out, unsigned char *fell, long long n)
{
	long long fell_back = 0;
	for (long long k = 0; k < n; ++k)
	{
		const vec3 v = V3(in[3 * k], in[3 * k + 1], in[3 * k + 2]);
		bool ok = true;
		if (what == 0)
		{
			out[2 * k] = snoise3<NoiseGradFormula>(v);
			out[2 * k + 1] = snoise3<HostGrads>(v);
			snoise3_grads<HostGrads>(v, ok);
		}
		else
		{
			out[2 * k] = turbulence3<NoiseGradFormula>(v);
			out[2 * k + 1] = turbulence3<HostGrads>(v);
			turbulence3_grads<HostGrads>(v, ok);
		}
		fell[k] = ok ? 0 : 1;
		fell_back += ok ? 0 : 1;
	}
	return fell_back;
}

// every integer permute argument x in [lo, hi]: out n x 6 = plain permute, fused permute, plain j of the plain permute, fused j
// of it, plain mod289(x), fused mod289(x)
extern "C" void nf_permutes(int lo, int hi, float *out)
{
	for (int x = lo; x <= hi; ++x)
	{
		float *o = out + 6 * (x - lo);
		const float p = noise_permute((float)x);
		o[0] = p;
		o[1] = NoiseHashExact::permute((float)x);
		o[2] = NoiseHashPlain::mod49(p);
		o[3] = NoiseHashExact::mod49(p);
		o[4] = noise_mod289((float)x);
		o[5] = NoiseHashExact::mod289((float)x);
	}
}

// the plain mod289 of every integer |i| <= lim: smallest and largest result, and how many results the range test of the fused
// hash refuses
extern "C" long long nf_lattice_range(int lim, float *lo, float *hi)
{
	long long refused = 0;
	float a = 1e30f, b = -1e30f;
	for (int i = -lim; i <= lim; ++i)
	{
		const float r = noise_mod289((float)i);
		a = r < a ? r : a;
		b = r > b ? r : b;
		refused += NoiseHashExact::reduced(r) ? 0 : 1;
	}
	*lo = a; *hi = b;
	return refused;
}

// Why the reduction of the lattice coordinates stays plain: over the n integer-valued floats in[], how many have the fused
// mod289 differ from the plain one although BOTH results pass the range test (first such input to *first)
extern "C" long long nf_fused_lattice_would_differ(const float *in, long long n, float *first)
{
	long long bad = 0;
	for (long long k = 0; k < n; ++k)
	{
		const float a = noise_mod289(in[k]), b = NoiseHashExact::mod289(in[k]);
		if (f32_bits(a) != f32_bits(b) && NoiseHashExact::reduced(a) && NoiseHashExact::reduced(b))
		{
			if (bad == 0) *first = in[k];
			++bad;
		}
	}
	return bad;
}

// the whole hash of a cell, plain and fused, for integer lattice coordinates: in n x 3 (i), every choice of the middle corners'
// offsets; returns the number of (cell, offsets) whose four hashed indices differ in a bit although the fused hash kept `ok`
extern "C" long long nf_corners(const float *in, long long n, long long *kept)
{
	static const float offs[6][2][3] = {
		{{1, 0, 0}, {1, 1, 0}}, {{1, 0, 0}, {1, 0, 1}}, {{0, 1, 0}, {1, 1, 0}}, {{0, 1, 0}, {0, 1, 1}}, {{0, 0, 1}, {1, 0, 1}}, {{0, 0, 1}, {0, 1, 1}}};
	long long bad = 0, k_ok = 0;
	for (long long k = 0; k < n; ++k)
		for (int o = 0; o < 6; ++o)
		{
			const vec3 i = V3(in[3 * k], in[3 * k + 1], in[3 * k + 2]);
			const vec3 i1 = V3(offs[o][0][0], offs[o][0][1], offs[o][0][2]), i2 = V3(offs[o][1][0], offs[o][1][1], offs[o][1][2]);
			bool ok = true, unused = true;
			const vec4 a = NoiseHashPlain::corners(i, i1, i2, unused), b = NoiseHashExact::corners(i, i1, i2, ok);
			if (!ok) continue;
			++k_ok;
			if (f32_bits(a.x) != f32_bits(b.x) || f32_bits(a.y) != f32_bits(b.y) || f32_bits(a.z) != f32_bits(b.z) || f32_bits(a.w) != f32_bits(b.w)) ++bad;
		}
	*kept = k_ok;
	return bad;
}

// tests/cpp/math_accuracy_host.cpp -- TEST INFRASTRUCTURE: how far the product's deterministic elementary functions
// (sdf_playground_amd/csrc/sdfr_math.h, host build: the bits the kernels compute) are from the functions they stand for.
//
// Truth is libm in double: correct to well under one double ulp, i.e. to about 2^-29 of an fp32 ulp.  The error of a result v
// against the truth t is given in ulps of the true value -- ulp(t) = 2^(floor(log2 |t|) - 23) -- and absolutely.  Where |t| is below
// 2^-126 (fp32 denormal range, which exp21 flushes) the result only enters the absolute figure and the count `tiny`.
//
// mah_run sweeps every function and returns one row per (function, sign, binade of the argument); tests/test_math_accuracy_cpu.py
// writes the rows to tests/golden/math_accuracy.json and holds every later run to them.  The sweep is deterministic: samples are
// hashes of their index, and a row's maxima break ties by the argument's bits, so the threads' order does not matter.
// mah_eval / mah_truth evaluate chosen points for the tests (the GPU tier compares the device's bits with mah_eval's).
#include "sdfr_math.h"
#include "detmath.h"

#include <atomic>
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

namespace {

enum Fn { F_SIN, F_COS, F_ATAN, F_ATAN_PAIRS, F_EXP2, F_LOG2, F_POW, F_COUNT };
const int BINADE_MIN = -150, BINADE_MAX = 130, BINADES = BINADE_MAX - BINADE_MIN + 1;

struct Stat
{
	uint64_t n, nonfinite, tiny, broken, compared, differ;
	double ulp, abs, maxres;
	uint64_t ulp_at, abs_at, maxres_at; // (first argument's bits << 32) | second argument's bits
};

struct Acc
{
	std::vector<Stat> s;
	Acc() : s((size_t)F_COUNT * 2 * BINADES) {}
	Stat &at(int fn, int sign, int binade)
	{
		if (binade < BINADE_MIN) binade = BINADE_MIN;
		if (binade > BINADE_MAX) binade = BINADE_MAX;
		return s[((size_t)fn * 2 + sign) * BINADES + (binade - BINADE_MIN)];
	}
};

inline uint32_t bits_of(float f) { return sdfr::f32_bits(f); }
inline float float_of(uint32_t u) { return sdfr::bits_f32(u); }
inline bool same_bits(float a, float b) { return bits_of(a) == bits_of(b) || (a != a && b != b); }
// binade of a double quantity (a ratio, a product): its unbiased exponent
inline int binade_of_double(double t)
{
	t = std::fabs(t); // (no row for zero: the ends of the range collect what lies beyond them)
	if (!(t > 0.0)) return BINADE_MIN;
	if (t == HUGE_VAL) return BINADE_MAX;
	int e;
	std::frexp(t, &e);
	return e - 1;
}
inline double ulp_of(double t)
{
	int e;
	std::frexp(std::fabs(t), &e);
	return std::ldexp(1.0, e - 1 - 23);
}
inline void keep_max(double v, uint64_t key, double &best, uint64_t &best_at)
{
	if (v > best || (v == best && key < best_at)) { best = v; best_at = key; }
}

void score(Stat &s, float v, double t, uint32_t a0, uint32_t a1)
{
	const uint64_t key = ((uint64_t)a0 << 32) | a1;
	s.n++;
	const bool v_finite = std::fabs(v) <= 3.402823466e+38f;
	// what the truth rounds to in fp32: infinite from 2^128 (1 - 2^-25) on
	const bool t_overflows = !(std::fabs(t) < 0x1.ffffffp+127);
	if (!v_finite || t != t || t_overflows)
	{
		const bool agree = (t != t) ? (v != v) : (t_overflows && !v_finite && v == v && (v > 0) == (t > 0));
		if (!agree) s.nonfinite++;
		return;
	}
	keep_max(std::fabs((double)v), key, s.maxres, s.maxres_at);
	const double d = std::fabs((double)v - t);
	keep_max(d, key, s.abs, s.abs_at);
	if (std::fabs(t) < 0x1p-126 && t != 0.0) { s.tiny++; return; }
	if (t == 0.0) { keep_max(d == 0.0 ? 0.0 : HUGE_VAL, key, s.ulp, s.ulp_at); return; }
	keep_max(d / ulp_of(t), key, s.ulp, s.ulp_at);
}

inline uint64_t mix(uint64_t x)
{
	x += 0x9e3779b97f4a7c15ull;
	x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
	x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
	return x ^ (x >> 31);
}
inline double unit(uint64_t h) { return (double)(h >> 11) * 0x1p-53; } // [0, 1)

// the seeded samples: item i of each, the same in every run
void atan_pair(uint64_t i, float &y, float &x)
{
	uint32_t by = (uint32_t)mix(2 * i + 0x5df0a7a2u), bx = (uint32_t)mix(2 * i + 1 + 0x5df0a7a2u);
	if ((by & 0x7f800000u) == 0x7f800000u) by &= ~0x40000000u; // finite
	if ((bx & 0x7f800000u) == 0x7f800000u) bx &= ~0x40000000u;
	y = float_of(by);
	x = float_of(bx);
}
void pow_pair(uint64_t i, float &x, float &y)
{
	const double u1 = unit(mix(3 * i + 0x5df0b0b0u)), u2 = unit(mix(3 * i + 1 + 0x5df0b0b0u));
	double dx, dy;
	switch (i & 3)
	{
	case 0: dx = 4.0 * (1.0 - u1); dy = 256.0 * u2 - 128.0; break;                                // x in (0, 4] uniform, y in [-128, 128)
	case 1: dx = 4.0 * std::exp2(-24.0 * u1); dy = 256.0 * u2 - 128.0; break;                     // x in (2^-22, 4] log-uniform
	case 2: dx = 1.0 - std::exp2(-1.0 - 22.0 * u1); dy = std::exp2(13.0 * u2); break;             // the Blinn case: x just below 1, y up to 8192
	default: dx = 1.0 - u1; dy = 128.0 * u2; break;                                               // x in (0, 1], y in [0, 128)
	}
	x = (float)dx;
	y = (float)dy;
	if (!(x > 0.f)) x = 1.17549435e-38f;
}

struct Task { int kind, binade; uint64_t lo, hi, stride; bool sample; }; // kinds: the Fn of the sweep (F_SIN stands for sin and cos)

void sweep_sincos(Acc &acc, const Task &t)
{
	Stat &ss = acc.at(F_SIN, 0, t.binade), &sc = acc.at(F_COS, 0, t.binade);
	for (uint64_t i = t.lo; i <= t.hi; i += t.stride)
	{
		uint32_t b = (uint32_t)i;
		if (t.sample) // a hashed mantissa in the binade of t.lo (of the denormals: never zero)
		{
			b = ((uint32_t)t.lo & 0xff800000u) | ((uint32_t)mix(i) & 0x007fffffu);
			if (b == 0) b = 1;
		}
		const float x = float_of(b);
		const float s = sdfr::sin1(x), c = sdfr::cos1(x);
		const double dx = (double)x;
		score(ss, s, std::sin(dx), b, 0);
		score(sc, c, std::cos(dx), b, 0);
		// one reduction, the same bits; odd and even, bit for bit (a zero result keeps the sign the function gives it: see the test)
		const sdfr::vec2 both = sdfr::sincos1(x);
		if (!same_bits(both.x, s) || !same_bits(both.y, c)) ss.broken++;
		const float sn = sdfr::sin1(-x), cn = sdfr::cos1(-x);
		if (b != 0 && !same_bits(sn, -s)) ss.broken++;
		if (!same_bits(cn, c)) sc.broken++;
		if (x <= 0.75f)
		{
			const sdfr::vec2 sp = sdfr::sincos1_small(x), sm = sdfr::sincos1_small(-x), bm = sdfr::sincos1(-x);
			if (!same_bits(sp.x, s) || !same_bits(sm.x, bm.x)) ss.broken++;
			if (!same_bits(sp.y, c) || !same_bits(sm.y, bm.y)) sc.broken++;
		}
		if (b % 251u == 0)
		{
			ss.compared++, sc.compared++;
			if (!same_bits(orc::dm::sinf_det(x), s) || !same_bits(orc::dm::sinf_det(-x), sn)) ss.differ++;
			if (!same_bits(orc::dm::cosf_det(x), c) || !same_bits(orc::dm::cosf_det(-x), cn)) sc.differ++;
		}
	}
}

void sweep_atan(Acc &acc, const Task &t)
{
	Stat &s = acc.at(F_ATAN, 0, t.binade);
	for (uint64_t i = t.lo; i <= t.hi; i += t.stride)
	{
		const uint32_t b = (uint32_t)i;
		const float y = float_of(b);
		const float v = sdfr::atan21(y, 1.f);
		score(s, v, std::atan2((double)y, 1.0), b, 0x3f800000u);
		if (!same_bits(sdfr::atan21(-y, 1.f), -v) || !same_bits(sdfr::atan1(y), v)) s.broken++;
		if (b % 251u == 0)
		{
			s.compared++;
			if (!same_bits(orc::dm::atan2f_det(y, 1.f), v)) s.differ++;
		}
	}
}

void sweep_atan_pairs(Acc &acc, const Task &t)
{
	for (uint64_t i = t.lo; i <= t.hi; ++i)
	{
		float y, x;
		atan_pair(i, y, x);
		const float v = sdfr::atan21(y, x);
		const double ratio = x == 0.f ? HUGE_VAL : std::fabs((double)y / (double)x);
		Stat &s = acc.at(F_ATAN_PAIRS, 0, binade_of_double(ratio));
		score(s, v, std::atan2((double)y, (double)x), bits_of(y), bits_of(x));
		if (i % 251u == 0)
		{
			s.compared++;
			if (!same_bits(orc::dm::atan2f_det(y, x), v)) s.differ++;
		}
	}
}

void sweep_exp2(Acc &acc, const Task &t)
{
	for (int sign = 0; sign < 2; ++sign)
	{
		Stat &s = acc.at(F_EXP2, sign, t.binade);
		for (uint64_t i = t.lo; i <= t.hi; i += t.stride)
		{
			const uint32_t b = (uint32_t)i | (sign ? 0x80000000u : 0u);
			const float x = float_of(b);
			const float v = sdfr::exp21(x);
			score(s, v, std::exp2((double)x), b, 0);
			if (b % 251u == 0)
			{
				s.compared++;
				if (!same_bits(orc::dm::exp2f_det(x), v)) s.differ++;
			}
		}
	}
}

void sweep_log2(Acc &acc, const Task &t)
{
	Stat &s = acc.at(F_LOG2, 0, t.binade);
	for (uint64_t i = t.lo; i <= t.hi; i += t.stride)
	{
		const uint32_t b = (uint32_t)i;
		const float x = float_of(b);
		const float v = sdfr::log21(x);
		score(s, v, std::log2((double)x), b, 0);
		if (b % 251u == 0)
		{
			s.compared++;
			if (!same_bits(orc::dm::log2f_det(x), v)) s.differ++;
		}
	}
}

void sweep_pow(Acc &acc, const Task &t)
{
	for (uint64_t i = t.lo; i <= t.hi; ++i)
	{
		float x, y;
		pow_pair(i, x, y);
		const float v = sdfr::pow1(x, y);
		// the binade of a pow is that of the product its exp2 receives: it scales the logarithm's error
		Stat &s = acc.at(F_POW, 0, binade_of_double((double)y * std::log2((double)x)));
		score(s, v, std::pow((double)x, (double)y), bits_of(x), bits_of(y));
		if (i % 251u == 0)
		{
			s.compared++;
			if (!same_bits(orc::dm::powf_det(x, y), v)) s.differ++;
		}
	}
}

const uint64_t CHUNK = 1u << 19; // floats of one task

void add_range(std::vector<Task> &tasks, int kind, int binade, uint64_t lo, uint64_t hi, uint64_t stride)
{
	for (uint64_t a = lo; a <= hi; a += CHUNK * stride)
	{
		const uint64_t last = a + (CHUNK - 1) * stride;
		tasks.push_back(Task{kind, binade, a, last < hi ? last : hi, stride, false});
	}
}
inline uint32_t base_of(int binade) { return (uint32_t)(binade + 127) << 23; } // 2^binade, binade >= -126
// the three floats below 2^binade (`below`) and that float with the three above it (`above`), each in the row of its own binade
void add_edge(std::vector<Task> &tasks, int kind, int binade, bool below, bool above)
{
	const uint32_t b = base_of(binade);
	if (below) tasks.push_back(Task{kind, binade == -126 ? -127 : binade - 1, (uint64_t)b - 3, (uint64_t)b - 1, 1, false});
	if (above) tasks.push_back(Task{kind, binade, b, (uint64_t)b + 3, 1, false});
}

} // namespace

extern "C" {

struct MahRow
{
	int32_t fn, sign, binade, pad;
	uint64_t n, nonfinite, tiny, broken, compared, differ;
	double ulp, abs, maxres;
	uint64_t ulp_at, abs_at, maxres_at;
};

const int MAH_SAMPLE = 4096;            // sampled floats of a binade that is not swept
const int MAH_SINCOS_LO = -14, MAH_SINCOS_HI = 16, MAH_SINCOS_FAR = 26; // sin, cos: every float of 2^-14 <= |x| < 2^16, strided to 2^26
const long long MAH_PAIRS = 1 << 24;    // atan21's random pairs, pow1's sample

// The sweep.  stride: every stride-th float of the ranges that are otherwise swept whole (1: all of them; odd, so that every
// mantissa bit still varies); far_stride: of sin and cos between 2^16 and 2^26.  -> rows written, or -1 if `cap` is too small.
int mah_run(int threads, int stride, int far_stride, MahRow *rows, int cap)
{
	std::vector<Task> tasks;
	const uint64_t S = (uint64_t)(stride < 1 ? 1 : stride), FS = (uint64_t)(far_stride < 1 ? 1 : far_stride);
	// sin, cos (x >= 0; the sweep itself holds -x to the same bits)
	tasks.push_back(Task{F_SIN, -128, 0, 0, 1, false});
	tasks.push_back(Task{F_SIN, -127, 1, 3, 1, false});
	tasks.push_back(Task{F_SIN, -127, 0x00000004u, 0x00000004u + MAH_SAMPLE - 1, 1, true});
	for (int e = -126; e <= MAH_SINCOS_LO; ++e)
	{
		add_edge(tasks, F_SIN, e, true, e < MAH_SINCOS_LO); // (a float of a swept binade is not taken twice)
		if (e == MAH_SINCOS_LO) break;
		tasks.push_back(Task{F_SIN, e, (uint64_t)base_of(e), (uint64_t)base_of(e) + MAH_SAMPLE - 1, 1, true});
	}
	for (int e = MAH_SINCOS_LO; e < MAH_SINCOS_HI; ++e)
		add_range(tasks, F_SIN, e, base_of(e), (uint64_t)base_of(e) + 0x7fffffu, S);
	for (int e = MAH_SINCOS_HI; e < MAH_SINCOS_FAR; ++e)
	{
		add_edge(tasks, F_SIN, e, e > MAH_SINCOS_HI && FS > 1, false);
		add_range(tasks, F_SIN, e, base_of(e), (uint64_t)base_of(e) + 0x7fffffu, FS);
		if (FS > 1) tasks.push_back(Task{F_SIN, e, (uint64_t)base_of(e) + 1, (uint64_t)base_of(e) + 3, 1, false});
	}
	add_edge(tasks, F_SIN, MAH_SINCOS_FAR, FS > 1, true);
	// atan21(y, 1): every y of [2^-30, 2^30]; random finite pairs
	for (int e = -30; e < 30; ++e)
		add_range(tasks, F_ATAN, e, base_of(e), (uint64_t)base_of(e) + 0x7fffffu, S);
	tasks.push_back(Task{F_ATAN, 30, base_of(30), base_of(30), 1, false});
	add_range(tasks, F_ATAN_PAIRS, 0, 0, (uint64_t)MAH_PAIRS - 1, 1);
	// exp21: every |x| of [2^-24, 150], both signs (the thresholds 128 and -126 and their neighbours lie inside)
	for (int e = -24; e <= 7; ++e)
	{
		const uint64_t top = e == 7 ? (uint64_t)bits_of(150.f) : (uint64_t)base_of(e) + 0x7fffffu;
		add_range(tasks, F_EXP2, e, base_of(e), top, S);
	}
	// log21: every positive float, denormals included
	add_range(tasks, F_LOG2, -127, 1, 0x007fffffu, S);
	for (int e = -126; e <= 127; ++e)
		add_range(tasks, F_LOG2, e, base_of(e), (uint64_t)base_of(e) + 0x7fffffu, S);
	// pow1: the seeded sample
	add_range(tasks, F_POW, 0, 0, (uint64_t)MAH_PAIRS - 1, 1);

	if (threads < 1) threads = 1;
	if (threads > 16) threads = 16;
	std::vector<Acc> accs((size_t)threads);
	std::atomic<size_t> next(0);
	std::vector<std::thread> pool;
	for (int w = 0; w < threads; ++w)
		pool.emplace_back([&, w]() {
			Acc &acc = accs[(size_t)w];
			for (size_t k; (k = next.fetch_add(1)) < tasks.size();)
			{
				const Task &t = tasks[k];
				switch (t.kind)
				{
				case F_SIN: sweep_sincos(acc, t); break;
				case F_ATAN: sweep_atan(acc, t); break;
				case F_ATAN_PAIRS: sweep_atan_pairs(acc, t); break;
				case F_EXP2: sweep_exp2(acc, t); break;
				case F_LOG2: sweep_log2(acc, t); break;
				case F_POW: sweep_pow(acc, t); break;
				}
			}
		});
	for (auto &th : pool)
		th.join();

	int count = 0;
	for (int fn = 0; fn < F_COUNT; ++fn)
		for (int sign = 0; sign < 2; ++sign)
			for (int b = BINADE_MIN; b <= BINADE_MAX; ++b)
			{
				Stat m = Stat();
				for (auto &acc : accs)
				{
					const Stat &s = acc.at(fn, sign, b);
					if (!s.n) continue;
					if (!m.n) { m = s; continue; }
					m.n += s.n, m.nonfinite += s.nonfinite, m.tiny += s.tiny, m.broken += s.broken, m.compared += s.compared, m.differ += s.differ;
					keep_max(s.ulp, s.ulp_at, m.ulp, m.ulp_at);
					keep_max(s.abs, s.abs_at, m.abs, m.abs_at);
					keep_max(s.maxres, s.maxres_at, m.maxres, m.maxres_at);
				}
				if (!m.n) continue;
				if (count >= cap) return -1;
				rows[count++] = MahRow{fn, sign, b, 0, m.n, m.nonfinite, m.tiny, m.broken, m.compared, m.differ, m.ulp, m.abs, m.maxres, m.ulp_at, m.abs_at, m.maxres_at};
			}
	return count;
}

// what = 0 sin1, 1 cos1, 2 atan21(x, y), 3 exp21, 4 log21, 5 pow1(x, y), 6 / 7 sincos1 .x / .y, 8 / 9 sincos1_small .x / .y;
// what + 100: the same function of oracle/detmath.h (0..5)
int mah_eval(int what, long long n, const float *x, const float *y, float *out)
{
	for (long long i = 0; i < n; ++i)
	{
		const float a = x[i], b = y ? y[i] : 0.f;
		switch (what)
		{
		case 0: out[i] = sdfr::sin1(a); break;
		case 1: out[i] = sdfr::cos1(a); break;
		case 2: out[i] = sdfr::atan21(a, b); break;
		case 3: out[i] = sdfr::exp21(a); break;
		case 4: out[i] = sdfr::log21(a); break;
		case 5: out[i] = sdfr::pow1(a, b); break;
		case 6: out[i] = sdfr::sincos1(a).x; break;
		case 7: out[i] = sdfr::sincos1(a).y; break;
		case 8: out[i] = sdfr::sincos1_small(a).x; break;
		case 9: out[i] = sdfr::sincos1_small(a).y; break;
		case 100: out[i] = orc::dm::sinf_det(a); break;
		case 101: out[i] = orc::dm::cosf_det(a); break;
		case 102: out[i] = orc::dm::atan2f_det(a, b); break;
		case 103: out[i] = orc::dm::exp2f_det(a); break;
		case 104: out[i] = orc::dm::log2f_det(a); break;
		case 105: out[i] = orc::dm::powf_det(a, b); break;
		default: return -1;
		}
	}
	return 0;
}

// libm's double value of function `what` (0..5 as above)
int mah_truth(int what, long long n, const float *x, const float *y, double *out)
{
	for (long long i = 0; i < n; ++i)
	{
		const double a = x[i], b = y ? (double)y[i] : 0.0;
		switch (what)
		{
		case 0: out[i] = std::sin(a); break;
		case 1: out[i] = std::cos(a); break;
		case 2: out[i] = std::atan2(a, b); break;
		case 3: out[i] = std::exp2(a); break;
		case 4: out[i] = std::log2(a); break;
		case 5: out[i] = std::pow(a, b); break;
		default: return -1;
		}
	}
	return 0;
}

// items [first, first + n) of the seeded samples: which = 0 atan21's pairs (y, x), 1 pow1's (x, y)
int mah_sample(int which, long long first, long long n, float *a, float *b)
{
	for (long long i = 0; i < n; ++i)
	{
		if (which == 0) atan_pair((uint64_t)(first + i), a[i], b[i]);
		else if (which == 1) pow_pair((uint64_t)(first + i), a[i], b[i]);
		else return -1;
	}
	return 0;
}

} // extern "C"

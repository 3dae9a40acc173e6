// tests/cpp/labyrinth_walls_host.cpp -- TEST-ONLY host build of the labyrinth's wall distance
// (SceneLabyrinth::sd_box_pair_min / walls, sdf_playground_amd/csrc/sdfr_scenes.h) against the
// formula it replaces, min1(sd_box, sd_box), bit for bit.  Loaded by tests/test_labyrinth_walls_cpu.py.
#include "sdfr_scenes.h"

#include <stdint.h>

using namespace sdfr;

namespace {

struct Rng // splitmix64
{
	uint64_t s;
	uint64_t next()
	{
		uint64_t z = (s += 0x9e3779b97f4a7c15ull);
		z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
		z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
		return z ^ (z >> 31);
	}
	float uniform(float lo, float hi) { return lo + (hi - lo) * (float)((next() >> 40) * (1.0 / 16777216.0)); }
	int below(int n) { return (int)(next() % (uint64_t)n); }
};

float nudge(float x, int ulps)
{
	uint32_t u = f32_bits(x);
	if (x == 0.f) return ulps == 0 ? x : bits_f32((uint32_t)(ulps > 0 ? ulps : -ulps) | (ulps < 0 ? 0x80000000u : 0u));
	return bits_f32((uint32_t)((int64_t)u + ((u >> 31) ? -ulps : ulps)));
}

// the walls as they were written before the pair: two sd_box calls and a min1
float walls_before(vec3 wp)
{
	float wall1 = sd_box(wp - V3(3.5f, 2.f, 3.f), V3(1.5f, 2.f, 1.f));
	float wall2 = sd_box(wp - V3(7.f, 2.f, 5.f), V3(3.f, 2.f, 1.f));
	return min1(wall1, wall2);
}

bool same(float a, float b) { return f32_bits(a) == f32_bits(b) || (a != a && b != b); }

// the faces, edges and corners of both walls, the centres, and 0, per axis
const float kX[] = {2.f, 5.f, 4.f, 10.f, 3.5f, 7.f, 0.f};
const float kY[] = {0.f, 4.f, 2.f};
const float kZ[] = {2.f, 4.f, 6.f, 3.f, 5.f, 0.f};

float pick(Rng &r, const float *k, int n, float lo, float hi)
{
	switch (r.below(4))
	{
	case 0: return r.uniform(lo, hi);
	case 1: return k[r.below(n)];
	case 2: return nudge(k[r.below(n)], r.below(7) - 3);
	default: return k[r.below(n)] + (r.below(2) ? 1.f : -1.f) * bits_f32(0x00000001u + (uint32_t)r.below(0x34000000)); // up to ~1e-7 off
	}
}

float component(Rng &r, float b)
{
	// p components on both sides of the box face |p| = b, exactly on it, a few ulps off it, +-0, tiny and huge
	switch (r.below(8))
	{
	case 0: return r.uniform(-3.f * b, 3.f * b);
	case 1: return (r.below(2) ? 1.f : -1.f) * b;
	case 2: return (r.below(2) ? 1.f : -1.f) * nudge(b, r.below(9) - 4);
	case 3: return r.below(2) ? 0.f : -0.f;
	case 4: return (r.below(2) ? 1.f : -1.f) * bits_f32((uint32_t)r.below(0x0c000000)); // denormal to ~1e-31
	case 5: return r.uniform(-b, b) * 1e-3f;
	case 6: return (r.below(2) ? 1.f : -1.f) * r.uniform(1e18f, 3e19f); // squares overflow from 1.8e19 on
	default: return (r.below(2) ? 1.f : -1.f) * (b + r.uniform(-1e-6f, 1e-6f));
	}
}

} // namespace

// every combination of the per-axis face / edge / corner coordinates, each moved by -3 .. +3 ulps; returns the number of
// points checked, mismatches in *bad
extern "C" int64_t walls_grid(int64_t *bad)
{
	int64_t n = 0;
	*bad = 0;
	for (float x : kX)
		for (float y : kY)
			for (float z : kZ)
				for (int dx = -3; dx <= 3; ++dx)
					for (int dy = -3; dy <= 3; ++dy)
						for (int dz = -3; dz <= 3; ++dz)
						{
							const vec3 wp = V3(nudge(x, dx), nudge(y, dy), nudge(z, dz));
							*bad += !same(SceneLabyrinth::walls(wp), walls_before(wp));
							++n;
						}
	return n;
}

// mode 0: walls(wp) against the two sd_box calls at points in and around the folded cell (faces, edges, corners, ulps off them)
// mode 1: sd_box_pair_min of random boxes (overlapping, nested, touching, degenerate) against min1(sd_box, sd_box)
// returns the number of mismatches; the first one's inputs and results go to first[0..7]
extern "C" int64_t walls_check(int mode, uint64_t seed, int64_t n, float *first)
{
	Rng r{seed};
	int64_t bad = 0;
	for (int64_t i = 0; i < n; ++i)
	{
		float got, want;
		vec3 a, b;
		if (mode == 0)
		{
			const bool wide = r.below(8) == 0;
			a = V3(pick(r, kX, 7, wide ? -30.f : -1.f, wide ? 30.f : 11.f), pick(r, kY, 3, wide ? -30.f : -1.f, wide ? 30.f : 5.f),
			       pick(r, kZ, 6, wide ? -30.f : -1.f, wide ? 30.f : 11.f));
			b = a;
			got = SceneLabyrinth::walls(a);
			want = walls_before(a);
		}
		else
		{
			const vec3 b1 = V3(r.uniform(0.f, 4.f), r.uniform(0.f, 4.f), r.uniform(0.f, 4.f));
			const vec3 b2 = r.below(4) == 0 ? b1 : V3(r.uniform(0.f, 4.f), r.uniform(0.f, 4.f), r.uniform(0.f, 4.f));
			a = V3(component(r, b1.x), component(r, b1.y), component(r, b1.z));
			// the second point: independent, or the first one moved a little (both boxes about the same place: nested or overlapping)
			b = r.below(2) ? V3(component(r, b2.x), component(r, b2.y), component(r, b2.z))
			               : a + V3(r.uniform(-0.5f, 0.5f), r.uniform(-0.5f, 0.5f), r.uniform(-0.5f, 0.5f)) * (float)r.below(2);
			got = SceneLabyrinth::sd_box_pair_min(a, b1, b, b2);
			want = min1(sd_box(a, b1), sd_box(b, b2));
		}
		if (!same(got, want))
		{
			if (bad == 0 && first)
			{
				const float v[8] = {a.x, a.y, a.z, b.x, b.y, b.z, got, want};
				for (int k = 0; k < 8; ++k) first[k] = v[k];
			}
			++bad;
		}
	}
	return bad;
}

// tests/cpp/labyrinth_shed_host.cpp -- TEST-ONLY host build of two exact rewrites that spare the labyrinth's pixel kernel work
// (sdf_playground_amd/csrc/sdfr_scenes.h): the walls with sums for clamps (SceneLabyrinth::sd_box_pair_min_adds) against the form with
// max1, written out here as it stood, and against the two sd_box calls; and the sun's direction as prepare() stores it against the
// light loop's own expression.  Loaded by tests/test_labyrinth_clamp_cpu.py and tests/test_labyrinth_shed_cpu.py.
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

bool same(float a, float b) { return f32_bits(a) == f32_bits(b); }

// the pair as it was written before the sums: the clamps with max1, the root added to the inside term
float pair_before(vec3 p1, vec3 b1, vec3 p2, vec3 b2)
{
	const vec3 q1 = abs(p1) - b1, q2 = abs(p2) - b2;
	const vec3 o1 = max(q1, 0.f), o2 = max(q2, 0.f);
	const float in = min1(min1(max1(q1.x, max1(q1.y, q1.z)), max1(q2.x, max1(q2.y, q2.z))), 0.f);
	return sqrt1(min1(dot(o2, o2), dot(o1, o1))) + in;
}
const vec3 kC1 = V3(3.5f, 2.f, 3.f), kB1 = V3(1.5f, 2.f, 1.f), kC2 = V3(7.f, 2.f, 5.f), kB2 = V3(3.f, 2.f, 1.f);
float walls_before(vec3 wp) { return pair_before(wp - kC1, kB1, wp - kC2, kB2); }
float walls_two_boxes(vec3 wp) { return min1(sd_box(wp - kC1, kB1), sd_box(wp - kC2, kB2)); }

// the faces of both walls per axis (a point with such a coordinate has q = +-0 in that component of one wall), and the centres
const float kX[] = {2.f, 5.f, 4.f, 10.f, 3.5f, 7.f};
const float kY[] = {0.f, 4.f, 2.f};
const float kZ[] = {2.f, 4.f, 6.f, 3.f, 5.f};

} // namespace

// the sun's direction as prepare() stores it and as the light loop formed it per hit
extern "C" void sun_dirs(float dist_eps, float *stored, float *formed)
{
	FrameU U{};
	U.dist_eps = dist_eps;
	SceneLabyrinth::prepare(U);
	const vec3 s = SceneLabyrinth::frame_sun_dir(U);
	Light L;
	sun_light(0, L);
	const vec3 f = L.pos / (length(L.pos) + U.dist_eps);
	stored[0] = s.x, stored[1] = s.y, stored[2] = s.z;
	formed[0] = f.x, formed[1] = f.y, formed[2] = f.z;
}

// the walls at one point of the folded cell: with sums, with max1, as two boxes
extern "C" void clamp_at(const float *wp, float *out)
{
	const vec3 p = V3(wp[0], wp[1], wp[2]);
	out[0] = SceneLabyrinth::walls(p);
	out[1] = walls_before(p);
	out[2] = walls_two_boxes(p);
}

// mode 0: uniform points of the folded cell and a little around it
// mode 1: every coordinate on a face of a wall or a centre, moved by up to 3 ulps, or uniform: faces, edges, corners, q = +-0
// mode 2: points inside wall 1 and inside wall 2
// mode 3: |y| up to 1e6, x and z in the cell
// returns the number of points where the three forms do not agree bit for bit; the first one goes to first[0..5]
extern "C" int64_t clamp_check(int mode, uint64_t seed, int64_t n, float *first)
{
	Rng r{seed};
	int64_t bad = 0;
	for (int64_t i = 0; i < n; ++i)
	{
		vec3 p;
		if (mode == 0)
			p = V3(r.uniform(-0.5f, 10.5f), r.uniform(-1.f, 5.f), r.uniform(-0.5f, 10.5f));
		else if (mode == 1)
		{
			auto pick = [&](const float *k, int nk, float lo, float hi) {
				switch (r.below(4))
				{
				case 0: return r.uniform(lo, hi);
				case 1: return k[r.below(nk)];
				default: return nudge(k[r.below(nk)], r.below(7) - 3);
				}
			};
			p = V3(pick(kX, 6, 0.f, 10.f), pick(kY, 3, -1.f, 5.f), pick(kZ, 5, 0.f, 10.f));
			if (r.below(16) == 0) p.y = r.below(2) ? 0.f : -0.f; // (q.y = |+-0 - 2| - 2 = +0; the y = 4 face gives the same)
		}
		else if (mode == 2)
		{
			const bool second = r.below(2) != 0;
			const vec3 c = second ? kC2 : kC1, b = second ? kB2 : kB1;
			p = c + V3(r.uniform(-b.x, b.x), r.uniform(-b.y, b.y), r.uniform(-b.z, b.z));
		}
		else
		{
			const float mag = bits_f32(0x3f800000u + (uint32_t)r.below(20 << 23) + (uint32_t)r.below(1 << 23)); // 1 .. 2^20 > 1e6, every exponent alike
			p = V3(r.uniform(0.f, 10.f), (r.below(2) ? 1.f : -1.f) * (mag > 1e6f ? 1e6f : mag), r.uniform(0.f, 10.f));
		}
		const float now = SceneLabyrinth::walls(p), before = walls_before(p), boxes = walls_two_boxes(p);
		if (!same(now, before) || !same(now, boxes))
		{
			if (bad == 0 && first)
			{
				const float v[6] = {p.x, p.y, p.z, now, before, boxes};
				for (int k = 0; k < 6; ++k) first[k] = v[k];
			}
			++bad;
		}
	}
	return bad;
}

// every combination of the per-axis faces and centres, each moved by -3 .. +3 ulps: returns the points checked, mismatches in *bad;
// *inside counts the points with a negative distance and *zero_q those exactly on a face (so that neither kind is absent)
extern "C" int64_t clamp_grid(int64_t *bad, int64_t *inside, int64_t *on_face)
{
	int64_t n = 0;
	*bad = *inside = *on_face = 0;
	for (float x : kX)
		for (float y : kY)
			for (float z : kZ)
				for (int dx = -3; dx <= 3; ++dx)
					for (int dy = -3; dy <= 3; ++dy)
						for (int dz = -3; dz <= 3; ++dz)
						{
							const vec3 p = V3(nudge(x, dx), nudge(y, dy), nudge(z, dz));
							const float now = SceneLabyrinth::walls(p);
							*bad += !same(now, walls_before(p)) || !same(now, walls_two_boxes(p));
							*inside += now < 0.f;
							*on_face += now == 0.f;
							++n;
						}
	return n;
}

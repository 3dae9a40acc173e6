// tests/cpp/labyrinth_step_host.cpp -- TEST-ONLY host build of the labyrinth's march step (SceneLabyrinth::fold and floor_dist,
// sdf_playground_amd/csrc/sdfr_scenes.h) beside the formulas they replace, written out here as they stood: the repetition
// x - 20 * floor(x / 20) - 10, the compare-and-swap of the two absolute values, and the floor's height as the three-term dot
// with (0, 1, 0).  Loaded by tests/test_labyrinth_step_cpu.py, which makes the points and compares the bits.
#include "sdfr_scenes.h"

#include <stdint.h>

using namespace sdfr;

namespace {

float rep_before(float p)
{
	float x = p + 20.f * 0.5f;
	return x - 20.f * floor1(div_c(x, 20.f, 1.0f / 20.f)) - 20.f * 0.5f;
}

vec3 fold_before(vec3 p)
{
	float wx = abs1(rep_before(p.x)), wz = abs1(rep_before(p.z));
	if (wz > wx) { float t = wx; wx = wz; wz = t; }
	return V3(wx, p.y, wz);
}

float floor_before(vec3 p, bool fast, const GroundInv &g)
{
	float d = (0.f * p.x + 1.f * p.y) + 0.f * p.z;
	return fast ? div_c(d, g.denom, g.rdenom) : d;
}

} // namespace

// n points (x, y, z): the fold as it is and as it was
extern "C" void step_fold(int64_t n, const float *p, float *now, float *before)
{
	for (int64_t i = 0; i < n; ++i)
	{
		const vec3 q = V3(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
		const vec3 a = SceneLabyrinth::fold(q), b = fold_before(q);
		now[3 * i] = a.x, now[3 * i + 1] = a.y, now[3 * i + 2] = a.z;
		before[3 * i] = b.x, before[3 * i + 1] = b.y, before[3 * i + 2] = b.z;
	}
}

// one coordinate's repetition alone (the domain's edge)
extern "C" void step_rep(int64_t n, const float *x, float *now, float *before)
{
	for (int64_t i = 0; i < n; ++i)
	{
		now[i] = SceneLabyrinth::rep20(x[i]);
		before[i] = rep_before(x[i]);
	}
}

// n points and ray directions: the floor's distance as it is, as it was, and the shared ground_dist (sdfr_lib.h) the other scenes keep
extern "C" void step_floor(int64_t n, const float *p, const float *dir, int fast, float *now, float *before, float *shared)
{
	for (int64_t i = 0; i < n; ++i)
	{
		const vec3 q = V3(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
		const GroundInv g = ground_setup(V3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]));
		now[i] = SceneLabyrinth::floor_dist(q, fast != 0, g);
		before[i] = floor_before(q, fast != 0, g);
		shared[i] = ground_dist(q, fast != 0, g);
	}
}

// the whole distance at n points with the floor as it is (SceneLabyrinth::dist)
extern "C" void step_dist(int64_t n, const float *p, const float *dir, int fast, float *out)
{
	FrameU U{};
	U.dist_eps = 0.0001f;
	for (int64_t i = 0; i < n; ++i)
	{
		const vec3 d = V3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
		RayFlags f{};
		const SceneLabyrinth::RayInv R = SceneLabyrinth::ray_setup(U, d, f);
		out[i] = SceneLabyrinth::dist(U, R, V3(p[3 * i], p[3 * i + 1], p[3 * i + 2]), d, fast != 0);
	}
}

// tests/cpp/labyrinth_range_clear.cpp -- TEST-ONLY stand-alone host program: SceneLabyrinth::ray_bounds (sdf_playground_amd/csrc/sdfr_scenes.h;
// RayBounds, sdfr_scene_traits.h) against a dense walk.  The rule lets a descending ray that is still above the wall tops where its range ends
// count as rising, so that ray_escapes ends it before its first evaluation; here, wherever the rule sets the flag on a descending ray,
// every sample from t = 0 to t = range must have march_pos' height above 4.01 (what ray_escapes tests) and the scene at least 0.002 away
// (twice the largest dist_eps the library accepts), evaluated as the march evaluates it (fast = true).
//   labyrinth_range_clear <rays> <seed>    prints one line of counts and the edge cases' verdicts; exit status 0 only if nothing is violated
// Run by tests/test_labyrinth_range_clear_cpu.py.
#include "sdfr_pixel.h"
#include "sdfr_scenes.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

using namespace sdfr;

static_assert(RayBounds<SceneLabyrinth>::value, "the labyrinth declares ray_bounds");
static_assert(!RayBounds<SceneCubeSea>::value && !RayBounds<SceneFastSphere>::value, "a scene without the member gets the no-op");
static_assert(!EscapesFrom<SceneLabyrinth>::value, "the rule is not an escapes_from: nothing per step");

namespace {

unsigned long long state;
float rnd()
{
	state = state * 6364136223846793005ull + 1442695040888963407ull;
	return (float)((state >> 40) & 0xffffff) / 16777216.f;
}

RayFlags plain_flags()
{
	RayFlags f;
	f.has_transparent = false;
	f.is_shadow = false;
	f.last_transparent_pos = V3s(0.f);
	return f;
}

// the flag as render_pixel forms it: ray_setup, then ray_bounds through the trait
SceneLabyrinth::RayInv setup(const FrameU &U, vec3 s, vec3 d, float range)
{
	SceneLabyrinth::RayInv R = SceneLabyrinth::ray_setup(U, d, plain_flags());
	RayBounds<SceneLabyrinth>::apply(U, R, s, d, range);
	return R;
}

// one sample of the walk: what ray_escapes sees there, and the scene's distance; false = violated
bool sample_ok(const FrameU &U, const SceneLabyrinth::RayInv &R, vec3 s, vec3 d, float t)
{
	const vec3 p = mad(d, t, s); // march_pos
	if (!SceneLabyrinth::ray_escapes(U, R, p, d)) return false;
	return SceneLabyrinth::dist(U, R, p, d, true) >= 0.002f;
}

// t from 0 to range: about 600 random steps, the last 2 % of the range (where a descending ray is lowest) in 100 more, and t = range itself
bool walk_ok(const FrameU &U, const SceneLabyrinth::RayInv &R, vec3 s, vec3 d, float range, float *where)
{
	const float coarse = range / 600.f, fine = range / 5000.f;
	float t = 0.f;
	while (t < range)
	{
		if (!sample_ok(U, R, s, d, t)) { *where = t; return false; }
		t += (t < 0.98f * range ? coarse : fine) * (0.5f + rnd());
	}
	*where = range;
	return sample_ok(U, R, s, d, range);
}

} // namespace

int main(int argc, char **argv)
{
	const long long n = argc > 1 ? atoll(argv[1]) : 200000;
	const unsigned seed = argc > 2 ? (unsigned)atoll(argv[2]) : 1u;
	state = seed * 2654435761ull + 4242ull;
	FrameU U{};
	U.dist_eps = 0.0001f;

	long long descending = 0, fired = 0, bad = 0, rising_changed = 0;
	for (long long i = 0; i < n; ++i)
	{
		const float span = (i % 3 == 0) ? 45.f : ((i % 3 == 1) ? 8.f : 2.5f);
		const vec3 s = V3((rnd() * 2.f - 1.f) * span, 4.f + rnd() * ((i % 4 == 0) ? 0.05f : ((i % 4 == 1) ? 3.f : 56.f)), (rnd() * 2.f - 1.f) * span);
		// |dir.y| from 1e-6 to 1, evenly in its logarithm; three in four descend
		const float ay = expf(-rnd() * 13.8155f);
		const float dy = (i % 4 == 3) ? ay : -ay;
		const float phi = rnd() * 6.2831853f, h = sqrtf(fmaxf(0.f, 1.f - dy * dy));
		const vec3 d = V3(h * cosf(phi), dy, h * sinf(phi)) * (1.f - ((i & 1) ? rnd() * 6e-4f : 0.f)); // up to 6e-4 short of a unit vector
		const float range = 0.5f * expf(rnd() * 7.6009f); // 0.5 to 1000
		const SceneLabyrinth::RayInv before = SceneLabyrinth::ray_setup(U, d, plain_flags());
		const SceneLabyrinth::RayInv R = setup(U, s, d, range);
		if (!(d.y < 0.f))
		{
			if (R.rising != before.rising) ++rising_changed; // a ray that does not descend keeps what ray_setup said
			continue;
		}
		++descending;
		if (!R.rising) continue;
		++fired;
		float t;
		if (!walk_ok(U, R, s, d, range, &t))
		{
			if (bad == 0) printf("witness start %.9g %.9g %.9g dir %.9g %.9g %.9g range %.9g t %.9g\n", s.x, s.y, s.z, d.x, d.y, d.z, range, t);
			++bad;
		}
	}

	// Edge cases.  dir.y = -0.25 and range = 8 make the product -2 exactly, and v + 2 is a float for v next to 4.01f (one ulp, 2^-21, up to 8):
	// fma1(dir.y, range, start.y) is v itself.
	int edge_bad = 0;
	const float top = 4.01f, above = nextafterf(top, 8.f), below = nextafterf(top, 0.f);
	const vec3 d = V3(0.96824584f, -0.25f, 0.f);
	const float v[3] = {above, top, below};
	const bool want[3] = {true, false, false}; // the comparison is strict
	for (int k = 0; k < 3; ++k)
	{
		const vec3 s = V3(1.f, v[k] + 2.f, 1.f);
		if (fma1(d.y, 8.f, s.y) != v[k]) ++edge_bad;
		const SceneLabyrinth::RayInv R = setup(U, s, d, 8.f);
		if (R.rising != want[k]) ++edge_bad;
		float t;
		if (R.rising && !walk_ok(U, R, s, d, 8.f, &t)) ++edge_bad;
	}
	// dir.y = -0 is rising already (ray_setup: -0 >= 0), whatever the start; the rule leaves it
	{
		const vec3 s = V3(1.f, 2.f, 1.f), dz = V3(1.f, -0.f, 0.f);
		if (!SceneLabyrinth::ray_setup(U, dz, plain_flags()).rising || !setup(U, s, dz, 100.f).rising) ++edge_bad;
	}
	// a NaN in any operand fails the comparison: the flag stays off
	{
		const float q = nanf("");
		if (setup(U, V3(1.f, 50.f, 1.f), V3(0.9f, q, 0.f), 10.f).rising) ++edge_bad;
		if (setup(U, V3(1.f, q, 1.f), V3(0.9f, -0.1f, 0.f), 10.f).rising) ++edge_bad;
		if (setup(U, V3(1.f, 50.f, 1.f), V3(0.9f, -0.1f, 0.f), q).rising) ++edge_bad;
		// and in a component the rule does not read, it decides as without it
		if (!setup(U, V3(q, 50.f, 1.f), V3(q, -0.1f, q), 10.f).rising) ++edge_bad;
	}
	// an infinite range ends every descending ray below the tops; a negative one asks about nothing behind the start
	if (setup(U, V3(1.f, 50.f, 1.f), V3(0.9f, -1e-6f, 0.f), INFINITY).rising) ++edge_bad;

	printf("rays %lld descending %lld fired %lld violations %lld rising_changed %lld edge_violations %d\n", n, descending, fired, bad, rising_changed, edge_bad);
	return (bad == 0 && rising_changed == 0 && edge_bad == 0) ? 0 : 1;
}

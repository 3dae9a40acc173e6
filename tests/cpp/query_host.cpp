// tests/cpp/query_host.cpp -- TEST-ONLY: the library's scene queries (sdf_playground_amd/csrc/sdfr_query.h) compiled for the CPU,
// as tests/hostsim compiles the per-pixel pipeline, so that the CPU test tier can compare them with the oracle's definitions
// (query_oracle.h) bit for bit without a GPU.  Built once for the scenes compiled ahead of time, and once per run-time scene with
// -DSDFR_HLSL_SCENE_FILE="<generated file>" (host_common.h).  The product never loads this.
#include "sdfr_hostframe.h"
#include "sdfr_query.h"
#include "host_common.h"

namespace {

struct Fns
{
	void (*points)(const FrameU &, int, const float *, float *, float *);
	void (*rays)(const FrameU &, int, const float *, const float *, float, uint32_t *);
	void (*pick)(const FrameU &, int, const int32_t *, uint32_t *);
};

template <class Scene, bool DBG>
void points_of(const FrameU &U, int n, const float *p, float *d, float *nrm)
{
	for (int i = 0; i < n; ++i)
	{
		vec3 nv;
		d[i] = query_point<Scene, DBG>(U, V3(p[3 * i], p[3 * i + 1], p[3 * i + 2]), nrm ? &nv : nullptr);
		if (nrm)
		{
			nrm[3 * i] = nv.x;
			nrm[3 * i + 1] = nv.y;
			nrm[3 * i + 2] = nv.z;
		}
	}
}
template <class Scene, bool DBG>
void rays_of(const FrameU &U, int n, const float *o, const float *d, float dist_max, uint32_t *hits)
{
	for (int i = 0; i < n; ++i)
		query_ray<Scene, DBG>(U, V3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), V3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), dist_max, V3s(0.f), V3s(0.f),
			hits + QUERY_HIT_WORDS * i);
}
template <class Scene, bool DBG>
void pick_of(const FrameU &U, int n, const int32_t *px, uint32_t *hits)
{
	for (int i = 0; i < n; ++i) query_pick<Scene, DBG>(U, px[2 * i], px[2 * i + 1], hits + QUERY_HIT_WORDS * i);
}
// the family's function for a scene and a frame, the debug or the plain instantiation: what latch hands out
struct Pick
{
	template <class Scene>
	static Fns of(const FrameU &U)
	{
		if (frame_needs_debug(U)) return Fns{&points_of<Scene, true>, &rays_of<Scene, true>, &pick_of<Scene, true>};
		return Fns{&points_of<Scene, false>, &rays_of<Scene, false>, &pick_of<Scene, false>};
	}
};

} // namespace

extern "C" {

// `frame`: the inputs of a FrameU (tests/hostsim frame_from_oracle); width and height are set here as the library sets them
int qh_points(const char *scene, const FrameU *frame, int n, const float *points, float *distance, float *normals)
{
	FrameU U;
	Fns f;
	if (!latch<Pick>(scene, frame, U, f)) return -1;
	parallel_items(n, 256, [&](int a, int b) { f.points(U, b - a, points + 3 * a, distance + a, normals ? normals + 3 * a : nullptr); });
	return 0;
}
int qh_rays(const char *scene, const FrameU *frame, int n, const float *origins, const float *dirs, float max_distance, uint32_t *hits)
{
	FrameU U;
	Fns f;
	if (!latch<Pick>(scene, frame, U, f)) return -1;
	const float dist_max = max_distance == 0.f ? U.range : max_distance;
	parallel_items(n, 256, [&](int a, int b) { f.rays(U, b - a, origins + 3 * a, dirs + 3 * a, dist_max, hits + QUERY_HIT_WORDS * a); });
	return 0;
}
int qh_pick(const char *scene, const FrameU *frame, int width, int height, int n, const int32_t *pixels, uint32_t *hits)
{
	FrameU U;
	Fns f;
	if (!latch<Pick>(scene, frame, U, f, width, height)) return -1;
	parallel_items(n, 256, [&](int a, int b) { f.pick(U, b - a, pixels + 2 * a, hits + QUERY_HIT_WORDS * a); });
	return 0;
}
int qh_frame_size() { return (int)sizeof(FrameU); }

} // extern "C"

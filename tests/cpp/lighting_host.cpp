// tests/cpp/lighting_host.cpp -- TEST-ONLY: the library's lighting queries (sdf_playground_amd/csrc/sdfr_lighting.h) compiled for the
// CPU, as surface_host.cpp compiles the surface queries, so that the CPU test tier can compare them with the oracle's definition
// (lighting_oracle.h) bit for bit without a GPU.  Built once for the scenes compiled ahead of time, and once per run-time scene
// with -DSDFR_HLSL_SCENE_FILE="<generated file>".  The product never loads this.
#include "sdfr_hostframe.h"
#include "sdfr_lighting.h"
#include "host_common.h"

namespace {

typedef void (*ItemFn)(const FrameU &, const Item &, uint32_t *, uint32_t *, uint32_t *);

// where an item's eight light samples go, as the kernel's LightSampleStore: nowhere if they are not wanted
struct HostSamples
{
	uint32_t *item;
	bool wanted() const { return item != nullptr; }
	void operator()(int slot, const uint32_t (&s)[QUERY_LIGHT_SAMPLE_WORDS]) const { memcpy(item + QUERY_LIGHT_SAMPLE_WORDS * slot, s, sizeof s); }
};

template <class Scene, bool DBG>
void item_of(const FrameU &U, const Item &it, uint32_t *hit, uint32_t *rec, uint32_t *samples)
{
	QueryRay ray;
	const bool in_frame = item_ray(U, it, ray);
	query_lighting<Scene, DBG>(U, ray, in_frame, hit, rec, HostSamples{samples});
}
// the family's function for a scene and a frame, the debug or the plain instantiation: what latch hands out
struct Pick
{
	template <class Scene>
	static ItemFn of(const FrameU &U)
	{
		return frame_needs_debug(U) ? &item_of<Scene, true> : &item_of<Scene, false>;
	}
};

// item i's eight samples in `lights`, which may be null
uint32_t *samples_of(uint32_t *lights, int i) { return lights ? lights + (size_t)QUERY_LIGHT_SLOTS * QUERY_LIGHT_SAMPLE_WORDS * i : nullptr; }

} // namespace

extern "C" {

// `frame`: the inputs of a FrameU (tests/hostsim frame_from_oracle); width and height are set as the library sets them (latch).
// lights may be null.  mesh = 0: rays a -> b, max_distance `reach` (0: the range); mesh = 1: the rays towards vertices a with normals b from `reach` outside
int lh_rays(const char *scene, const FrameU *frame, int mesh, int n, const float *a, const float *b, float reach, uint32_t *hits, uint32_t *lighting, uint32_t *lights)
{
	FrameU U;
	ItemFn f;
	if (!latch<Pick>(scene, frame, U, f)) return -1;
	ray_items(U, mesh, n, a, b, reach,
		[&](const Item &it, int i) { f(U, it, hits + QUERY_HIT_WORDS * i, lighting + QUERY_LIGHTING_WORDS * i, samples_of(lights, i)); });
	return 0;
}
int lh_pick(const char *scene, const FrameU *frame, int width, int height, int n, const int32_t *pixels, uint32_t *hits, uint32_t *lighting, uint32_t *lights)
{
	FrameU U;
	ItemFn f;
	if (!latch<Pick>(scene, frame, U, f, width, height)) return -1;
	pick_items(n, pixels, [&](const Item &it, int i) { f(U, it, hits + QUERY_HIT_WORDS * i, lighting + QUERY_LIGHTING_WORDS * i, samples_of(lights, i)); });
	return 0;
}
int lh_frame_size() { return (int)sizeof(FrameU); }

} // extern "C"

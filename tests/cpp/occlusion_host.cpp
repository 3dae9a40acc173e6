// tests/cpp/occlusion_host.cpp -- TEST-ONLY: the library's occlusion queries (sdf_playground_amd/csrc/sdfr_occlusion.h) compiled for
// the CPU, as surface_host.cpp compiles the surface queries, so that the CPU test tier can compare them with the oracle's definition
// (occlusion_oracle.h) bit for bit without a GPU.  An item is done as the kernel's wave does it: the validity test, then lane k's
// ray for k = 0..63, the hit flags gathered into the mask (the kernel's ballot).  Built once for the scenes compiled ahead of time,
// and once per run-time scene with -DSDFR_HLSL_SCENE_FILE="<generated file>".  The product never loads this.
#include "sdfr_hostframe.h"
#include "sdfr_occlusion.h"
#include "host_common.h"

namespace {

typedef void (*ItemFn)(const FrameU &, vec3, vec3, uint32_t, float, float, uint32_t *);

// `valid`: 1 for a point with a normal, occlusion_hit_valid of a hit record's word
template <class Scene, bool DBG>
void item_of(const FrameU &U, vec3 p, vec3 n, uint32_t valid, float bias, float radius, uint32_t *rec)
{
	if (valid == 1u && !occlusion_item_ok(p, n)) valid = 0u;
	if (valid != 1u)
	{
		occlusion_none(valid, rec);
		return;
	}
	uint64_t mask = 0;
	uint32_t count = 0;
	for (uint32_t lane = 0; lane < OCCLUSION_DIRS; ++lane)
		if (occlusion_ray_hits<Scene, DBG>(U, p, n, bias, radius, lane))
		{
			mask |= (uint64_t)1 << lane;
			++count;
		}
	occlusion_record(mask, count, rec);
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

} // namespace

extern "C" {

// `frame`: the inputs of a FrameU (tests/hostsim frame_from_oracle); width and height are set as the library sets them (latch).
// hits = null: items points[i], normals[i]; else the hit records [n][12]
int oh_occlusion(const char *scene, const FrameU *frame, int n, const float *points, const float *normals, const uint32_t *hits, float bias, float radius,
	uint32_t *out)
{
	FrameU U;
	ItemFn f;
	if (!latch<Pick>(scene, frame, U, f)) return -1;
	parallel_items(n, 8, [&](int lo, int hi) {
		for (int i = lo; i < hi; ++i)
		{
			if (hits)
			{
				const uint32_t *h = hits + QUERY_HIT_WORDS * i;
				f(U, V3(bits_f32(h[2]), bits_f32(h[3]), bits_f32(h[4])), V3(bits_f32(h[5]), bits_f32(h[6]), bits_f32(h[7])), occlusion_hit_valid(h[10]), bias, radius,
					out + QUERY_OCCLUSION_WORDS * i);
			}
			else
				f(U, V3(points[3 * i], points[3 * i + 1], points[3 * i + 2]), V3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]), 1u, bias, radius,
					out + QUERY_OCCLUSION_WORDS * i);
		}
	});
	return 0;
}
void oh_directions(float *out) { memcpy(out, k_occlusion_dirs, sizeof k_occlusion_dirs); }
int oh_frame_size() { return (int)sizeof(FrameU); }

} // extern "C"

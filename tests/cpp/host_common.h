// tests/cpp/host_common.h -- TEST-ONLY: what the CPU stand-ins of the query families (query_host.cpp, surface_host.cpp, lighting_host.cpp,
// occlusion_host.cpp, atlas_host.cpp) share: the run-time scene, the threads, the frame as the library latches it for a query, and
// the item -> ray mapping of the surface and lighting kernels.  A stand-in includes its family's header first, then this, and keeps
// what is its own: the per-item function, its entry points and its *_frame_size().  The product never includes this.
#pragma once
#include "sdfr_hostframe.h"
#include "sdfr_surface.h"
// a run-time scene: the build defines SDFR_HLSL_SCENE_FILE="<generated file>" (tests/cppbuild.py: scene_include), which holds `Scene`
#ifdef SDFR_HLSL_SCENE_FILE
#include "sdfr_hlsl.h"
namespace sdfr {
#include SDFR_HLSL_SCENE_FILE
} // namespace sdfr
#endif

#include <cstring>
#include <thread>
#include <vector>

using namespace sdfr;

namespace {

// fn(a, b) for [0, n) in contiguous chunks over up to 16 threads; one thread below `serial_below` items
template <class F>
void parallel_items(int n, int serial_below, F fn)
{
	int t = (int)std::thread::hardware_concurrency();
	t = t < 1 ? 1 : (t > 16 ? 16 : t);
	if (n < serial_below) t = 1;
	std::vector<std::thread> pool;
	const int chunk = (n + t - 1) / t;
	for (int k = 0; k < t; ++k)
	{
		const int a = k * chunk, b = a + chunk < n ? a + chunk : n;
		if (a >= b) break;
		pool.emplace_back([=]() { fn(a, b); });
	}
	for (auto &th : pool) th.join();
}

// U = the caller's frame as the library latches it for a query (latch_into, sdfr_api.cpp) and f = Pick::of<Scene>(U), the family's
// function for that scene and frame; false: no such scene.  width x height: the frame of the pixel kinds, 1 x 1 for every other kind.
template <class Pick, class Fn>
bool latch(const char *scene, const FrameU *frame, FrameU &U, Fn &f, int width = 1, int height = 1)
{
	U = *frame;
	U.width = width;
	U.height = height;
#ifdef SDFR_HLSL_SCENE_FILE
	(void)scene;
	frame_derive(U, -1);
#ifdef SDFR_SCENE_HAS_PREPARE
	Scene::prepare(U);
#endif
	f = Pick::template of<Scene>(U);
	return true;
#else
	const int si = scene_index(scene);
	if (si < 0) return false;
	frame_derive(U, si);
	switch (si)
	{
#define SDFR_FN(I, S) case I: f = Pick::template of<S>(U); return true;
		SDFR_FOR_EACH_SCENE(SDFR_FN)
#undef SDFR_FN
	}
	return false;
#endif
}

// one item of a kind (QUERY_RAYS, QUERY_MESH: a = origin / position, b = dir / normal; QUERY_PICK: px, py), as the kernel's lane does it
struct Item
{
	int kind;
	const float *a, *b;
	int px, py;
	float dist_max, reach;
};

// fn(item, i) for the n items of sh_rays / lh_rays.  mesh = 0: rays a -> b of max_distance `reach` (0: the range); mesh = 1: the rays
// towards vertices a with normals b from `reach` outside
template <class F>
void ray_items(const FrameU &U, int mesh, int n, const float *a, const float *b, float reach, F fn)
{
	Item it = {};
	it.kind = mesh ? QUERY_MESH : QUERY_RAYS;
	it.dist_max = reach == 0.f ? U.range : reach; // (a mesh's rays: 2 * reach, query_mesh_ray)
	it.reach = reach;
	parallel_items(n, 256, [&](int lo, int hi) {
		Item mine = it;
		for (int i = lo; i < hi; ++i)
		{
			mine.a = a + 3 * i;
			mine.b = b + 3 * i;
			fn(mine, i);
		}
	});
}
// fn(item, i) for the n pixels of sh_pick / lh_pick
template <class F>
void pick_items(int n, const int32_t *pixels, F fn)
{
	parallel_items(n, 256, [&](int lo, int hi) {
		Item mine = {};
		mine.kind = QUERY_PICK;
		for (int i = lo; i < hi; ++i)
		{
			mine.px = pixels[2 * i];
			mine.py = pixels[2 * i + 1];
			fn(mine, i);
		}
	});
}

// the item's ray as the surface and lighting kernels map it (sdfr_query_kernel.h, which repeats these lines per kernel on purpose);
// false: a pixel outside the frame
inline bool item_ray(const FrameU &U, const Item &it, QueryRay &ray)
{
	if (it.kind == QUERY_PICK) return query_pixel_ray(U, it.px, it.py, ray);
	if (it.kind == QUERY_MESH)
		ray = query_mesh_ray(V3(it.a[0], it.a[1], it.a[2]), V3(it.b[0], it.b[1], it.b[2]), it.reach);
	else
		ray = query_plain_ray(V3(it.a[0], it.a[1], it.a[2]), V3(it.b[0], it.b[1], it.b[2]), it.dist_max);
	return true;
}

} // namespace

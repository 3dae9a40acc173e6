// tests/cpp/record_oracle.h -- TEST-ONLY: what the record oracles (query_oracle.h, surface_oracle.h, lighting_oracle.h,
// occlusion_oracle.h; one library, record_oracle.cpp) share: the frame (oracle/frame_abi.h), the threads, the table of scenes, and the
// hit record of include/sdfr.h (sdfr_hit) written from one turn of the driver (oracle/driver.h: ray_turn).  Every line of the driver
// they need is a step of driver.h, called; none is restated here.
#pragma once
#include "driver.h"
#include "frame_abi.h"
#include "scene_list.h"

#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

using namespace orc;

namespace {

// items [0, n) over up to 16 threads, in contiguous chunks
template <class F>
void parallel_items(int n, F fn)
{
	int t = (int)std::thread::hardware_concurrency();
	t = t < 1 ? 1 : (t > 16 ? 16 : t);
	if (n < 256) t = 1;
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

uint32_t bits(float f)
{
	uint32_t u;
	memcpy(&u, &f, 4);
	return u;
}

void put3(uint32_t *rec, float3 v)
{
	rec[0] = bits(val(v.x));
	rec[1] = bits(val(v.y));
	rec[2] = bits(val(v.z));
}

enum { HIT_WORDS = 12 };

// The turn of a primary-shaped ray (driver.h: camera_ray) over dist_max, and its hit record.  -> whether the scene was hit
template <class Scene>
bool primary_turn(const Frame &F, const Ray &ray, real dist_max, float3 right_off, float3 bottom_off, Turn &turn, uint32_t *hit)
{
	PixelStats st = {0, 0, 0};
	const bool scene_hit = ray_turn<Scene>(F, ray, right_off, bottom_off, dist_max, turn, st);
	hit[0] = bits(val(turn.geometry_input.camera_distance));
	hit[1] = bits(val(turn.scene_distance));
	put3(hit + 2, mad(ray.dir, turn.geometry_input.camera_distance, ray.pos));
	put3(hit + 5, scene_hit ? turn.normal_output.normal : float3(real(0.f)));
	hit[8] = turn.iter_count;
	hit[9] = scene_hit ? (uint32_t)turn.material_output.material_id : 0u;
	hit[10] = scene_hit ? 1u : 0u;
	hit[11] = 0u;
	return scene_hit;
}

// a pick outside the frame: no ray, and the hit record that says so
bool outside_frame(const Frame &F, int px, int py, uint32_t *hit)
{
	if (px >= 0 && py >= 0 && px < F.width && py < F.height) return false;
	for (int k = 0; k < HIT_WORDS; ++k) hit[k] = 0u;
	hit[10] = 0xffffffffu;
	return true;
}

// one scene's queries; the table (record_oracle.cpp) is generated from scene_list.h
struct Entry
{
	const char *name;
	void (*points)(const Frame &, const float *, float *, float *);
	void (*rays)(const Frame &, float3, float3, real, float3, float3, uint32_t *);
	void (*pick)(const Frame &, int, int, uint32_t *);
	void (*surface_rays)(const Frame &, float3, float3, real, float3, float3, uint32_t *, uint32_t *);
	void (*surface_pick)(const Frame &, int, int, uint32_t *, uint32_t *);
	void (*lighting_rays)(const Frame &, float3, float3, real, float3, float3, uint32_t *, uint32_t *, uint32_t *);
	void (*lighting_pick)(const Frame &, int, int, uint32_t *, uint32_t *, uint32_t *);
};
const Entry *find(const char *name);

// n caller-supplied rays, each to fn(i, origin, dir); they have no ray offsets, and a max_distance of 0 is the frame's range
const float3 no_offset = float3(real(0.f));
template <class Fn>
void each_ray(int n, const float *origins, const float *dirs, Fn fn)
{
	parallel_items(n, [&](int a, int b) {
		for (int i = a; i < b; ++i)
		{
			const float *o = origins + 3 * i, *d = dirs + 3 * i;
			fn(i, float3(o[0], o[1], o[2]), float3(d[0], d[1], d[2]));
		}
	});
}
real ray_range(const Frame &F, float max_distance) { return max_distance == 0.f ? F.range : real(max_distance); }

} // namespace

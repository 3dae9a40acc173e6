// tests/cpp/query_oracle.h -- TEST-ONLY: the three scene queries of include/sdfr.h (sdfr_query_distance, sdfr_query_rays,
// sdfr_pick) defined with the CPU oracle's own restatement of the reference's driver (oracle/driver.h), by calling its steps:
// map_geometry and first_normal at a point, ray_turn for a ray, primary_ray for a pixel.  The query tests compare the library (on
// the GPU) and its CPU build (query_host.cpp) with these, bit for bit.  Part of record_oracle.cpp; the product never loads it.
#pragma once
#include "record_oracle.h"

namespace {

template <class Scene>
void point_query(const Frame &F, const float *p, float *dist, float *normal)
{
	GeometryInput g;
	g.pos = float3(p[0], p[1], p[2]);
	g.dir = float4(real(0.f));
	g.camera_distance = 0.f;
	g.right_ray_offset = float3(real(0.f));
	g.bottom_ray_offset = float3(real(0.f));
	const MarchingInput march = plain_march();
	const real d = map_geometry<Scene>(F, g, march);
	*dist = val(d);
	if (normal)
	{
		const float3 n = first_normal<Scene>(F, g, march, d).normal;
		normal[0] = val(n.x);
		normal[1] = val(n.y);
		normal[2] = val(n.z);
	}
}

// the driver's turn for one primary-shaped ray: rec, the 12 words of sdfr_hit
template <class Scene>
void ray_query(const Frame &F, float3 origin, float3 dir, real dist_max, float3 right_off, float3 bottom_off, uint32_t *rec)
{
	Turn turn;
	primary_turn<Scene>(F, camera_ray(origin, dir), dist_max, right_off, bottom_off, turn, rec);
}

template <class Scene>
void pick_query(const Frame &F, int px, int py, uint32_t *rec)
{
	if (outside_frame(F, px, py, rec)) return;
	const PrimaryRay primary = primary_ray(F, px, py);
	ray_query<Scene>(F, F.eye, primary.dir, F.range, primary.right_ray_vec, primary.bottom_ray_vec, rec);
}

} // namespace

extern "C" {

int qo_points(const char *scene, const orc_frame *f, int n, const float *points, float *distance, float *normals)
{
	const Entry *e = find(scene);
	if (!e) return -1;
	const Frame F = enter_frame(*f);
	parallel_items(n, [&](int a, int b) {
		for (int i = a; i < b; ++i) e->points(F, points + 3 * i, distance + i, normals ? normals + 3 * i : nullptr);
	});
	return 0;
}

int qo_rays(const char *scene, const orc_frame *f, int n, const float *origins, const float *dirs, float max_distance, uint32_t *hits)
{
	const Entry *e = find(scene);
	if (!e) return -1;
	const Frame F = enter_frame(*f);
	const real dist_max = ray_range(F, max_distance);
	each_ray(n, origins, dirs, [&](int i, float3 o, float3 d) { e->rays(F, o, d, dist_max, no_offset, no_offset, hits + HIT_WORDS * i); });
	return 0;
}

int qo_pick(const char *scene, const orc_frame *f, int n, const int32_t *pixels, uint32_t *hits)
{
	const Entry *e = find(scene);
	if (!e) return -1;
	const Frame F = enter_frame(*f);
	parallel_items(n, [&](int a, int b) {
		for (int i = a; i < b; ++i) e->pick(F, pixels[2 * i], pixels[2 * i + 1], hits + HIT_WORDS * i);
	});
	return 0;
}

// what the loader checks against pyoracle.OrcFrame
int qo_frame_size() { return (int)sizeof(orc_frame); }

} // extern "C"

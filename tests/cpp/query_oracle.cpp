// tests/cpp/query_oracle.cpp -- TEST-ONLY: the three scene queries of include/sdfr.h (sdfr_query_distance, sdfr_query_rays,
// sdfr_pick) defined with the CPU oracle's own restatement of the reference's driver (oracle/driver.h): map_geometry, map_normal
// + grad, march_ray, map_material, and ps_main's pixel -> ray lines.  The query tests compare the library (on the GPU) and its
// CPU build (query_host.cpp) with these, bit for bit.  Built by tests/query_util.py; the product never loads it.
#include "driver.h"
#include "scenes.h"
#include "scenes2.h"
#include "scenes3.h"
#include "scenes4.h"
#include "test_scenes.h"

#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

using namespace orc;

extern "C" {
// the layout of struct orc_frame (oracle/oracle_api.cpp, pyoracle.OrcFrame)
struct qo_frame
{
	float eye[3], front[3], right[3], top[3];
	float stime;
	int width, height;
	int iter_count, bounce_count, ray_count, light_count;
	float range;
	int max_cost_default;
	float debug_nx, debug_ny, debug_nz, debug_scale, debug_x, debug_y, debug_z, show_objects;
	float scene_var[8];
	int extension_lights;
	float extension_marble_reflection;
	float dist_eps, grad_eps, reflect_eps, refract_eps, shadow_eps;
};
}

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

Frame to_frame(const qo_frame &f)
{
	Frame F;
	F.eye = float3(f.eye[0], f.eye[1], f.eye[2]);
	F.front_vec = float3(f.front[0], f.front[1], f.front[2]);
	F.right_vec = float3(f.right[0], f.right[1], f.right[2]);
	F.top_vec = float3(f.top[0], f.top[1], f.top[2]);
	F.stime = f.stime;
	F.width = f.width;
	F.height = f.height;
	F.iter_count = f.iter_count;
	F.bounce_count = f.bounce_count;
	F.ray_count = f.ray_count;
	F.light_count = f.light_count;
	F.range = f.range;
	F.max_cost_default = (uint)f.max_cost_default;
	F.debug_nx = f.debug_nx;
	F.debug_ny = f.debug_ny;
	F.debug_nz = f.debug_nz;
	F.debug_scale = f.debug_scale;
	F.debug_x = f.debug_x;
	F.debug_y = f.debug_y;
	F.debug_z = f.debug_z;
	F.show_objects = f.show_objects;
	for (int i = 0; i < MAX_SCENE_VARS; ++i) F.scene_var[i] = f.scene_var[i];
	F.extension_lights = f.extension_lights < 0 ? 0 : (f.extension_lights > 7 ? 7 : f.extension_lights);
	F.extension_marble_reflection = f.extension_marble_reflection;
	F.dist_eps = f.dist_eps;
	F.grad_eps = f.grad_eps;
	F.reflect_eps = f.reflect_eps;
	F.refract_eps = f.refract_eps;
	F.shadow_eps = f.shadow_eps;
	// the driver's epsilons, as orc_render sets them
	dist_eps = F.dist_eps;
	grad_eps = F.grad_eps;
	reflect_eps = F.reflect_eps;
	refract_eps = F.refract_eps;
	shadow_eps = F.shadow_eps;
	return F;
}

MarchingInput default_march()
{
	MarchingInput m;
	m.is_inside = false;
	m.last_transparent_pos = float3(real(0.f));
	m.has_transparent = false;
	m.is_shadow_pass = false;
	return m;
}

// the normal of pshader_sdf.hlsl:320-330 at `geometry` (whose dir.w the driver has set to 0)
template <class Scene>
float3 driver_normal(const Frame &F, GeometryInput geometry, const MarchingInput &march, real baseline)
{
	NormalOutput no;
	no.use_normal = false;
	no.normal = float3(real(0.f));
	no.normal_sample_dist = grad_eps;
	geometry.dir.w = 0.f;
	Scene::map_normal(F, geometry, no);
	if (!no.use_normal) no.normal = grad<Scene>(F, geometry, march, baseline, no.normal_sample_dist);
	return no.normal;
}

template <class Scene>
void point_query(const Frame &F, const float *p, float *dist, float *normal)
{
	GeometryInput g;
	g.pos = float3(p[0], p[1], p[2]);
	g.dir = float4(real(0.f));
	g.camera_distance = 0.f;
	g.right_ray_offset = float3(real(0.f));
	g.bottom_ray_offset = float3(real(0.f));
	const MarchingInput march = default_march();
	const real d = map_geometry<Scene>(F, g, march);
	*dist = val(d);
	if (normal)
	{
		const float3 n = driver_normal<Scene>(F, g, march, d);
		normal[0] = val(n.x);
		normal[1] = val(n.y);
		normal[2] = val(n.z);
	}
}

uint32_t bits(float f)
{
	uint32_t u;
	memcpy(&u, &f, 4);
	return u;
}

// pshader_sdf.hlsl:299-353 for one primary-shaped ray: march_ray, then normal and map_material on a hit
template <class Scene>
void ray_query(const Frame &F, float3 origin, float3 dir, real dist_max, float3 right_off, float3 bottom_off, uint32_t *rec)
{
	GeometryInput g;
	g.pos = origin;
	g.dir = float4(dir, real(1.f));
	g.camera_distance = 0.f;
	g.right_ray_offset = right_off;
	g.bottom_ray_offset = bottom_off;
	const MarchingInput march = default_march();
	uint iter = 0;
	real scene_distance = 0.f;
	PixelStats st = {0, 0, 0};
	const bool hit = march_ray<Scene>(F, g, march, dist_max, real(1.f), iter, scene_distance, st);
	const float3 pos = mad(g.dir.xyz(), g.camera_distance, origin);
	float3 n = float3(real(0.f));
	uint32_t material = 0;
	if (hit)
	{
		n = driver_normal<Scene>(F, g, march, scene_distance);
		MaterialInput mi;
		mi.obj_normal = n;
		mi.iteration_count = iter;
		mi.scene_distance = scene_distance;
		MaterialOutput mo;
		mo.material_id = MATERIAL_NONE;
		mo.material_position = float4(g.pos, real(0.f));
		mo.material_properties = float4(real(0.f));
		mo.diffuse_color = float4(real(0.f), real(0.f), real(0.f), real(1.f));
		mo.specular_color = float4(real(0.f), real(0.f), real(0.f), real(60.f));
		mo.emissive_color = float3(real(0.f));
		mo.reflection_color = float3(real(0.f));
		mo.refraction_color = float3(real(0.f));
		mo.optical_index = 1.4f;
		mo.optical_density = 0.f;
		mo.normal = float4(real(0.f));
		mo.max_cost = F.max_cost_default;
		mo.use_hdr = true;
		GeometryInput gm = g;
		gm.dir.w = 0.f;
		map_material<Scene>(F, gm, mi, mo);
		material = mo.material_id;
	}
	rec[0] = bits(val(g.camera_distance));
	rec[1] = bits(val(scene_distance));
	rec[2] = bits(val(pos.x));
	rec[3] = bits(val(pos.y));
	rec[4] = bits(val(pos.z));
	rec[5] = bits(val(n.x));
	rec[6] = bits(val(n.y));
	rec[7] = bits(val(n.z));
	rec[8] = iter;
	rec[9] = material;
	rec[10] = hit ? 1u : 0u;
	rec[11] = 0u;
}

// ps_main's pixel -> primary ray (driver.h: pshader_sdf.hlsl:263-267 with the NDC mapping of the full-screen quad)
template <class Scene>
void pick_query(const Frame &F, int px, int py, uint32_t *rec)
{
	if (px < 0 || py < 0 || px >= F.width || py >= F.height)
	{
		for (int k = 0; k < 12; ++k) rec[k] = 0u;
		rec[10] = 0xffffffffu;
		return;
	}
	real screen_x = (real((float)px) + real(0.5f)) / real((float)F.width) * real(2.f) - real(1.f);
	real screen_y = real(1.f) - (real((float)py) + real(0.5f)) / real((float)F.height) * real(2.f);
	real ddx_x = real(2.f) / real((float)F.width);
	real ddy_y = real(-2.f) / real((float)F.height);
	float3 dir = F.front_vec + screen_x * F.right_vec + screen_y * F.top_vec;
	real dir_invlen = real(1.f) / length(dir);
	dir = dir * dir_invlen;
	float3 right_ray_vec = ddx_x * F.right_vec * dir_invlen;
	float3 bottom_ray_vec = ddy_y * F.top_vec * dir_invlen;
	ray_query<Scene>(F, F.eye, dir, F.range, right_ray_vec, bottom_ray_vec, rec);
}

struct Entry
{
	const char *name;
	void (*points)(const Frame &, const float *, float *, float *);
	void (*rays)(const Frame &, float3, float3, real, float3, float3, uint32_t *);
	void (*pick)(const Frame &, int, int, uint32_t *);
};
#define QO(name, S) {name, &point_query<S>, &ray_query<S>, &pick_query<S>}
const Entry k_scenes[] = {
	QO("fast_sphere", SceneFastSphere), QO("cube_sea", SceneCubeSea), QO("labyrinth", SceneLabyrinth), QO("fractal", SceneFractal),
	QO("lense", SceneLense), QO("gems", SceneGems), QO("light_shadows", SceneLightShadows), QO("cube", SceneCube), QO("gyroid", SceneGyroid),
	QO("basic_transparency", SceneBasicTransparency), QO("basic_clouds", SceneBasicClouds), QO("coordinate_material", SceneCoordinateMaterial),
	QO("distortion", SceneDistortion), QO("table", SceneTable), QO("sierpinski", SceneSierpinski), QO("neon", SceneNeon), QO("fractal2", SceneFractal2),
	QO("shell", SceneShell), QO("spiral", SceneSpiral), QO("terrain", SceneTerrain), QO("tiling", SceneTiling), QO("tree", SceneTree),
	QO("debug_materials", SceneDebugMaterials), QO("normal_test", SceneNormalTest), QO("noise_lod", SceneNoiseLod), QO("dialect_tour", SceneDialectTour),
};
#undef QO

const Entry *find(const char *name)
{
	for (const Entry &e : k_scenes)
		if (strcmp(e.name, name) == 0) return &e;
	return nullptr;
}

} // namespace

extern "C" {

int qo_points(const char *scene, const qo_frame *f, int n, const float *points, float *distance, float *normals)
{
	const Entry *e = find(scene);
	if (!e) return -1;
	const Frame F = to_frame(*f);
	parallel_items(n, [&](int a, int b) {
		for (int i = a; i < b; ++i) e->points(F, points + 3 * i, distance + i, normals ? normals + 3 * i : nullptr);
	});
	return 0;
}

// max_distance 0: the frame's range
int qo_rays(const char *scene, const qo_frame *f, int n, const float *origins, const float *dirs, float max_distance, uint32_t *hits)
{
	const Entry *e = find(scene);
	if (!e) return -1;
	const Frame F = to_frame(*f);
	const real dist_max = max_distance == 0.f ? F.range : real(max_distance);
	parallel_items(n, [&](int a, int b) {
		for (int i = a; i < b; ++i)
		{
			const float *o = origins + 3 * i, *d = dirs + 3 * i;
			e->rays(F, float3(o[0], o[1], o[2]), float3(d[0], d[1], d[2]), dist_max, float3(real(0.f)), float3(real(0.f)), hits + 12 * i);
		}
	});
	return 0;
}

int qo_pick(const char *scene, const qo_frame *f, int n, const int32_t *pixels, uint32_t *hits)
{
	const Entry *e = find(scene);
	if (!e) return -1;
	const Frame F = to_frame(*f);
	parallel_items(n, [&](int a, int b) {
		for (int i = a; i < b; ++i) e->pick(F, pixels[2 * i], pixels[2 * i + 1], hits + 12 * i);
	});
	return 0;
}

int qo_frame_size() { return (int)sizeof(qo_frame); }

} // extern "C"

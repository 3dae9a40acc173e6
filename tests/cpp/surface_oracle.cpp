// tests/cpp/surface_oracle.cpp -- TEST-ONLY: the surface record of include/sdfr.h (sdfr_surface: sdfr_query_ray_surfaces,
// sdfr_pick_surfaces, sdfr_mesh_surfaces) defined with the CPU oracle's own restatement of the reference's driver (oracle/driver.h):
// march_ray, map_normal + grad, the material's initialisation and map_material as query_oracle.cpp's ray_query has them, then the
// marble extension's line and the material switch of driver.h's ps_main.  The surface tests compare the library (on the GPU) and its
// CPU build (surface_host.cpp) with these, bit for bit.  Built by tests/surface_util.py; the product never loads it.
//
// The frame, the threads, the driver's normal and the pixel -> ray lines are query_oracle.cpp's, included as they are.
#include "query_oracle.cpp"

namespace {

void surface_none(uint32_t valid, uint32_t *rec)
{
	for (int k = 0; k < 32; ++k) rec[k] = 0u;
	rec[3] = valid;
}

void put3(uint32_t *rec, float3 v)
{
	rec[0] = bits(val(v.x));
	rec[1] = bits(val(v.y));
	rec[2] = bits(val(v.z));
}

// pshader_sdf.hlsl:299-481 for one primary-shaped ray, without the rays it would spawn: `hit` as ray_query's record, `rec` the
// 32 words of sdfr_surface
template <class Scene>
void surface_query(const Frame &F, float3 origin, float3 dir, real dist_max, float3 right_off, float3 bottom_off, uint32_t *hit, uint32_t *rec)
{
	GeometryInput g;
	g.pos = origin;
	g.dir = float4(dir, real(1.f));
	g.camera_distance = 0.f;
	g.right_ray_offset = right_off;
	g.bottom_ray_offset = bottom_off;
	const MarchingInput march = default_march();
	uint iter_count = 0;
	real scene_distance = 0.f;
	PixelStats st = {0, 0, 0};
	const bool scene_hit = march_ray<Scene>(F, g, march, dist_max, real(1.f), iter_count, scene_distance, st);
	const float3 pos = mad(g.dir.xyz(), g.camera_distance, origin);
	float3 normal = float3(real(0.f));
	uint32_t material = 0;
	surface_none(0u, rec);
	if (scene_hit)
	{
		normal = driver_normal<Scene>(F, g, march, scene_distance);
		MaterialInput material_input;
		material_input.obj_normal = normal;
		material_input.iteration_count = iter_count;
		material_input.scene_distance = scene_distance;
		MaterialOutput material_output;
		material_output.material_id = MATERIAL_NONE;
		material_output.material_position = float4(g.pos, real(0.f));
		material_output.material_properties = float4(real(0.f));
		material_output.diffuse_color = float4(real(0.f), real(0.f), real(0.f), real(1.f));
		material_output.specular_color = float4(real(0.f), real(0.f), real(0.f), real(60.f));
		material_output.emissive_color = float3(real(0.f));
		material_output.reflection_color = float3(real(0.f));
		material_output.refraction_color = float3(real(0.f));
		material_output.optical_index = 1.4f;
		material_output.optical_density = 0.f;
		material_output.normal = float4(real(0.f));
		material_output.max_cost = F.max_cost_default;
		material_output.use_hdr = true;
		GeometryInput geometry_input = g;
		geometry_input.dir.w = 0.f;
		map_material<Scene>(F, geometry_input, material_input, material_output);
		material = material_output.material_id;

		// the marble extension's line
		if (F.extension_marble_reflection != real(0.f) &&
			(material_output.material_id == MATERIAL_MARBLE_DARK || material_output.material_id == MATERIAL_MARBLE_LIGHT))
			material_output.reflection_color = float3(F.extension_marble_reflection);
		// normal, second pass (:362)
		float3 new_normal = lerp(normal, material_output.normal.xyz(), material_output.normal.w);

		float3 diffuse_color = material_output.diffuse_color.xyz();
		float3 color = float3(real(0.f));
		bool use_light = true;
		// material switch (:430-481)
		if (material_output.material_id == MATERIAL_ITER)
		{
			color = color + iter_count_to_color(iter_count, (uint)(F.iter_count - 1));
			use_light = false;
		}
		else if (material_output.material_id == MATERIAL_PLAIN)
		{
			color = color + diffuse_color;
			use_light = false;
		}
		else if (material_output.material_id == MATERIAL_NORMAL1)
		{
			float3 normal_color = v_max(real(0.01f), new_normal);
			normal_color = normal_color / r_max(r_max(normal_color.x, normal_color.y), normal_color.z);
			color = color + normal_color;
			use_light = false;
		}
		else if (material_output.material_id == MATERIAL_NORMAL2)
		{
			color = color + v_abs(new_normal);
			use_light = false;
		}
		else if (material_output.material_id == MATERIAL_DISTANCE_PLANE)
		{
			color = color + debug_plane_color(material_output.material_properties.x);
			use_light = false;
		}
		else if (material_output.material_id == MATERIAL_WOOD)
		{
			diffuse_color = diffuse_color + wood(material_output.material_position.xyz());
		}
		else if (material_output.material_id == MATERIAL_MARBLE_DARK)
		{
			diffuse_color = diffuse_color + marble(material_output.material_position.xyz(), float3(real(0.556f), real(0.478f), real(0.541f)));
		}
		else if (material_output.material_id == MATERIAL_MARBLE_LIGHT)
		{
			diffuse_color = diffuse_color + marble(material_output.material_position.xyz(), float3(real(0.7f), real(0.7f), real(0.7f)));
		}
		else if (material_output.material_id == MATERIAL_FIRE)
		{
			real fadeout = r_saturate(dot(-geometry_input.dir.xyz(), new_normal));
			float4 fire_color = fire(material_output.material_position.xyz(), real(1.f) - fadeout);
			color = color + fire_color.xyz();
			material_output.diffuse_color.w = r_saturate(fire_color.w);
			material_output.diffuse_color.x = material_output.diffuse_color.y = material_output.diffuse_color.z = real(1.f);
		}

		rec[0] = material_output.material_id;
		rec[1] = (material_output.use_hdr ? 1u : 0u) | (use_light ? 2u : 0u);
		rec[2] = material_output.max_cost;
		rec[3] = 1u;
		put3(rec + 4, diffuse_color);
		rec[7] = bits(val(material_output.diffuse_color.w));
		put3(rec + 8, material_output.specular_color.xyz());
		rec[11] = bits(val(material_output.specular_color.w));
		put3(rec + 12, material_output.emissive_color);
		rec[15] = bits(val(material_output.optical_index));
		put3(rec + 16, color);
		put3(rec + 20, material_output.reflection_color);
		put3(rec + 24, material_output.refraction_color);
		put3(rec + 28, new_normal);
	}
	hit[0] = bits(val(g.camera_distance));
	hit[1] = bits(val(scene_distance));
	put3(hit + 2, pos);
	put3(hit + 5, normal);
	hit[8] = iter_count;
	hit[9] = material;
	hit[10] = scene_hit ? 1u : 0u;
	hit[11] = 0u;
}

// ps_main's pixel -> primary ray, as pick_query
template <class Scene>
void surface_pick(const Frame &F, int px, int py, uint32_t *hit, uint32_t *rec)
{
	if (px < 0 || py < 0 || px >= F.width || py >= F.height)
	{
		for (int k = 0; k < 12; ++k) hit[k] = 0u;
		hit[10] = 0xffffffffu;
		surface_none(0xffffffffu, rec);
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
	surface_query<Scene>(F, F.eye, dir, F.range, right_ray_vec, bottom_ray_vec, hit, rec);
}

struct SurfaceEntry
{
	const char *name;
	void (*rays)(const Frame &, float3, float3, real, float3, float3, uint32_t *, uint32_t *);
	void (*pick)(const Frame &, int, int, uint32_t *, uint32_t *);
};
#define SO(name, S) {name, &surface_query<S>, &surface_pick<S>}
const SurfaceEntry k_surface_scenes[] = {
	SO("fast_sphere", SceneFastSphere), SO("cube_sea", SceneCubeSea), SO("labyrinth", SceneLabyrinth), SO("fractal", SceneFractal),
	SO("lense", SceneLense), SO("gems", SceneGems), SO("light_shadows", SceneLightShadows), SO("cube", SceneCube), SO("gyroid", SceneGyroid),
	SO("basic_transparency", SceneBasicTransparency), SO("basic_clouds", SceneBasicClouds), SO("coordinate_material", SceneCoordinateMaterial),
	SO("distortion", SceneDistortion), SO("table", SceneTable), SO("sierpinski", SceneSierpinski), SO("neon", SceneNeon), SO("fractal2", SceneFractal2),
	SO("shell", SceneShell), SO("spiral", SceneSpiral), SO("terrain", SceneTerrain), SO("tiling", SceneTiling), SO("tree", SceneTree),
	SO("debug_materials", SceneDebugMaterials), SO("normal_test", SceneNormalTest), SO("noise_lod", SceneNoiseLod), SO("dialect_tour", SceneDialectTour),
};
#undef SO

const SurfaceEntry *find_surface(const char *name)
{
	for (const SurfaceEntry &e : k_surface_scenes)
		if (strcmp(e.name, name) == 0) return &e;
	return nullptr;
}

} // namespace

extern "C" {

// max_distance 0: the frame's range
int so_rays(const char *scene, const qo_frame *f, int n, const float *origins, const float *dirs, float max_distance, uint32_t *hits, uint32_t *surfaces)
{
	const SurfaceEntry *e = find_surface(scene);
	if (!e) return -1;
	const Frame F = to_frame(*f);
	const real dist_max = max_distance == 0.f ? F.range : real(max_distance);
	parallel_items(n, [&](int a, int b) {
		for (int i = a; i < b; ++i)
		{
			const float *o = origins + 3 * i, *d = dirs + 3 * i;
			e->rays(F, float3(o[0], o[1], o[2]), float3(d[0], d[1], d[2]), dist_max, float3(real(0.f)), float3(real(0.f)), hits + 12 * i, surfaces + 32 * i);
		}
	});
	return 0;
}

int so_pick(const char *scene, const qo_frame *f, int n, const int32_t *pixels, uint32_t *hits, uint32_t *surfaces)
{
	const SurfaceEntry *e = find_surface(scene);
	if (!e) return -1;
	const Frame F = to_frame(*f);
	parallel_items(n, [&](int a, int b) {
		for (int i = a; i < b; ++i) e->pick(F, pixels[2 * i], pixels[2 * i + 1], hits + 12 * i, surfaces + 32 * i);
	});
	return 0;
}

} // extern "C"

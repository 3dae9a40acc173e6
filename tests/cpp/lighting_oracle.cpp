// tests/cpp/lighting_oracle.cpp -- TEST-ONLY: the lighting records of include/sdfr.h (sdfr_lighting, sdfr_light_sample:
// sdfr_query_ray_lighting, sdfr_pick_lighting, sdfr_mesh_lighting) defined with the CPU oracle's own restatement of the reference's
// driver (oracle/driver.h): the lines of ps_main for a primary ray -- march_ray, map_normal + grad, map_material, the marble
// extension, the material switch, the light loop with the scenes' map_light -- and, in place of the ray queue, each shadow ray's turns
// of the bounce loop one after the other.  The lighting tests compare the library (on the GPU) and its CPU build (lighting_host.cpp)
// with these, bit for bit.  Built by tests/lighting_util.py; the product never loads it.
//
// The frame, the threads and the pixel -> ray lines are query_oracle.cpp's, included as they are.
#include "query_oracle.cpp"

namespace {

enum { LIGHTING_WORDS = 16, SAMPLE_WORDS = 20, SLOTS = 8, CHAIN_SEGMENTS = 64 };

void put3(uint32_t *rec, float3 v)
{
	rec[0] = bits(val(v.x));
	rec[1] = bits(val(v.y));
	rec[2] = bits(val(v.z));
}

// pshader_sdf.hlsl:338-351
MaterialOutput fresh_material(const Frame &F, float3 pos)
{
	MaterialOutput material_output;
	material_output.material_id = MATERIAL_NONE;
	material_output.material_position = float4(pos, real(0.f));
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
	return material_output;
}

// the driver's turn for one ray up to its material (:299-353); false: the ray missed
template <class Scene>
bool ray_turn(const Frame &F, GeometryInput &geometry_input, const MarchingInput &marching_input, real max_range, uint &iter_count, real &scene_distance,
	NormalOutput &normal_output, MaterialOutput &material_output)
{
	PixelStats st = {0, 0, 0};
	iter_count = 0;
	scene_distance = 0.f;
	if (!march_ray<Scene>(F, geometry_input, marching_input, max_range, real(1.f), iter_count, scene_distance, st)) return false;
	normal_output.use_normal = false;
	normal_output.normal = float3(real(0.f));
	normal_output.normal_sample_dist = grad_eps;
	geometry_input.dir.w = 0.f;
	Scene::map_normal(F, geometry_input, normal_output);
	if (!normal_output.use_normal) normal_output.normal = grad<Scene>(F, geometry_input, marching_input, scene_distance * real(1.f), normal_output.normal_sample_dist);
	MaterialInput material_input;
	material_input.obj_normal = normal_output.normal;
	material_input.iteration_count = iter_count;
	material_input.scene_distance = scene_distance;
	material_output = fresh_material(F, geometry_input.pos);
	map_material<Scene>(F, geometry_input, material_input, material_output);
	if (F.extension_marble_reflection != real(0.f) && (material_output.material_id == MATERIAL_MARBLE_DARK || material_output.material_id == MATERIAL_MARBLE_LIGHT))
		material_output.reflection_color = float3(F.extension_marble_reflection);
	return true;
}

// hit: the 12 words of sdfr_hit; rec: the 16 of sdfr_lighting; samples: 8 x 20 words of sdfr_light_sample, or null
template <class Scene>
void lighting_query(const Frame &F, float3 origin, float3 dir, real dist_max, float3 right_off, float3 bottom_off, uint32_t *hit, uint32_t *rec,
	uint32_t *samples)
{
	const real RANGE = F.range;
	const int LIGHT_COUNT = F.light_count;
	for (int k = 0; k < LIGHTING_WORDS; ++k) rec[k] = 0u;
	if (samples)
		for (int k = 0; k < SLOTS * SAMPLE_WORDS; ++k) samples[k] = 0u;

	// the primary ray: depth 0, contribution (1, 1, 1), outside
	const float3 contribution = float3(real(1.f), real(1.f), real(1.f));
	const uint depth = 0;
	GeometryInput geometry_input;
	geometry_input.pos = origin;
	geometry_input.dir = float4(dir, real(1.f));
	geometry_input.camera_distance = 0.f;
	geometry_input.right_ray_offset = right_off;
	geometry_input.bottom_ray_offset = bottom_off;
	const MarchingInput primary_march = default_march();
	uint iter_count;
	real scene_distance;
	NormalOutput normal_output;
	normal_output.normal = float3(real(0.f));
	MaterialOutput material_output = fresh_material(F, origin);
	const bool scene_hit = ray_turn<Scene>(F, geometry_input, primary_march, dist_max, iter_count, scene_distance, normal_output, material_output);

	hit[0] = bits(val(geometry_input.camera_distance));
	hit[1] = bits(val(scene_distance));
	put3(hit + 2, mad(float3(dir), geometry_input.camera_distance, origin));
	put3(hit + 5, scene_hit ? normal_output.normal : float3(real(0.f)));
	hit[8] = iter_count;
	hit[9] = scene_hit ? (uint32_t)material_output.material_id : 0u;
	hit[10] = scene_hit ? 1u : 0u;
	hit[11] = 0u;
	if (!scene_hit) return;

	// normal, second pass (:362)
	float3 new_normal = lerp(normal_output.normal, material_output.normal.xyz(), material_output.normal.w);
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

	uint32_t used_mask = 0, traced_mask = 0, visible_mask = 0, segments = 0;
	real ambient_lighting_factor = 0.f;
	float3 delivered[SLOTS];
	for (int i = 0; i < SLOTS; ++i) delivered[i] = float3(real(0.f));
	if (use_light)
	{
		// :505-516
		LightOutput light_output[MAX_LIGHT_COUNT];
		for (int i1 = 0; i1 < MAX_LIGHT_COUNT; ++i1)
		{
			light_output[i1].used = false;
			light_output[i1].pos = float4(real(0.f));
			light_output[i1].color = float3(real(0.f));
			light_output[i1].falloff = 0.f;
			light_output[i1].extend = 0.f;
		}
		ambient_lighting_factor = 0.075f;
		Scene::map_light(F, geometry_input, light_output, ambient_lighting_factor);
		extension_lights(F, light_output);

		// :519-521
		float3 view_dir = geometry_input.dir.xyz();
		real shadow_move_distance = r_max(real(shadow_eps), normal_output.normal_sample_dist) + r_max(real(0.f), -scene_distance);
		float3 scene_pos = mad(new_normal, shadow_move_distance, geometry_input.pos);

		// :524-587
		for (int i2 = 0; i2 < LIGHT_COUNT && i2 < SLOTS; ++i2)
		{
			if (!light_output[i2].used) continue;
			used_mask |= 1u << i2;
			float3 lighting_dir;
			real distance_to_trace;
			real falloff_factor = 1.f;
			const bool directional = light_output[i2].pos.w == real(1.f);
			if (directional)
			{
				lighting_dir = light_output[i2].pos.xyz();
				lighting_dir = lighting_dir / (length(lighting_dir) + real(dist_eps));
				distance_to_trace = RANGE;
			}
			else
			{
				lighting_dir = scene_pos - light_output[i2].pos.xyz();
				distance_to_trace = length(lighting_dir);
				lighting_dir = lighting_dir / distance_to_trace;
				distance_to_trace -= light_output[i2].extend;
				falloff_factor = r_pow(real(0.1f), light_output[i2].falloff);
			}
			float3 light_color = light_output[i2].color * falloff_factor;
			color = color + diffuse_color * light_color * ambient_lighting_factor;
			float3 light_influenced_color = float3(real(0.f));
			real light_dot = r_saturate(dot(-new_normal, lighting_dir));
			light_influenced_color = light_influenced_color + diffuse_color * light_color * light_dot;
			float3 half_vec = -normalize(view_dir + lighting_dir);
			real specular_dot = r_saturate(dot(new_normal, half_vec));
			real specular_factor = r_pow(specular_dot, material_output.specular_color.w);
			light_influenced_color = light_influenced_color + material_output.specular_color.xyz() * light_color * specular_factor;

			uint32_t state = 1, chain_segments = 0;
			// shadow ray (:568-585), and its turns of the bounce loop (:299-353, :598-632) in place of the queue
			if (depth + 2 < material_output.max_cost && light_dot > real(0.f))
			{
				traced_mask |= 1u << i2;
				float3 ray_pos = scene_pos, ray_dir = -lighting_dir;
				float3 ray_contribution = light_influenced_color * contribution * r_saturate(material_output.diffuse_color.w);
				float3 ray_last_transparent_pos = float3(real(0.f));
				bool ray_has_transparent = false;
				real ray_shadow_range = distance_to_trace;
				uint ray_depth = depth + 2;
				state = 2;
				while (chain_segments < CHAIN_SEGMENTS)
				{
					++chain_segments;
					GeometryInput g;
					g.pos = ray_pos;
					g.dir = float4(ray_dir, real(1.f));
					g.camera_distance = 0.f;
					g.right_ray_offset = right_off;
					g.bottom_ray_offset = bottom_off;
					MarchingInput marching_input;
					marching_input.is_inside = false;
					marching_input.has_transparent = ray_has_transparent;
					marching_input.last_transparent_pos = ray_last_transparent_pos;
					marching_input.is_shadow_pass = true;
					real max_range = ray_shadow_range;
					uint it;
					real sd;
					NormalOutput no;
					MaterialOutput mo = fresh_material(F, ray_pos);
					if (!ray_turn<Scene>(F, g, marching_input, max_range, it, sd, no, mo))
					{
						state = 3; // (:621-626) output_color += contribution
						delivered[i2] = ray_contribution;
						break;
					}
					// :598-619
					if (!(mo.diffuse_color.w < real(1.f) && ray_depth + 2 < mo.max_cost)) break;
					ray_contribution = (real(1.f) - mo.diffuse_color.w) * mo.diffuse_color.xyz() * ray_contribution;
					ray_pos = g.pos;
					ray_last_transparent_pos = g.pos;
					ray_has_transparent = true;
					ray_shadow_range = max_range - g.camera_distance;
					ray_depth = ray_depth + 2;
				}
				segments += chain_segments;
				if (state == 3) visible_mask |= 1u << i2;
			}
			if (samples)
			{
				uint32_t *s = samples + SAMPLE_WORDS * i2;
				s[0] = state;
				s[1] = directional ? 1u : 0u;
				s[2] = chain_segments;
				put3(s + 4, lighting_dir);
				s[7] = bits(val(distance_to_trace));
				put3(s + 8, light_color);
				s[11] = bits(val(light_dot));
				put3(s + 12, light_influenced_color);
				s[15] = bits(val(specular_factor));
				put3(s + 16, delivered[i2]);
			}
		}
		// emissive + alpha (:590-593)
		color = color + material_output.emissive_color;
		color = color * r_saturate(material_output.diffuse_color.w);
	}

	// the driver's sums: out_color += (0 + color * contribution) for the primary ray's turn, then += (0 + contribution) for each
	// escaped shadow ray, popped in slot order when every chain is one segment long
	float3 direct = float3(real(0.f)), lit = float3(real(0.f));
	{
		float3 output_color = float3(real(0.f));
		output_color = output_color + color * contribution;
		lit = lit + output_color;
	}
	for (int i = 0; i < SLOTS; ++i)
		if (visible_mask & (1u << i))
		{
			float3 output_color = float3(real(0.f));
			output_color = output_color + delivered[i];
			direct = direct + output_color;
			lit = lit + output_color;
		}

	rec[0] = 1u;
	rec[1] = used_mask;
	rec[2] = traced_mask;
	rec[3] = visible_mask;
	put3(rec + 4, color);
	rec[7] = bits(val(ambient_lighting_factor));
	put3(rec + 8, direct);
	rec[11] = segments;
	put3(rec + 12, lit);
}

template <class Scene>
void lighting_pick(const Frame &F, int px, int py, uint32_t *hit, uint32_t *rec, uint32_t *samples)
{
	if (px < 0 || py < 0 || px >= F.width || py >= F.height)
	{
		for (int k = 0; k < 12; ++k) hit[k] = 0u;
		hit[10] = 0xffffffffu;
		for (int k = 0; k < LIGHTING_WORDS; ++k) rec[k] = 0u;
		rec[0] = 0xffffffffu;
		if (samples)
			for (int k = 0; k < SLOTS * SAMPLE_WORDS; ++k) samples[k] = 0u;
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
	lighting_query<Scene>(F, F.eye, dir, F.range, right_ray_vec, bottom_ray_vec, hit, rec, samples);
}

struct LightingEntry
{
	const char *name;
	void (*rays)(const Frame &, float3, float3, real, float3, float3, uint32_t *, uint32_t *, uint32_t *);
	void (*pick)(const Frame &, int, int, uint32_t *, uint32_t *, uint32_t *);
};
#define LO(name, S) {name, &lighting_query<S>, &lighting_pick<S>}
const LightingEntry k_lighting_scenes[] = {
	LO("fast_sphere", SceneFastSphere), LO("cube_sea", SceneCubeSea), LO("labyrinth", SceneLabyrinth), LO("fractal", SceneFractal),
	LO("lense", SceneLense), LO("gems", SceneGems), LO("light_shadows", SceneLightShadows), LO("cube", SceneCube), LO("gyroid", SceneGyroid),
	LO("basic_transparency", SceneBasicTransparency), LO("basic_clouds", SceneBasicClouds), LO("coordinate_material", SceneCoordinateMaterial),
	LO("distortion", SceneDistortion), LO("table", SceneTable), LO("sierpinski", SceneSierpinski), LO("neon", SceneNeon), LO("fractal2", SceneFractal2),
	LO("shell", SceneShell), LO("spiral", SceneSpiral), LO("terrain", SceneTerrain), LO("tiling", SceneTiling), LO("tree", SceneTree),
	LO("debug_materials", SceneDebugMaterials), LO("normal_test", SceneNormalTest), LO("noise_lod", SceneNoiseLod), LO("dialect_tour", SceneDialectTour),
};
#undef LO

const LightingEntry *find_lighting(const char *name)
{
	for (const LightingEntry &e : k_lighting_scenes)
		if (strcmp(e.name, name) == 0) return &e;
	return nullptr;
}

} // namespace

extern "C" {

// max_distance 0: the frame's range; lights may be null
int lo_rays(const char *scene, const qo_frame *f, int n, const float *origins, const float *dirs, float max_distance, uint32_t *hits, uint32_t *lighting,
	uint32_t *lights)
{
	const LightingEntry *e = find_lighting(scene);
	if (!e) return -1;
	const Frame F = to_frame(*f);
	const real dist_max = max_distance == 0.f ? F.range : real(max_distance);
	parallel_items(n, [&](int a, int b) {
		for (int i = a; i < b; ++i)
		{
			const float *o = origins + 3 * i, *d = dirs + 3 * i;
			e->rays(F, float3(o[0], o[1], o[2]), float3(d[0], d[1], d[2]), dist_max, float3(real(0.f)), float3(real(0.f)), hits + 12 * i, lighting + LIGHTING_WORDS * i,
				lights ? lights + (size_t)SLOTS * SAMPLE_WORDS * i : nullptr);
		}
	});
	return 0;
}

int lo_pick(const char *scene, const qo_frame *f, int n, const int32_t *pixels, uint32_t *hits, uint32_t *lighting, uint32_t *lights)
{
	const LightingEntry *e = find_lighting(scene);
	if (!e) return -1;
	const Frame F = to_frame(*f);
	parallel_items(n, [&](int a, int b) {
		for (int i = a; i < b; ++i)
			e->pick(F, pixels[2 * i], pixels[2 * i + 1], hits + 12 * i, lighting + LIGHTING_WORDS * i, lights ? lights + (size_t)SLOTS * SAMPLE_WORDS * i : nullptr);
	});
	return 0;
}

} // extern "C"

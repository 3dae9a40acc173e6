// sdfr.hpp -- C++ host mirror of the reference's SDF render stage, header-only over the C ABI
// (include/sdfr.h).  A user of the reference's `class SDFRenderer` (Engine/SDFRenderer.h:17-44)
// and `class Camera` (Engine/Camera.h:5-64, FPS mode) finds the same methods with the same
// meaning here; the D3D plumbing arguments (Graphics&, ShaderIncluder&, FullscreenQuad&,
// GPUProfiler&) are replaced by what this build needs (device ordinal, scene name, target).
#pragma once
#include "sdfr.h"

#include <map>
#include <string>
#include <string_view>

namespace sdfr {

// Engine/ShaderVariable.h:6-12
struct Variable
{
	float minval, maxval, start, step;
	float value; // the current value
};
using VariableMap = std::map<std::string, Variable, std::less<>>;

struct Vector3
{
	float x = 0.f, y = 0.f, z = 0.f;
	Vector3() {}
	Vector3(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
};

// Parameters of the reference's first-person camera; the basis arithmetic
// (Camera.cpp:36-49,156-166) runs inside libsdfr.so.
class Camera
{
public:
	void SetEye(const Vector3 &e) { eye = e; }
	const Vector3 &GetEye() const { return eye; }
	void SetLookat(const Vector3 &l) { target = l; target_is_direction = false; }
	void SetDirection(const Vector3 &d) { target = d; target_is_direction = true; }
	void SetAspect(float a) { aspect = a; }
	float GetAspect() const { return aspect; }
	void SetFOVY(float f) { fovy = f; }
	float GetFOVY() const { return fovy; }
	void SetRoll(float r) { roll = r; }
	float GetRoll() const { return roll; }

	// start-up values of Application.cpp:214-224
	Vector3 eye = Vector3(0.f, 2.f, -3.f), target = Vector3(0.f, 1.f, 0.f);
	bool target_is_direction = false;
	float fovy = 60.f * 3.14159265358979f / 180.f, aspect = 1200.f / 800.f, roll = 0.f;
};

class SDFRenderer
{
public:
	SDFRenderer() = default;
	SDFRenderer(const SDFRenderer &) = delete;
	SDFRenderer &operator=(const SDFRenderer &) = delete;
	~SDFRenderer() { sdfr_destroy(handle); }

	// bool init(Graphics &graphics)
	bool init(int device_ordinal = 0)
	{
		sdfr_destroy(handle);
		handle = nullptr;
		return sdfr_create(device_ordinal, &handle) == SDFR_OK;
	}

	// bool initShader(ShaderIncluder &includer) with the scene substitution of
	// Application::loadScene (Application.cpp:318-322): rebuilds the variable table
	bool initShader(const std::string &scene)
	{
		if (sdfr_load_scene(handle, scene.c_str()) != SDFR_OK) return false;
		return refreshVariables();
	}

	// the same with the scene given as source text, compiled at run time (the reference re-runs
	// initShader when a scene file changes, SceneManager.cpp:102-133); false = does not compile,
	// lastError() has the compiler's messages and the previous scene stays active
	bool initShaderSource(const std::string &name, const std::string &source)
	{
		if (sdfr_load_scene_source(handle, name.c_str(), source.c_str()) != SDFR_OK) return false;
		return refreshVariables();
	}

	// the same with the scene in the reference's own dialect: the text of a scenes/*.hlsl file as the reference compiles it
	// (map / map_normal / map_light / map_background, the OBJECT and MATERIAL macros; sdfr_load_scene_hlsl)
	bool initShaderHlsl(const std::string &name, const std::string &hlsl_text)
	{
		if (sdfr_load_scene_hlsl(handle, name.c_str(), hlsl_text.c_str()) != SDFR_OK) return false;
		return refreshVariables();
	}

	// void setParameters(float stime)
	void setParameters(float stime_) { stime = stime_; }

	// VariableMap &getVariableMap(): values edited in place are latched by the next render,
	// like ShaderVariableManager::updateBuffer (ShaderUtil.cpp:257-267)
	VariableMap &getVariableMap() { return variables; }

	// bool render(FullscreenQuad &quad, GPUProfiler &profiler, Camera &camera):
	// true if it did render something, false otherwise (no valid scene)
	bool render(const Camera &camera, int width, int height, void *target, int format = SDFR_RGBA32F, bool target_on_host = false)
	{
		if (!handle || !pushState(&camera)) return false;
		return sdfr_render(handle, width, height, target, format, target_on_host ? 1 : 0, nullptr) == SDFR_OK;
	}

	// the same anti-aliased (sdfr_render_aa in sdfr.h): factor x factor sub-samples per pixel, factor one of 1, 2, 4, 8, rendered and
	// resolved on the device in passes; pixel_stats (optional, where the target is): [height][width][3] summed counters
	bool renderAA(const Camera &camera, int width, int height, int factor, void *target, int format = SDFR_RGBA32F, bool target_on_host = false,
		uint32_t *pixel_stats = nullptr)
	{
		if (!handle || !pushState(&camera)) return false;
		return sdfr_render_aa(handle, width, height, factor, target, format, target_on_host ? 1 : 0, pixel_stats) == SDFR_OK;
	}

	// Questions put to the loaded scene with this renderer's variables and time (sdfr_query_distance, sdfr_query_rays, sdfr_pick in
	// sdfr.h); pick also takes the camera the pixels belong to.  on_host: every pointer is host memory and the answers are there
	// when the call returns; else device memory, enqueued.  Points and rays [n][3], pixels [n][2].
	bool queryDistance(int64_t n, const float *points, float *distance, float *normals = nullptr, bool on_host = true)
	{
		return handle && pushState() && sdfr_query_distance(handle, n, points, distance, normals, on_host ? 1 : 0) == SDFR_OK;
	}
	bool queryRays(int64_t n, const float *origins, const float *dirs, sdfr_hit *hits, float max_distance = 0.f, bool on_host = true)
	{
		return handle && pushState() && sdfr_query_rays(handle, n, origins, dirs, max_distance, hits, on_host ? 1 : 0) == SDFR_OK;
	}
	bool pick(const Camera &camera, int width, int height, int64_t n, const int32_t *pixels_xy, sdfr_hit *hits, bool on_host = true)
	{
		return handle && pushState(&camera) && sdfr_pick(handle, width, height, n, pixels_xy, hits, on_host ? 1 : 0) == SDFR_OK;
	}

	// What the surface looks like at the first hit (sdfr_query_ray_surfaces, sdfr_pick_surfaces, sdfr_mesh_surfaces in sdfr.h): hits may
	// be null; pickSurfaces with pixels_xy null is the G-buffer of the frame, n = width * height.
	bool queryRaySurfaces(int64_t n, const float *origins, const float *dirs, sdfr_hit *hits, sdfr_surface *surfaces, float max_distance = 0.f,
		bool on_host = true)
	{
		return handle && pushState() && sdfr_query_ray_surfaces(handle, n, origins, dirs, max_distance, hits, surfaces, on_host ? 1 : 0) == SDFR_OK;
	}
	bool pickSurfaces(const Camera &camera, int width, int height, int64_t n, const int32_t *pixels_xy, sdfr_hit *hits, sdfr_surface *surfaces,
		bool on_host = true)
	{
		return handle && pushState(&camera) && sdfr_pick_surfaces(handle, width, height, n, pixels_xy, hits, surfaces, on_host ? 1 : 0) == SDFR_OK;
	}
	bool meshSurfaces(int64_t n, const float *positions, const float *normals, float reach, sdfr_hit *hits, sdfr_surface *surfaces, bool on_host = true)
	{
		return handle && pushState() && sdfr_mesh_surfaces(handle, n, positions, normals, reach, hits, surfaces, on_host ? 1 : 0) == SDFR_OK;
	}

	// How the scene's lights fall on the first hit (sdfr_query_ray_lighting, sdfr_pick_lighting, sdfr_mesh_lighting in sdfr.h): hits and
	// lights ([n][8] samples) may be null; pickLighting with pixels_xy null is the whole frame, n = width * height.
	bool queryRayLighting(int64_t n, const float *origins, const float *dirs, sdfr_hit *hits, sdfr_lighting *lighting, sdfr_light_sample *lights,
		float max_distance = 0.f, bool on_host = true)
	{
		return handle && pushState() && sdfr_query_ray_lighting(handle, n, origins, dirs, max_distance, hits, lighting, lights, on_host ? 1 : 0) == SDFR_OK;
	}
	bool pickLighting(const Camera &camera, int width, int height, int64_t n, const int32_t *pixels_xy, sdfr_hit *hits, sdfr_lighting *lighting,
		sdfr_light_sample *lights, bool on_host = true)
	{
		return handle && pushState(&camera) && sdfr_pick_lighting(handle, width, height, n, pixels_xy, hits, lighting, lights, on_host ? 1 : 0) == SDFR_OK;
	}
	bool meshLighting(int64_t n, const float *positions, const float *normals, float reach, sdfr_hit *hits, sdfr_lighting *lighting,
		sdfr_light_sample *lights, bool on_host = true)
	{
		return handle && pushState() && sdfr_mesh_lighting(handle, n, positions, normals, reach, hits, lighting, lights, on_host ? 1 : 0) == SDFR_OK;
	}

	// Ambient occlusion (sdfr_query_occlusion, sdfr_hit_occlusion in sdfr.h): which of 64 fixed directions above each point, or each hit
	// of a query, meet the scene within `radius`.
	bool queryOcclusion(int64_t n, const float *points, const float *normals, float bias, float radius, sdfr_occlusion *out, bool on_host = true)
	{
		return handle && pushState() && sdfr_query_occlusion(handle, n, points, normals, bias, radius, out, on_host ? 1 : 0) == SDFR_OK;
	}
	bool hitOcclusion(int64_t n, const sdfr_hit *hits, float bias, float radius, sdfr_occlusion *out, bool on_host = true)
	{
		return handle && pushState() && sdfr_hit_occlusion(handle, n, hits, bias, radius, out, on_host ? 1 : 0) == SDFR_OK;
	}

	// The loaded scene as a triangle mesh (sdfr_mesh_extract in sdfr.h: surface nets over `grid`), with this renderer's variables and
	// time.  counts is always filled; the arrays only if both capacities suffice (capacities 0, arrays null: the counting call).
	bool extractMesh(const sdfr_mesh_grid &grid, int64_t vertex_capacity, int64_t triangle_capacity, float *positions, float *normals, uint32_t *indices,
		sdfr_mesh_counts &counts, bool on_host = true)
	{
		return handle && pushState() &&
			sdfr_mesh_extract(handle, &grid, vertex_capacity, triangle_capacity, positions, normals, indices, &counts, on_host ? 1 : 0) == SDFR_OK;
	}
	// ... with the vertices on the scene's edges and corners (sdfr_mesh_extract_sharp in sdfr.h): the same counts and indices
	bool extractMeshSharp(const sdfr_mesh_grid &grid, int64_t vertex_capacity, int64_t triangle_capacity, float *positions, float *normals, uint32_t *indices,
		sdfr_mesh_counts &counts, bool on_host = true)
	{
		return handle && pushState() &&
			sdfr_mesh_extract_sharp(handle, &grid, vertex_capacity, triangle_capacity, positions, normals, indices, &counts, on_host ? 1 : 0) == SDFR_OK;
	}

	// Where the surface is (sdfr_mesh_survey and sdfr_mesh_fit in sdfr.h), with this renderer's variables and time: what the lattice of
	// `grid` holds, counted in integers; and `search` (up to 2^20 cells per axis) shrunk onto the surface coarse to fine -- out.grid is
	// then what extractMesh takes, if out.state == SDFR_FIT_FOUND.
	bool surveyMesh(const sdfr_mesh_grid &grid, float band, sdfr_mesh_survey_result &out)
	{
		return handle && pushState() && sdfr_mesh_survey(handle, &grid, band, &out) == SDFR_OK;
	}
	bool fitMesh(const sdfr_mesh_grid &search, int levels, int margin, sdfr_mesh_fit_result &out)
	{
		return handle && pushState() && sdfr_mesh_fit(handle, &search, levels, margin, &out) == SDFR_OK;
	}

	// Whether the solid is in one piece (sdfr_components_label and sdfr_components_label_lattice in sdfr.h): the 6-connected parts and
	// voids of the lattice of `grid`, with this renderer's variables and time, or of the caller's `lattice` of distances, which needs no
	// scene.  counts is always filled, labels ([points], may be null) whenever given; records only if the components fit the capacity
	// (capacity 0, records null: the counting call).
	bool labelComponents(const sdfr_mesh_grid &grid, int64_t capacity, sdfr_component *records, uint32_t *labels, sdfr_component_counts &counts, bool on_host = true)
	{
		return handle && pushState() && sdfr_components_label(handle, &grid, capacity, records, labels, &counts, on_host ? 1 : 0) == SDFR_OK;
	}
	bool labelLattice(const sdfr_mesh_grid &grid, const float *lattice, int64_t capacity, sdfr_component *records, uint32_t *labels, sdfr_component_counts &counts,
		bool on_host = true)
	{
		return handle && sdfr_components_label_lattice(handle, &grid, lattice, capacity, records, labels, &counts, on_host ? 1 : 0) == SDFR_OK;
	}

	// The loaded scene's contours on a stack of planes (sdfr_slice_extract in sdfr.h: marching squares over `grid`), with this renderer's
	// variables and time.  counts and the two layer arrays ([layers + 1], host, may be null) are always filled; positions, coords (may be
	// null) and segments only if both capacities suffice (capacities 0, arrays null: the counting call).
	bool extractSlices(const sdfr_slice_grid &grid, int64_t vertex_capacity, int64_t segment_capacity, float *positions, float *coords, uint32_t *segments,
		int64_t *layer_vertices, int64_t *layer_segments, sdfr_slice_counts &counts, bool on_host = true)
	{
		return handle && pushState() &&
			sdfr_slice_extract(handle, &grid, vertex_capacity, segment_capacity, positions, coords, segments, layer_vertices, layer_segments, &counts,
				on_host ? 1 : 0) == SDFR_OK;
	}

	// The intervals of rays that lie inside the solid (sdfr_query_ray_spans, sdfr_pick_spans, sdfr_mesh_spans in sdfr.h), with this
	// renderer's variables and time: one summary per item, and its first params.max_spans spans (spans may be null if that is 0).
	// pickSpans with pixels_xy null: every pixel of the frame, n = width * height.
	bool querySpans(int64_t n, const float *origins, const float *dirs, const sdfr_span_params &params, sdfr_span_summary *summaries, sdfr_span *spans,
		bool on_host = true)
	{
		return handle && pushState() && sdfr_query_ray_spans(handle, n, origins, dirs, &params, summaries, spans, on_host ? 1 : 0) == SDFR_OK;
	}
	bool pickSpans(int width, int height, int64_t n, const int32_t *pixels_xy, const sdfr_span_params &params, sdfr_span_summary *summaries, sdfr_span *spans,
		bool on_host = true)
	{
		return handle && pushState() && sdfr_pick_spans(handle, width, height, n, pixels_xy, &params, summaries, spans, on_host ? 1 : 0) == SDFR_OK;
	}
	bool meshSpans(int64_t n, const float *positions, const float *normals, float reach, const sdfr_span_params &params, sdfr_span_summary *summaries,
		sdfr_span *spans, bool on_host = true)
	{
		return handle && pushState() && sdfr_mesh_spans(handle, n, positions, normals, reach, &params, summaries, spans, on_host ? 1 : 0) == SDFR_OK;
	}

	// How much solid there is (sdfr_measure, sdfr_measure_properties in sdfr.h), with this renderer's variables and time: the moments of
	// the solid over the columns of `grid`, marched under params (max_spans 0), integrated and summed on the GPU in a defined order;
	// columns: null, or one record per column (host memory, or device memory with on_host false).  measureProperties: volume, mass,
	// centre of mass and inertia tensor from a result, on the host.
	bool measure(const sdfr_measure_grid &grid, const sdfr_span_params &params, sdfr_measure_result &out, sdfr_measure_column *columns = nullptr, bool on_host = true)
	{
		return handle && pushState() && sdfr_measure(handle, &grid, &params, &out, columns, on_host ? 1 : 0) == SDFR_OK;
	}
	static bool measureProperties(const sdfr_measure_grid &grid, const sdfr_measure_result &result, double density, sdfr_solid_properties &out)
	{
		return sdfr_measure_properties(&grid, &result, density, &out) == SDFR_OK;
	}

	// The texture atlas of an extracted mesh (sdfr_atlas_layout, sdfr_atlas_uvs, sdfr_atlas_texels, sdfr_atlas_bake in sdfr.h): one square
	// tile of texels per quad.  atlasTexels looks at the mesh alone; bakeAtlas looks at every texel as meshSurfaces / meshLighting look at
	// a vertex, with this renderer's variables and time.  layers: SDFR_ATLAS_*; a plane that is not asked for may be null.
	static bool atlasLayout(int64_t triangles, int tile, int width, sdfr_atlas &out) { return sdfr_atlas_layout(triangles, tile, width, &out) == SDFR_OK; }
	static bool atlasUVs(const sdfr_atlas &atlas, float *uvs) { return sdfr_atlas_uvs(&atlas, uvs) == SDFR_OK; }
	bool atlasTexels(const sdfr_atlas &atlas, int64_t vertex_count, const float *positions, const float *normals, const uint32_t *indices, float *texel_positions,
		float *texel_normals, int32_t *valid, bool on_host = true)
	{
		return handle && sdfr_atlas_texels(handle, &atlas, vertex_count, positions, normals, indices, texel_positions, texel_normals, valid, on_host ? 1 : 0) == SDFR_OK;
	}
	bool bakeAtlas(const sdfr_atlas &atlas, int64_t vertex_count, const float *positions, const float *normals, const uint32_t *indices, float reach, uint32_t layers,
		float *albedo, float *normal, float *lit, int32_t *valid, bool on_host = true)
	{
		return handle && pushState() &&
			sdfr_atlas_bake(handle, &atlas, vertex_count, positions, normals, indices, reach, layers, albedo, normal, lit, valid, on_host ? 1 : 0) == SDFR_OK;
	}

	// two frames in flight inside this renderer (sdfr_set_frames_in_flight): render into two targets in turn, sync() waits for both
	bool setFramesInFlight(int n) { return sdfr_set_frames_in_flight(handle, n) == SDFR_OK; }
	bool sync() { return sdfr_sync(handle) == SDFR_OK; }
	const char *lastError() const { return sdfr_last_error(handle); }
	sdfr_renderer *native() { return handle; }

private:
	// what render() hands the library before it renders, and the queries too: the variables, the time and (if given) the camera
	bool pushState(const Camera *camera = nullptr)
	{
		for (const auto &kv : variables) sdfr_var_set(handle, kv.first.c_str(), kv.second.value);
		if (camera)
		{
			const float eye[3] = {camera->eye.x, camera->eye.y, camera->eye.z};
			const float tgt[3] = {camera->target.x, camera->target.y, camera->target.z};
			const int rc = camera->target_is_direction ? sdfr_set_camera_direction(handle, eye, tgt, camera->fovy, camera->aspect, camera->roll)
													   : sdfr_set_camera_lookat(handle, eye, tgt, camera->fovy, camera->aspect, camera->roll);
			if (rc != SDFR_OK) return false;
		}
		sdfr_set_time(handle, stime); // (as render() always did: a time the library refuses leaves the last one)
		return true;
	}

	bool refreshVariables()
	{
		variables.clear();
		const int n = sdfr_var_count(handle);
		for (int i = 0; i < n; ++i)
		{
			sdfr_variable v;
			if (sdfr_var_info(handle, i, &v) != SDFR_OK) return false;
			variables[v.name] = Variable{v.minval, v.maxval, v.start, v.step, v.value};
		}
		return true;
	}

	sdfr_renderer *handle = nullptr;
	VariableMap variables;
	float stime = 0.f;
};

} // namespace sdfr

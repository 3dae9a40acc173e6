// sdfr_api.cpp -- implementation of the C ABI declared in include/sdfr.h.
//
// Host logic only: handle state (scene, variable table, camera, limits), per-frame uniform
// preparation, device buffers and launches.  All pixels are produced by the HIP kernels in
// sdfr_kernels.hip; there is no CPU rendering path.
#include "sdfr_aa_plan.h"
#include "sdfr_atlas_plan.h"
#include "sdfr_components_plan.h"
#include "sdfr_handle.h"
#include "sdfr_hlsl_translate.h"
#include "sdfr_mesh_plan.h"
#include "sdfr_slice_plan.h"
#include "sdfr_span_plan.h"
#include "sdfr_measure_plan.h"
#include "sdfr_occlusion.h"
#include "sdfr_query.h"
#include "sdfr_query_plan.h"
#include "sdfr_resolve.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

using namespace sdfr;

// VAR_ tags of the raymarch driver itself (reference: pshader_sdf.hlsl:88-90,97-99,108,142)
static const char *k_driver_variables =
	"VAR_debug_x(min = -10, max = +10, step = 0.02) VAR_debug_y(min = -10, max = +10, step = 0.02) "
	"VAR_debug_z(min = -10, max = +10, step = 0.02) VAR_debug_nx(min = -1, max = +1, step = 0.02) "
	"VAR_debug_ny(min = -1, max = +1, step = 0.02) VAR_debug_nz(min = -1, max = +1, step = 0.02) "
	"VAR_show_objects(min = 0, max = 1, step = 1, start = 1) VAR_debug_scale(min = 0.005, max = 2, step = 0.005, start = 0.2)";


namespace sdfr {
size_t image_bytes(size_t pixels, int format)
{
	if (format == SDFR_RGBA32F) return pixels * 16;
	if (format == SDFR_RGBA16F) return pixels * 8;
	if (format == SDFR_STRIP_RGB16F_A8) return (pixels * 7 + 3) & ~(size_t)3;
	return (pixels * 13 + 3) & ~(size_t)3;
}
bool is_wire_format(int format)
{
	return format == SDFR_RGBA32F || format == SDFR_RGBA16F || format == SDFR_STRIP_RGB32F_A8 || format == SDFR_STRIP_RGB16F_A8;
}
} // namespace sdfr

static void free_workspace(sdfr_renderer::Lane &l)
{
	WavefrontWorkspace &w = l.ws;
	(void)hipFree(w.ray_cur);
	(void)hipFree(w.ray_queue);
	(void)hipFree(w.qdepth_lo);
	(void)hipFree(w.qdepth_hi);
	(void)hipFree(w.result);
	(void)hipFree(w.accum);
	(void)hipFree(w.list_a);
	(void)hipFree(w.list_b);
	(void)hipFree(w.counters);
	(void)hipFree(w.partials);
	(void)hipFree(w.tile_cursors);
	w = WavefrontWorkspace{};
	l.wavefront_capacity = 0;
}

// Per-pixel scratch of lane `l` sized for `pixels` work items.  Both schedules use the pending-ray queue and
// the counter partials; the per-round state of the wavefront schedule (another 116 B per pixel)
// is allocated only once that schedule is used.  On failure everything is released (hipFree
// waits for the device, so buffers of frames still in flight are safe to drop).
static int ensure_workspace(sdfr_renderer *r, sdfr_renderer::Lane &l, size_t pixels, bool wavefront)
{
	WavefrontWorkspace &w = l.ws;
	// the pixel kernel indexes the pending-ray records with 32 bits (GlobalRayStore::record)
	if (pixels * (size_t)SDFR_MAX_RAYS >= ((size_t)1 << 32)) return fail(r, SDFR_ERR_INVALID_ARGUMENT, "frame too large: more than 2^32 / 8 pixels per launch");
	if (w.capacity < pixels || (wavefront && l.wavefront_capacity < pixels))
	{
		if (w.capacity < pixels) free_workspace(l);
		const size_t n = w.capacity < pixels ? pixels : w.capacity;
		hipError_t e = hipSuccess;
		auto alloc = [&](void **p, size_t bytes) {
			if (e == hipSuccess && *p == nullptr) e = hipMalloc(p, bytes);
		};
		alloc((void **)&w.ray_queue, sizeof(float) * 12 * SDFR_MAX_RAYS * n); // 48-byte records (pixel schedule) / 11 field arrays (wavefront)
		alloc((void **)&w.partials, sizeof(RenderTotals) * (n / 64 + 1));
		if (e == hipSuccess && w.tile_cursors == nullptr)
		{
			alloc((void **)&w.tile_cursors, sizeof(uint32_t) * (size_t)pixel_tile_cursor_words());
			// on the stream of the launch that uses them: hipMemset runs on the null stream, which the non-blocking streams of
			// two frames in flight do not wait for -- a launch could take tiles from cursors not yet cleared
			if (e == hipSuccess) e = hipMemsetAsync(w.tile_cursors, 0, sizeof(uint32_t) * (size_t)pixel_tile_cursor_words(), l.stream);
		}
		if (wavefront)
		{
			alloc((void **)&w.ray_cur, sizeof(float) * 11 * n);
			alloc((void **)&w.qdepth_lo, sizeof(uint32_t) * n);
			alloc((void **)&w.qdepth_hi, sizeof(uint32_t) * n);
			alloc((void **)&w.result, sizeof(float) * 8 * n);
			alloc((void **)&w.accum, sizeof(float) * 4 * n);
			alloc((void **)&w.list_a, sizeof(uint32_t) * n);
			alloc((void **)&w.list_b, sizeof(uint32_t) * n);
			alloc((void **)&w.counters, sizeof(uint32_t) * 64);
		}
		if (e != hipSuccess)
		{
			free_workspace(l);
			return hip_fail(r, e, "workspace allocation");
		}
		w.capacity = n;
		if (wavefront) l.wavefront_capacity = n;
		w.pstat = nullptr;
	}
	return SDFR_OK;
}

// the counters and events of a lane; its stream is the caller's to set
static hipError_t create_lane(sdfr_renderer::Lane &l)
{
	hipError_t e = hipMalloc((void **)&l.d_totals, 2 * sizeof(RenderTotals));
	if (e == hipSuccess) e = hipEventCreate(&l.ev_begin);
	if (e == hipSuccess) e = hipEventCreate(&l.ev_end);
	return e;
}
// frees what create_lane and ensure_workspace gave the lane (its stream is the caller's) and empties it
static void release_lane(sdfr_renderer::Lane &l)
{
	free_workspace(l);
	(void)hipFree(l.d_totals);
	if (l.ev_begin) (void)hipEventDestroy(l.ev_begin);
	if (l.ev_end) (void)hipEventDestroy(l.ev_end);
	l = sdfr_renderer::Lane();
}
// waits for every frame in flight: the current lane and, with two frames in flight, the other one
static int sync_lanes(sdfr_renderer *r)
{
	SDFR_HIP(hipStreamSynchronize(r->lane.stream));
	if (r->frames_in_flight == 2) SDFR_HIP(hipStreamSynchronize(r->other.stream));
	return SDFR_OK;
}
// back to one frame in flight: the current lane keeps its workspace and runs on the caller's stream again.  The handle's two own
// streams stay (own_streams): events that outlive this -- the lane's ev_begin / ev_end, ev_mesh -- were last recorded on them
static void release_second_lane(sdfr_renderer *r)
{
	if (r->frames_in_flight != 2) return;
	(void)sync_lanes(r);
	release_lane(r->other);
	r->lane.stream = r->user_stream;
	r->frames_in_flight = 1;
}

// the reference's camera (Camera.h) as the camera entries configure it; the caller aims it (SetLookat / SetDirection)
static host::Camera make_camera(float fovy, float aspect, float roll, const host::Vec3 &eye)
{
	host::Camera cam;
	cam.SetAspect(aspect);
	cam.SetFOVY(fovy);
	cam.SetRoll(roll);
	cam.SetEye(eye);
	return cam;
}
static int set_camera_from(sdfr_renderer *r, const host::Camera &cam)
{
	host::Vec3 e, f, rt, tp;
	cam.GetBasis(e, f, rt, tp);
	r->U.eye = V3(e.x, e.y, e.z);
	r->U.front = V3(f.x, f.y, f.z);
	r->U.right = V3(rt.x, rt.y, rt.z);
	r->U.top = V3(tp.x, tp.y, tp.z);
	return SDFR_OK;
}

// the limits of sdfr_limits and where the frame keeps them: copy(limit, frame's) for each, in either direction
template <class Limits, class Frame, class Copy>
static void for_each_limit(Limits &l, Frame &U, Copy copy)
{
	copy(l.iter_count, U.iter_count);
	copy(l.bounce_count, U.bounce_count);
	copy(l.ray_count, U.ray_count);
	copy(l.light_count, U.light_count);
	copy(l.range, U.range);
	copy(l.max_cost_default, U.max_cost_default); // (unsigned in the frame)
	copy(l.extension_lights, U.extension_lights);
	copy(l.extension_marble_reflection, U.extension_marble_reflection);
	copy(l.dist_eps, U.dist_eps);
	copy(l.grad_eps, U.grad_eps);
	copy(l.reflect_eps, U.reflect_eps);
	copy(l.refract_eps, U.refract_eps);
	copy(l.shadow_eps, U.shadow_eps);
}

extern "C" {

int sdfr_set_frames_in_flight(sdfr_renderer *r, int n)
{
	return guarded(r, [&]() -> int {
		if (!r || (n != 1 && n != 2)) return SDFR_ERR_INVALID_ARGUMENT;
		SDFR_HIP(hipSetDevice(r->device));
		if (n == r->frames_in_flight) return SDFR_OK;
		if (n == 1)
		{
			release_second_lane(r);
			return SDFR_OK;
		}
		SDFR_HIP(hipStreamSynchronize(r->lane.stream));
		sdfr_renderer::Lane second;
		hipError_t e = hipSuccess;
		for (hipStream_t &s : r->own_streams)
			if (!s && e == hipSuccess) e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
		if (e == hipSuccess) e = create_lane(second);
		if (e != hipSuccess)
		{
			release_lane(second);
			return hip_fail(r, e, "sdfr_set_frames_in_flight");
		}
		second.stream = r->own_streams[1];
		r->lane.stream = r->own_streams[0]; // the current lane's from now on: it keeps its workspace and the row order it has learned
		r->lane.out_lo = r->lane.out_hi = nullptr;
		r->lane.pst_lo = r->lane.pst_hi = nullptr;
		r->other = second;
		r->frames_in_flight = 2;
		return SDFR_OK;
	});
}

int sdfr_wait_frame(sdfr_renderer *r, void *hip_stream)
{
	return guarded(r, [&]() -> int {
		if (!r) return SDFR_ERR_INVALID_ARGUMENT;
		if (!r->lane.have_render) return SDFR_OK;
		SDFR_HIP(hipSetDevice(r->device));
		SDFR_HIP(hipStreamWaitEvent((hipStream_t)hip_stream, r->lane.ev_end, 0));
		return SDFR_OK;
	});
}

int sdfr_create(int device_ordinal, sdfr_renderer **out)
{
	return guarded(nullptr, [&]() -> int {
		if (!out) return SDFR_ERR_INVALID_ARGUMENT;
		*out = nullptr;
		int count = 0;
		if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return SDFR_ERR_NO_DEVICE;
		if (device_ordinal < 0 || device_ordinal >= count) return SDFR_ERR_INVALID_ARGUMENT;
		if (hipSetDevice(device_ordinal) != hipSuccess) return SDFR_ERR_HIP;
		sdfr_renderer *r = new sdfr_renderer();
		r->device = device_ordinal;
		if (const char *t = getenv("SDFR_TILE_W_LOG2")) // developer knob: wave tile shape (3 = 8x8 ... 6 = 64x1)
		{
			int v = atoi(t);
			if (v >= 3 && v <= 6) r->tile_w_log2 = v;
		}
		if (const char *t = getenv("SDFR_STEP_SHORTCUTS")) r->step_shortcuts = atoi(t) != 0; // default of sdfr_set_step_shortcuts
		frame_defaults(r->U);
		// start-up camera of the reference (Application.cpp:214-224), aspect of its 1200x800 window
		host::Camera cam = make_camera(60.f * 3.14159265358979f / 180.f, 1200.f / 800.f, 0.f, host::Vec3(0.f, 2.f, -3.f));
		cam.SetLookat(host::Vec3(0.f, 1.f, 0.f));
		set_camera_from(r, cam);
		if (create_lane(r->lane) != hipSuccess)
		{
			release_lane(r->lane);
			delete r;
			return SDFR_ERR_HIP;
		}
		for (int i = 0; i < 32; ++i)
		{
			if (i < 3) (void)hipEventCreate(&r->ev_post[i]);
			(void)hipEventCreate(&r->ev_march[i]);
			(void)hipEventCreate(&r->ev_shade[i]);
		}
		*out = r;
		return SDFR_OK;
	});
}

void sdfr_destroy(sdfr_renderer *r)
{
	if (!r) return;
	(void)hipSetDevice(r->device);
	(void)hipStreamSynchronize(r->lane.stream);
	if (r->comm_stream) (void)hipStreamSynchronize(r->comm_stream);
	comm_forget_renderer(r);
	release_second_lane(r); // waits for it, frees its workspace, counters and events
	release_lane(r->lane);
	jit_unload(r->jit);
	for (sdfr_device_buffer *b : {&r->stage, &r->pstat, &r->query, &r->mesh, &r->wire, &r->post_flags, &r->aa_color, &r->aa_stats, &r->aa_totals}) b->release();
	if (r->ev_aa_done) (void)hipEventDestroy(r->ev_aa_done);
	for (hipEvent_t e : r->ev_aa) (void)hipEventDestroy(e);
	for (hipEvent_t e : r->ev_mesh)
		if (e) (void)hipEventDestroy(e);
	if (r->pinned_host) (void)hipHostUnregister(r->pinned_host);
	if (r->comm_stream) (void)hipStreamDestroy(r->comm_stream);
	if (r->ev_strips) (void)hipEventDestroy(r->ev_strips);
	if (r->ev_gathered) (void)hipEventDestroy(r->ev_gathered);
	for (hipEvent_t e : r->ev_xfer)
		if (e) (void)hipEventDestroy(e);
	for (hipEvent_t e : r->ev_post) (void)hipEventDestroy(e);
	for (int i = 0; i < 32; ++i)
	{
		(void)hipEventDestroy(r->ev_march[i]);
		(void)hipEventDestroy(r->ev_shade[i]);
	}
	for (hipStream_t s : r->own_streams) // after every event that was recorded on them
		if (s) (void)hipStreamDestroy(s);
	delete r;
}

const char *sdfr_last_error(const sdfr_renderer *r) { return r ? r->error.c_str() : "null handle"; }

int sdfr_set_stream(sdfr_renderer *r, void *hip_stream)
{
	return guarded(r, [&]() -> int {
		if (!r) return SDFR_ERR_INVALID_ARGUMENT;
		r->user_stream = (hipStream_t)hip_stream;
		if (r->frames_in_flight == 1) r->lane.stream = r->user_stream; // (two frames in flight run on the handle's own two streams)
		return SDFR_OK;
	});
}

int sdfr_scene_count(void) { return SDFR_PUBLIC_SCENE_COUNT; }
const char *sdfr_scene_name(int index) { return index >= 0 && index < SDFR_PUBLIC_SCENE_COUNT ? scene_name(index) : nullptr; }

// rebuild the variable table like SDFRenderer::initShader (SDFRenderer.cpp:35-47): clear, then
// collect the tags of the driver and of the scene text
static int build_variable_table(sdfr_renderer *r, const std::string &scene_text, host::ShaderVariableManager &vm, std::vector<std::string> &slots)
{
	// scene slots: distinct names of the scene's tags in order of appearance
	std::vector<std::string_view> code, tags;
	host::split_tagged(scene_text, "VAR_", ")", code, tags);
	for (std::string_view t : tags)
	{
		const size_t lb = t.find('(');
		if (lb == std::string_view::npos || lb <= 4) return fail(r, SDFR_ERR_INVALID_ARGUMENT, "malformed VAR_ tag: '" + std::string(t) + "'");
		std::string nm(t.substr(4, lb - 4));
		for (char c : nm)
			if (!isalnum((unsigned char)c) && c != '_') return fail(r, SDFR_ERR_INVALID_ARGUMENT, "malformed VAR_ tag: '" + std::string(t) + "'");
		bool seen = false;
		for (const auto &s : slots) seen = seen || s == nm;
		if (!seen) slots.push_back(nm);
	}
	if (slots.size() > SDFR_MAX_SCENE_VARS) return fail(r, SDFR_ERR_INVALID_ARGUMENT, "too many scene variables");
	try
	{
		if (!vm.parseFile(std::string(k_driver_variables) + " " + scene_text)) return fail(r, SDFR_ERR_INVALID_ARGUMENT, "malformed VAR_ tag");
	}
	catch (const std::exception &) // a value that is not a number
	{
		return fail(r, SDFR_ERR_INVALID_ARGUMENT, "malformed VAR_ tag: value is not a number");
	}
	return SDFR_OK;
}

// the last step of every load: the handle takes the scene (an index, or SDFR_SCENE_COUNT: r->jit) with its variable table and slots
static int install_scene(sdfr_renderer *r, int scene, const host::ShaderVariableManager &vm, const std::vector<std::string> &slots)
{
	r->vars = vm;
	r->scene_var_slots = slots;
	r->scene = scene;
	return SDFR_OK;
}

// Scenes compiled at run time, in the library's own form or (hlsl) in the reference's dialect (sdfr_hlsl.h / sdfr_hlsl.cpp).  The
// variable table of a dialect scene comes from the tags of the ORIGINAL text (ShaderUtil.cpp:122-191); the class generated from it
// (hlsl_scene_source) reads them through the same VAR_<name>(...) macros as any run-time scene.  Tags first: a text whose tags
// are malformed is neither translated nor compiled.
static int load_runtime_scene(sdfr_renderer *r, const char *name, const char *text, bool hlsl)
{
	SDFR_HIP(hipSetDevice(r->device));
	host::ShaderVariableManager vm;
	std::vector<std::string> slots;
	int rc = build_variable_table(r, text, vm, slots);
	if (rc != SDFR_OK) return rc;
	JitScene js;
	std::string err;
	// like the reference, a scene that fails to compile leaves the previous one in place
	// (SceneManager.cpp:118-127 keeps the old shader and shows the compiler's message)
	if (!jit_compile(r->device, name, hlsl ? hlsl_scene_source(text) : std::string(text), slots, js, err)) return fail(r, SDFR_ERR_COMPILE, err);
	rc = sync_lanes(r); // the frame before may still run the old module
	if (rc != SDFR_OK) return rc;
	jit_unload(r->jit);
	r->jit = js;
	return install_scene(r, SDFR_SCENE_COUNT, vm, slots);
}
static int check_runtime_scene(const char *text, bool hlsl, const char *arch, char *log, size_t log_bytes)
{
	if (log && log_bytes) log[0] = 0;
	sdfr_renderer scratch; // only its error string is used
	host::ShaderVariableManager vm;
	std::vector<std::string> slots;
	std::string err;
	int rc = build_variable_table(&scratch, text, vm, slots);
	if (rc != SDFR_OK) err = scratch.error;
	std::vector<char> code;
	if (rc == SDFR_OK && !jit_compile_code(arch && arch[0] ? arch : "gfx950", "scene", hlsl ? hlsl_scene_source(text) : std::string(text), slots, code, err))
		rc = SDFR_ERR_COMPILE;
	if (rc != SDFR_OK && log && log_bytes) snprintf(log, log_bytes, "%s", err.c_str());
	return rc;
}

int sdfr_load_scene(sdfr_renderer *r, const char *name)
{
	return guarded(r, [&]() -> int {
		if (!r || !name) return SDFR_ERR_INVALID_ARGUMENT;
		const int idx = scene_index(name);
		if (idx < 0) return fail(r, SDFR_ERR_UNKNOWN_SCENE, std::string("unknown scene '") + name + "'");
		host::ShaderVariableManager vm;
		std::vector<std::string> slots;
		const int rc = build_variable_table(r, scene_variables(idx), vm, slots);
		if (rc != SDFR_OK) return rc;
		return install_scene(r, idx, vm, slots);
	});
}

int sdfr_check_scene_source(const char *source, const char *arch, char *log, size_t log_bytes)
{
	return guarded(nullptr, [&]() -> int { return source ? check_runtime_scene(source, false, arch, log, log_bytes) : SDFR_ERR_INVALID_ARGUMENT; });
}

int sdfr_translate_scene_hlsl(const char *hlsl_source, char *out, size_t out_bytes)
{
	return guarded(nullptr, [&]() -> int {
		if (!hlsl_source) return SDFR_ERR_INVALID_ARGUMENT;
		const std::string text = hlsl_scene_source(hlsl_source);
		if (out && out_bytes) snprintf(out, out_bytes, "%s", text.c_str());
		return (int)text.size() + 1;
	});
}

int sdfr_check_scene_hlsl(const char *hlsl_source, const char *arch, char *log, size_t log_bytes)
{
	return guarded(nullptr, [&]() -> int { return hlsl_source ? check_runtime_scene(hlsl_source, true, arch, log, log_bytes) : SDFR_ERR_INVALID_ARGUMENT; });
}

int sdfr_load_scene_hlsl(sdfr_renderer *r, const char *name, const char *hlsl_source)
{
	return guarded(r, [&]() -> int { return r && name && hlsl_source ? load_runtime_scene(r, name, hlsl_source, true) : SDFR_ERR_INVALID_ARGUMENT; });
}

int sdfr_load_scene_source(sdfr_renderer *r, const char *name, const char *source)
{
	return guarded(r, [&]() -> int { return r && name && source ? load_runtime_scene(r, name, source, false) : SDFR_ERR_INVALID_ARGUMENT; });
}

const char *sdfr_current_scene(const sdfr_renderer *r)
{
	if (!r || r->scene < 0) return nullptr;
	return r->scene == SDFR_SCENE_COUNT ? r->jit.name.c_str() : scene_name(r->scene);
}

int sdfr_var_count(const sdfr_renderer *r) { return r ? (int)r->vars.getVariables().size() : SDFR_ERR_INVALID_ARGUMENT; }

int sdfr_var_info(const sdfr_renderer *r, int index, sdfr_variable *out)
{
	return guarded(r, [&]() -> int {
		if (!r || !out) return SDFR_ERR_INVALID_ARGUMENT;
		const auto &m = r->vars.getVariables();
		if (index < 0 || index >= (int)m.size()) return fail(r, SDFR_ERR_INVALID_ARGUMENT, "variable index out of range");
		auto it = m.begin();
		std::advance(it, index);
		memset(out, 0, sizeof *out);
		snprintf(out->name, sizeof out->name, "%s", it->first.c_str());
		out->minval = it->second.minval;
		out->maxval = it->second.maxval;
		out->start = it->second.start;
		out->step = it->second.step;
		out->value = it->second.value;
		return SDFR_OK;
	});
}

int sdfr_var_set(sdfr_renderer *r, const char *name, float value)
{
	return guarded(r, [&]() -> int {
		if (!r || !name) return SDFR_ERR_INVALID_ARGUMENT;
		if (!r->vars.setValue(name, value)) return fail(r, SDFR_ERR_UNKNOWN_VARIABLE, std::string("unknown variable '") + name + "' (ignored)");
		return SDFR_OK;
	});
}

int sdfr_var_get(const sdfr_renderer *r, const char *name, float *out)
{
	return guarded(r, [&]() -> int {
		if (!r || !name || !out) return SDFR_ERR_INVALID_ARGUMENT;
		const auto &m = r->vars.getVariables();
		auto it = m.find(std::string_view(name));
		if (it == m.end()) return fail(r, SDFR_ERR_UNKNOWN_VARIABLE, std::string("unknown variable '") + name + "'");
		*out = it->second.value;
		return SDFR_OK;
	});
}

int sdfr_vars_reset(sdfr_renderer *r)
{
	return guarded(r, [&]() -> int {
		if (!r) return SDFR_ERR_INVALID_ARGUMENT;
		for (auto &kv : r->vars.getVariables()) kv.second.value = kv.second.start;
		return SDFR_OK;
	});
}

int sdfr_set_camera(sdfr_renderer *r, const float eye[3], const float front[3], const float right[3], const float top[3])
{
	return guarded(r, [&]() -> int {
		if (!r || !eye || !front || !right || !top) return SDFR_ERR_INVALID_ARGUMENT;
		r->U.eye = V3(eye[0], eye[1], eye[2]);
		r->U.front = V3(front[0], front[1], front[2]);
		r->U.right = V3(right[0], right[1], right[2]);
		r->U.top = V3(top[0], top[1], top[2]);
		return SDFR_OK;
	});
}

int sdfr_set_camera_lookat(sdfr_renderer *r, const float eye[3], const float lookat[3], float fovy, float aspect, float roll)
{
	return guarded(r, [&]() -> int {
		if (!r || !eye || !lookat) return SDFR_ERR_INVALID_ARGUMENT;
		host::Camera cam = make_camera(fovy, aspect, roll, host::Vec3(eye[0], eye[1], eye[2]));
		cam.SetLookat(host::Vec3(lookat[0], lookat[1], lookat[2]));
		return set_camera_from(r, cam);
	});
}

int sdfr_set_camera_direction(sdfr_renderer *r, const float eye[3], const float direction[3], float fovy, float aspect, float roll)
{
	return guarded(r, [&]() -> int {
		if (!r || !eye || !direction) return SDFR_ERR_INVALID_ARGUMENT;
		host::Camera cam = make_camera(fovy, aspect, roll, host::Vec3(eye[0], eye[1], eye[2]));
		cam.SetDirection(host::Vec3(direction[0], direction[1], direction[2]));
		return set_camera_from(r, cam);
	});
}

int sdfr_get_camera(const sdfr_renderer *r, float out[12])
{
	return guarded(r, [&]() -> int {
		if (!r || !out) return SDFR_ERR_INVALID_ARGUMENT;
		const vec3 v[4] = {r->U.eye, r->U.front, r->U.right, r->U.top};
		for (int i = 0; i < 4; ++i)
		{
			out[3 * i + 0] = v[i].x;
			out[3 * i + 1] = v[i].y;
			out[3 * i + 2] = v[i].z;
		}
		return SDFR_OK;
	});
}

int sdfr_set_time(sdfr_renderer *r, float stime)
{
	return guarded(r, [&]() -> int {
		if (!r) return SDFR_ERR_INVALID_ARGUMENT;
		r->U.stime = stime;
		return SDFR_OK;
	});
}

int sdfr_get_limits(const sdfr_renderer *r, sdfr_limits *out)
{
	return guarded(r, [&]() -> int {
		if (!r || !out) return SDFR_ERR_INVALID_ARGUMENT;
		for_each_limit(*out, r->U, [](auto &limit, const auto &frame) { limit = frame; });
		return SDFR_OK;
	});
}

int sdfr_set_limits(sdfr_renderer *r, const sdfr_limits *l)
{
	return guarded(r, [&]() -> int {
		if (!r || !l) return SDFR_ERR_INVALID_ARGUMENT;
		if (l->iter_count < 1 || l->iter_count > 0xffffff || l->bounce_count < 0 || l->bounce_count > 16 || l->ray_count < 1 ||
			l->ray_count > SDFR_MAX_RAYS || l->light_count < 0 || l->light_count > SDFR_MAX_LIGHTS || l->max_cost_default < 0 ||
			l->max_cost_default > 250 || !(l->range == l->range) || l->extension_lights < 0 || l->extension_lights > SDFR_MAX_LIGHTS - 1 ||
			!(l->extension_marble_reflection >= 0.f && l->extension_marble_reflection <= 1.f))
			return fail(r, SDFR_ERR_INVALID_ARGUMENT, "limits out of range");
		if (!(l->dist_eps > 0.f && l->dist_eps <= SDFR_MAX_DIST_EPS) || !(l->grad_eps > 0.f && l->grad_eps <= 1.f) || !(l->reflect_eps >= 0.f && l->reflect_eps <= 1.f) ||
			!(l->refract_eps >= 0.f && l->refract_eps <= 1.f) || !(l->shadow_eps >= 0.f && l->shadow_eps <= 1.f))
			return fail(r, SDFR_ERR_INVALID_ARGUMENT, "epsilons out of range (0 < dist_eps <= 1e-3, 0 < grad_eps <= 1, 0 <= reflect_eps, refract_eps, shadow_eps <= 1)");
		for_each_limit(*l, r->U, [](const auto &limit, auto &frame) { frame = limit; });
		return SDFR_OK;
	});
}

int sdfr_set_profiling(sdfr_renderer *r, int enabled)
{
	return guarded(r, [&]() -> int {
		if (!r) return SDFR_ERR_INVALID_ARGUMENT;
		r->profiling = enabled != 0;
		return SDFR_OK;
	});
}

int sdfr_set_launch_mode(sdfr_renderer *r, int mode)
{
	return guarded(r, [&]() -> int {
		if (!r || mode < SDFR_LAUNCH_AUTO || mode > SDFR_LAUNCH_PERSISTENT) return SDFR_ERR_INVALID_ARGUMENT;
		r->launch_mode = mode;
		return SDFR_OK;
	});
}

int sdfr_set_step_shortcuts(sdfr_renderer *r, int enabled)
{
	return guarded(r, [&]() -> int {
		if (!r) return SDFR_ERR_INVALID_ARGUMENT;
		r->step_shortcuts = enabled != 0;
		return SDFR_OK;
	});
}

int sdfr_set_schedule(sdfr_renderer *r, int schedule)
{
	return guarded(r, [&]() -> int {
		if (!r || (schedule != SDFR_SCHEDULE_WAVEFRONT && schedule != SDFR_SCHEDULE_PIXEL)) return SDFR_ERR_INVALID_ARGUMENT;
		r->schedule = schedule;
		return SDFR_OK;
	});
}

int64_t sdfr_strip_buffer_bytes(int width, int height, int world, int format) { return sdfr_strip_buffer_bytes_split(width, height, world, format, 0, 1); }

int64_t sdfr_strip_buffer_bytes_split(int width, int height, int world, int format, int priv_count, int priv_period)
{
	const int64_t n = sdfr_strip_buffer_pixels_split(width, height, world, priv_count, priv_period);
	if (n < 0 || !is_wire_format(format)) return -1;
	return (int64_t)image_bytes((size_t)n, format);
}

int64_t sdfr_strip_buffer_pixels(int width, int height, int world)
{
	return sdfr_strip_buffer_pixels_split(width, height, world, 0, 1);
}

int64_t sdfr_strip_buffer_pixels_split(int width, int height, int world, int priv_count, int priv_period)
{
	if (width < 1 || height < 1 || world < 1 || priv_count < 0 || priv_period < 1 || priv_count >= priv_period) return 0;
	return strip_buffer_pixels(width, height, world, priv_count, priv_period);
}

int sdfr_set_strip_split(sdfr_renderer *r, int priv_count, int priv_period)
{
	return guarded(r, [&]() -> int {
		if (!r || priv_count < 0 || priv_period < 1 || priv_count >= priv_period || priv_period > 4096) return SDFR_ERR_INVALID_ARGUMENT;
		r->priv_count = priv_count;
		r->priv_period = priv_period;
		return SDFR_OK;
	});
}

// the arguments of render_impl, in the order their errors win; a private render without private strips renders nothing
// and needs no scene
static int check_render(sdfr_renderer *r, int width, int height, int rank, int world, const void *out, int format, RenderMode mode)
{
	if (!r || !out) return SDFR_ERR_INVALID_ARGUMENT;
	// an image is RGBA32F or RGBA16F; a strip buffer may also be in one of the packed wire formats
	if (mode == RENDER_STRIPS ? !is_wire_format(format) : format != SDFR_RGBA32F && format != SDFR_RGBA16F) return fail(r, SDFR_ERR_INVALID_ARGUMENT, "bad format");
	if (mode == RENDER_PRIVATE && r->priv_count == 0) return SDFR_OK;
	if (world < 1 || rank < 0 || rank >= world) return fail(r, SDFR_ERR_INVALID_ARGUMENT, "bad rank/world");
	if (r->scene < 0) return fail(r, SDFR_ERR_NO_SCENE, "no scene loaded");
	if (!frame_size_ok(width, height)) return fail(r, SDFR_ERR_INVALID_ARGUMENT, "bad frame size");
	return SDFR_OK;
}

// latch the variable values into the frame uniforms U (the reference uploads them every frame,
// SDFRenderer.cpp:75-78) and derive the per-frame constants; a run-time scene's prepare kernel runs on `stream`
static int latch_into(sdfr_renderer *r, FrameU &U, int width, int height, hipStream_t stream)
{
	U.width = width;
	U.height = height;
	const auto &m = r->vars.getVariables();
	auto val = [&](const char *n) { auto it = m.find(std::string_view(n)); return it != m.end() ? it->second.value : 0.f; };
	U.debug_nx = val("debug_nx");
	U.debug_ny = val("debug_ny");
	U.debug_nz = val("debug_nz");
	U.debug_scale = val("debug_scale");
	U.debug_x = val("debug_x");
	U.debug_y = val("debug_y");
	U.debug_z = val("debug_z");
	U.show_objects = val("show_objects");
	for (int i = 0; i < SDFR_MAX_SCENE_VARS; ++i) U.scene_var[i] = 0.f;
	for (size_t k = 0; k < r->scene_var_slots.size(); ++k) U.scene_var[k] = val(r->scene_var_slots[k].c_str());
	U.step_shortcuts = r->step_shortcuts ? 1 : 0;
	frame_derive(U, r->scene);
	if (r->scene == SDFR_SCENE_COUNT) SDFR_HIP(jit_prepare(r->jit, U, stream));
	return SDFR_OK;
}
// ... the handle's own, for a render
static int latch_frame(sdfr_renderer *r, int width, int height) { return latch_into(r, r->U, width, height, r->lane.stream); }

// The kernels of the loaded scene, built in or compiled at run time: the two places that ask which it is for a launch.
// The pixel kernel for the handle's frame, and how the scene wants it launched ...
static int loaded_pixel_kernel(sdfr_renderer *r, PixelKernel &pk)
{
	const bool dbg = frame_needs_debug(r->U);
	if (r->scene == SDFR_SCENE_COUNT) pk = jit_pixel_kernel(r->jit, dbg);
	else if (!scene_pixel_kernel(r->scene, dbg, pk)) return hip_fail(r, hipErrorInvalidValue, "kernel launch");
	return SDFR_OK;
}
// ... and the query kernel of `kind` (QUERY_KERNEL_*) for frame U; a run-time scene compiles its query module on its first query
static int loaded_query_kernel(sdfr_renderer *r, int kind, const FrameU &U, KernelRef &k)
{
	const QueryKernels *qk = nullptr;
	if (r->scene == SDFR_SCENE_COUNT)
	{
		std::string err;
		const JitQueryStatus js = jit_query_kernels(r->jit, r->device, qk, err);
		if (js != JIT_QUERY_OK) return fail(r, js == JIT_QUERY_COMPILE ? SDFR_ERR_COMPILE : SDFR_ERR_HIP, err);
	}
	else if (!(qk = scene_query_kernels(r->scene)))
		return hip_fail(r, hipErrorInvalidValue, kind == QUERY_KERNEL_LATTICE ? "lattice launch" : "query launch");
	k = qk->k[kind][frame_needs_debug(U) ? 1 : 0];
	return SDFR_OK;
}
// one launch of the loaded scene's kernel of `kind` for frame U with that kind's arguments, in `blocks` blocks of one wave; what: the
// error text of a launch that fails
extern "C++" {
template <class A>
static int launch_loaded(sdfr_renderer *r, int kind, const FrameU &U, const A &args, uint32_t blocks, hipStream_t stream, const char *what)
{
	KernelRef k;
	const int rc = loaded_query_kernel(r, kind, U, k);
	if (rc != SDFR_OK) return rc;
	const hipError_t e = launch_scene_kernel(k, U, args, blocks, stream);
	return e == hipSuccess ? SDFR_OK : hip_fail(r, e, what);
}
} // (a template, inside this file's extern "C")
// one query of the loaded scene, every pointer of `q` device memory
static int run_query(sdfr_renderer *r, const FrameU &U, const QueryArgs &q, hipStream_t stream)
{
	KernelRef k;
	const int rc = loaded_query_kernel(r, query_kernel_of(q), U, k);
	if (rc != SDFR_OK) return rc;
	const hipError_t e = launch_query(k, U, q, stream);
	return e == hipSuccess ? SDFR_OK : hip_fail(r, e, "query launch");
}

// The calls that put a question to the loaded scene without rendering a frame -- the queries (sdfr_query.h, sdfr_surface.h, sdfr_occlusion.h,
// sdfr_lighting.h), the mesh extraction and the texture atlas -- share one protocol: the plan's argument checks, begin_query, for a
// host call stage_host_arrays, the launches, and for a host call copy_answers_back.  The frame is latched into a copy, and nothing a render uses
// or reports is written: not the handle's FrameU or ms_setup, not a lane's workspace, counters, events or row order, not `launches`.
static const size_t k_query_stage_keep = (size_t)64 << 20; // bytes a handle keeps of `query` and of `mesh` between calls
static_assert(sizeof(sdfr_hit) == 4 * QUERY_HIT_WORDS, "sdfr_hit is the query kernels' 12-word record");
static_assert(sizeof(sdfr_surface) == 4 * QUERY_SURFACE_WORDS, "sdfr_surface is the surface kernel's 32-word record");
static_assert(sizeof(sdfr_occlusion) == 4 * QUERY_OCCLUSION_WORDS, "sdfr_occlusion is the occlusion kernel's 4-word record");
static_assert(sizeof(sdfr_lighting) == 4 * QUERY_LIGHTING_WORDS, "sdfr_lighting is the lighting kernel's 16-word record");
static_assert(sizeof(sdfr_light_sample) == 4 * QUERY_LIGHT_SAMPLE_WORDS && SDFR_MAX_LIGHTS == QUERY_LIGHT_SLOTS, "sdfr_light_sample[8] is the lighting kernel's 8 x 20 words");
// What such a call starts with once its arguments stand: the scene, if it needs one; the device; the handle's stream, or the lane of the
// frame submitted last (as sdfr_postprocess); and with a scene its frame of width x height latched into the copy U
static int begin_query(sdfr_renderer *r, bool needs_scene, int width, int height, FrameU &U, hipStream_t &stream)
{
	if (needs_scene && r->scene < 0) return fail(r, SDFR_ERR_NO_SCENE, "no scene loaded");
	SDFR_HIP(hipSetDevice(r->device));
	stream = r->lane.stream;
	if (!needs_scene) return SDFR_OK;
	U = r->U;
	return latch_into(r, U, width, height, stream);
}
// The caller's arrays are host memory: each of `arrays` that is there (bytes > 0) gets its piece of the handle's query buffer, in their
// order.  An input's copy to the device is enqueued, an answer is noted for copy_answers_back, and the field is pointed at the piece; an
// array of no bytes keeps its pointer (null stays null, and an absent array's alignment class does not matter)
static int stage_host_arrays(sdfr_renderer *r, Carving &st, const StagedArray *arrays, int n, hipStream_t stream)
{
	assert(n <= (int)SDFR_STAGE_MAX_PIECES);
	size_t bytes[SDFR_STAGE_MAX_PIECES];
	for (int k = 0; k < n; ++k) bytes[k] = arrays[k].bytes;
	st.cut(bytes, n);
	SDFR_HIP(st.reserve(r->query)); // (host calls are synchronous: none is using the old one)
	for (int k = 0; k < n; ++k)
	{
		const StagedArray &a = arrays[k];
		if (!a.bytes) continue;
		void *host, *piece = st.piece<void>(k);
		memcpy(&host, a.field, sizeof host);
		if (a.input) SDFR_HIP(hipMemcpyAsync(piece, host, a.bytes, hipMemcpyHostToDevice, stream));
		else st.answers[st.n_answers++] = {host, piece, a.bytes};
		memcpy(a.field, &piece, sizeof piece);
	}
	return SDFR_OK;
}
// ... for the pointer members of an arguments struct: piece k is the member at slots[k] with bytes[k] bytes, the first `inputs` are read
static int stage_host_members(sdfr_renderer *r, Carving &st, void *args, const size_t *slots, const size_t *bytes, int n, int inputs, hipStream_t stream)
{
	assert(n <= (int)SDFR_STAGE_MAX_PIECES);
	StagedArray arrays[SDFR_STAGE_MAX_PIECES];
	for (int k = 0; k < n; ++k) arrays[k] = {static_cast<char *>(args) + slots[k], bytes[k], k < inputs};
	return stage_host_arrays(r, st, arrays, n, stream);
}
// A buffer past what a handle keeps is given back once the work on `stream` that uses it is done: a large call does not hold its
// staging or workspace for the rest of the handle's life; small ones keep reusing theirs
static int release_large(sdfr_renderer *r, sdfr_device_buffer &b, hipStream_t stream)
{
	if (b.bytes <= k_query_stage_keep) return SDFR_OK;
	SDFR_HIP(hipStreamSynchronize(stream));
	b.release();
	return SDFR_OK;
}
// the end of a host call: the answers back to the caller in the order they were named, and `stream` synchronised (for a large call's
// release once more, drained as it is: what a host extraction has always done for its workspace)
static int copy_answers_back(sdfr_renderer *r, Carving &st, hipStream_t stream)
{
	for (int k = 0; k < st.n_answers; ++k) SDFR_HIP(hipMemcpyAsync(st.answers[k].host, st.answers[k].device, st.answers[k].bytes, hipMemcpyDeviceToHost, stream));
	SDFR_HIP(hipStreamSynchronize(stream));
	return release_large(r, *st.buffer, stream);
}
static_assert(QUERY_PLAN_OK == SDFR_OK && QUERY_PLAN_INVALID_ARGUMENT == SDFR_ERR_INVALID_ARGUMENT, "the plans speak in the library's statuses");
// One query: what the entry point asks for (QueryRequest), planned by sdfr_query_plan.h and carried out here.  In: kind's inputs (pos / dir /
// pixels); out: distance + normals, or hits and / or surfaces, or occlusion records, or lighting records with hits and light samples on request.
static int query_impl(sdfr_renderer *r, const QueryRequest &c)
{
	if (!r) return SDFR_ERR_INVALID_ARGUMENT;
	const QueryPlan p = plan_query(c, r->U.range);
	if (p.status != QUERY_PLAN_OK) return fail(r, p.status, p.error);
	if (p.nothing_to_do) return SDFR_OK;
	FrameU U;
	hipStream_t stream;
	int rc = begin_query(r, true, p.width, p.height, U, stream);
	if (rc != SDFR_OK) return rc;

	QueryArgs q = p.q;
	Carving st;
	if (c.on_host)
	{
		// the arrays of the kind in the order of p.bytes, each through its member of q
		const QueryKind &kind = k_query_kinds[q.kind];
		const size_t slots[6] = {kind.in[0].member, kind.in[1].member, kind.out[0].member, kind.out[1].member, k_query_lighting_slots[0].member, k_query_lighting_slots[1].member};
		rc = stage_host_members(r, st, &q, slots, p.bytes, 6, 2, stream);
		if (rc != SDFR_OK) return rc;
	}
	rc = run_query(r, U, q, stream);
	if (rc != SDFR_OK) return rc;
	return c.on_host ? copy_answers_back(r, st, stream) : SDFR_OK;
}
// a caller's records as the kernels' words
static uint32_t *words(void *records) { return static_cast<uint32_t *>(records); }
static const uint32_t *words(const void *records) { return static_cast<const uint32_t *>(records); }

int sdfr_query_distance(sdfr_renderer *r, int64_t n, const float *points, float *distance, float *normals, int on_host)
{
	return guarded(r, [&]() -> int {
		QueryRequest c = query_request(QUERY_POINTS, n, on_host);
		c.q.pos = points;
		c.q.distance = distance;
		c.q.normals = normals;
		return query_impl(r, c);
	});
}

// rays -> hits, or with want_surfaces surfaces and perhaps hits
static QueryRequest ray_request(int64_t n, const float *origins, const float *dirs, float max_distance, sdfr_hit *hits, sdfr_surface *surfaces, bool want_surfaces, int on_host)
{
	QueryRequest c = query_request(QUERY_RAYS, n, on_host);
	c.q.pos = origins;
	c.q.dir = dirs;
	c.q.reach = max_distance;
	c.q.hits = words(hits);
	c.q.surfaces = words(surfaces);
	c.want_surfaces = want_surfaces;
	return c;
}
// pixels of a width x height frame, or without a list every pixel of it, likewise
static QueryRequest pick_request(int width, int height, int64_t n, const int32_t *pixels_xy, sdfr_hit *hits, sdfr_surface *surfaces, bool want_surfaces, int on_host)
{
	QueryRequest c = query_request(pixels_xy || !want_surfaces ? QUERY_PICK : QUERY_FRAME, n, on_host);
	c.width = width;
	c.height = height;
	c.q.pixels = pixels_xy;
	c.q.hits = words(hits);
	c.q.surfaces = words(surfaces);
	c.want_surfaces = want_surfaces;
	return c;
}

int sdfr_query_rays(sdfr_renderer *r, int64_t n, const float *origins, const float *dirs, float max_distance, sdfr_hit *hits, int on_host)
{
	return guarded(r, [&]() -> int { return query_impl(r, ray_request(n, origins, dirs, max_distance, hits, nullptr, false, on_host)); });
}

int sdfr_pick(sdfr_renderer *r, int width, int height, int64_t n, const int32_t *pixels_xy, sdfr_hit *hits, int on_host)
{
	return guarded(r, [&]() -> int { return query_impl(r, pick_request(width, height, n, pixels_xy, hits, nullptr, false, on_host)); });
}

int sdfr_query_ray_surfaces(sdfr_renderer *r, int64_t n, const float *origins, const float *dirs, float max_distance, sdfr_hit *hits, sdfr_surface *surfaces,
	int on_host)
{
	return guarded(r, [&]() -> int { return query_impl(r, ray_request(n, origins, dirs, max_distance, hits, surfaces, true, on_host)); });
}

int sdfr_pick_surfaces(sdfr_renderer *r, int width, int height, int64_t n, const int32_t *pixels_xy, sdfr_hit *hits, sdfr_surface *surfaces, int on_host)
{
	return guarded(r, [&]() -> int { return query_impl(r, pick_request(width, height, n, pixels_xy, hits, surfaces, true, on_host)); });
}

int sdfr_mesh_surfaces(sdfr_renderer *r, int64_t n, const float *positions, const float *normals, float reach, sdfr_hit *hits, sdfr_surface *surfaces, int on_host)
{
	return guarded(r, [&]() -> int {
		QueryRequest c = ray_request(n, positions, normals, reach, hits, surfaces, true, on_host);
		c.q.kind = QUERY_MESH;
		return query_impl(r, c);
	});
}

// the lighting entries: the ray kinds' requests with `lighting` and perhaps `lights` instead of surfaces
static QueryRequest with_lighting(QueryRequest c, sdfr_lighting *lighting, sdfr_light_sample *lights)
{
	c.q.lighting = words(lighting);
	c.q.lights = words(lights);
	c.want_surfaces = false;
	c.want_lighting = true;
	return c;
}

int sdfr_query_ray_lighting(sdfr_renderer *r, int64_t n, const float *origins, const float *dirs, float max_distance, sdfr_hit *hits, sdfr_lighting *lighting,
	sdfr_light_sample *lights, int on_host)
{
	return guarded(r, [&]() -> int { return query_impl(r, with_lighting(ray_request(n, origins, dirs, max_distance, hits, nullptr, false, on_host), lighting, lights)); });
}

int sdfr_pick_lighting(sdfr_renderer *r, int width, int height, int64_t n, const int32_t *pixels_xy, sdfr_hit *hits, sdfr_lighting *lighting, sdfr_light_sample *lights,
	int on_host)
{
	// (pick_request: without a pixel list the whole frame, as the surface entry)
	return guarded(r, [&]() -> int { return query_impl(r, with_lighting(pick_request(width, height, n, pixels_xy, hits, nullptr, true, on_host), lighting, lights)); });
}

int sdfr_mesh_lighting(sdfr_renderer *r, int64_t n, const float *positions, const float *normals, float reach, sdfr_hit *hits, sdfr_lighting *lighting,
	sdfr_light_sample *lights, int on_host)
{
	return guarded(r, [&]() -> int {
		QueryRequest c = with_lighting(ray_request(n, positions, normals, reach, hits, nullptr, false, on_host), lighting, lights);
		c.q.kind = QUERY_MESH;
		return query_impl(r, c);
	});
}

// ---- the span queries (the definition: include/sdfr.h; the plan: sdfr_span_plan.h; the stage function: sdfr_span.h; the kernel:
// sdfr_query_kernel.h), calls of the queries' protocol with arguments of their own (SpanArgs)
static_assert(sizeof(sdfr_span_params) == sizeof(SpanParams) && offsetof(sdfr_span_params, min_step) == offsetof(SpanParams, min_step) &&
		offsetof(sdfr_span_params, iso) == offsetof(SpanParams, iso) && offsetof(sdfr_span_params, max_steps) == offsetof(SpanParams, max_steps) &&
		offsetof(sdfr_span_params, max_spans) == offsetof(SpanParams, max_spans),
	"sdfr_span_params is the plan's SpanParams");
static_assert(sizeof(sdfr_span_summary) == 4 * SPAN_SUMMARY_WORDS && offsetof(sdfr_span_summary, valid) == 12 && offsetof(sdfr_span_summary, inside_length) == 16 &&
		offsetof(sdfr_span_summary, flags) == 24 && sizeof(sdfr_span) == 8,
	"sdfr_span_summary is the span kernel's 8-word record, sdfr_span its two floats");
static_assert(SDFR_SPAN_STARTS_INSIDE == SPAN_STARTS_INSIDE && SDFR_SPAN_ENDS_INSIDE == SPAN_ENDS_INSIDE && SDFR_SPAN_OUT_OF_STEPS == SPAN_OUT_OF_STEPS, "the flag bits are the kernel's");
static int span_impl(sdfr_renderer *r, const SpanRequest &c)
{
	if (!r) return SDFR_ERR_INVALID_ARGUMENT;
	const SpanPlan p = plan_spans(c, r->U.range);
	if (p.status != QUERY_PLAN_OK) return fail(r, p.status, p.error);
	if (p.nothing_to_do) return SDFR_OK;
	FrameU U;
	hipStream_t stream;
	int rc = begin_query(r, true, p.width, p.height, U, stream);
	if (rc != SDFR_OK) return rc;

	SpanArgs s = p.a;
	Carving st;
	if (c.on_host)
	{
		rc = stage_host_members(r, st, &s, k_span_stage_slots[s.kind == QUERY_PICK ? 1 : 0], p.bytes, SPAN_STAGE_PIECES, SPAN_STAGE_INPUTS, stream);
		if (rc != SDFR_OK) return rc;
	}
	rc = launch_loaded(r, QUERY_KERNEL_SPANS, U, s, p.blocks, stream, "span launch");
	if (rc != SDFR_OK) return rc;
	return c.on_host ? copy_answers_back(r, st, stream) : SDFR_OK;
}
static SpanRequest span_request(int kind, int64_t n, const void *in0, const void *in1, const sdfr_span_params *params, sdfr_span_summary *summaries, sdfr_span *spans, int on_host)
{
	SpanRequest c = {};
	c.kind = kind;
	c.n = n;
	c.in0 = in0;
	c.in1 = in1;
	c.params = reinterpret_cast<const SpanParams *>(params);
	c.summaries = summaries;
	c.spans = spans;
	c.on_host = on_host;
	return c;
}

int sdfr_query_ray_spans(sdfr_renderer *r, int64_t n, const float *origins, const float *dirs, const sdfr_span_params *params, sdfr_span_summary *summaries,
	sdfr_span *spans, int on_host)
{
	return guarded(r, [&]() -> int { return span_impl(r, span_request(QUERY_RAYS, n, origins, dirs, params, summaries, spans, on_host)); });
}

int sdfr_pick_spans(sdfr_renderer *r, int width, int height, int64_t n, const int32_t *pixels_xy, const sdfr_span_params *params, sdfr_span_summary *summaries,
	sdfr_span *spans, int on_host)
{
	return guarded(r, [&]() -> int {
		SpanRequest c = span_request(QUERY_PICK, n, pixels_xy, nullptr, params, summaries, spans, on_host);
		c.width = width;
		c.height = height;
		return span_impl(r, c);
	});
}

int sdfr_mesh_spans(sdfr_renderer *r, int64_t n, const float *positions, const float *normals, float reach, const sdfr_span_params *params,
	sdfr_span_summary *summaries, sdfr_span *spans, int on_host)
{
	return guarded(r, [&]() -> int {
		SpanRequest c = span_request(QUERY_MESH, n, positions, normals, params, summaries, spans, on_host);
		c.reach = reach;
		return span_impl(r, c);
	});
}

int sdfr_occlusion_directions(float *out)
{
	if (!out) return SDFR_ERR_INVALID_ARGUMENT;
	memcpy(out, k_occlusion_dirs, sizeof k_occlusion_dirs);
	return SDFR_OK;
}

int sdfr_query_occlusion(sdfr_renderer *r, int64_t n, const float *points, const float *normals, float bias, float radius, sdfr_occlusion *out, int on_host)
{
	return guarded(r, [&]() -> int {
		QueryRequest c = query_request(QUERY_OCCLUSION, n, on_host);
		c.q.pos = points;
		c.q.dir = normals;
		c.q.reach = radius;
		c.q.bias = bias;
		c.q.occlusion = words(out);
		return query_impl(r, c);
	});
}

int sdfr_hit_occlusion(sdfr_renderer *r, int64_t n, const sdfr_hit *hits, float bias, float radius, sdfr_occlusion *out, int on_host)
{
	return guarded(r, [&]() -> int {
		QueryRequest c = query_request(QUERY_HIT_OCCLUSION, n, on_host);
		c.q.hit_items = words(hits);
		c.q.reach = radius;
		c.q.bias = bias;
		c.q.occlusion = words(out);
		return query_impl(r, c);
	});
}

// sdfr_mesh_extract (the definition: include/sdfr.h; the plan: sdfr_mesh_plan.h; stages: sdfr_mesh.h, sdfr_mesh.hip), a call of the queries'
// protocol.  Sample the lattice, classify and scan, read the two totals back; then, if the capacities allow, emit vertices and indices
// and ask the point query for the normals at the vertices.  sharp: sdfr_mesh_extract_sharp -- the emit stage leaves each vertex's cell
// index instead of the vertex, and the scene's sharp-vertex kernel (sdfr_mesh_sharp.h) makes the vertices from them; all else is the same.
static_assert(sizeof(sdfr_mesh_grid) == sizeof(MeshGrid) && offsetof(sdfr_mesh_grid, cell) == offsetof(MeshGrid, cell) && offsetof(sdfr_mesh_grid, nx) == offsetof(MeshGrid, n) &&
		offsetof(sdfr_mesh_grid, iso) == offsetof(MeshGrid, iso), "sdfr_mesh_grid is the plan's MeshGrid");
// `work` cut out of the handle's mesh workspace, for work on `stream`
static int reserve_mesh_workspace(sdfr_renderer *r, Carving &work, hipStream_t stream)
{
	for (hipEvent_t &e : r->ev_mesh)
		if (!e) SDFR_HIP(hipEventCreate(&e));
	// the last extraction's emit work (device arrays: enqueued, perhaps on the other lane's stream) still reads the workspace
	SDFR_HIP(hipStreamWaitEvent(stream, r->ev_mesh[6], 0));
	if (r->mesh.bytes < work.total) SDFR_HIP(hipEventSynchronize(r->ev_mesh[6]));
	SDFR_HIP(work.reserve(r->mesh));
	return SDFR_OK;
}
// the loaded scene's distances at the lattice points of `la`, into d_lattice
static int sample_lattice(sdfr_renderer *r, const FrameU &U, LatticeArgs la, float *d_lattice, hipStream_t stream)
{
	static const int rows = [] { const char *e = getenv("SDFR_MESH_LATTICE_ROWS"); return e && atoi(e) != 0 ? 1 : 0; }(); // developer knob: the A/B
	la.rows = rows;
	la.out = d_lattice;
	return launch_loaded(r, QUERY_KERNEL_LATTICE, U, la, query_lattice_blocks(la), stream, "lattice launch");
}
static int mesh_impl(sdfr_renderer *r, const MeshRequest &c, sdfr_mesh_counts *counts, bool sharp)
{
	if (!r) return SDFR_ERR_INVALID_ARGUMENT;
	const MeshPlan p = plan_mesh(c);
	if (p.status != QUERY_PLAN_OK) return fail(r, p.status, p.error);
	FrameU U;
	hipStream_t stream;
	int rc = begin_query(r, true, 1, 1, U, stream);
	if (rc != SDFR_OK) return rc;

	Carving work({p.work[0], p.work[1], p.work[2], p.work[3]});
	rc = reserve_mesh_workspace(r, work, stream);
	if (rc != SDFR_OK) return rc;
	hipEvent_t *ev = r->profiling ? r->ev_mesh : nullptr;
	r->mesh_timed = 0;
	float *d_lattice = work.piece<float>(0);
	uint32_t *d_cells = work.piece<uint32_t>(1), *d_points = work.piece<uint32_t>(2), *d_sums = work.piece<uint32_t>(3);

	if (ev) SDFR_HIP(hipEventRecord(ev[0], stream));
	rc = sample_lattice(r, U, p.lattice, d_lattice, stream);
	if (rc != SDFR_OK) return rc;
	if (ev) SDFR_HIP(hipEventRecord(ev[1], stream));
	SDFR_HIP(launch_mesh_count(p.g, d_lattice, d_cells, d_points, d_sums, stream));
	if (ev) SDFR_HIP(hipEventRecord(ev[2], stream));
	uint32_t n_vertices = 0, n_quads = 0;
	SDFR_HIP(hipMemcpyAsync(&n_vertices, d_cells + p.cells, 4, hipMemcpyDeviceToHost, stream));
	SDFR_HIP(hipMemcpyAsync(&n_quads, d_points + p.points, 4, hipMemcpyDeviceToHost, stream));
	SDFR_HIP(hipStreamSynchronize(stream));
	if (ev) r->mesh_timed = 1;
	const MeshFill f = plan_mesh_fill(c, n_vertices, n_quads);
	counts->vertices = f.vertices;
	counts->triangles = f.triangles;
	if (!f.fill) return release_large(r, r->mesh, stream);

	float *d_pos = c.positions, *d_nrm = c.normals;
	uint32_t *d_idx = f.bytes[2] ? c.indices : nullptr;
	Carving st;
	if (c.on_host)
	{
		const StagedArray arrays[3] = {{&d_pos, f.bytes[0], false}, {&d_nrm, f.bytes[1], false}, {&d_idx, f.bytes[2], false}};
		rc = stage_host_arrays(r, st, arrays, 3, stream); // (in `query`, never in `mesh`)
		if (rc != SDFR_OK) return rc;
	}
	if (ev) SDFR_HIP(hipEventRecord(ev[3], stream));
	SDFR_HIP(launch_mesh_emit(p.g, d_lattice, d_cells, d_points, d_pos, d_idx, sharp, stream));
	if (sharp)
	{
		const MeshSharpArgs m = {{p.g.origin[0], p.g.origin[1], p.g.origin[2]}, p.g.cell, {p.g.n[0], p.g.n[1], p.g.n[2]}, p.g.iso, d_lattice, d_pos, n_vertices};
		rc = launch_loaded(r, QUERY_KERNEL_MESH_SHARP, U, m, mesh_sharp_blocks(n_vertices), stream, "sharp vertex launch");
		if (rc != SDFR_OK) return rc;
	}
	if (ev) SDFR_HIP(hipEventRecord(ev[4], stream));
	if (d_nrm)
	{
		QueryArgs q = {};
		q.kind = QUERY_POINTS;
		q.n = (int)n_vertices; // <= 2^30
		q.pos = d_pos;
		q.distance = d_lattice; // the point query also writes its distances: into the lattice, which nothing reads any more
		q.normals = d_nrm;
		rc = run_query(r, U, q, stream);
		if (rc != SDFR_OK) return rc;
		if (ev) SDFR_HIP(hipEventRecord(ev[5], stream));
	}
	if (ev) r->mesh_timed = d_nrm ? 2 : 3;
	if (c.on_host) rc = copy_answers_back(r, st, stream);
	else SDFR_HIP(hipEventRecord(r->ev_mesh[6], stream)); // the end of the device work the next extraction waits for
	if (rc != SDFR_OK) return rc;
	return release_large(r, r->mesh, stream);
}

int sdfr_mesh_extract(sdfr_renderer *r, const sdfr_mesh_grid *grid, int64_t vertex_capacity, int64_t triangle_capacity, float *positions, float *normals,
	uint32_t *indices, sdfr_mesh_counts *counts, int on_host)
{
	return guarded(r, [&]() -> int {
		const MeshRequest c = {reinterpret_cast<const MeshGrid *>(grid), vertex_capacity, triangle_capacity, positions, normals, indices, counts, on_host};
		return mesh_impl(r, c, counts, false);
	});
}

int sdfr_mesh_extract_sharp(sdfr_renderer *r, const sdfr_mesh_grid *grid, int64_t vertex_capacity, int64_t triangle_capacity, float *positions, float *normals,
	uint32_t *indices, sdfr_mesh_counts *counts, int on_host)
{
	return guarded(r, [&]() -> int {
		const MeshRequest c = {reinterpret_cast<const MeshGrid *>(grid), vertex_capacity, triangle_capacity, positions, normals, indices, counts, on_host};
		return mesh_impl(r, c, counts, true);
	});
}

int sdfr_mesh_get_timings(sdfr_renderer *r, double ms[4])
{
	return guarded(r, [&]() -> int {
		if (!r || !ms) return SDFR_ERR_INVALID_ARGUMENT;
		if (!r->mesh_timed) return fail(r, SDFR_ERR_INVALID_ARGUMENT, "the last sdfr_mesh_extract was not timed (sdfr_set_profiling)");
		SDFR_HIP(hipSetDevice(r->device));
		const int pairs[4][2] = {{0, 1}, {1, 2}, {3, 4}, {4, 5}};
		const int have = r->mesh_timed == 1 ? 2 : r->mesh_timed == 2 ? 4 : 3;
		for (int k = 0; k < 4; ++k)
		{
			float t = 0.f;
			if (k < have)
			{
				SDFR_HIP(hipEventSynchronize(r->ev_mesh[pairs[k][1]]));
				SDFR_HIP(hipEventElapsedTime(&t, r->ev_mesh[pairs[k][0]], r->ev_mesh[pairs[k][1]]));
			}
			ms[k] = t;
		}
		return SDFR_OK;
	});
}

// ---- sdfr_slice_extract (the definition: include/sdfr.h; the plan: sdfr_slice_plan.h; stages: sdfr_slice.h, sdfr_slice.hip), a call of the
// queries' protocol and in every step sdfr_mesh_extract's sibling.  Sample the stack of lattices, classify and scan, gather the layers'
// offsets and read them back -- their last entries are the two totals --; then, if the capacities allow, emit vertices and segments.
// The workspace is the extraction's; no profiling event is recorded: sdfr_mesh_get_timings keeps the last mesh extraction's.
static_assert(sizeof(sdfr_slice_grid) == sizeof(SliceGrid) && offsetof(sdfr_slice_grid, du) == offsetof(SliceGrid, du) && offsetof(sdfr_slice_grid, dv) == offsetof(SliceGrid, dv) &&
		offsetof(sdfr_slice_grid, dw) == offsetof(SliceGrid, dw) && offsetof(sdfr_slice_grid, nu) == offsetof(SliceGrid, nu) &&
		offsetof(sdfr_slice_grid, layers) == offsetof(SliceGrid, layers) && offsetof(sdfr_slice_grid, iso) == offsetof(SliceGrid, iso),
	"sdfr_slice_grid is the plan's SliceGrid");
static int slice_impl(sdfr_renderer *r, const SliceRequest &c, int64_t *layer_vertices, int64_t *layer_segments, sdfr_slice_counts *counts)
{
	if (!r) return SDFR_ERR_INVALID_ARGUMENT;
	const SlicePlan p = plan_slice(c);
	if (p.status != QUERY_PLAN_OK) return fail(r, p.status, p.error);
	FrameU U;
	hipStream_t stream;
	int rc = begin_query(r, true, 1, 1, U, stream);
	if (rc != SDFR_OK) return rc;

	Carving work({p.work[0], p.work[1], p.work[2], p.work[3], p.work[4]});
	rc = reserve_mesh_workspace(r, work, stream);
	if (rc != SDFR_OK) return rc;
	float *d_lattice = work.piece<float>(0);
	uint32_t *d_vertices = work.piece<uint32_t>(1), *d_segments = work.piece<uint32_t>(2), *d_sums = work.piece<uint32_t>(3), *d_layers = work.piece<uint32_t>(4);

	static const int rows = [] { const char *e = getenv("SDFR_SLICE_ROWS"); return e && atoi(e) != 0 ? 1 : 0; }(); // developer knob: the A/B
	SliceArgs sample = p.sample;
	sample.rows = rows;
	sample.out = d_lattice;
	rc = launch_loaded(r, QUERY_KERNEL_SLICES, U, sample, slice_sample_blocks(sample), stream, "slice launch");
	if (rc != SDFR_OK) return rc;
	SDFR_HIP(launch_slice_count(p.g, d_lattice, d_vertices, d_segments, d_sums, d_layers, stream));
	const size_t per = (size_t)p.g.layers + 1;
	std::vector<uint32_t> offsets(2 * per);
	SDFR_HIP(hipMemcpyAsync(offsets.data(), d_layers, p.work[4], hipMemcpyDeviceToHost, stream));
	SDFR_HIP(hipStreamSynchronize(stream));
	const uint32_t n_vertices = offsets[per - 1], n_segments = offsets[2 * per - 1];
	const SliceFill f = plan_slice_fill(c, n_vertices, n_segments);
	counts->vertices = f.vertices;
	counts->segments = f.segments;
	for (size_t l = 0; l < per; ++l)
	{
		if (layer_vertices) layer_vertices[l] = (int64_t)offsets[l];
		if (layer_segments) layer_segments[l] = (int64_t)offsets[per + l];
	}
	if (!f.fill) return release_large(r, r->mesh, stream);

	float *d_pos = c.positions, *d_uv = c.coords;
	uint32_t *d_seg = f.bytes[2] ? c.segments : nullptr;
	Carving st;
	if (c.on_host)
	{
		const StagedArray arrays[3] = {{&d_pos, f.bytes[0], false}, {&d_uv, f.bytes[1], false}, {&d_seg, f.bytes[2], false}};
		rc = stage_host_arrays(r, st, arrays, 3, stream); // (in `query`, never in `mesh`)
		if (rc != SDFR_OK) return rc;
	}
	SDFR_HIP(launch_slice_emit(p.g, d_lattice, d_vertices, d_segments, d_pos, d_uv, d_seg, stream));
	if (c.on_host) rc = copy_answers_back(r, st, stream);
	else SDFR_HIP(hipEventRecord(r->ev_mesh[6], stream)); // the end of the device work the next extraction waits for
	if (rc != SDFR_OK) return rc;
	return release_large(r, r->mesh, stream);
}

int sdfr_slice_extract(sdfr_renderer *r, const sdfr_slice_grid *grid, int64_t vertex_capacity, int64_t segment_capacity, float *positions, float *coords,
	uint32_t *segments, int64_t *layer_vertices, int64_t *layer_segments, sdfr_slice_counts *counts, int on_host)
{
	return guarded(r, [&]() -> int {
		const SliceRequest c = {reinterpret_cast<const SliceGrid *>(grid), vertex_capacity, segment_capacity, positions, coords, segments, counts, on_host};
		return slice_impl(r, c, layer_vertices, layer_segments, counts);
	});
}

// ---- sdfr_mesh_survey and sdfr_mesh_fit (the definitions: include/sdfr.h; the plans: sdfr_mesh_plan.h; the predicates and the fit's loop:
// sdfr_mesh_survey.h; the kernel: sdfr_mesh.hip), calls of the queries' protocol and synchronous like the counting call.  The workspace is
// the extraction's, of which a survey takes the lattice and the result words; no profiling event is recorded: sdfr_mesh_get_timings keeps
// the last extraction's.
static_assert(sizeof(sdfr_mesh_survey_result) == sizeof(MeshSurvey) && offsetof(sdfr_mesh_survey_result, active_lo) == offsetof(MeshSurvey, active_lo) &&
		offsetof(sdfr_mesh_survey_result, near_hi) == offsetof(MeshSurvey, near_hi) && offsetof(sdfr_mesh_survey_result, face_active) == offsetof(MeshSurvey, face_active),
	"sdfr_mesh_survey_result is the kernel's MeshSurvey");
static_assert(sizeof(sdfr_mesh_fit_result) == sizeof(MeshFit) && offsetof(sdfr_mesh_fit_result, lo) == offsetof(MeshFit, lo) && offsetof(sdfr_mesh_fit_result, grid) == offsetof(MeshFit, grid) &&
		offsetof(sdfr_mesh_fit_result, last) == offsetof(MeshFit, last) && SDFR_FIT_EMPTY == MESH_FIT_EMPTY && SDFR_FIT_FOUND == MESH_FIT_FOUND && SDFR_FIT_TOO_LARGE == MESH_FIT_TOO_LARGE,
	"sdfr_mesh_fit_result is the loop's MeshFit");
// one planned survey with the frame U on `stream`, read back into `out`
static int survey_lattice(sdfr_renderer *r, const FrameU &U, const MeshSurveyPlan &p, float band, MeshSurvey &out, hipStream_t stream)
{
	Carving work({p.work[0], p.work[1]});
	int rc = reserve_mesh_workspace(r, work, stream);
	if (rc != SDFR_OK) return rc;
	float *d_lattice = work.piece<float>(0);
	MeshSurvey *d_survey = work.piece<MeshSurvey>(1);
	rc = sample_lattice(r, U, p.lattice, d_lattice, stream);
	if (rc != SDFR_OK) return rc;
	SDFR_HIP(launch_mesh_survey(p.g, d_lattice, band, d_survey, stream));
	SDFR_HIP(hipMemcpyAsync(&out, d_survey, sizeof out, hipMemcpyDeviceToHost, stream));
	SDFR_HIP(hipStreamSynchronize(stream));
	return release_large(r, r->mesh, stream);
}

int sdfr_mesh_survey(sdfr_renderer *r, const sdfr_mesh_grid *grid, float band, sdfr_mesh_survey_result *out)
{
	return guarded(r, [&]() -> int {
		if (!r) return SDFR_ERR_INVALID_ARGUMENT;
		const MeshSurveyPlan p = plan_mesh_survey(reinterpret_cast<const MeshGrid *>(grid), band, out);
		if (p.status != QUERY_PLAN_OK) return fail(r, p.status, p.error);
		FrameU U;
		hipStream_t stream;
		int rc = begin_query(r, true, 1, 1, U, stream);
		if (rc != SDFR_OK) return rc;
		MeshSurvey s;
		rc = survey_lattice(r, U, p, band, s, stream);
		if (rc != SDFR_OK) return rc;
		memcpy(out, &s, sizeof s);
		return SDFR_OK;
	});
}

int sdfr_mesh_fit(sdfr_renderer *r, const sdfr_mesh_grid *search, int levels, int margin, sdfr_mesh_fit_result *out)
{
	return guarded(r, [&]() -> int {
		if (!r) return SDFR_ERR_INVALID_ARGUMENT;
		const MeshGrid *g = reinterpret_cast<const MeshGrid *>(search);
		if (const char *error = plan_mesh_fit(g, levels, margin, out)) return fail(r, SDFR_ERR_INVALID_ARGUMENT, error);
		FrameU U;
		hipStream_t stream;
		int rc = begin_query(r, true, 1, 1, U, stream);
		if (rc != SDFR_OK) return rc;
		MeshFit f;
		rc = mesh_fit(*g, levels, margin, [&](const MeshGrid &level, float band, MeshSurvey &s) -> int {
			const MeshSurveyPlan p = plan_mesh_survey(&level, band, &s); // (stands: the loop surveys no grid mesh_grid_ok refuses)
			return p.status != QUERY_PLAN_OK ? fail(r, p.status, p.error) : survey_lattice(r, U, p, band, s, stream);
		}, f);
		if (rc != SDFR_OK) return rc;
		memcpy(out, &f, sizeof f);
		return SDFR_OK;
	});
}

// ---- sdfr_components_label and sdfr_components_label_lattice (the definition: include/sdfr.h; the plan: sdfr_components_plan.h; the rules:
// sdfr_components.h; the kernels: sdfr_components.hip), calls of the queries' protocol and synchronous like the counting call.  Sample the
// lattice (or take the caller's), unite and flatten, flag the roots and scan them, read the number of components back; cut the table behind
// the workspace's other pieces; then number, tally and pack, and read the 64 bytes of counts back.  The workspace is the extraction's under
// its keep rule; a host call's lattice and labels are staged in `query`, its records are copied from the table, which holds them in
// order.  No profiling event is recorded.
static_assert(sizeof(sdfr_component) == sizeof(Component) && offsetof(sdfr_component, flags) == offsetof(Component, flags) && offsetof(sdfr_component, points) == offsetof(Component, points) &&
		offsetof(sdfr_component, lo) == offsetof(Component, lo) && offsetof(sdfr_component, hi) == offsetof(Component, hi) && alignof(sdfr_component) == 8,
	"sdfr_component is the kernels' Component");
static_assert(sizeof(sdfr_component_counts) == sizeof(ComponentCounts) && offsetof(sdfr_component_counts, inside_points) == offsetof(ComponentCounts, inside_points) &&
		offsetof(sdfr_component_counts, largest_void_points) == offsetof(ComponentCounts, largest_void_points) && SDFR_COMPONENT_INSIDE == COMPONENT_INSIDE &&
		SDFR_COMPONENT_FACES == COMPONENT_FACES && (1u << SDFR_COMPONENT_FACE_SHIFT) == COMPONENT_FACE,
	"sdfr_component_counts is the kernels' ComponentCounts");
// `work`, cut anew with a last piece added, in the handle's mesh workspace with what the pieces before it hold (the stream is drained)
static int grow_mesh_workspace(sdfr_renderer *r, Carving &work, const size_t *bytes, int n, hipStream_t stream)
{
	work.cut(bytes, n);
	if (r->mesh.bytes >= work.total) return SDFR_OK;
	sdfr_device_buffer grown;
	SDFR_HIP(grown.reserve(work.total));
	const hipError_t e = hipMemcpyAsync(grown.ptr, r->mesh.ptr, work.offset[n - 1], hipMemcpyDeviceToDevice, stream);
	const hipError_t s = e == hipSuccess ? hipStreamSynchronize(stream) : e;
	if (s != hipSuccess)
	{
		grown.release();
		SDFR_HIP(s);
	}
	r->mesh.release();
	r->mesh = grown;
	return SDFR_OK;
}
static int components_impl(sdfr_renderer *r, const ComponentsRequest &c, sdfr_component_counts *counts)
{
	if (!r) return SDFR_ERR_INVALID_ARGUMENT;
	const ComponentsPlan p = plan_components(c);
	if (p.status != QUERY_PLAN_OK) return fail(r, p.status, p.error);
	FrameU U;
	hipStream_t stream;
	int rc = begin_query(r, !c.own_lattice, 1, 1, U, stream);
	if (rc != SDFR_OK) return rc;

	Carving work;
	work.cut(p.work, COMPONENTS_WORK_PIECES);
	rc = reserve_mesh_workspace(r, work, stream);
	if (rc != SDFR_OK) return rc;
	const float *d_lattice = c.own_lattice ? static_cast<const float *>(c.lattice) : work.piece<float>(COMPONENTS_WORK_LATTICE);
	uint32_t *d_labels = static_cast<uint32_t *>(const_cast<void *>(c.labels));
	Carving st;
	if (c.on_host)
	{
		const StagedArray arrays[2] = {{(void *)&d_lattice, p.lattice_bytes, true}, {&d_labels, p.label_bytes, false}};
		rc = stage_host_arrays(r, st, arrays, 2, stream); // (in `query`, never in `mesh`)
		if (rc != SDFR_OK) return rc;
	}
	if (!c.own_lattice)
	{
		rc = sample_lattice(r, U, p.lattice, work.piece<float>(COMPONENTS_WORK_LATTICE), stream);
		if (rc != SDFR_OK) return rc;
	}
	uint32_t *d_parent = work.piece<uint32_t>(COMPONENTS_WORK_PARENT), *d_scan = work.piece<uint32_t>(COMPONENTS_WORK_SCAN);
	SDFR_HIP(launch_components_union(p, d_lattice, d_parent, d_scan, work.piece<uint32_t>(COMPONENTS_WORK_SUMS), stream));
	uint32_t n_components = 0;
	SDFR_HIP(hipMemcpyAsync(&n_components, d_scan + p.points, 4, hipMemcpyDeviceToHost, stream));
	SDFR_HIP(hipStreamSynchronize(stream));

	const ComponentsFill f = plan_components_fill(c, p, n_components);
	size_t pieces[COMPONENTS_WORK_PIECES];
	for (int k = 0; k < COMPONENTS_WORK_PIECES; ++k) pieces[k] = p.work[k];
	pieces[COMPONENTS_WORK_TABLE] = f.table_bytes;
	rc = grow_mesh_workspace(r, work, pieces, COMPONENTS_WORK_PIECES, stream);
	if (rc != SDFR_OK) return rc;
	if (!c.own_lattice) d_lattice = work.piece<float>(COMPONENTS_WORK_LATTICE);
	d_parent = work.piece<uint32_t>(COMPONENTS_WORK_PARENT);
	d_scan = work.piece<uint32_t>(COMPONENTS_WORK_SCAN);
	Component *d_table = work.piece<Component>(COMPONENTS_WORK_TABLE);
	void *d_result = work.piece<void>(COMPONENTS_WORK_RESULT);
	Component *d_records = c.on_host ? nullptr : static_cast<Component *>(const_cast<void *>(c.records));
	SDFR_HIP(launch_components_tally(p, f, d_lattice, d_parent, d_scan, d_labels, d_table, d_records, d_result, stream));
	ComponentCounts n;
	SDFR_HIP(hipMemcpyAsync(&n, d_result, sizeof n, hipMemcpyDeviceToHost, stream));
	if (c.on_host)
	{
		if (f.fill) st.answers[st.n_answers++] = {const_cast<void *>(c.records), d_table, f.record_bytes};
		rc = copy_answers_back(r, st, stream);
		if (rc != SDFR_OK) return rc;
	}
	else SDFR_HIP(hipStreamSynchronize(stream));
	memcpy(counts, &n, sizeof n);
	return release_large(r, r->mesh, stream);
}

int sdfr_components_label(sdfr_renderer *r, const sdfr_mesh_grid *grid, int64_t capacity, sdfr_component *records, uint32_t *labels, sdfr_component_counts *counts,
	int on_host)
{
	return guarded(r, [&]() -> int {
		const ComponentsRequest c = {reinterpret_cast<const MeshGrid *>(grid), false, nullptr, capacity, records, labels, counts, on_host};
		return components_impl(r, c, counts);
	});
}

int sdfr_components_label_lattice(sdfr_renderer *r, const sdfr_mesh_grid *grid, const float *lattice, int64_t capacity, sdfr_component *records, uint32_t *labels,
	sdfr_component_counts *counts, int on_host)
{
	return guarded(r, [&]() -> int {
		const ComponentsRequest c = {reinterpret_cast<const MeshGrid *>(grid), true, lattice, capacity, records, labels, counts, on_host};
		return components_impl(r, c, counts);
	});
}

// ---- sdfr_measure (the definition: include/sdfr.h; the plan and the properties: sdfr_measure_plan.h; the column and the reductions:
// sdfr_measure.h; the kernels: sdfr_query_kernel.h and sdfr_mesh.hip), a call of the queries' protocol and synchronous like the counting
// call of the mesh.  The partials and the tally lie in the extraction's workspace under its keep rule; a host call's `columns` are staged
// in `query`; the result comes back as its 160 bytes.  No profiling event is recorded.
static_assert(sizeof(sdfr_measure_grid) == sizeof(MeasureGrid) && offsetof(sdfr_measure_grid, du) == offsetof(MeasureGrid, du) && offsetof(sdfr_measure_grid, dw) == offsetof(MeasureGrid, dw) &&
		offsetof(sdfr_measure_grid, nu) == offsetof(MeasureGrid, nu) && offsetof(sdfr_measure_grid, nv) == offsetof(MeasureGrid, nv),
	"sdfr_measure_grid is the plan's MeasureGrid");
static_assert(sizeof(sdfr_measure_result) == sizeof(MeasureResult) && offsetof(sdfr_measure_result, columns_hit) == offsetof(MeasureResult, columns_hit) &&
		offsetof(sdfr_measure_result, crossings) == offsetof(MeasureResult, crossings) && offsetof(sdfr_measure_result, hit_hi) == offsetof(MeasureResult, hit_hi) &&
		offsetof(sdfr_measure_result, t_hi) == offsetof(MeasureResult, t_hi),
	"sdfr_measure_result is the kernels' MeasureResult");
static_assert(sizeof(sdfr_measure_column) == 4 * MEASURE_COLUMN_WORDS && offsetof(sdfr_measure_column, spans) == 24 && offsetof(sdfr_measure_column, valid) == 36 &&
		sizeof(MeasureColumn) == sizeof(sdfr_measure_column), "sdfr_measure_column is the measure kernel's 10-word record");
static_assert(sizeof(sdfr_solid_properties) == sizeof(SolidProperties) && offsetof(sdfr_solid_properties, centroid) == offsetof(SolidProperties, centroid) &&
		offsetof(sdfr_solid_properties, inertia) == offsetof(SolidProperties, inertia), "sdfr_solid_properties is the plan's SolidProperties");
static int measure_impl(sdfr_renderer *r, const MeasureRequest &c, sdfr_measure_result *out)
{
	if (!r) return SDFR_ERR_INVALID_ARGUMENT;
	const MeasurePlan p = plan_measure(c, r->U.range);
	if (p.status != QUERY_PLAN_OK) return fail(r, p.status, p.error);
	FrameU U;
	hipStream_t stream;
	int rc = begin_query(r, true, 1, 1, U, stream);
	if (rc != SDFR_OK) return rc;

	Carving work({p.work[0], p.work[1], p.work[2]});
	rc = reserve_mesh_workspace(r, work, stream);
	if (rc != SDFR_OK) return rc;
	double *const partials[2] = {work.piece<double>(0), work.piece<double>(1)};
	MeasureArgs g = p.a;
	g.partials = partials[0];
	g.tally = work.piece<void>(2);
	Carving st;
	if (c.on_host && p.column_bytes)
	{
		const StagedArray arrays[1] = {{&g.columns, p.column_bytes, false}};
		rc = stage_host_arrays(r, st, arrays, 1, stream); // (in `query`, never in `mesh`)
		if (rc != SDFR_OK) return rc;
	}
	SDFR_HIP(launch_measure_init(g.tally, g.nu, g.nv, stream));
	rc = launch_loaded(r, QUERY_KERNEL_MEASURE, U, g, p.blocks, stream, "measure launch");
	if (rc != SDFR_OK) return rc;
	SDFR_HIP(launch_measure_reduce(partials, p.pass_records, p.passes, g.tally, stream));
	MeasureResult res;
	SDFR_HIP(hipMemcpyAsync(&res, g.tally, sizeof res, hipMemcpyDeviceToHost, stream));
	if (c.on_host && p.column_bytes) rc = copy_answers_back(r, st, stream);
	else SDFR_HIP(hipStreamSynchronize(stream));
	if (rc != SDFR_OK) return rc;
	memcpy(out, &res, sizeof res);
	return release_large(r, r->mesh, stream);
}

int sdfr_measure(sdfr_renderer *r, const sdfr_measure_grid *grid, const sdfr_span_params *params, sdfr_measure_result *out, sdfr_measure_column *columns, int on_host)
{
	return guarded(r, [&]() -> int {
		const MeasureRequest c = {reinterpret_cast<const MeasureGrid *>(grid), reinterpret_cast<const SpanParams *>(params), out, columns, on_host};
		return measure_impl(r, c, out);
	});
}

int sdfr_measure_properties(const sdfr_measure_grid *grid, const sdfr_measure_result *res, double density, sdfr_solid_properties *out)
{
	if (!grid || !res || !out || !std::isfinite(density)) return SDFR_ERR_INVALID_ARGUMENT;
	SolidProperties o;
	measure_properties(*reinterpret_cast<const MeasureGrid *>(grid), *reinterpret_cast<const MeasureResult *>(res), density, o);
	memcpy(out, &o, sizeof o);
	return SDFR_OK;
}

// ---- the texture atlas of a mesh (the definition: include/sdfr.h; the plan: sdfr_atlas_plan.h; the texel map and the bake: sdfr_atlas.h).
// sdfr_atlas_texels looks at the mesh alone and needs no scene, as a bake of no quads; any other sdfr_atlas_bake is a call of the queries'
// protocol.  A host call stages three inputs and up to four answers.
static_assert(sizeof(sdfr_atlas) == sizeof(AtlasLayout) && offsetof(sdfr_atlas, tile) == offsetof(AtlasLayout, tile) && offsetof(sdfr_atlas, rows) == offsetof(AtlasLayout, rows),
	"sdfr_atlas is the plan's AtlasLayout");
static_assert(SDFR_ATLAS_ALBEDO == ATLAS_ALBEDO && SDFR_ATLAS_NORMAL == ATLAS_NORMAL && SDFR_ATLAS_LIT == ATLAS_LIT, "the layer bits are the kernel's");
static const AtlasLayout *layout_of(const sdfr_atlas *a) { return reinterpret_cast<const AtlasLayout *>(a); }

int sdfr_atlas_layout(int64_t triangles, int tile, int width, sdfr_atlas *out)
{
	AtlasLayout l;
	if (!out || !atlas_layout(triangles, tile, width, l)) return SDFR_ERR_INVALID_ARGUMENT;
	memcpy(out, &l, sizeof l);
	return SDFR_OK;
}

int sdfr_atlas_uvs(const sdfr_atlas *atlas, float *uvs)
{
	if (!atlas || !atlas_layout_ok(*layout_of(atlas)) || (atlas->triangles > 0 && !uvs)) return SDFR_ERR_INVALID_ARGUMENT;
	atlas_uvs(*layout_of(atlas), uvs);
	return SDFR_OK;
}

static int atlas_impl(sdfr_renderer *r, const AtlasRequest &c)
{
	if (!r) return SDFR_ERR_INVALID_ARGUMENT;
	const AtlasPlan p = plan_atlas(c);
	if (p.status != QUERY_PLAN_OK) return fail(r, p.status, p.error);
	FrameU U;
	hipStream_t stream;
	int rc = begin_query(r, p.needs_scene, 1, 1, U, stream);
	if (rc != SDFR_OK) return rc;

	AtlasArgs g = p.a;
	Carving st;
	if (c.on_host)
	{
		rc = stage_host_members(r, st, &g, k_atlas_stage_slots[c.bake ? 1 : 0], p.bytes, ATLAS_STAGE_PIECES, ATLAS_STAGE_INPUTS, stream);
		if (rc != SDFR_OK) return rc;
	}
	if (p.needs_scene) rc = launch_loaded(r, QUERY_KERNEL_ATLAS, U, g, p.blocks, stream, "atlas launch");
	else SDFR_HIP(launch_atlas_texels(g, p.blocks, stream));
	if (rc != SDFR_OK) return rc;
	return c.on_host ? copy_answers_back(r, st, stream) : SDFR_OK;
}

// what both entries ask for: the atlas, the mesh, the validity map
static AtlasRequest atlas_request(const sdfr_atlas *atlas, int64_t vertex_count, const float *positions, const float *normals, const uint32_t *indices, int32_t *valid,
	bool bake, int on_host)
{
	AtlasRequest c = {};
	c.atlas = layout_of(atlas);
	c.vertex_count = vertex_count;
	c.a.positions = positions;
	c.a.normals = normals;
	c.a.indices = indices;
	c.a.valid = valid;
	c.bake = bake;
	c.on_host = on_host;
	return c;
}

int sdfr_atlas_texels(sdfr_renderer *r, const sdfr_atlas *atlas, int64_t vertex_count, const float *positions, const float *normals, const uint32_t *indices,
	float *texel_positions, float *texel_normals, int32_t *valid, int on_host)
{
	return guarded(r, [&]() -> int {
		AtlasRequest c = atlas_request(atlas, vertex_count, positions, normals, indices, valid, false, on_host);
		c.a.texel_positions = texel_positions;
		c.a.texel_normals = texel_normals;
		return atlas_impl(r, c);
	});
}

int sdfr_atlas_bake(sdfr_renderer *r, const sdfr_atlas *atlas, int64_t vertex_count, const float *positions, const float *normals, const uint32_t *indices,
	float reach, uint32_t layers, float *albedo, float *normal, float *lit, int32_t *valid, int on_host)
{
	return guarded(r, [&]() -> int {
		AtlasRequest c = atlas_request(atlas, vertex_count, positions, normals, indices, valid, true, on_host);
		c.a.reach = reach;
		c.a.layers = layers;
		c.a.albedo = albedo;
		c.a.normal = normal;
		c.a.lit = lit;
		return atlas_impl(r, c);
	});
}

} // extern "C"

// Where a render writes when the caller's image and pixel_stats (or null) are host memory: the handle's staging buffers ...
static int stage_frame(sdfr_renderer *r, int on_host, size_t out_bytes, size_t pixels, void *&d_out, uint32_t *&d_pstat)
{
	if (!on_host) return SDFR_OK;
	SDFR_HIP(r->stage.reserve(out_bytes));
	d_out = r->stage.ptr;
	if (!d_pstat) return SDFR_OK;
	SDFR_HIP(r->pstat.reserve(pixels * 12));
	d_pstat = static_cast<uint32_t *>(r->pstat.ptr);
	return SDFR_OK;
}
// ... and from there to the caller once `stream` has rendered them
static int unstage_frame(sdfr_renderer *r, void *out, const void *d_out, size_t out_bytes, uint32_t *pixel_stats, const uint32_t *d_pstat, size_t pixels, hipStream_t stream)
{
	SDFR_HIP(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, stream));
	if (pixel_stats) SDFR_HIP(hipMemcpyAsync(pixel_stats, d_pstat, pixels * 12, hipMemcpyDeviceToHost, stream));
	SDFR_HIP(hipStreamSynchronize(stream));
	return SDFR_OK;
}

int sdfr::render_impl(sdfr_renderer *r, int width, int height, int rank, int world, void *out, int format, int out_on_host, uint32_t *pixel_stats,
	RenderMode mode, RenderTotals *totals, bool caller_times)
{
	int rc = check_render(r, width, height, rank, world, out, format, mode);
	if (rc != SDFR_OK || (mode == RENDER_PRIVATE && r->priv_count == 0)) return rc; // (no private strips: nothing to render)
	if (!totals) totals = r->lane.d_totals;
	r->aa_timed_passes = 0; // (sdfr_render_aa sets it once its passes are through)
	SDFR_HIP(hipSetDevice(r->device));
	const auto t_setup = std::chrono::steady_clock::now();
	rc = latch_frame(r, width, height);
	if (rc != SDFR_OK) return rc;
	r->ms_setup = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_setup).count();

	const FrameRows rows = frame_rows(mode, width, height, rank, world, r->tile_w_log2 ? r->tile_w_log2 : scene_tile_w_log2(r->scene), r->priv_count, r->priv_period);
	const RowMap &rm = rows.rm;
	const size_t local_pixels = rows.local_pixels;
	const size_t out_bytes = image_bytes(local_pixels, format);

	void *d_out = out;
	uint32_t *d_pstat = pixel_stats;
	rc = stage_frame(r, out_on_host, out_bytes, local_pixels, d_out, d_pstat);
	if (rc != SDFR_OK) return rc;
	// rows of a strip buffer past the end of the frame are never written: define them (only the ranks whose last strip is
	// missing or cut short have any)
	if (mode == RENDER_STRIPS && strips_end_past_frame(rm, height) && out_bytes) SDFR_HIP(hipMemsetAsync(d_out, 0, out_bytes, r->lane.stream));

	const bool pixel_schedule = r->scene == SDFR_SCENE_COUNT || r->schedule == SDFR_SCHEDULE_PIXEL; // (scenes compiled at run time exist for the PIXEL schedule only)
	if (!pixel_schedule) SDFR_HIP(hipMemsetAsync(totals, 0, sizeof(RenderTotals), r->lane.stream)); // the wavefront kernels add to it
	hipError_t e;
	if (rm.local_rows == 0) return SDFR_OK; // e.g. every strip of a small frame is private
	{
		size_t need = (size_t)launch_capacity_items(width, rm);
		if (need < local_pixels) need = local_pixels; // private strips index the workspace by image position
		rc = ensure_workspace(r, r->lane, need, !pixel_schedule);
	}
	if (rc != SDFR_OK) return rc;
	if (!caller_times) SDFR_HIP(hipEventRecord(r->lane.ev_begin, r->lane.stream));
	if (pixel_schedule)
	{
		PixelKernel pk;
		r->last_wavefront = false;
		rc = loaded_pixel_kernel(r, pk);
		if (rc != SDFR_OK) return rc;
		e = launch_pixel(pk, r->U, rm, d_out, format, d_pstat, totals, r->lane.ws, r->lane.stream, r->launch_mode);
	}
	else
	{
		e = launch_wavefront_schedule(r->scene, r->U, rm, d_out, format, d_pstat, totals, r->lane.ws, r->lane.stream, r->profiling ? r->ev_march : nullptr,
			r->profiling ? r->ev_shade : nullptr, &r->last_rounds);
		r->last_wavefront = true;
		r->last_profiled = r->profiling;
	}
	if (e != hipSuccess) return hip_fail(r, e, "kernel launch");
	++r->launches;
	if (!caller_times)
	{
		SDFR_HIP(hipEventRecord(r->lane.ev_end, r->lane.stream));
		r->lane.totals_parts = 1;
	}
	r->lane.have_render = true;

	return out_on_host ? unstage_frame(r, out, d_out, out_bytes, pixel_stats, d_pstat, local_pixels, r->lane.stream) : SDFR_OK;
}

// sdfr_render_aa (the definition: include/sdfr.h; the plan: sdfr_aa_plan.h; the kernel: sdfr_resolve.hip).  The supersampled frame
// S is rendered pass by pass as strip launches into the handle's compact buffer, and every pass is resolved into its rows of the
// image before the next one reuses the buffer: one stream, no host synchronisation between passes.
static int render_aa_impl(sdfr_renderer *r, int width, int height, int factor, void *out, int format, int out_on_host, uint32_t *pixel_stats)
{
	if (!r || !out) return SDFR_ERR_INVALID_ARGUMENT;
	if (format != SDFR_RGBA32F && format != SDFR_RGBA16F) return fail(r, SDFR_ERR_INVALID_ARGUMENT, "bad format");
	if (aa_factor_log2(factor) < 0) return fail(r, SDFR_ERR_INVALID_ARGUMENT, "factor must be 1, 2, 4 or 8");
	if (!is_flag(out_on_host)) return fail(r, SDFR_ERR_INVALID_ARGUMENT, "out_on_host must be 0 or 1");
	if (width < 1 || height < 1 || (int64_t)width * factor * factor > ((int64_t)1 << 30) / height) return fail(r, SDFR_ERR_INVALID_ARGUMENT, "bad frame size");
	if (r->scene < 0) return fail(r, SDFR_ERR_NO_SCENE, "no scene loaded");
	SDFR_HIP(hipSetDevice(r->device));

	unsigned long long budget = SDFR_AA_DEFAULT_BUDGET;
	if (const char *e = getenv("SDFR_AA_BUDGET_BYTES")) // developer knob, read on every call: bytes of one pass's compact colour buffer
	{
		const unsigned long long v = strtoull(e, nullptr, 10);
		if (v > 0) budget = v;
	}
	const AaPlan plan = plan_aa(width, height, factor, budget);
	const size_t pixels = (size_t)width * height;
	hipStream_t stream = r->lane.stream; // the handle's stream, or the lane of the frame submitted last

	if (!r->ev_aa_done) SDFR_HIP(hipEventCreate(&r->ev_aa_done));
	// the last call's passes (device destination: enqueued, perhaps on the other lane's stream) still use the buffers
	SDFR_HIP(hipStreamWaitEvent(stream, r->ev_aa_done, 0));
	const size_t color_bytes = plan.pass_pixels * 16, stats_bytes = pixel_stats ? plan.pass_pixels * 12 : 0;
	if (r->aa_color.bytes < color_bytes || r->aa_stats.bytes < stats_bytes || !r->aa_totals.ptr)
	{
		const int synced = sync_lanes(r); // before a buffer in use is replaced
		if (synced != SDFR_OK) return synced;
		SDFR_HIP(r->aa_color.reserve(color_bytes));
		SDFR_HIP(r->aa_stats.reserve(stats_bytes));
		SDFR_HIP(r->aa_totals.reserve(sizeof(RenderTotals)));
	}
	void *d_out = out;
	uint32_t *d_pstat = pixel_stats;
	int rc = stage_frame(r, out_on_host, image_bytes(pixels, format), pixels, d_out, d_pstat);
	if (rc != SDFR_OK) return rc;
	const bool timed = r->profiling;
	while (timed && r->ev_aa.size() < 2 * (size_t)plan.passes)
	{
		hipEvent_t e = nullptr;
		SDFR_HIP(hipEventCreate(&e));
		r->ev_aa.push_back(e);
	}

	const int tile_w_log2 = r->tile_w_log2 ? r->tile_w_log2 : scene_tile_w_log2(r->scene);
	const int split_count = r->priv_count, split_period = r->priv_period; // ignored, as a full frame ignores it
	r->priv_count = 0;
	r->priv_period = 1;
	SDFR_HIP(hipEventRecord(r->lane.ev_begin, stream));
	for (uint32_t p = 0; p < plan.passes && rc == SDFR_OK; ++p)
	{
		rc = render_impl(r, plan.s_width, plan.s_height, (int)p, (int)plan.passes, r->aa_color.ptr, SDFR_RGBA32F, 0,
			pixel_stats ? static_cast<uint32_t *>(r->aa_stats.ptr) : nullptr, RENDER_STRIPS, static_cast<RenderTotals *>(r->aa_totals.ptr), true);
		if (rc != SDFR_OK) break;
		ResolveArgs a = {};
		a.color = static_cast<const float *>(r->aa_color.ptr);
		a.stats = pixel_stats ? static_cast<const uint32_t *>(r->aa_stats.ptr) : nullptr;
		a.out = d_out;
		a.out_stats = d_pstat;
		a.rm = aa_pass_row_map(plan, p, tile_w_log2);
		a.s_width = plan.s_width;
		a.width = width;
		a.height = height;
		a.factor_log2 = plan.factor_log2;
		a.format = format;
		a.local_strips = aa_pass_strips(plan, p);
		a.pass_totals = static_cast<const RenderTotals *>(r->aa_totals.ptr);
		a.frame_totals = r->lane.d_totals;
		a.first_pass = p == 0;
		hipError_t e = timed ? hipEventRecord(r->ev_aa[2 * p], stream) : hipSuccess;
		if (e == hipSuccess) e = launch_resolve(a, stream);
		if (e == hipSuccess && timed) e = hipEventRecord(r->ev_aa[2 * p + 1], stream);
		if (e != hipSuccess) rc = hip_fail(r, e, "resolve launch");
	}
	r->priv_count = split_count;
	r->priv_period = split_period;
	// (also after a pass that failed: what was enqueued is ordered before the next call's use of the buffers)
	(void)hipEventRecord(r->lane.ev_end, stream);
	(void)hipEventRecord(r->ev_aa_done, stream);
	r->lane.totals_parts = 1;
	if (rc != SDFR_OK) return rc;
	r->aa_timed_passes = timed ? (int)plan.passes : 0;
	if (out_on_host) return unstage_frame(r, out, d_out, image_bytes(pixels, format), pixel_stats, d_pstat, pixels, stream);
	if (r->frames_in_flight == 2)
	{
		// the lane now also writes this image: the next frame, on the other lane, must see it in the range it checks for overlap
		auto widen = [](const char *&lo, const char *&hi, const char *a, const char *b) {
			if (!a) return;
			lo = lo && lo < a ? lo : a;
			hi = hi && hi > b ? hi : b;
		};
		const char *o = static_cast<const char *>(out), *s = reinterpret_cast<const char *>(pixel_stats);
		widen(r->lane.out_lo, r->lane.out_hi, o, o + image_bytes(pixels, format));
		widen(r->lane.pst_lo, r->lane.pst_hi, s, s ? s + pixels * 12 : nullptr);
	}
	return SDFR_OK;
}

extern "C" {

int sdfr_render_aa(sdfr_renderer *r, int width, int height, int factor, void *out, int format, int out_on_host, uint32_t *pixel_stats)
{
	return guarded(r, [&]() -> int { return render_aa_impl(r, width, height, factor, out, format, out_on_host, pixel_stats); });
}

int sdfr_render(sdfr_renderer *r, int width, int height, void *out, int format, int out_on_host, uint32_t *pixel_stats)
{
	return guarded(r, [&]() -> int {
		if (r && r->frames_in_flight == 2)
		{
			// checked before the lanes change: a call that fails leaves "the frame submitted last" (sdfr_get_stats,
			// sdfr_wait_frame) and the ranges the two lanes write as they were
			int rc = check_render(r, width, height, 0, 1, out, format, RENDER_FULL);
			if (rc != SDFR_OK) return rc;
			SDFR_HIP(hipSetDevice(r->device));
			const size_t pixels = (size_t)width * height;
			const char *lo = out_on_host ? nullptr : (const char *)out;
			const char *hi = lo ? lo + image_bytes(pixels, format) : nullptr;
			const char *plo = out_on_host ? nullptr : (const char *)pixel_stats;
			const char *phi = plo ? plo + pixels * 12 : nullptr;
			// the lane of the frame before last takes this one; its stream orders it behind that frame (same workspace).  The
			// frame still in flight writes [out_lo, out_hi) and [pst_lo, pst_hi): the same memory twice in a row is a hazard
			// between the two streams
			auto overlaps = [](const char *a, const char *b, const char *c, const char *d) { return a && c && a < d && c < b; };
			const sdfr_renderer::Lane &o = r->lane;
			if (o.have_render && (overlaps(lo, hi, o.out_lo, o.out_hi) || overlaps(lo, hi, o.pst_lo, o.pst_hi) || overlaps(plo, phi, o.out_lo, o.out_hi) ||
					overlaps(plo, phi, o.pst_lo, o.pst_hi)))
				SDFR_HIP(hipStreamWaitEvent(r->other.stream, o.ev_end, 0));
			std::swap(r->lane, r->other);
			const unsigned launches = r->launches;
			rc = render_impl(r, width, height, 0, 1, out, format, out_on_host, pixel_stats, RENDER_FULL);
			if (r->launches == launches) // nothing launched: the lanes go back to where they were
				std::swap(r->lane, r->other);
			else
			{
				r->lane.out_lo = lo;
				r->lane.out_hi = hi;
				r->lane.pst_lo = plo;
				r->lane.pst_hi = phi;
			}
			return rc;
		}
		return render_impl(r, width, height, 0, 1, out, format, out_on_host, pixel_stats, RENDER_FULL);
	});
}

int sdfr_render_strips(sdfr_renderer *r, int width, int height, int rank, int world, void *out_compact, int format)
{
	return guarded(r, [&]() -> int {
		return render_impl(r, width, height, rank, world, out_compact, format, 0, nullptr, RENDER_STRIPS);
	});
}

int sdfr_render_private_strips(sdfr_renderer *r, int width, int height, void *out_image, int format)
{
	return guarded(r, [&]() -> int {
		return render_impl(r, width, height, 0, 1, out_image, format, 0, nullptr, RENDER_PRIVATE);
	});
}

int sdfr_assemble_strips(sdfr_renderer *r, int width, int height, int world, const void *gathered, void *out_image, int format)
{
	return guarded(r, [&]() -> int {
		if (!r || !gathered || !out_image || width < 1 || height < 1 || world < 1) return SDFR_ERR_INVALID_ARGUMENT;
		if (!is_wire_format(format)) return fail(r, SDFR_ERR_INVALID_ARGUMENT, "bad format");
		SDFR_HIP(hipSetDevice(r->device));
		hipError_t e = launch_assemble_strips(width, height, world, gathered, out_image, format, r->priv_count, r->priv_period, r->lane.stream);
		if (e != hipSuccess) return hip_fail(r, e, "assemble launch");
		return SDFR_OK;
	});
}

int sdfr_postprocess(sdfr_renderer *r, int width, int height, const void *scene_rgba16f, void *bloom_scratch_rgba16f, void *out_rgba8)
{
	return guarded(r, [&]() -> int {
		if (!r || !scene_rgba16f || !bloom_scratch_rgba16f || !out_rgba8) return SDFR_ERR_INVALID_ARGUMENT;
		if (!frame_size_ok(width, height)) return fail(r, SDFR_ERR_INVALID_ARGUMENT, "bad frame size");
		SDFR_HIP(hipSetDevice(r->device));
		const size_t flag_bytes = postprocess_flag_bytes(width, height);
		if (r->post_flags.bytes < flag_bytes) SDFR_HIP(hipStreamSynchronize(r->lane.stream)); // a postprocess still in flight reads the old one
		SDFR_HIP(r->post_flags.reserve(flag_bytes));
		SDFR_HIP(hipEventRecord(r->ev_post[0], r->lane.stream));
		hipError_t e = launch_postprocess(width, height, scene_rgba16f, bloom_scratch_rgba16f, out_rgba8, static_cast<unsigned char *>(r->post_flags.ptr), r->lane.stream, r->ev_post[1]);
		if (e != hipSuccess) return hip_fail(r, e, "postprocess launch");
		SDFR_HIP(hipEventRecord(r->ev_post[2], r->lane.stream));
		r->have_post = true;
		return SDFR_OK;
	});
}

int sdfr_selftest_exception(sdfr_renderer *r, int what)
{
	return guarded(r, [&]() -> int {
		if (what == 0) throw std::runtime_error("sdfr_selftest_exception: thrown on purpose");
		if (what == 1) throw std::bad_alloc();
		if (what == 2) throw 42;
		return SDFR_OK;
	});
}

int sdfr_selftest_math(sdfr_renderer *r, int what, float constant, uint64_t *mismatches)
{
	return guarded(r, [&]() -> int {
		if (!r || !mismatches || what < 0 || what > 5) return SDFR_ERR_INVALID_ARGUMENT;
		if (what >= 1 && !(constant != 0.f && constant == constant)) return fail(r, SDFR_ERR_INVALID_ARGUMENT, "bad divisor");
		SDFR_HIP(hipSetDevice(r->device));
		unsigned long long *d = nullptr;
		SDFR_HIP(hipMalloc((void **)&d, sizeof(unsigned long long)));
		hipError_t e = hipMemsetAsync(d, 0, sizeof(unsigned long long), r->lane.stream);
		if (e == hipSuccess) e = launch_selftest_math(what, constant, d, r->lane.stream);
		unsigned long long h = 0;
		if (e == hipSuccess) e = hipMemcpyAsync(&h, d, sizeof h, hipMemcpyDeviceToHost, r->lane.stream);
		if (e == hipSuccess) e = hipStreamSynchronize(r->lane.stream);
		(void)hipFree(d);
		if (e != hipSuccess) return hip_fail(r, e, "selftest");
		*mismatches = h;
		return SDFR_OK;
	});
}

#ifdef SDFR_WAVE_TRACE
// developer build only (tools/wave_trace.py): the per-block records of the last pixel-schedule launch
int sdfr_debug_read_partials(sdfr_renderer *r, void *host, size_t records)
{
	return guarded(r, [&]() -> int {
		if (!r || !host) return SDFR_ERR_INVALID_ARGUMENT;
		SDFR_HIP(hipStreamSynchronize(r->lane.stream));
		if (records > r->lane.ws.capacity / 64 + 1) records = r->lane.ws.capacity / 64 + 1;
		SDFR_HIP(hipMemcpy(host, r->lane.ws.partials, records * sizeof(RenderTotals), hipMemcpyDeviceToHost));
		SDFR_HIP(hipMemset(r->lane.ws.partials, 0, records * sizeof(RenderTotals))); // records the next launch does not write read as empty
		return SDFR_OK;
	});
}
#endif

int sdfr_register_host_target(sdfr_renderer *r, void *host_image, size_t bytes)
{
	return guarded(r, [&]() -> int {
		if (!r || (host_image && bytes == 0)) return SDFR_ERR_INVALID_ARGUMENT;
		SDFR_HIP(hipSetDevice(r->device));
		SDFR_HIP(hipStreamSynchronize(r->lane.stream));
		if (r->pinned_host) (void)hipHostUnregister(r->pinned_host);
		r->pinned_host = nullptr;
		r->pinned_bytes = 0;
		if (!host_image) return SDFR_OK;
		SDFR_HIP(hipHostRegister(host_image, bytes, hipHostRegisterDefault));
		r->pinned_host = host_image;
		r->pinned_bytes = bytes;
		return SDFR_OK;
	});
}

int sdfr_sync(sdfr_renderer *r)
{
	return guarded(r, [&]() -> int {
		return r ? sync_lanes(r) : SDFR_ERR_INVALID_ARGUMENT;
	});
}

// the profiled rounds of the last frame, if the wavefront schedule rendered it: their number, and the milliseconds of each
// round's march and shade launches (-1: that time cannot be read)
struct RoundTime { float march, shade; };
static int round_times(const sdfr_renderer *r, RoundTime t[16])
{
	int n = 0;
	for (; r->last_wavefront && r->last_profiled && n < r->last_rounds && n < 16; ++n)
	{
		if (hipEventElapsedTime(&t[n].march, r->ev_march[2 * n], r->ev_march[2 * n + 1]) != hipSuccess) t[n].march = -1.f;
		if (hipEventElapsedTime(&t[n].shade, r->ev_shade[2 * n], r->ev_shade[2 * n + 1]) != hipSuccess) t[n].shade = -1.f;
	}
	return n;
}

int sdfr_get_stats(sdfr_renderer *r, sdfr_stats *out)
{
	return guarded(r, [&]() -> int {
		if (!r || !out) return SDFR_ERR_INVALID_ARGUMENT;
		memset(out, 0, sizeof *out);
		if (!r->lane.have_render) return fail(r, SDFR_ERR_INVALID_ARGUMENT, "nothing rendered yet");
		SDFR_HIP(hipEventSynchronize(r->lane.ev_end));
		float ms = 0.f;
		SDFR_HIP(hipEventElapsedTime(&ms, r->lane.ev_begin, r->lane.ev_end));
		out->ms_gpu = ms;
		RenderTotals t[2];
		SDFR_HIP(hipMemcpy(t, r->lane.d_totals, sizeof t, hipMemcpyDeviceToHost));
		for (int k = 0; k < r->lane.totals_parts; ++k)
		{
			out->pixels += t[k].pixels;
			out->rays += t[k].rays;
			out->march_evals += t[k].march_evals;
			out->hits += t[k].hits;
		}
		if (r->last_wavefront)
		{
			RoundTime t[16];
			for (int i = 0, n = round_times(r, t); i < n; ++i) // whichever of the two times can be read
			{
				if (t[i].march >= 0.f) out->ms_march += t[i].march;
				if (t[i].shade >= 0.f) out->ms_shade += t[i].shade;
			}
			out->march_launches = (uint32_t)r->last_rounds;
			out->shade_launches = (uint32_t)r->last_rounds;
		}
		else
		{
			out->march_launches = 1;
		}
		return SDFR_OK;
	});
}

int sdfr_get_timings(sdfr_renderer *r, sdfr_timing *out, int capacity)
{
	return guarded(r, [&]() -> int {
		if (!r || (!out && capacity > 0) || capacity < 0) return SDFR_ERR_INVALID_ARGUMENT;
		int n = 0;
		auto put = [&](const char *name, double ms) {
			if (n < capacity)
			{
				memset(&out[n], 0, sizeof out[n]);
				snprintf(out[n].name, sizeof out[n].name, "%s", name);
				out[n].ms = ms;
			}
			++n;
		};
		if (r->lane.have_render)
		{
			SDFR_HIP(hipEventSynchronize(r->lane.ev_end));
			float ms = 0.f;
			SDFR_HIP(hipEventElapsedTime(&ms, r->lane.ev_begin, r->lane.ev_end));
			put("setup", r->ms_setup);
			put("draw", ms);
			RoundTime t[16];
			for (int i = 0, rounds = round_times(r, t); i < rounds; ++i)
			{
				if (t[i].march < 0.f || t[i].shade < 0.f) continue; // a round is listed with both of its times or not at all
				char nm[32];
				snprintf(nm, sizeof nm, "draw: march %d", i);
				put(nm, t[i].march);
				snprintf(nm, sizeof nm, "draw: shade %d", i);
				put(nm, t[i].shade);
			}
			if (r->aa_timed_passes > 0) // a profiled sdfr_render_aa: the time inside its resolve launches, summed over the passes
			{
				double sum = 0.0;
				for (int p = 0; p < r->aa_timed_passes; ++p)
				{
					float t = 0.f;
					SDFR_HIP(hipEventElapsedTime(&t, r->ev_aa[2 * p], r->ev_aa[2 * p + 1]));
					sum += t;
				}
				put("draw: resolve", sum);
			}
		}
		if (r->lane.have_render && r->have_xfer)
		{
			// the last sdfr_render_gather's transfer on the comm stream: rank 0 receives world - 1 messages at once (one per link),
			// a peer sends one; the bytes ride in the name so that a caller can turn the time into a rate
			SDFR_HIP(hipEventSynchronize(r->ev_xfer[1]));
			float t = 0.f;
			SDFR_HIP(hipEventElapsedTime(&t, r->ev_xfer[0], r->ev_xfer[1]));
			char nm[32];
			snprintf(nm, sizeof nm, "gather transfer %zu B", r->xfer_bytes);
			put(nm, t);
		}
		if (r->have_post)
		{
			SDFR_HIP(hipEventSynchronize(r->ev_post[2]));
			float a = 0.f, b = 0.f;
			SDFR_HIP(hipEventElapsedTime(&a, r->ev_post[0], r->ev_post[1]));
			SDFR_HIP(hipEventElapsedTime(&b, r->ev_post[1], r->ev_post[2]));
			put("Bloom 1", a);
			put("Bloom 2 + HDR", b); // the vertical blur and the tone map are one kernel here
		}
		return n;
	});
}

} // extern "C"

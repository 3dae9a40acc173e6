// sdfr_jit.h -- scenes compiled at run time with hiprtc (sdfr_jit.cpp).
#pragma once
#include "sdfr_kernels.h"

#include <string>
#include <vector>

namespace sdfr {

struct JitScene
{
	std::string name;
	hipModule_t module = nullptr;
	hipFunction_t prepare = nullptr, pixel = nullptr, pixel_debug = nullptr;
	FrameU *d_frame = nullptr; // device copy of the frame uniforms for Scene::prepare
	// the query kernels (sdfr_query_kernel.h) in a module of their own, compiled on the scene's first query (jit_launch_query)
	std::string source;
	std::vector<std::string> var_slots;
	hipModule_t query_module = nullptr;
	hipFunction_t query_points = nullptr, query_points_debug = nullptr, query_rays = nullptr, query_rays_debug = nullptr;
	hipFunction_t query_lattice = nullptr, query_lattice_debug = nullptr;
};

// the translation unit compiled for a scene: variable macros, the scene text, the kernels (the pixel kernels, or with
// `query` the query kernels)
std::string jit_translation_unit(const std::string &scene_source, const std::vector<std::string> &var_slots, bool query = false);

// compile only (no device needed): code object for `arch_name` ("gfx950")
bool jit_compile_code(const std::string &arch_name, const std::string &name, const std::string &scene_source, const std::vector<std::string> &var_slots,
	std::vector<char> &code, std::string &error, bool query = false);
// compile + load; on failure `error` carries the compiler log
bool jit_compile(int device, const std::string &name, const std::string &scene_source, const std::vector<std::string> &var_slots, JitScene &out,
	std::string &error);
void jit_unload(JitScene &js);

// runs Scene::prepare(U) on the device and brings the frame uniforms back (synchronises `stream`)
hipError_t jit_prepare(const JitScene &js, FrameU &U, hipStream_t stream);

// one query (sdfr_query.h) of the run-time scene, every pointer of `q` device memory; compiles and loads the scene's query
// module first if this is its first query
// JIT_QUERY_COMPILE: the query module did not compile (the compiler's log in `error`); JIT_QUERY_HIP: it did not load or launch
enum JitQueryStatus { JIT_QUERY_OK = 0, JIT_QUERY_COMPILE = 1, JIT_QUERY_HIP = 2 };
JitQueryStatus jit_launch_query(JitScene &js, int device, const FrameU &U, const QueryArgs &q, hipStream_t stream, std::string &error);
// the same for the distance query over a lattice (sdfr_query.h: LatticeArgs; sdfr_mesh_extract)
JitQueryStatus jit_launch_query_lattice(JitScene &js, int device, const FrameU &U, const LatticeArgs &g, hipStream_t stream, std::string &error);

hipError_t jit_launch_pixel(const JitScene &js, const FrameU &U, const RowMap &rm, void *out, int format, uint32_t *pixel_stats,
	RenderTotals *totals, const WavefrontWorkspace &ws, hipStream_t stream, int launch_mode = 0);

} // namespace sdfr

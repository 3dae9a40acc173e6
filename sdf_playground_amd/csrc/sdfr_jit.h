// sdfr_jit.h -- scenes compiled at run time with hiprtc (sdfr_jit.cpp).
#pragma once
#include "sdfr_jit_unit.h"
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
	// the query kernels (sdfr_query_kernel.h) in a module of their own, compiled on the scene's first query (jit_query_kernels)
	std::string source;
	std::vector<std::string> var_slots;
	hipModule_t query_module = nullptr;
	QueryKernels query = {};
};

// compile only (no device needed): code object for `arch_name` ("gfx950")
bool jit_compile_code(const std::string &arch_name, const std::string &name, const std::string &scene_source, const std::vector<std::string> &var_slots,
	std::vector<char> &code, std::string &error, bool query = false);
// compile + load; on failure `error` carries the compiler log
bool jit_compile(int device, const std::string &name, const std::string &scene_source, const std::vector<std::string> &var_slots, JitScene &out,
	std::string &error);
void jit_unload(JitScene &js);

// runs Scene::prepare(U) on the device and brings the frame uniforms back (synchronises `stream`)
hipError_t jit_prepare(const JitScene &js, FrameU &U, hipStream_t stream);

// the scene's query kernels, as a built-in scene's unit exports them (scene_query_kernels); compiles and loads the scene's query
// module first if this is its first query
// JIT_QUERY_COMPILE: the query module did not compile (the compiler's log in `error`); JIT_QUERY_HIP: it did not load
enum JitQueryStatus { JIT_QUERY_OK = 0, JIT_QUERY_COMPILE = 1, JIT_QUERY_HIP = 2 };
JitQueryStatus jit_query_kernels(JitScene &js, int device, const QueryKernels *&out, std::string &error);

// the scene's pixel kernel with the traits of a run-time scene, as scene_pixel_kernel gives a built-in scene's
PixelKernel jit_pixel_kernel(const JitScene &js, bool dbg);

} // namespace sdfr

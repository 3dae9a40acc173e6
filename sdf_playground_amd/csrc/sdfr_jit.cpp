// sdfr_jit.cpp -- scenes compiled at run time.
//
// The reference builds a scene INTO its pixel shader when the scene is selected and again
// whenever its file changes (SceneManager.cpp:102-133, SDFRenderer::initShader
// SDFRenderer.cpp:27-53 with D3DCompile).  The equivalent here: the text of a scene functor
// (the same shape as the ahead-of-time scenes of sdfr_scenes*.h, named `Scene`) is wrapped
// into a translation unit around sdfr_pixel_kernel.h (sdfr_jit_unit.h writes its text, and that
// of the query kernels' unit), compiled for the device's architecture with hiprtc and loaded as
// a module: this file.  The pixel kernel body is the one the ahead-of-time scenes use, so a
// scene renders the same bits either way.
//
// VAR_ tags: as in the reference (ShaderUtil.cpp:122-191) the variable table is discovered by
// scanning the source text for `VAR_<name>(key = value, ...)`.  Inside a method that receives
// the frame uniforms as `U`, the tag itself is an expression: the generated prelude defines
// `VAR_<name>(...)` as `(U.scene_var[k])`, k = order of first appearance.
//
// libhiprtc.so is opened on first use: the library has no load-time dependency on it.
#include "sdfr_jit.h"
#include "sdfr_pixel.h"

#include <dlfcn.h>
#include <hip/hiprtc.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace sdfr {

namespace {

struct Hiprtc
{
	void *lib = nullptr;
	decltype(&hiprtcCreateProgram) create = nullptr;
	decltype(&hiprtcCompileProgram) compile = nullptr;
	decltype(&hiprtcGetProgramLogSize) log_size = nullptr;
	decltype(&hiprtcGetProgramLog) log = nullptr;
	decltype(&hiprtcGetCodeSize) code_size = nullptr;
	decltype(&hiprtcGetCode) code = nullptr;
	decltype(&hiprtcDestroyProgram) destroy = nullptr;
	decltype(&hiprtcGetErrorString) error_string = nullptr;
	bool ok = false;
};

Hiprtc &hiprtc()
{
	static Hiprtc h;
	if (h.lib) return h;
	const char *names[] = {"libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"};
	for (const char *n : names)
		if ((h.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
	if (!h.lib) return h;
	h.create = (decltype(h.create))dlsym(h.lib, "hiprtcCreateProgram");
	h.compile = (decltype(h.compile))dlsym(h.lib, "hiprtcCompileProgram");
	h.log_size = (decltype(h.log_size))dlsym(h.lib, "hiprtcGetProgramLogSize");
	h.log = (decltype(h.log))dlsym(h.lib, "hiprtcGetProgramLog");
	h.code_size = (decltype(h.code_size))dlsym(h.lib, "hiprtcGetCodeSize");
	h.code = (decltype(h.code))dlsym(h.lib, "hiprtcGetCode");
	h.destroy = (decltype(h.destroy))dlsym(h.lib, "hiprtcDestroyProgram");
	h.error_string = (decltype(h.error_string))dlsym(h.lib, "hiprtcGetErrorString");
	h.ok = h.create && h.compile && h.log_size && h.log && h.code_size && h.code && h.destroy && h.error_string;
	return h;
}

// directory of the kernel headers: $SDFR_JIT_INCLUDE, or csrc/ beside the loaded library
std::string header_dir()
{
	if (const char *e = getenv("SDFR_JIT_INCLUDE")) return e;
	Dl_info info;
	if (dladdr((const void *)&header_dir, &info) && info.dli_fname)
	{
		std::string p = info.dli_fname;
		const size_t slash = p.rfind('/');
		return (slash == std::string::npos ? std::string(".") : p.substr(0, slash)) + "/csrc";
	}
	return "csrc";
}

} // namespace

void jit_unload(JitScene &js)
{
	if (js.module) (void)hipModuleUnload(js.module);
	if (js.query_module) (void)hipModuleUnload(js.query_module);
	if (js.d_frame) (void)hipFree(js.d_frame);
	js = JitScene();
}

bool jit_compile_code(const std::string &arch_name, const std::string &name, const std::string &scene_source, const std::vector<std::string> &var_slots,
	std::vector<char> &code, std::string &error, bool query)
{
	Hiprtc &rtc = hiprtc();
	if (!rtc.ok)
	{
		error = "run-time scene compilation needs libhiprtc.so, which could not be loaded";
		return false;
	}
	const std::string tu = jit_translation_unit(scene_source, var_slots, query);
	hiprtcProgram prog = nullptr;
	hiprtcResult rc = rtc.create(&prog, tu.c_str(), (name + ".scene.hip").c_str(), 0, nullptr, nullptr);
	if (rc != HIPRTC_SUCCESS)
	{
		error = std::string("hiprtcCreateProgram: ") + rtc.error_string(rc);
		return false;
	}
	// same code generation rules as the ahead-of-time build (buildlib.py): only explicit fma() fuses
	const std::string arch = "--offload-arch=" + arch_name;
	const std::string inc = "-I" + header_dir();
	const std::string block = "-DSDFR_PIXEL_BLOCK=" + std::to_string(pixel_block_threads()); // must match the launch
	// sqrt1 / rcp1 / div_c are exact only on verified domains (sdfr_math.h), which the built-in scenes are
	// checked against and a user's text is not: run-time scenes get the plain IEEE forms unless the text
	// opts in by containing the token SDFR_FAST_EXACT_MATH (say, in a comment)
	const char *math = scene_source.find("SDFR_FAST_EXACT_MATH") != std::string::npos ? "-DSDFR_FAST_EXACT_MATH=1" : "-DSDFR_SAFE_MATH=1";
	const std::string sharp_lanes = "-DSDFR_MESH_SHARP_LANES=" + std::to_string(SDFR_MESH_SHARP_LANES); // must match the launch (mesh_sharp_blocks)
	const char *opts[] = {arch.c_str(), "-std=c++17", "-O3", "-ffp-contract=off", "-fno-slp-vectorize", inc.c_str(), block.c_str(), math, sharp_lanes.c_str()};
	rc = rtc.compile(prog, (int)(sizeof opts / sizeof opts[0]), opts);
	size_t log_bytes = 0;
	rtc.log_size(prog, &log_bytes);
	std::string log(log_bytes, '\0');
	if (log_bytes > 1) rtc.log(prog, log.data());
	if (rc != HIPRTC_SUCCESS)
	{
		error = "scene '" + name + "' does not compile (" + rtc.error_string(rc) + "):\n" + log.c_str();
		rtc.destroy(&prog);
		return false;
	}
	size_t code_bytes = 0;
	rtc.code_size(prog, &code_bytes);
	code.resize(code_bytes);
	rtc.code(prog, code.data());
	rtc.destroy(&prog);
	return true;
}

bool jit_compile(int device, const std::string &name, const std::string &scene_source, const std::vector<std::string> &var_slots, JitScene &out,
	std::string &error)
{
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) != hipSuccess)
	{
		error = "hipGetDeviceProperties failed";
		return false;
	}
	std::vector<char> code;
	if (!jit_compile_code(prop.gcnArchName, name, scene_source, var_slots, code, error)) return false;

	JitScene js;
	js.name = name;
	js.source = scene_source;
	js.var_slots = var_slots;
	hipError_t e = hipModuleLoadData(&js.module, code.data());
	if (e == hipSuccess) e = hipModuleGetFunction(&js.prepare, js.module, "sdfr_jit_prepare");
	if (e == hipSuccess) e = hipModuleGetFunction(&js.pixel, js.module, "sdfr_jit_pixel");
	if (e == hipSuccess) e = hipModuleGetFunction(&js.pixel_debug, js.module, "sdfr_jit_pixel_debug");
	if (e == hipSuccess) e = hipMalloc((void **)&js.d_frame, sizeof(FrameU));
	if (e != hipSuccess)
	{
		error = std::string("loading the compiled scene failed: ") + hipGetErrorString(e);
		jit_unload(js);
		return false;
	}
	out = js;
	return true;
}

hipError_t jit_prepare(const JitScene &js, FrameU &U, hipStream_t stream)
{
	hipError_t e = hipMemcpyAsync(js.d_frame, &U, sizeof U, hipMemcpyHostToDevice, stream);
	if (e != hipSuccess) return e;
	FrameU *d = js.d_frame;
	void *args[] = {&d};
	e = hipModuleLaunchKernel(js.prepare, 1, 1, 1, 1, 1, 1, 0, stream, args, nullptr);
	if (e != hipSuccess) return e;
	e = hipMemcpyAsync(&U, js.d_frame, sizeof U, hipMemcpyDeviceToHost, stream);
	if (e != hipSuccess) return e;
	return hipStreamSynchronize(stream);
}

JitQueryStatus jit_query_kernels(JitScene &js, int device, const QueryKernels *&out, std::string &error)
{
	if (!js.query_module)
	{
		hipDeviceProp_t prop;
		if (hipGetDeviceProperties(&prop, device) != hipSuccess)
		{
			error = "hipGetDeviceProperties failed";
			return JIT_QUERY_HIP;
		}
		std::vector<char> code;
		if (!jit_compile_code(prop.gcnArchName, js.name, js.source, js.var_slots, code, error, true)) return JIT_QUERY_COMPILE;
		hipModule_t m = nullptr;
		QueryKernels found = {};
		hipError_t e = hipModuleLoadData(&m, code.data());
		for (int kind = 0; kind < QUERY_KERNEL_KINDS; ++kind)
			for (int dbg = 0; dbg < 2 && e == hipSuccess; ++dbg)
				e = hipModuleGetFunction(&found.k[kind][dbg].function, m, jit_query_symbol(kind, dbg != 0).c_str());
		if (e != hipSuccess)
		{
			error = std::string("loading the scene's query kernels failed: ") + hipGetErrorString(e);
			if (m) (void)hipModuleUnload(m);
			return JIT_QUERY_HIP;
		}
		js.query_module = m;
		js.query = found;
	}
	out = &js.query;
	return JIT_QUERY_OK;
}

PixelKernel jit_pixel_kernel(const JitScene &js, bool dbg)
{
	// launched like the scenes compiled ahead of time (launch_pixel, sdfr_kernels.hip), with the traits of a run-time scene: one wave
	// per tile unless asked otherwise, tile rows only (squares of tiles -- RowMap::unit_log2 -- are a built-in scene's own choice)
	uint32_t name_hash = 2166136261u; // a run-time scene is known by its name
	for (char ch : js.name) name_hash = (name_hash ^ (unsigned char)ch) * 16777619u;
	const PixelSceneTraits traits = {false, 8, false, 0x80000000u | name_hash | (dbg ? 1u : 0u)};
	return {{nullptr, dbg ? js.pixel_debug : js.pixel}, nullptr, traits}; // (a module's occupancy is asked on every launch)
}

} // namespace sdfr

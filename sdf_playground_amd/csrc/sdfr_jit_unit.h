// sdfr_jit_unit.h -- the text of the translation unit compiled for a run-time scene, and the names of its kernels.  Plain host code, no
// HIP header: sdfr_jit.cpp compiles and loads what this header writes, tests/cpp/query_kernels_host.cpp prints it on a machine without a GPU.
#pragma once
#include <string>
#include <vector>

#include "sdfr_query_args.h"

namespace sdfr {

// the list of query kernel kinds (sdfr_query_args.h) as text, by kind
struct QueryKernelRow
{
	const char *kind, *stem, *body, *args;
};
#define SDFR_QUERY_KERNEL_ROW(kind, stem, body, args) {#kind, #stem, #body, #args},
static const QueryKernelRow k_query_kernel_rows[QUERY_KERNEL_KINDS] = {SDFR_FOR_EACH_QUERY_KERNEL(SDFR_QUERY_KERNEL_ROW)};
#undef SDFR_QUERY_KERNEL_ROW

// the symbol of a run-time scene's query kernel of `kind` (QUERY_KERNEL_*)
inline std::string jit_query_symbol(int kind, bool dbg) { return std::string("sdfr_jit_") + k_query_kernel_rows[kind].stem + (dbg ? "_debug" : ""); }

// the translation unit compiled for a scene: variable macros, the scene text, the kernels (the pixel kernels, or with
// `query` the query kernels: of every kind the plain one, then the debug one)
inline std::string jit_translation_unit(const std::string &scene_source, const std::vector<std::string> &var_slots, bool query = false)
{
	std::string tu;
	tu += query ? "#include \"sdfr_query_kernel.h\"\n" : "#include \"sdfr_pixel_kernel.h\"\n";
	// a scene that came in the reference's dialect (sdfr_hlsl.cpp) needs the HLSL vocabulary
	if (scene_source.find("hlsl::SceneAdapter") != std::string::npos) tu += "#include \"sdfr_hlsl.h\"\n";
	tu += "namespace sdfr {\n";
	for (size_t k = 0; k < var_slots.size(); ++k)
		tu += "#define VAR_" + var_slots[k] + "(...) (U.scene_var[" + std::to_string(k) + "])\n";
	tu += "#line 1 \"scene\"\n";
	tu += scene_source;
	tu += "\n#line 1 \"sdfr_jit_kernels\"\n";
	if (query)
	{
		for (int kind = 0; kind < QUERY_KERNEL_KINDS; ++kind)
			for (int dbg = 0; dbg < 2; ++dbg)
				tu += "extern \"C\" __global__ SDFR_PIXEL_KERNEL_ATTRS(Scene) void " + jit_query_symbol(kind, dbg != 0) + "(SceneKernelArgs<" + k_query_kernel_rows[kind].args +
					"> a) { " + k_query_kernel_rows[kind].body + "<Scene, " + (dbg ? "true" : "false") + ">(a); }\n";
	}
	else
	{
		tu += "extern \"C\" __global__ void sdfr_jit_prepare(FrameU *U) { if (blockIdx.x == 0 && threadIdx.x == 0) Scene::prepare(*U); }\n";
		tu += "extern \"C\" __global__ SDFR_PIXEL_KERNEL_ATTRS(Scene) void sdfr_jit_pixel(PixelKernelArgs args) { pixel_kernel<Scene, false>(args); }\n";
		tu += "extern \"C\" __global__ SDFR_PIXEL_KERNEL_ATTRS(Scene) void sdfr_jit_pixel_debug(PixelKernelArgs args) { pixel_kernel<Scene, true>(args); }\n";
	}
	tu += "} // namespace sdfr\n";
	return tu;
}

} // namespace sdfr

// tests/hostsim/hlsl_host.cpp -- TEST-ONLY: a scene in the reference's dialect, translated by the library
// (sdfr_translate_scene_hlsl) and compiled for the CPU with the product's per-pixel pipeline, so that the CPU test tier can
// bit-compare it with the oracle.  Built once per scene with -DSDFR_HLSL_SCENE_FILE="<generated file>" and the scene's VAR_
// macros in -include'd form.  The product never loads this.
#include "render_rows.h"
#include "sdfr_hlsl.h"

namespace sdfr {
#include SDFR_HLSL_SCENE_FILE
} // namespace sdfr

using namespace sdfr;

extern "C" int hlslsim_render(FrameU *frame, float *out_rgba, unsigned *out_stats, int nthreads)
{
	frame_derive(*frame, -1); // no ahead-of-time scene: only the frame-level derivations (sky rotation, debug plane, extension lights)
	Scene::prepare(*frame);   // a scene in the library's C++ form may stage per-frame constants (the HLSL adapter's is empty)
	if (frame_needs_debug(*frame))
		render_rows(*frame, &render_pixel<Scene, true, HostStore>, out_rgba, out_stats, nthreads);
	else
		render_rows(*frame, &render_pixel<Scene, false, HostStore>, out_rgba, out_stats, nthreads);
	return 0;
}
extern "C" int hlslsim_frame_size() { return (int)sizeof(FrameU); }

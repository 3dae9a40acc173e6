// tests/cpp/labyrinth_fallback_host.cpp -- TEST-ONLY: the labyrinth's per-pixel pipeline for the CPU with the gradient table as the
// noise's gradient source, as the pixel kernel runs it (NoiseGradTable, sdfr_noise.h; the kernel keeps the table in LDS, this build in
// a static array filled by the same simplex_grad), and a count of what the table path sends back to the formula.  A lane whose `ok` is
// cleared -- a lattice coordinate whose mod289 left [-1, 289], or a gradient index that is no integer of the table -- evaluates the noise
// once more with the formula: on the GPU that is a divergent second pass, and tests/test_labyrinth_fallback_cpu.py uses the counts to
// show that the far frames of tests/labyrinth_step_cameras.py make some lanes, and not all, take it.  The product never loads this.
#include "render_rows.h"

using namespace sdfr;

namespace {

struct HostTab
{
	static float t[3][SDFR_NOISE_GRADS];
	static float at(int c, uint32_t k) { return t[c][k]; }
};
float HostTab::t[3][SDFR_NOISE_GRADS];

// per thread, per pixel: gradients read, and gradients read with `ok` cleared (by the hash before them or by their own index)
thread_local unsigned tl_grads, tl_cleared;

// NoiseGradTable<HostTab> and a counter on cleared `ok`
struct CountedTable
{
	typedef NoiseGradTable<HostTab>::Hash Hash;
	static vec3 grad(float j, bool &ok)
	{
		const vec3 g = NoiseGradTable<HostTab>::grad(j, ok);
		tl_grads++;
		if (!ok) tl_cleared++;
		return g;
	}
};

} // namespace

// The labyrinth's frame through render_pixel with the table.  out_rgba [h][w][4], out_stats [h][w][3] as hostsim_render;
// out_noise [h][w][2]: gradients read in the pixel, and how many of them with `ok` cleared.
extern "C" int lf_render(FrameU *frame, float *out_rgba, unsigned *out_stats, unsigned *out_noise, int nthreads)
{
	for (int k = 0; k < SDFR_NOISE_GRADS; ++k)
	{
		const vec3 g = simplex_grad((float)k);
		HostTab::t[0][k] = g.x; HostTab::t[1][k] = g.y; HostTab::t[2][k] = g.z;
	}
	const int si = scene_index("labyrinth");
	if (si < 0) return -1;
	frame_derive(*frame, si);
	if (frame_needs_debug(*frame)) return -2; // the debug variables are off in these frames
	const int width = frame->width;
	render_rows(*frame, [=](const FrameU &U, int x, int y, PixelCounters &c, HostStore &store) {
		tl_grads = tl_cleared = 0;
		const vec4 v = render_pixel<SceneLabyrinth, false, HostStore, CountedTable>(U, x, y, c, store);
		out_noise[2 * ((size_t)y * width + x) + 0] = tl_grads;
		out_noise[2 * ((size_t)y * width + x) + 1] = tl_cleared;
		return v;
	}, out_rgba, out_stats, nthreads);
	return 0;
}
extern "C" int lf_frame_size() { return (int)sizeof(FrameU); }

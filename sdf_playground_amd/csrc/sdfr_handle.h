// sdfr_handle.h -- the renderer handle behind the C ABI (include/sdfr.h) and the helpers the
// translation units that implement it share (sdfr_api.cpp: single-GPU entries; sdfr_comm.cpp:
// the multi-GPU gather over RCCL).  Host code only.
#pragma once
#include "../../include/sdfr.h"

#include "sdfr_hostframe.h"
#include "sdfr_hostlib.h"
#include "sdfr_jit.h"
#include "sdfr_kernels.h"
#include "sdfr_stage.h"

#include <cassert>
#include <cstdio>
#include <exception>
#include <initializer_list>
#include <string>
#include <vector>

// A device buffer that only grows, kept from call to call.  reserve() replaces a buffer that is too small (the old contents are
// gone); the caller first waits for whatever may still use the old one.  Empty after a failed reserve().
struct sdfr_device_buffer
{
	void *ptr = nullptr;
	size_t bytes = 0;
	hipError_t reserve(size_t need)
	{
		if (bytes >= need) return hipSuccess;
		release();
		const hipError_t e = hipMalloc(&ptr, need);
		if (e == hipSuccess) bytes = need;
		return e;
	}
	void release()
	{
		(void)hipFree(ptr);
		ptr = nullptr;
		bytes = 0;
	}
};

// One device buffer cut into pieces (sdfr_stage.h): the parts of a workspace, or the device stand-ins of a caller's host arrays, of
// which the answers are copied back at the end of the call (stage_host_arrays and copy_answers_back, sdfr_api.cpp).
struct Carving
{
	size_t offset[sdfr::SDFR_STAGE_MAX_PIECES], total = 0;
	sdfr_device_buffer *buffer = nullptr;
	struct { void *host; const void *device; size_t bytes; } answers[sdfr::SDFR_STAGE_MAX_PIECES];
	int n_answers = 0;
	Carving() {}
	Carving(std::initializer_list<size_t> bytes) { cut(bytes.begin(), (int)bytes.size()); }
	void cut(const size_t *bytes, int n)
	{
		assert(n <= (int)sdfr::SDFR_STAGE_MAX_PIECES);
		total = sdfr::stage_offsets(bytes, n, offset);
	}
	hipError_t reserve(sdfr_device_buffer &b) // (the caller first waits for whatever may still use the old one)
	{
		buffer = &b;
		return b.reserve(total);
	}
	template <class T>
	T *piece(int k) const
	{
		return reinterpret_cast<T *>(static_cast<char *>(buffer->ptr) + offset[k]);
	}
};
// An array of a call whose arrays are host or device memory: the pointer the kernel is handed it through (any T *: read and written
// as a void *), its bytes, and whether the kernel reads it (an input) or writes it (an answer)
struct StagedArray
{
	void *field;
	size_t bytes;
	bool input;
};

struct sdfr_renderer
{
	// What one frame in flight owns: its stream, its workspace (ray queue, counter records, tile cursors with the row order
	// learned from ITS last frame), its counters and its two events.  `lane` is the lane of the frame submitted last; every
	// entry point but sdfr_render works on it.  With two frames in flight (sdfr_set_frames_in_flight) `other` is the lane of
	// the frame before, and sdfr_render swaps the two before it launches.
	struct Lane
	{
		hipStream_t stream = nullptr; // user_stream with one frame in flight; the library's own with two
		sdfr::WavefrontWorkspace ws = {};
		size_t wavefront_capacity = 0; // pixels the wavefront-only part of `ws` is allocated for
		sdfr::RenderTotals *d_totals = nullptr; // [2]: counters of the last launch; [1] = the private strips of a gather (sdfr_comm.cpp)
		int totals_parts = 1;                   // how many of them the last render filled
		hipEvent_t ev_begin = nullptr, ev_end = nullptr;
		bool have_render = false;
		const char *out_lo = nullptr, *out_hi = nullptr; // device range its last frame was rendered into (two frames in flight only)
		const char *pst_lo = nullptr, *pst_hi = nullptr; // ... and the device range of that frame's pixel_stats
	};
	Lane lane, other;
	int frames_in_flight = 1;
	hipStream_t user_stream = nullptr; // what sdfr_set_stream gave (in use while frames_in_flight == 1)
	// the two streams of two frames in flight, made at the first switch to it and kept until the handle goes: the lanes' and the
	// extraction's events were last recorded on them, and the runtime looks at an event's last stream whenever the event is waited for
	hipStream_t own_streams[2] = {nullptr, nullptr};

	int device = 0;
	int scene = -1; // index of an ahead-of-time scene, or SDFR_SCENE_COUNT: `jit` holds a scene compiled at run time
	sdfr::JitScene jit;
	int schedule = SDFR_SCHEDULE_PIXEL; // the faster one on every measured scene
	bool profiling = false;
	int tile_w_log2 = 0; // 0: the scene's own tile shape (SceneTileShape, 8 x 8 unless it says otherwise); SDFR_TILE_W_LOG2 sets 3 .. 6
	int launch_mode = 0; // sdfr_set_launch_mode
	int priv_count = 0, priv_period = 1; // sdfr_set_strip_split
	sdfr::FrameU U;
	sdfr::host::ShaderVariableManager vars;
	std::vector<std::string> scene_var_slots; // slot k of FrameU::scene_var <- this variable
	mutable std::string error;

	sdfr_device_buffer stage, pstat; // staging image and pixel_stats of host-destination renders
	sdfr_device_buffer query;        // staging of host-memory queries (sdfr_query_*, sdfr_pick): inputs and answers; kept up to 64 MiB
	// sdfr_mesh_extract: the lattice's distances, the vertex index per cell, the quad offset per lattice point and the scans' block
	// sums (the handle's own: never a lane's workspace); kept up to 64 MiB like `query`, which stages the arrays of a host extraction
	sdfr_device_buffer mesh;
	hipEvent_t ev_mesh[7] = {}; // made by the first extraction.  [6]: the end of the last one's device work, which the next one waits
	                            // for before it reuses `mesh`; [0..5]: around its stages when profiling is on (sdfr_mesh_get_timings)
	int mesh_timed = 0;         // 0: the last extraction was not timed; 1: up to its counts; 2: all four stages; 3: no normals asked
	// sdfr_render_aa: one pass's compact strips of the supersampled frame (RGBA32F), their per-sub-sample counters when pixel_stats is
	// wanted, and the counters of one pass's launch.  The handle's own and kept between calls (an animation calls every frame): never
	// a lane's workspace.  ev_aa_done: the end of the last call's device work, which the next call -- perhaps on the other lane's
	// stream -- waits for before it reuses them.  ev_aa: around each pass's resolve when profiling is on ("draw: resolve").
	sdfr_device_buffer aa_color, aa_stats, aa_totals;
	hipEvent_t ev_aa_done = nullptr;
	std::vector<hipEvent_t> ev_aa;
	int aa_timed_passes = 0; // passes of the last render if it was a profiled sdfr_render_aa, else 0
	// sdfr_register_host_target: the caller's persistent host image, page-locked with the runtime
	void *pinned_host = nullptr;
	size_t pinned_bytes = 0;

	hipEvent_t ev_post[3] = {}; // before / between / after the two post-processing kernels
	bool have_post = false;
	bool step_shortcuts = true; // sdfr_set_step_shortcuts
	sdfr_device_buffer post_flags; // per row segment: did the horizontal bloom pass store any light (sdfr_post.hip)
	double ms_setup = 0.0;      // host time of the last latch_frame (+ Scene::prepare of a run-time scene)
	hipEvent_t ev_march[32] = {}, ev_shade[32] = {};
	int last_rounds = 0;
	bool last_wavefront = false;
	bool last_profiled = false;

	// multi-GPU gather (sdfr_comm.cpp): send / receive / assembly run on a stream of their own so
	// that the root's private strips render while the peers' strips travel
	hipStream_t comm_stream = nullptr;
	hipEvent_t ev_strips = nullptr, ev_gathered = nullptr;
	hipEvent_t ev_xfer[2] = {nullptr, nullptr}; // around the last gather's transfer on the comm stream ("gather transfer", sdfr_get_timings)
	bool have_xfer = false;
	size_t xfer_bytes = 0;                      // bytes this rank sent (peers) or received (rank 0) in that transfer
	sdfr_device_buffer wire;   // this rank's compact strips; on the root: world x that, slot 0 = its own
	std::vector<void *> comms_used; // sdfr_comm* whose transfers ran on comm_stream (sdfr_comm.cpp keeps both sides of the list)

	unsigned launches = 0; // render launches so far: did a call that failed launch anything before it failed
};

static inline int fail(const sdfr_renderer *r, int code, const std::string &msg)
{
	if (r) r->error = msg;
	return code;
}
// No C++ exception crosses the C boundary: every extern "C" entry point with a body of more than a line runs inside this
// (std::bad_alloc, std::regex_error from the scene translation, std::system_error from a thread that cannot start ...
// would otherwise reach a C or ctypes caller as std::terminate -> abort()).
template <class F>
static inline int guarded(const sdfr_renderer *r, F body) noexcept
{
	try
	{
		return body();
	}
	catch (const std::exception &e)
	{
		try
		{
			if (r) r->error = std::string("internal error: ") + e.what();
			fprintf(stderr, "libsdfr: internal error: %s\n", e.what());
		}
		catch (...)
		{
		}
		return SDFR_ERR_INTERNAL;
	}
	catch (...)
	{
		return SDFR_ERR_INTERNAL;
	}
}
static inline int hip_fail(const sdfr_renderer *r, hipError_t e, const char *what)
{
	return fail(r, SDFR_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define SDFR_HIP(call) \
	do { hipError_t e_ = (call); if (e_ != hipSuccess) return hip_fail(r, e_, #call); } while (0)

namespace sdfr {

// bytes of a compact image of `pixels` pixels (the packed strip formats are padded to 4)
size_t image_bytes(size_t pixels, int format);
bool is_wire_format(int format);

// one launch of the handle's scene over the rows `mode` selects, on the current lane (sdfr_api.cpp).  `totals` receives
// the launch's counters (nullptr: the lane's d_totals).  caller_times: the caller records the lane's ev_begin / ev_end
// and sets its totals_parts (a gather times strips, transfer and assembly as one frame).
int render_impl(sdfr_renderer *r, int width, int height, int rank, int world, void *out, int format, int out_on_host, uint32_t *pixel_stats,
	RenderMode mode, RenderTotals *totals = nullptr, bool caller_times = false);

// the stream and events of a gathered frame (sdfr_comm.cpp)
int gather_prepare_streams(sdfr_renderer *r);
// the handle is going away: communicators that remember it must forget it (sdfr_comm.cpp)
void comm_forget_renderer(sdfr_renderer *r);

} // namespace sdfr

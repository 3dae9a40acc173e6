// sdfr_span_plan.h -- the span queries (sdfr_query_ray_spans, sdfr_pick_spans, sdfr_mesh_spans in include/sdfr.h) as far as the host decides
// them: the argument checks in the order their errors win, the effective t_max, the kernel's arguments, the blocks of the launch and the
// staging sizes of a host call.  Plain host arithmetic, no HIP call, like sdfr_query_plan.h: span_impl (sdfr_api.cpp) carries the plan
// out, tests/test_span_cpu.py checks it on a machine without a GPU.
#pragma once
#include "sdfr_query_plan.h"
#include "sdfr_span.h"

namespace sdfr {

// the parameters the entries accept: t_max finite and >= 0 (0: limits.range), min_step finite and > 0, iso finite, 1 .. 2^20 steps,
// 0 .. 64 spans stored per item
inline bool span_params_ok(const SpanParams &p)
{
	return std::isfinite(p.t_max) && p.t_max >= 0.f && std::isfinite(p.min_step) && p.min_step > 0.f && std::isfinite(p.iso) && p.max_steps >= 1 &&
		p.max_steps <= SPAN_MAX_STEPS && p.max_spans >= 0 && p.max_spans <= SPAN_MAX_SPANS;
}

// What an entry point was given.  kind: QUERY_RAYS (in0, in1 = origins, dirs), QUERY_PICK (in0 = pixels; null: QUERY_FRAME, every pixel of
// the frame) or QUERY_MESH (in0, in1 = positions, normals; reach).  The pointers are only compared with null here.
struct SpanRequest
{
	int kind;
	int64_t n;
	const void *in0, *in1;
	int width, height; // picks
	float reach;       // meshes
	const SpanParams *params;
	void *summaries, *spans;
	int on_host;
};
enum { SPAN_STAGE_PIECES = 4, SPAN_STAGE_INPUTS = 2 };
// the pointer members of SpanArgs a host call stages, in the order of SpanPlan::bytes, for an item list (0) and for pixels (1)
static const size_t k_span_stage_slots[2][SPAN_STAGE_PIECES] = {
	{offsetof(SpanArgs, pos), offsetof(SpanArgs, dir), offsetof(SpanArgs, summaries), offsetof(SpanArgs, spans)},
	{offsetof(SpanArgs, pixels), offsetof(SpanArgs, dir), offsetof(SpanArgs, summaries), offsetof(SpanArgs, spans)},
};
struct SpanPlan
{
	int status; // QUERY_PLAN_*
	const char *error;
	bool nothing_to_do; // n = 0
	SpanArgs a;         // for the caller's arrays as device memory; a host call points the slots at its staging pieces
	size_t bytes[SPAN_STAGE_PIECES]; // the first input, the second, the summaries, the spans
	int width, height;  // of the frame to latch
	uint32_t blocks;    // of one wave
};

// blocks of one wave: an 8 x 8 tile of the frame each, or 64 consecutive items
inline uint32_t span_blocks(int kind, uint32_t n, int width, int height)
{
	if (kind == QUERY_FRAME) return (((uint32_t)width + QUERY_TILE - 1u) / QUERY_TILE) * (((uint32_t)height + QUERY_TILE - 1u) / QUERY_TILE);
	return (n + QUERY_BLOCK_ITEMS - 1u) / QUERY_BLOCK_ITEMS;
}

// The checks after the handle's and before the scene's, in the order their errors win.  range: limits.range.
inline SpanPlan plan_spans(const SpanRequest &c, float range)
{
	SpanPlan p = {};
	auto fail = [&p](const char *text) {
		p.status = QUERY_PLAN_INVALID_ARGUMENT;
		p.error = text;
		return p;
	};
	const bool pick = c.kind == QUERY_PICK || c.kind == QUERY_FRAME, frame = pick && !c.in0;
	if (!c.params || !c.summaries || (!pick && (!c.in0 || !c.in1))) return fail("null pointer");
	if (!is_flag(c.on_host)) return fail("on_host must be 0 or 1");
	const SpanParams &sp = *c.params;
	if (!span_params_ok(sp)) return fail("bad span parameters");
	const int64_t most = (int64_t)1 << 30; // n * max(max_spans, 1) <= 2^30
	if (c.n < 0 || c.n > most || c.n * (int64_t)(sp.max_spans > 1 ? sp.max_spans : 1) > most) return fail("bad item count");
	if (pick && !frame_size_ok(c.width, c.height)) return fail("bad frame size");
	if (c.kind == QUERY_MESH && !(std::isfinite(c.reach) && c.reach > 0.f)) return fail("reach must be finite and > 0");
	if (sp.max_spans > 0 && !c.spans) return fail("null spans with max_spans > 0");
	p.nothing_to_do = c.n == 0;
	if (p.nothing_to_do) return p;
	if (frame && c.n != (int64_t)c.width * c.height) return fail("without a pixel list n must be width * height");

	SpanArgs &a = p.a;
	a.kind = frame ? QUERY_FRAME : pick ? QUERY_PICK : c.kind;
	a.n = (int32_t)c.n;
	if (pick) a.pixels = static_cast<const int32_t *>(c.in0);
	else
	{
		a.pos = static_cast<const float *>(c.in0);
		a.dir = static_cast<const float *>(c.in1);
	}
	a.reach = c.kind == QUERY_MESH ? c.reach : 0.f;
	a.t_max = sp.t_max == 0.f ? range : sp.t_max;
	a.min_step = sp.min_step;
	a.iso = sp.iso;
	a.max_steps = sp.max_steps;
	a.max_spans = sp.max_spans;
	a.summaries = static_cast<uint32_t *>(c.summaries);
	a.spans = sp.max_spans > 0 ? static_cast<float *>(c.spans) : nullptr;
	p.bytes[0] = frame ? 0 : (size_t)c.n * (pick ? 8 : 12);
	p.bytes[1] = pick ? 0 : (size_t)c.n * 12;
	p.bytes[2] = (size_t)c.n * 4 * SPAN_SUMMARY_WORDS;
	p.bytes[3] = (size_t)c.n * (size_t)sp.max_spans * 8;
	p.width = pick ? c.width : 1;
	p.height = pick ? c.height : 1;
	p.blocks = span_blocks(a.kind, (uint32_t)c.n, p.width, p.height);
	return p;
}

} // namespace sdfr

// sdfr_slice_plan.h -- sdfr_slice_extract (include/sdfr.h) as far as the host decides it: the argument checks in the order their errors
// win, the grid, the sampling launch's arguments and blocks, the sizes of the workspace's five pieces, and once the totals are read back
// whether the call fills the caller's arrays and how many bytes of each.  Plain host arithmetic, no HIP call, like sdfr_mesh_plan.h:
// slice_impl (sdfr_api.cpp) carries the plan out, tests/test_slice_cpu.py checks it on a machine without a GPU.
#pragma once
#include "sdfr_mesh.h"
#include "sdfr_query_plan.h"
#include "sdfr_slice.h"

namespace sdfr {

enum { SLICE_MAX_CELLS = 16384, SLICE_MAX_LAYERS = 65536 };

// the grid sdfr_slice_extract accepts: origin, steps and iso finite; du and dv not all zero (dw may be: layers on top of each other);
// 1 .. 16384 cells along u and v, 1 .. 65536 layers; at most 2^30 lattice points
inline bool slice_grid_ok(const SliceGrid &g)
{
	bool ok = std::isfinite(g.iso), u = false, v = false;
	for (int c = 0; c < 3; ++c)
	{
		ok = ok && std::isfinite(g.origin[c]) && std::isfinite(g.du[c]) && std::isfinite(g.dv[c]) && std::isfinite(g.dw[c]);
		u = u || g.du[c] != 0.f;
		v = v || g.dv[c] != 0.f;
	}
	ok = ok && u && v && g.nu >= 1 && g.nu <= SLICE_MAX_CELLS && g.nv >= 1 && g.nv <= SLICE_MAX_CELLS && g.layers >= 1 && g.layers <= SLICE_MAX_LAYERS;
	return ok && (int64_t)(g.nu + 1) * (g.nv + 1) * g.layers <= (int64_t)1 << 30;
}

// What sdfr_slice_extract was given; but for the grid's, the pointers are only compared with null here
struct SliceRequest
{
	const SliceGrid *grid; // sdfr_slice_grid, field for field
	int64_t vertex_capacity, segment_capacity;
	float *positions, *coords;
	uint32_t *segments;
	const void *counts;
	int on_host;
};
struct SlicePlan
{
	int status; // QUERY_PLAN_*
	const char *error;
	SliceGrid g;
	SliceArgs sample; // but `rows` and `out`, which are the entry point's
	size_t points;
	// bytes of the workspace's pieces: the lattice, the points' vertex scan, the points' segment scan, both scans' block sums, the layer
	// offsets (layers + 1 of the vertices, then layers + 1 of the segments)
	size_t work[5];
};

// the launch that samples the grid's lattice, but `rows` and `out`
inline SliceArgs slice_sample_args(const SliceGrid &g)
{
	SliceArgs a = {};
	for (int c = 0; c < 3; ++c)
	{
		a.origin[c] = g.origin[c];
		a.du[c] = g.du[c];
		a.dv[c] = g.dv[c];
		a.dw[c] = g.dw[c];
	}
	a.pu = g.nu + 1;
	a.pv = g.nv + 1;
	a.layers = g.layers;
	return a;
}
// blocks of one wave that cover the stack in the mapping a.rows selects: 8 x 8 tiles of each layer, or runs of 64 points
inline uint32_t slice_sample_blocks(const SliceArgs &a)
{
	const uint32_t pu = (uint32_t)a.pu, pv = (uint32_t)a.pv, layers = (uint32_t)a.layers;
	return a.rows ? (pu * pv * layers + 63u) / 64u : ((pu + 7u) / 8u) * ((pv + 7u) / 8u) * layers;
}

// The checks after the handle's and before the scene's, in the order their errors win.
inline SlicePlan plan_slice(const SliceRequest &c)
{
	SlicePlan p = {};
	auto fail = [&p](const char *text) {
		p.status = QUERY_PLAN_INVALID_ARGUMENT;
		p.error = text;
		return p;
	};
	if (!c.grid || !c.counts) return fail("null pointer");
	if (!is_flag(c.on_host)) return fail("on_host must be 0 or 1");
	const SliceGrid &g = *c.grid;
	if (!slice_grid_ok(g)) return fail("bad slice grid");
	if (c.vertex_capacity < 0 || c.segment_capacity < 0) return fail("negative capacity");
	if ((c.vertex_capacity > 0 && !c.positions) || (c.segment_capacity > 0 && !c.segments)) return fail("null array with a capacity");

	p.g = g;
	p.sample = slice_sample_args(g);
	p.points = slice_point_count(g);
	p.work[0] = p.points * 4;
	p.work[1] = (p.points + 1) * 4;
	p.work[2] = (p.points + 1) * 4;
	p.work[3] = 2 * mesh_scan_sum_words(p.points + 1) * 4;
	p.work[4] = 2 * ((size_t)g.layers + 1) * 4;
	return p;
}

// The second phase, with the totals the device counted: the counts the caller is told, whether the capacities allow the call to fill the
// arrays (a stack without a vertex fills nothing), and the bytes of positions, coords (not wanted: 0) and segments it then writes
struct SliceFill
{
	int64_t vertices, segments;
	bool fill;
	size_t bytes[3];
};
inline SliceFill plan_slice_fill(const SliceRequest &c, uint32_t vertices, uint32_t segments)
{
	SliceFill f = {};
	f.vertices = (int64_t)vertices;
	f.segments = (int64_t)segments;
	f.fill = f.vertices <= c.vertex_capacity && f.segments <= c.segment_capacity && vertices != 0;
	f.bytes[0] = (size_t)vertices * 12;
	f.bytes[1] = c.coords ? (size_t)vertices * 8 : 0;
	f.bytes[2] = (size_t)segments * 8;
	return f;
}

} // namespace sdfr

// sdfr_measure_plan.h -- sdfr_measure (include/sdfr.h) as far as the host decides it: the argument checks in the order their errors win, the
// effective t_max, the kernel's arguments, the blocks of the launch, the sizes of the reduction's passes and the workspace.  Plain host
// arithmetic, no HIP call, like sdfr_span_plan.h: measure_impl (sdfr_api.cpp) carries the plan out, tests/test_measure_cpu.py checks it on
// a machine without a GPU.
#pragma once
#include "sdfr_measure.h"
#include "sdfr_span_plan.h"

namespace sdfr {

// the grids the entry accepts: everything finite, du, dv and dw not all zero, 1 .. 8192 columns per axis and at most 2^24 in all
inline bool measure_grid_ok(const MeasureGrid &g)
{
	bool ok = true, u = false, v = false, w = false;
	for (int c = 0; c < 3; ++c)
	{
		ok = ok && std::isfinite(g.origin[c]) && std::isfinite(g.du[c]) && std::isfinite(g.dv[c]) && std::isfinite(g.dw[c]);
		u = u || g.du[c] != 0.f;
		v = v || g.dv[c] != 0.f;
		w = w || g.dw[c] != 0.f;
	}
	return ok && u && v && w && g.nu >= 1 && g.nu <= MEASURE_MAX_AXIS && g.nv >= 1 && g.nv <= MEASURE_MAX_AXIS && (int64_t)g.nu * g.nv <= (int64_t)MEASURE_MAX_COLUMNS;
}

// What the entry point was given.  The pointers are only compared with null here.
struct MeasureRequest
{
	const MeasureGrid *grid;
	const SpanParams *params;
	void *out, *columns;
	int on_host;
};
enum { MEASURE_MAX_PASSES = 4 }; // 64^4 = 2^24 records, and there are fewer tiles than columns
struct MeasurePlan
{
	int status; // QUERY_PLAN_*
	const char *error;
	MeasureArgs a;       // for the caller's `columns` as device memory; a host call points it at its staging piece.  partials, tally: null
	uint32_t blocks;     // of one wave: the tiles
	int passes;          // of k_measure_reduce
	uint32_t pass_records[MEASURE_MAX_PASSES]; // the records pass k reads; it writes ceil(that / 64)
	int result_in;       // which partials buffer holds the one record at the end: 0 or 1 (pass k reads buffer k % 2 and writes the other)
	size_t work[3];      // the two partials buffers and the tally
	size_t column_bytes; // of `columns`, 0 if not wanted
};

// The checks after the handle's and before the scene's, in the order their errors win.  range: limits.range.
inline MeasurePlan plan_measure(const MeasureRequest &c, float range)
{
	MeasurePlan p = {};
	auto fail = [&p](const char *text) {
		p.status = QUERY_PLAN_INVALID_ARGUMENT;
		p.error = text;
		return p;
	};
	if (!c.grid || !c.params || !c.out) return fail("null pointer");
	if (!is_flag(c.on_host)) return fail("on_host must be 0 or 1");
	const MeasureGrid &g = *c.grid;
	if (!measure_grid_ok(g)) return fail("bad measure grid");
	const SpanParams &sp = *c.params;
	if (!span_params_ok(sp) || sp.max_spans != 0) return fail("bad span parameters");

	MeasureArgs &a = p.a;
	for (int k = 0; k < 3; ++k) a.origin[k] = g.origin[k], a.du[k] = g.du[k], a.dv[k] = g.dv[k], a.dw[k] = g.dw[k];
	a.nu = g.nu;
	a.nv = g.nv;
	a.t_max = sp.t_max == 0.f ? range : sp.t_max;
	a.min_step = sp.min_step;
	a.iso = sp.iso;
	a.max_steps = sp.max_steps;
	a.columns = static_cast<uint32_t *>(c.columns);
	p.blocks = measure_tiles(g.nu) * measure_tiles(g.nv);
	for (uint32_t n = p.blocks; n > 1u; n = (n + (uint32_t)MEASURE_RUN - 1u) / (uint32_t)MEASURE_RUN) p.pass_records[p.passes++] = n;
	p.result_in = p.passes % 2;
	p.work[0] = (size_t)p.blocks * MEASURE_MOMENTS * sizeof(double);
	p.work[1] = (size_t)((p.blocks + (uint32_t)MEASURE_RUN - 1u) / (uint32_t)MEASURE_RUN) * MEASURE_MOMENTS * sizeof(double);
	p.work[2] = MEASURE_TALLY_BYTES;
	p.column_bytes = c.columns ? (size_t)g.nu * (size_t)g.nv * 4 * MEASURE_COLUMN_WORDS : 0;
	return p;
}

// ---- the physical properties (sdfr_measure_properties), pure host arithmetic in fp64, every operation separate, in the order written in
// include/sdfr.h
struct SolidProperties // sdfr_solid_properties
{
	double volume, mass;
	double centroid[3];
	double inertia[6]; // xx, yy, zz, xy, yz, zx
};
inline void measure_properties(const MeasureGrid &g, const MeasureResult &res, double density, SolidProperties &out)
{
	SolidProperties o = {};
	const double *M = res.moments;
	if (!(M[0] > 0.0))
	{
		out = o;
		return;
	}
	double A[3][3]; // the columns du, dv, dw
	for (int r = 0; r < 3; ++r) A[r][0] = (double)g.du[r], A[r][1] = (double)g.dv[r], A[r][2] = (double)g.dw[r];
	const double cx = A[1][1] * A[2][2] - A[2][1] * A[1][2], cy = A[2][1] * A[0][2] - A[0][1] * A[2][2], cz = A[0][1] * A[1][2] - A[1][1] * A[0][2];
	const double det = (A[0][0] * cx + A[1][0] * cy) + A[2][0] * cz;
	const double scale = std::fabs(det);
	o.volume = M[0] * scale;
	o.mass = density * o.volume;
	const double cu = M[1] / M[0], cv = M[2] / M[0], cw = M[3] / M[0];
	for (int r = 0; r < 3; ++r) o.centroid[r] = (((double)g.origin[r] + cu * A[r][0]) + cv * A[r][1]) + cw * A[r][2];
	const double foot = M[0] / 12.0;
	double C[3][3];
	C[0][0] = (M[4] - cu * M[1]) + foot;
	C[1][1] = (M[5] - cv * M[2]) + foot;
	C[2][2] = M[6] - cw * M[3];
	C[0][1] = C[1][0] = M[7] - cu * M[2];
	C[1][2] = C[2][1] = M[8] - cv * M[3];
	C[2][0] = C[0][2] = M[9] - cw * M[1];
	double T[3][3], P[3][3];
	for (int k = 0; k < 3; ++k)
		for (int s = 0; s < 3; ++s) T[k][s] = (C[k][0] * A[s][0] + C[k][1] * A[s][1]) + C[k][2] * A[s][2];
	for (int r = 0; r < 3; ++r)
		for (int s = 0; s < 3; ++s) P[r][s] = (A[r][0] * T[0][s] + A[r][1] * T[1][s]) + A[r][2] * T[2][s];
	const double k = density * scale;
	o.inertia[0] = k * (P[1][1] + P[2][2]);
	o.inertia[1] = k * (P[2][2] + P[0][0]);
	o.inertia[2] = k * (P[0][0] + P[1][1]);
	o.inertia[3] = -(k * P[0][1]);
	o.inertia[4] = -(k * P[1][2]);
	o.inertia[5] = -(k * P[2][0]);
	out = o;
}

} // namespace sdfr

// sdfr_mesh_plan.h -- sdfr_mesh_extract (include/sdfr.h) as far as the host decides it: the argument checks in the order their errors
// win, the grid, the lattice launch's arguments, the sizes of the workspace's four pieces, and once the two totals are read back whether
// the call fills the caller's arrays and how many bytes of each.  Plain host arithmetic, no HIP call, like sdfr_query_plan.h and
// sdfr_atlas_plan.h: mesh_impl (sdfr_api.cpp) carries the plan out, tests/test_mesh_plan_cpu.py checks it on a machine without a GPU.
#pragma once
#include "sdfr_mesh.h"
#include "sdfr_mesh_survey.h"
#include "sdfr_query_plan.h"

namespace sdfr {

// What sdfr_mesh_extract was given; but for the grid's, the pointers are only compared with null here
struct MeshRequest
{
	const MeshGrid *grid; // sdfr_mesh_grid, field for field
	int64_t vertex_capacity, triangle_capacity;
	float *positions, *normals;
	uint32_t *indices;
	const void *counts;
	int on_host;
};
struct MeshPlan
{
	int status; // QUERY_PLAN_*
	const char *error;
	MeshGrid g;
	LatticeArgs lattice; // but `rows` and `out`, which are the entry point's
	size_t points, cells;
	size_t work[4]; // bytes of the workspace's pieces: the lattice, the cells' scan, the points' scan, both scans' block sums
};

// the launch that samples the grid's lattice, but `rows` and `out`
inline LatticeArgs mesh_lattice_args(const MeshGrid &g)
{
	LatticeArgs la = {};
	for (int a = 0; a < 3; ++a) la.origin[a] = g.origin[a];
	la.cell = g.cell;
	la.px = g.n[0] + 1;
	la.py = g.n[1] + 1;
	la.pz = g.n[2] + 1;
	return la;
}
// blocks of one wave that cover the lattice in the mapping g.rows selects: 4 x 4 x 4 bricks of points, or runs of 64
inline uint32_t query_lattice_blocks(const LatticeArgs &g)
{
	const uint32_t px = (uint32_t)g.px, py = (uint32_t)g.py, pz = (uint32_t)g.pz;
	return g.rows ? (px * py * pz + 63u) / 64u : ((px + 3u) / 4u) * ((py + 3u) / 4u) * ((pz + 3u) / 4u);
}
// ... and the sharp-vertex launch's: 64 / SDFR_MESH_SHARP_LANES vertices per block of one wave
inline uint32_t mesh_sharp_blocks(uint32_t vertices)
{
	const uint32_t per_block = (uint32_t)QUERY_BLOCK_ITEMS / SDFR_MESH_SHARP_LANES;
	return (vertices + per_block - 1u) / per_block;
}

// The checks after the handle's and before the scene's, in the order their errors win.
inline MeshPlan plan_mesh(const MeshRequest &c)
{
	MeshPlan p = {};
	auto fail = [&p](const char *text) {
		p.status = QUERY_PLAN_INVALID_ARGUMENT;
		p.error = text;
		return p;
	};
	if (!c.grid || !c.counts) return fail("null pointer");
	if (!is_flag(c.on_host)) return fail("on_host must be 0 or 1");
	const MeshGrid &g = *c.grid;
	if (!mesh_grid_ok(g)) return fail("bad mesh grid");
	if (c.vertex_capacity < 0 || c.triangle_capacity < 0) return fail("negative capacity");
	if ((c.vertex_capacity > 0 && !c.positions) || (c.triangle_capacity > 0 && !c.indices)) return fail("null array with a capacity");

	p.g = g;
	p.lattice = mesh_lattice_args(g);
	p.points = mesh_point_count(g);
	p.cells = mesh_cell_count(g);
	p.work[0] = p.points * 4;
	p.work[1] = (p.cells + 1) * 4;
	p.work[2] = (p.points + 1) * 4;
	p.work[3] = (mesh_scan_sum_words(p.cells + 1) + mesh_scan_sum_words(p.points + 1)) * 4;
	return p;
}

// The second phase, with the totals the device counted: the counts the caller is told, whether the capacities allow the call to fill the
// arrays (a mesh without a vertex fills nothing), and the bytes of positions, normals (not wanted: 0) and indices it then writes
struct MeshFill
{
	int64_t vertices, triangles;
	bool fill;
	size_t bytes[3];
};
inline MeshFill plan_mesh_fill(const MeshRequest &c, uint32_t vertices, uint32_t quads)
{
	MeshFill f = {};
	f.vertices = (int64_t)vertices;
	f.triangles = 2 * (int64_t)quads;
	f.fill = f.vertices <= c.vertex_capacity && f.triangles <= c.triangle_capacity && vertices != 0;
	f.bytes[0] = (size_t)vertices * 12;
	f.bytes[1] = c.normals ? (size_t)vertices * 12 : 0;
	f.bytes[2] = (size_t)f.triangles * 12;
	return f;
}

// ---- sdfr_mesh_survey and sdfr_mesh_fit (include/sdfr.h; the predicates and the fit's loop: sdfr_mesh_survey.h) ---------------------------
// The survey of one grid: the checks in the order their errors win -- null pointers, the grid (sdfr_mesh_extract's rule), the band --,
// then the lattice launch and the workspace's two pieces: the lattice, and the result with the words it is counted in.
struct MeshSurveyPlan
{
	int status; // QUERY_PLAN_*
	const char *error;
	MeshGrid g;
	LatticeArgs lattice; // but `rows` and `out`
	size_t points;
	size_t work[2];
};
inline MeshSurveyPlan plan_mesh_survey(const MeshGrid *grid, float band, const void *out)
{
	MeshSurveyPlan p = {};
	auto fail = [&p](const char *text) {
		p.status = QUERY_PLAN_INVALID_ARGUMENT;
		p.error = text;
		return p;
	};
	if (!grid || !out) return fail("null pointer");
	if (!mesh_grid_ok(*grid)) return fail("bad mesh grid");
	if (!(std::isfinite(band) && band >= 0.f)) return fail("band must be finite and >= 0");
	p.g = *grid;
	p.lattice = mesh_lattice_args(p.g);
	p.points = mesh_point_count(p.g);
	p.work[0] = p.points * 4;
	p.work[1] = MESH_SURVEY_WORK_BYTES;
	return p;
}

// The arguments of a fit, in the order their errors win: null pointers; the search grid -- origin, cell and iso finite, cell > 0, 1 .. 2^20
// cells per axis --; levels, 0 .. 10 with cell * 2^levels finite; margin, 0 .. 8.  -> null, or the text of the fault
inline const char *plan_mesh_fit(const MeshGrid *search, int levels, int margin, const void *out)
{
	if (!search || !out) return "null pointer";
	const MeshGrid &g = *search;
	bool ok = std::isfinite(g.cell) && g.cell > 0.f && std::isfinite(g.iso);
	for (int a = 0; a < 3; ++a) ok = ok && std::isfinite(g.origin[a]) && g.n[a] >= 1 && g.n[a] <= MESH_FIT_MAX_CELLS;
	if (!ok) return "bad search grid";
	if (levels < 0 || levels > MESH_FIT_MAX_LEVELS || !std::isfinite(g.cell * (float)(1 << levels))) return "levels must be 0..10 and cell * 2^levels finite";
	if (margin < 0 || margin > MESH_FIT_MAX_MARGIN) return "margin must be 0..8";
	return nullptr;
}

} // namespace sdfr

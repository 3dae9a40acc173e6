// sdfr_mesh_survey.h -- what a lattice of scene distances holds, and the grid that fits its surface: sdfr_mesh_survey and sdfr_mesh_fit
// (include/sdfr.h, where both definitions stand in full) as far as they are scene-independent.  Host-compilable, like
// sdfr_mesh.h, whose inside test, active cells and quad rule these are: k_mesh_survey (sdfr_mesh.hip) calls mesh_survey_point one lane per
// lattice point and reduces what it returns with integer atomics; tests/cpp/mesh_survey_host.cpp calls the same text point after point
// and adds it up with mesh_survey_add.  The coarse-to-fine loop of the fit, mesh_fit, is written once: sdfr_api.cpp hands it the survey
// on the GPU, the CPU stand-in its own.  Everything counted is an integer, so neither order nor machine changes a result.
#pragma once
#include <cmath>

#include "sdfr_mesh.h"

namespace sdfr {

// a grid sdfr_mesh_extract takes: every number finite, cell > 0, 1 .. 1024 cells per axis, at most 2^30 lattice points (host only)
inline bool mesh_grid_ok(const MeshGrid &g)
{
	bool ok = std::isfinite(g.cell) && g.cell > 0.f && std::isfinite(g.iso);
	for (int a = 0; a < 3; ++a) ok = ok && std::isfinite(g.origin[a]) && g.n[a] >= 1 && g.n[a] <= 1024;
	return ok && (int64_t)(g.n[0] + 1) * (g.n[1] + 1) * (g.n[2] + 1) <= (int64_t)1 << 30;
}

struct MeshSurvey // sdfr_mesh_survey_result, field for field
{
	int64_t active_cells, quads, near_cells, inside_points;
	int32_t active_lo[3], active_hi[3], near_lo[3], near_hi[3]; // inclusive cell indices; none: lo = n, hi = -1
	int64_t face_active[6];                                     // active cells with i == 0, i == nx - 1, j == 0, j == ny - 1, k == 0, k == nz - 1
};
enum
{
	MESH_SURVEY_COUNTS = 10, // the 64-bit words: the four counts, then the six faces
	MESH_SURVEY_BOUNDS = 12, // the 32-bit words: active lo, active hi, near lo, near hi
	MESH_SURVEY_WORD_STRIDE = 4096, // bytes between the words while the kernel adds into them: atomics on one line queue up (sdfr_mesh.hip)
	MESH_SURVEY_WORK_BYTES = 4096 * (1 + 10 + 12), // the packed result, then each word in a page of its own
};

// a survey of nothing: the words before the first point is added
SDF_HD MeshSurvey mesh_survey_empty(const MeshGrid &g)
{
	MeshSurvey s = {};
	for (int a = 0; a < 3; ++a)
	{
		s.active_lo[a] = s.near_lo[a] = g.n[a];
		s.active_hi[a] = s.near_hi[a] = -1;
	}
	return s;
}

// near: |s| <= band (NaN is never near)
SDF_HD bool mesh_near(const MeshGrid &g, float d, float band) { return fabsf(d - g.iso) <= band; }

// the faces of the grid cell (i, j, k) lies on: bit 2a its low face on axis a, bit 2a + 1 its high one
SDF_HD uint32_t mesh_cell_faces(const MeshGrid &g, int i, int j, int k)
{
	const int c[3] = {i, j, k};
	uint32_t faces = 0;
	for (int a = 0; a < 3; ++a) faces |= (c[a] == 0 ? 1u << (2 * a) : 0u) | (c[a] == g.n[a] - 1 ? 2u << (2 * a) : 0u);
	return faces;
}

// What lattice point (i, j, k) adds to a survey: its quads (0 .. 3), whether it is inside, and for the cell whose lowest corner it is
// (the points with i == nx, j == ny or k == nz have none) whether that cell is active, whether it is near -- active, or a corner with
// |s| <= band --, and the faces an active cell lies on
struct MeshSurveyPoint
{
	uint32_t quads, inside, active, near, faces;
};
SDF_HD MeshSurveyPoint mesh_survey_point(const MeshGrid &g, const float *D, float band, int i, int j, int k)
{
	MeshSurveyPoint c = {};
	c.quads = mesh_point_quads(g, D, i, j, k);
	c.inside = mesh_inside(g, D[mesh_point_index(g, i, j, k)]) ? 1u : 0u;
	if (i < g.n[0] && j < g.n[1] && k < g.n[2])
	{
		c.active = mesh_cell_active(g, D, i, j, k);
		bool near = c.active != 0u;
		for (int m = 0; m < 8; ++m) near = near || mesh_near(g, D[mesh_point_index(g, i + (m & 1), j + ((m >> 1) & 1), k + (m >> 2))], band);
		c.near = near ? 1u : 0u;
		c.faces = c.active ? mesh_cell_faces(g, i, j, k) : 0u;
	}
	return c;
}

// one point after the other (the CPU stand-in; the kernel reduces the same contributions per wave and per block instead)
inline void mesh_survey_add(MeshSurvey &s, const MeshSurveyPoint &c, int i, int j, int k)
{
	const int cell[3] = {i, j, k};
	s.quads += c.quads;
	s.inside_points += c.inside;
	s.active_cells += c.active;
	s.near_cells += c.near;
	for (int f = 0; f < 6; ++f) s.face_active[f] += (c.faces >> f) & 1u;
	for (int a = 0; a < 3; ++a)
	{
		if (c.active && cell[a] < s.active_lo[a]) s.active_lo[a] = cell[a];
		if (c.active && cell[a] > s.active_hi[a]) s.active_hi[a] = cell[a];
		if (c.near && cell[a] < s.near_lo[a]) s.near_lo[a] = cell[a];
		if (c.near && cell[a] > s.near_hi[a]) s.near_hi[a] = cell[a];
	}
}

// ---- sdfr_mesh_fit: shrink a search grid onto the surface, coarse to fine (host only) --------------------------------------------------
enum { MESH_FIT_EMPTY = 0, MESH_FIT_FOUND = 1, MESH_FIT_TOO_LARGE = 2 };
enum { MESH_FIT_MAX_CELLS = 1 << 20, MESH_FIT_MAX_LEVELS = 10, MESH_FIT_MAX_MARGIN = 8 };
struct MeshFit // sdfr_mesh_fit_result, field for field
{
	int32_t state;
	int32_t level, surveys;
	int32_t lo[3], hi[3]; // the window in cells of the search grid, hi exclusive
	MeshGrid grid;
	MeshSurvey last;
};

// the grid of level l over the window [lo, hi) of `search`: cells of 2^l search cells, as many as cover the window
inline MeshGrid mesh_fit_level_grid(const MeshGrid &search, const int32_t lo[3], const int32_t hi[3], int l)
{
	const int32_t step = 1 << l;
	MeshGrid g;
	for (int a = 0; a < 3; ++a)
	{
		const float offset = (float)lo[a] * search.cell; // one multiply, then one add
		g.origin[a] = search.origin[a] + offset;
		g.n[a] = (hi[a] - lo[a] + step - 1) / step;
	}
	g.cell = search.cell * (float)step;
	g.iso = search.iso;
	return g;
}

// The loop.  search, levels and margin have passed plan_mesh_fit (sdfr_mesh_plan.h).  survey(level grid, band, MeshSurvey &) -> 0, or a
// status that ends the fit and is returned as it is, with `f` then of no meaning.  A level grid that sdfr_mesh_extract would refuse
// (mesh_grid_ok) is TOO_LARGE before it is surveyed.
template <class Survey>
inline int mesh_fit(const MeshGrid &search, int levels, int margin, Survey &&survey, MeshFit &f)
{
	f = MeshFit();
	for (int a = 0; a < 3; ++a) f.hi[a] = search.n[a];
	for (int l = levels; l >= 0; --l)
	{
		const int32_t step = 1 << l;
		f.level = l;
		const MeshGrid g = mesh_fit_level_grid(search, f.lo, f.hi, l);
		if (!mesh_grid_ok(g))
		{
			f.state = MESH_FIT_TOO_LARGE;
			return 0;
		}
		const float band = l >= 1 ? 1.75f * g.cell : 0.f;
		const int rc = survey(g, band, f.last);
		if (rc != 0) return rc;
		f.surveys += 1;
		const bool coarse = l >= 1;
		const int32_t *b_lo = coarse ? f.last.near_lo : f.last.active_lo, *b_hi = coarse ? f.last.near_hi : f.last.active_hi;
		if ((coarse ? f.last.near_cells : f.last.active_cells) == 0)
		{
			f.state = MESH_FIT_EMPTY;
			return 0;
		}
		const int32_t guard = coarse ? 1 : margin;
		for (int a = 0; a < 3; ++a)
		{
			const int32_t lo = f.lo[a] + (b_lo[a] - guard) * step, hi = f.lo[a] + (b_hi[a] + 1 + guard) * step;
			f.lo[a] = lo > 0 ? lo : 0;
			f.hi[a] = hi < search.n[a] ? hi : search.n[a];
		}
	}
	f.state = MESH_FIT_FOUND;
	f.grid = mesh_fit_level_grid(search, f.lo, f.hi, 0);
	return 0;
}

} // namespace sdfr

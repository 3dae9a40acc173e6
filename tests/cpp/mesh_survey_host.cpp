// tests/cpp/mesh_survey_host.cpp -- TEST-ONLY: sdfr_mesh_survey and sdfr_mesh_fit without a GPU.  The predicates k_mesh_survey runs one lane
// per lattice point (sdf_playground_amd/csrc/sdfr_mesh_survey.h) run here point after point over a lattice of given distances, and the
// fit's loop -- the same template sdfr_api.cpp hands the GPU survey -- runs over a survey whose distances the caller supplies level by
// level; the two plans (sdfr_mesh_plan.h) answer as the entry points would.  tests/test_mesh_survey_cpu.py compares all of it with the
// definitions restated in numpy (tests/mesh_survey_util.py).  With -DMESH_SURVEY_MAIN: a stand-alone program for the sanitizers, which
// surveys one lattice and runs one fit over a sphere's distance.  The product never loads this.
#include "sdfr_mesh_plan.h"
#include "sdfr_mesh_survey.h"

#include <cstdio>
#include <vector>

using namespace sdfr;

static MeshSurvey survey(const MeshGrid &g, const float *D, float band)
{
	MeshSurvey s = mesh_survey_empty(g);
	for (int k = 0; k <= g.n[2]; ++k)
		for (int j = 0; j <= g.n[1]; ++j)
			for (int i = 0; i <= g.n[0]; ++i) mesh_survey_add(s, mesh_survey_point(g, D, band, i, j, k), i, j, k);
	return s;
}

extern "C" {

// the distances at the lattice points of a level grid, [points] in the order of the linear index; null: give up
typedef const float *(*msh_lattice_fn)(const MeshGrid *level);

int msh_sizes(int which) { return (int)(which == 0 ? sizeof(MeshGrid) : which == 1 ? sizeof(MeshSurvey) : sizeof(MeshFit)); }

// sdfr_mesh_survey after its scene: status and error text of the plan; with status 0 the survey of D
int msh_survey(const MeshGrid *grid, const float *D, float band, MeshSurvey *out, char error[64])
{
	const MeshSurveyPlan p = plan_mesh_survey(grid, band, out);
	snprintf(error, 64, "%s", p.error ? p.error : "");
	if (p.status != QUERY_PLAN_OK) return p.status;
	*out = survey(p.g, D, band);
	return 0;
}

// sdfr_mesh_fit likewise; the lattice of every level comes from `lattice`
int msh_fit(const MeshGrid *search, int levels, int margin, msh_lattice_fn lattice, MeshFit *out, char error[64])
{
	const char *text = plan_mesh_fit(search, levels, margin, out);
	snprintf(error, 64, "%s", text ? text : "");
	if (text) return QUERY_PLAN_INVALID_ARGUMENT;
	MeshFit f;
	const int rc = mesh_fit(*search, levels, margin, [&](const MeshGrid &level, float band, MeshSurvey &s) -> int {
		const float *D = lattice(&level);
		if (!D) return -9;
		s = survey(level, D, band);
		return 0;
	}, f);
	if (rc == 0) *out = f;
	return rc;
}

} // extern "C"

#ifdef MESH_SURVEY_MAIN
static std::vector<float> g_lattice;
static const float *sphere_lattice(const MeshGrid *g)
{
	g_lattice.resize(mesh_point_count(*g));
	for (int k = 0; k <= g->n[2]; ++k)
		for (int j = 0; j <= g->n[1]; ++j)
			for (int i = 0; i <= g->n[0]; ++i)
			{
				const float x = mesh_coord(*g, 0, i) - 3.3f, y = mesh_coord(*g, 1, j) - 1.1f, z = mesh_coord(*g, 2, k) - 0.7f;
				g_lattice[mesh_point_index(*g, i, j, k)] = sqrtf(x * x + y * y + z * z) - 0.8f;
			}
	return g_lattice.data();
}

static void print_survey(const MeshSurvey &s)
{
	printf("%lld %lld %lld %lld", (long long)s.active_cells, (long long)s.quads, (long long)s.near_cells, (long long)s.inside_points);
	for (const int32_t *b : {s.active_lo, s.active_hi, s.near_lo, s.near_hi}) printf(" %d %d %d", b[0], b[1], b[2]);
	for (int f = 0; f < 6; ++f) printf(" %lld", (long long)s.face_active[f]);
	printf("\n");
}

int main()
{
	char error[64];
	// one survey: a ragged grid that cuts the sphere
	const MeshGrid g = {{2.5f, 0.f, -0.25f}, 0.125f, {13, 9, 11}, 0.f};
	MeshSurvey s;
	if (msh_survey(&g, sphere_lattice(&g), 0.25f, &s, error) != 0) return 2;
	print_survey(s);
	// one fit: the sphere in a search of 200 x 96 x 80 cells, three coarse levels
	const MeshGrid search = {{-4.f, -2.f, -3.f}, 0.0625f, {200, 96, 80}, 0.f};
	MeshFit f;
	if (msh_fit(&search, 3, 1, sphere_lattice, &f, error) != 0) return 3;
	printf("%d %d %d  %d %d %d  %d %d %d  %d %d %d\n", f.state, f.level, f.surveys, f.lo[0], f.lo[1], f.lo[2], f.hi[0], f.hi[1], f.hi[2], f.grid.n[0], f.grid.n[1],
		f.grid.n[2]);
	print_survey(f.last);
	return f.state == MESH_FIT_FOUND && f.surveys == 4 && f.last.active_cells > 0 ? 0 : 4;
}
#endif

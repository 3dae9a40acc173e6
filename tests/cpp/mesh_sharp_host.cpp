// tests/cpp/mesh_sharp_host.cpp -- TEST-ONLY: sdfr_mesh_extract_sharp's stage functions (sdf_playground_amd/csrc/sdfr_mesh_sharp.h, over
// sdfr_mesh.h) compiled for the CPU and run sequentially over a lattice of given distances, with the scene bound to a callback, so that
// the CPU test tier can compare them with the definition restated in numpy (tests/mesh_sharp_util.py) bit for bit without a GPU.  Also
// the analytic scenes of those tests, so that the callback, the restatement and the stand-alone program all ask one function.  Built as
// a library, and with -DMESH_SHARP_MAIN as a program of its own that runs every analytic case and writes the meshes to stdout: that
// one is what the sanitizers look at.  Built with -ffp-contract=off, as the library.  The product never loads this.
#include "sdfr_mesh_sharp.h"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace sdfr;

// distance at p and, if wanted, the normal there: out = {d, nx, ny, nz}
typedef void (*msh_callback)(const float *p, int want_normal, float *out);

namespace {

struct CallbackScene
{
	msh_callback f;
	float distance(vec3 p) const
	{
		const float q[3] = {p.x, p.y, p.z};
		float out[4] = {0.f, 0.f, 0.f, 0.f};
		f(q, 0, out);
		return out[0];
	}
	float distance_normal(vec3 p, vec3 &n) const
	{
		const float q[3] = {p.x, p.y, p.z};
		float out[4] = {0.f, 0.f, 0.f, 0.f};
		f(q, 1, out);
		n = V3(out[1], out[2], out[3]);
		return out[0];
	}
};

// ---- the analytic scenes: exact distances and normals in double, rounded once.  Centred off the lattice.
const double k_centre[3] = {0.03, 0.05, 0.07};
const double k_half[3] = {0.6, 0.45, 0.5};

void box(const double q[3], double &d, double n[3])
{
	double a[3], out2 = 0.0;
	int widest = 0;
	for (int k = 0; k < 3; ++k)
	{
		a[k] = std::fabs(q[k]) - k_half[k];
		if (a[k] > a[widest]) widest = k;
		if (a[k] > 0.0) out2 += a[k] * a[k];
	}
	n[0] = n[1] = n[2] = 0.0;
	if (out2 > 0.0)
	{
		d = std::sqrt(out2);
		for (int k = 0; k < 3; ++k) n[k] = a[k] > 0.0 ? (q[k] < 0.0 ? -a[k] : a[k]) / d : 0.0;
	}
	else
	{
		d = a[widest];
		n[widest] = q[widest] < 0.0 ? -1.0 : 1.0;
	}
}

void analytic(int scene, const float *p, float *d_out, float *n_out)
{
	double q[3] = {(double)p[0] - k_centre[0], (double)p[1] - k_centre[1], (double)p[2] - k_centre[2]}, d = 0.0, n[3] = {0.0, 0.0, 0.0};
	switch (scene)
	{
	case 0: // the axis-aligned box
		box(q, d, n);
		break;
	case 1: // the box rotated by 0.5 rad about y, then by 0.3 rad about x
	{
		const double cy = std::cos(0.5), sy = std::sin(0.5), cx = std::cos(0.3), sx = std::sin(0.3);
		// world -> box: undo x, then undo y
		const double u[3] = {q[0], cx * q[1] + sx * q[2], -sx * q[1] + cx * q[2]};
		const double w[3] = {cy * u[0] - sy * u[2], u[1], sy * u[0] + cy * u[2]};
		double m[3];
		box(w, d, m);
		const double v[3] = {cy * m[0] + sy * m[2], m[1], -sy * m[0] + cy * m[2]};
		n[0] = v[0];
		n[1] = cx * v[1] - sx * v[2];
		n[2] = sx * v[1] + cx * v[2];
		break;
	}
	case 2: // the sphere of radius 0.7
	{
		const double l = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
		d = l - 0.7;
		for (int k = 0; k < 3; ++k) n[k] = l > 0.0 ? q[k] / l : 0.0;
		break;
	}
	case 3: // the torus 0.6 / 0.25 about y
	{
		const double ring = std::sqrt(q[0] * q[0] + q[2] * q[2]);
		const double a = ring - 0.6, l = std::sqrt(a * a + q[1] * q[1]);
		d = l - 0.25;
		if (ring > 0.0 && l > 0.0)
		{
			n[0] = a / l * q[0] / ring;
			n[1] = q[1] / l;
			n[2] = a / l * q[2] / ring;
		}
		break;
	}
	default: // the cliff: two nearly parallel planes that do not meet where they change over -- a floor, and right of x = 0 a floor
	         // 0.04 higher and tilted by 0.2 rad: their planes meet far outside the cells that see both, which therefore need the clamp
	{
		if (q[0] < 0.0)
		{
			d = q[1];
			n[1] = 1.0;
		}
		else
		{
			n[0] = -std::sin(0.2);
			n[1] = std::cos(0.2);
			d = n[0] * q[0] + n[1] * (q[1] - 0.04);
		}
		break;
	}
	}
	*d_out = (float)d;
	if (n_out)
		for (int k = 0; k < 3; ++k) n_out[k] = (float)n[k];
}

} // namespace

extern "C" {

// D: the distances at the lattice points, [points].  counts[2]: vertices, triangles (always written); positions [vertices][3] and
// indices [triangles][3] only if both capacities suffice, as sdfr_mesh_extract_sharp.
int msh_extract(const MeshGrid *grid, const float *D, msh_callback f, int64_t vertex_capacity, int64_t triangle_capacity, float *positions, uint32_t *indices,
	int64_t counts[2])
{
	const MeshGrid g = *grid;
	const uint32_t points = mesh_point_count(g), cells = mesh_cell_count(g);
	std::vector<uint32_t> cell_vertex(cells + 1u, 0u), point_quad(points + 1u, 0u);
	for (int k = 0; k <= g.n[2]; ++k)
		for (int j = 0; j <= g.n[1]; ++j)
			for (int i = 0; i <= g.n[0]; ++i)
			{
				point_quad[mesh_point_index(g, i, j, k)] = mesh_point_quads(g, D, i, j, k);
				if (i < g.n[0] && j < g.n[1] && k < g.n[2]) cell_vertex[mesh_cell_index(g, i, j, k)] = mesh_cell_active(g, D, i, j, k);
			}
	for (std::vector<uint32_t> *a : {&cell_vertex, &point_quad})
	{
		uint32_t run = 0;
		for (uint32_t &v : *a)
		{
			const uint32_t x = v;
			v = run;
			run += x;
		}
	}
	counts[0] = cell_vertex[cells];
	counts[1] = 2 * (int64_t)point_quad[points];
	if (counts[0] > vertex_capacity || counts[1] > triangle_capacity) return 0;
	const CallbackScene scene = {f};
	for (int k = 0; k < g.n[2]; ++k)
		for (int j = 0; j < g.n[1]; ++j)
			for (int i = 0; i < g.n[0]; ++i)
			{
				const uint32_t c = mesh_cell_index(g, i, j, k);
				if (cell_vertex[c + 1u] == cell_vertex[c]) continue;
				MeshSharpCrossing x[12];
				for (int e = 0; e < 12; ++e) mesh_sharp_crossing(g, D, scene, i, j, k, e, x[e]);
				mesh_sharp_vertex(g, i, j, k, [&x](int e) { return x[e]; }, positions + (size_t)3 * cell_vertex[c]);
			}
	for (int k = 0; k <= g.n[2]; ++k)
		for (int j = 0; j <= g.n[1]; ++j)
			for (int i = 0; i <= g.n[0]; ++i)
			{
				const uint32_t p = mesh_point_index(g, i, j, k);
				if (point_quad[p + 1u] != point_quad[p]) mesh_point_emit(g, D, cell_vertex.data(), i, j, k, point_quad[p], indices);
			}
	return 0;
}
int msh_grid_size() { return (int)sizeof(MeshGrid); }

// the analytic scenes at n points: d [n] and, unless null, normals [n][3]
void msh_analytic(int scene, int64_t n, const float *points, float *d, float *normals)
{
	for (int64_t i = 0; i < n; ++i) analytic(scene, points + 3 * i, d + i, normals ? normals + 3 * i : nullptr);
}

} // extern "C"

#ifdef MESH_SHARP_MAIN
// Every analytic scene on the tests' grid (tests/mesh_sharp_util.py: GRID): counts, positions and indices to stdout as raw words
namespace {
int g_scene = 0;
void scene_callback(const float *p, int want_normal, float *out) { analytic(g_scene, p, out, want_normal ? out + 1 : nullptr); }
} // namespace

int main()
{
	MeshGrid g = {{-0.75f, -0.6f, -0.65f}, 0.125f, {12, 10, 11}, 0.f};
	for (g_scene = 0; g_scene < 5; ++g_scene)
	{
		std::vector<float> points, D;
		for (int k = 0; k <= g.n[2]; ++k)
			for (int j = 0; j <= g.n[1]; ++j)
				for (int i = 0; i <= g.n[0]; ++i)
				{
					points.push_back(mesh_coord(g, 0, i));
					points.push_back(mesh_coord(g, 1, j));
					points.push_back(mesh_coord(g, 2, k));
				}
		D.resize(points.size() / 3);
		msh_analytic(g_scene, (int64_t)D.size(), points.data(), D.data(), nullptr);
		int64_t counts[2] = {0, 0};
		msh_extract(&g, D.data(), scene_callback, 0, 0, nullptr, nullptr, counts);
		std::vector<float> positions((size_t)counts[0] * 3);
		std::vector<uint32_t> indices((size_t)counts[1] * 3);
		msh_extract(&g, D.data(), scene_callback, counts[0], counts[1], positions.data(), indices.data(), counts);
		fwrite(counts, sizeof counts[0], 2, stdout);
		fwrite(positions.data(), 4, positions.size(), stdout);
		fwrite(indices.data(), 4, indices.size(), stdout);
	}
	return 0;
}
#endif

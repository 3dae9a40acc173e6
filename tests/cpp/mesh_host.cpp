// tests/cpp/mesh_host.cpp -- TEST-ONLY: the stage functions of sdfr_mesh_extract (sdf_playground_amd/csrc/sdfr_mesh.h) compiled for
// the CPU and run sequentially over a lattice of given distances, the way sdfr_mesh.hip runs them one lane per cell / point between
// prefix sums, so that the CPU test tier can compare them with the definition restated in numpy (tests/mesh_util.py) bit for bit
// without a GPU.  Built with -ffp-contract=off, as the library.  The product never loads this.
#include "sdfr_mesh.h"

#include <vector>

using namespace sdfr;

extern "C" {

// D: the distances at the lattice points, [points].  counts[2]: vertices, triangles (always written); positions [vertices][3] and
// indices [triangles][3] only if both capacities suffice, as sdfr_mesh_extract.
int mh_extract(const MeshGrid *grid, const float *D, int64_t vertex_capacity, int64_t triangle_capacity, float *positions, uint32_t *indices,
	int64_t counts[2])
{
	const MeshGrid g = *grid;
	const uint32_t points = mesh_point_count(g), cells = mesh_cell_count(g);
	std::vector<uint32_t> cell_vertex(cells + 1u, 0u), point_quad(points + 1u, 0u);
	// classify
	for (int k = 0; k <= g.n[2]; ++k)
		for (int j = 0; j <= g.n[1]; ++j)
			for (int i = 0; i <= g.n[0]; ++i)
			{
				point_quad[mesh_point_index(g, i, j, k)] = mesh_point_quads(g, D, i, j, k);
				if (i < g.n[0] && j < g.n[1] && k < g.n[2]) cell_vertex[mesh_cell_index(g, i, j, k)] = mesh_cell_active(g, D, i, j, k);
			}
	// exclusive prefix sums, in place; the element after the last is the total
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
	// emit
	for (int k = 0; k < g.n[2]; ++k)
		for (int j = 0; j < g.n[1]; ++j)
			for (int i = 0; i < g.n[0]; ++i)
			{
				const uint32_t c = mesh_cell_index(g, i, j, k);
				if (cell_vertex[c + 1u] != cell_vertex[c]) mesh_cell_vertex(g, D, i, j, k, positions + (size_t)3 * cell_vertex[c]);
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
int mh_grid_size() { return (int)sizeof(MeshGrid); }

} // extern "C"

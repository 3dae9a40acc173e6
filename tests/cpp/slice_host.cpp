// tests/cpp/slice_host.cpp -- TEST-ONLY: the stage functions of sdfr_slice_extract (sdf_playground_amd/csrc/sdfr_slice.h) compiled for
// the CPU and run sequentially over a stack of lattices of given distances, the way sdfr_slice.hip runs them one lane per lattice point
// between prefix sums, so that the CPU test tier can compare them with the definition restated in numpy (tests/slice_util.py) word for
// word without a GPU.  Built with -ffp-contract=off, as the library.  The product never loads this.
#include "sdfr_slice.h"

#include <vector>

using namespace sdfr;

extern "C" {

// D: the distances at the lattice points, [points].  counts[2]: vertices, segments, and layer_vertices, layer_segments [layers + 1]
// (always written); positions [vertices][3], coords [vertices][2] (or null) and segments [segments][2] only if both capacities suffice,
// as sdfr_slice_extract.
int sh_extract(const SliceGrid *grid, const float *D, int64_t vertex_capacity, int64_t segment_capacity, float *positions, float *coords, uint32_t *segments,
	int64_t *layer_vertices, int64_t *layer_segments, int64_t counts[2])
{
	const SliceGrid g = *grid;
	const uint32_t points = slice_point_count(g);
	std::vector<uint32_t> point_vertex(points + 1u, 0u), cell_segment(points + 1u, 0u);
	// classify
	for (uint32_t p = 0; p < points; ++p)
	{
		int i, j, l;
		slice_point_coords(g, p, i, j, l);
		point_vertex[p] = slice_point_vertices(g, D, i, j, l);
		cell_segment[p] = slice_cell_segments(g, D, i, j, l);
	}
	// exclusive prefix sums, in place; the element after the last is the total
	for (std::vector<uint32_t> *a : {&point_vertex, &cell_segment})
	{
		uint32_t run = 0;
		for (uint32_t &v : *a)
		{
			const uint32_t x = v;
			v = run;
			run += x;
		}
	}
	// the layers' offsets
	for (int l = 0; l <= g.layers; ++l)
	{
		layer_vertices[l] = point_vertex[(uint32_t)l * slice_layer_points(g)];
		layer_segments[l] = cell_segment[(uint32_t)l * slice_layer_points(g)];
	}
	counts[0] = point_vertex[points];
	counts[1] = cell_segment[points];
	if (counts[0] > vertex_capacity || counts[1] > segment_capacity) return 0;
	// emit
	for (uint32_t p = 0; p < points; ++p)
	{
		int i, j, l;
		slice_point_coords(g, p, i, j, l);
		if (point_vertex[p + 1u] != point_vertex[p]) slice_point_emit(g, D, i, j, l, point_vertex[p], positions, coords);
		if (cell_segment[p + 1u] != cell_segment[p]) slice_cell_emit(g, D, point_vertex.data(), i, j, l, cell_segment[p], segments);
	}
	return 0;
}
// the lattice points themselves, [points][3]
void sh_points(const SliceGrid *grid, float *out)
{
	const SliceGrid g = *grid;
	for (uint32_t p = 0; p < slice_point_count(g); ++p)
	{
		int i, j, l;
		slice_point_coords(g, p, i, j, l);
		for (int c = 0; c < 3; ++c) out[(size_t)3 * p + c] = slice_coord(g, c, i, j, l);
	}
}
int sh_grid_size() { return (int)sizeof(SliceGrid); }

} // extern "C"

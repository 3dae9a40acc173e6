// sdfr_slice.hip -- the scene-independent kernels of sdfr_slice_extract (stage functions: sdfr_slice.h): classify the lattice points,
// exclusive prefix sums of the two count arrays (the mesh's launches: launch_mesh_scan, sdfr_mesh.hip), gather the layers' offsets, emit
// vertices, emit segments.  The distances they read come from the scene's slice kernel (sdfr_query_kernel.h: query_slices_kernel).
//
// One lane per lattice point throughout, in blocks of SDFR_MESH_BLOCK.  Neighbouring lanes are neighbouring points of a row: the
// lattice and the scanned counts are read as consecutive words, and the few lanes that emit write where the scan put them.  No kernel
// uses LDS, an atomic or another workgroup's result: the phases are separate launches of one stream, and the order of both outputs
// (by the point's linear index) is the scan's.
#include "sdfr_kernels.h"
#include "sdfr_mesh.h"
#include "sdfr_slice.h"

namespace sdfr {

// one lane per lattice point: the vertex count of its two edges, and the segment count of the cell whose corner c0 it is; the element
// after the last of each array is the 0 whose prefix sum is the total
__global__ __launch_bounds__(SDFR_MESH_BLOCK) void k_slice_classify(SliceGrid g, const float *__restrict__ lattice, uint32_t *__restrict__ point_vertex,
	uint32_t *__restrict__ cell_segment)
{
	const uint32_t p = blockIdx.x * (uint32_t)SDFR_MESH_BLOCK + threadIdx.x;
	const uint32_t points = slice_point_count(g);
	if (p > points) return;
	if (p == points)
	{
		point_vertex[points] = 0u;
		cell_segment[points] = 0u;
		return;
	}
	int i, j, l;
	slice_point_coords(g, p, i, j, l);
	point_vertex[p] = slice_point_vertices(g, lattice, i, j, l);
	cell_segment[p] = slice_cell_segments(g, lattice, i, j, l);
}

// the layers' offsets out of the scanned counts: word t <= layers is the first vertex of layer t (t = layers: the total), word
// layers + 1 + t the first segment -- the scanned count at the layer's first point, and the totals at the element after the last
__global__ __launch_bounds__(SDFR_MESH_BLOCK) void k_slice_layer_offsets(SliceGrid g, const uint32_t *__restrict__ point_vertex,
	const uint32_t *__restrict__ cell_segment, uint32_t *__restrict__ out)
{
	const uint32_t t = blockIdx.x * (uint32_t)SDFR_MESH_BLOCK + threadIdx.x;
	const uint32_t per = (uint32_t)g.layers + 1u;
	if (t >= 2u * per) return;
	const uint32_t layer = t < per ? t : t - per; // <= layers: the index below is <= the point count
	out[t] = (t < per ? point_vertex : cell_segment)[layer * slice_layer_points(g)];
}

// one lane per lattice point: a point with vertices (its scanned index differs from the next point's) writes them
__global__ __launch_bounds__(SDFR_MESH_BLOCK) void k_slice_emit_vertices(SliceGrid g, const float *__restrict__ lattice, const uint32_t *__restrict__ point_vertex,
	float *__restrict__ positions, float *__restrict__ coords)
{
	const uint32_t p = blockIdx.x * (uint32_t)SDFR_MESH_BLOCK + threadIdx.x;
	if (p >= slice_point_count(g)) return;
	const uint32_t v = point_vertex[p];
	if (point_vertex[p + 1u] == v) return;
	int i, j, l;
	slice_point_coords(g, p, i, j, l);
	slice_point_emit(g, lattice, i, j, l, v, positions, coords);
}

// one lane per lattice point: a point whose cell has segments writes them
__global__ __launch_bounds__(SDFR_MESH_BLOCK) void k_slice_emit_segments(SliceGrid g, const float *__restrict__ lattice, const uint32_t *__restrict__ point_vertex,
	const uint32_t *__restrict__ cell_segment, uint32_t *__restrict__ segments)
{
	const uint32_t p = blockIdx.x * (uint32_t)SDFR_MESH_BLOCK + threadIdx.x;
	if (p >= slice_point_count(g)) return;
	const uint32_t q = cell_segment[p];
	if (cell_segment[p + 1u] == q) return;
	int i, j, l;
	slice_point_coords(g, p, i, j, l);
	slice_cell_emit(g, lattice, point_vertex, i, j, l, q, segments);
}

hipError_t launch_slice_count(const SliceGrid &g, const float *lattice, uint32_t *point_vertex, uint32_t *cell_segment, uint32_t *sums, uint32_t *layer_offsets,
	hipStream_t stream)
{
	const uint32_t points = slice_point_count(g), words = 2u * ((uint32_t)g.layers + 1u);
	hipLaunchKernelGGL(k_slice_classify, dim3(points / SDFR_MESH_BLOCK + 1u), dim3(SDFR_MESH_BLOCK), 0, stream, g, lattice, point_vertex, cell_segment);
	launch_mesh_scan(point_vertex, points + 1u, sums, stream);
	launch_mesh_scan(cell_segment, points + 1u, sums + mesh_scan_sum_words((size_t)points + 1), stream);
	hipLaunchKernelGGL(k_slice_layer_offsets, dim3((words + SDFR_MESH_BLOCK - 1u) / SDFR_MESH_BLOCK), dim3(SDFR_MESH_BLOCK), 0, stream, g,
		(const uint32_t *)point_vertex, (const uint32_t *)cell_segment, layer_offsets);
	return hipGetLastError();
}

hipError_t launch_slice_emit(const SliceGrid &g, const float *lattice, const uint32_t *point_vertex, const uint32_t *cell_segment, float *positions, float *coords,
	uint32_t *segments, hipStream_t stream)
{
	const uint32_t blocks = (slice_point_count(g) + SDFR_MESH_BLOCK - 1u) / SDFR_MESH_BLOCK;
	hipLaunchKernelGGL(k_slice_emit_vertices, dim3(blocks), dim3(SDFR_MESH_BLOCK), 0, stream, g, lattice, point_vertex, positions, coords);
	if (segments)
		hipLaunchKernelGGL(k_slice_emit_segments, dim3(blocks), dim3(SDFR_MESH_BLOCK), 0, stream, g, lattice, point_vertex, cell_segment, segments);
	return hipGetLastError();
}

} // namespace sdfr

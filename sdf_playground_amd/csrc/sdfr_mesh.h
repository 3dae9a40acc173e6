// sdfr_mesh.h -- surface nets over a lattice of scene distances: the stages of sdfr_mesh_extract (include/sdfr.h, where the
// definition stands in full) as functions of one cell or one lattice point, scene-independent and host-compilable.
// sdfr_mesh.hip runs them one lane per cell / point between exclusive prefix sums; tests/cpp/mesh_host.cpp runs the same text
// sequentially on the CPU.  All arithmetic is fp32 in source order (-ffp-contract=off), so both give the same bits.
//
// The lattice has (nx + 1)(ny + 1)(nz + 1) <= 2^30 points, point (i, j, k) at index i + (nx + 1) * (j + (ny + 1) * k); cell (i, j, k)
// is at index i + nx * (j + ny * k).  Those indices fit 32 bits; an offset into a [.][3] array does not (3 * 2^30), nor does an
// offset into the index array (six words per quad): both are size_t.
#pragma once
#include "sdfr_math.h"

namespace sdfr {

struct MeshGrid // sdfr_mesh_grid
{
	float origin[3];
	float cell;
	int32_t n[3]; // cells per axis
	float iso;
};

SDF_HD uint32_t mesh_point_index(const MeshGrid &g, int i, int j, int k)
{
	return (uint32_t)i + (uint32_t)(g.n[0] + 1) * ((uint32_t)j + (uint32_t)(g.n[1] + 1) * (uint32_t)k);
}
SDF_HD uint32_t mesh_cell_index(const MeshGrid &g, int i, int j, int k)
{
	return (uint32_t)i + (uint32_t)g.n[0] * ((uint32_t)j + (uint32_t)g.n[1] * (uint32_t)k);
}
SDF_HD uint32_t mesh_point_count(const MeshGrid &g) { return (uint32_t)(g.n[0] + 1) * (uint32_t)(g.n[1] + 1) * (uint32_t)(g.n[2] + 1); }
SDF_HD uint32_t mesh_cell_count(const MeshGrid &g) { return (uint32_t)g.n[0] * (uint32_t)g.n[1] * (uint32_t)g.n[2]; }

#define SDFR_MESH_BLOCK 256 // threads of every kernel of sdfr_mesh.hip = elements a block of its prefix sums owns
// words of scratch the exclusive prefix sum of n elements needs: the totals of its blocks, of their blocks ... while they are more than
// one block (host only; the declaration: sdfr_kernels.h)
inline size_t mesh_scan_sum_words(size_t n)
{
	size_t words = 0;
	while (n > SDFR_MESH_BLOCK)
	{
		n = (n + SDFR_MESH_BLOCK - 1) / SDFR_MESH_BLOCK;
		words += n;
	}
	return words;
}

// coordinate `axis` of the lattice points with index `i` on that axis: one multiply, then one add
SDF_HD float mesh_coord(const MeshGrid &g, int axis, int i) { return g.origin[axis] + (float)i * g.cell; }

// inside: s = D - iso < 0 (NaN is outside)
SDF_HD bool mesh_inside(const MeshGrid &g, float d) { return d - g.iso < 0.f; }

// 1: cell (i, j, k) is active -- at least one corner inside and at least one not -- and gets a vertex
SDF_HD uint32_t mesh_cell_active(const MeshGrid &g, const float *D, int i, int j, int k)
{
	int inside = 0;
	for (int c = 0; c < 8; ++c) inside += mesh_inside(g, D[mesh_point_index(g, i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2))]) ? 1 : 0;
	return inside != 0 && inside != 8 ? 1u : 0u;
}

// Does the lattice edge from P = (i, j, k) along `axis` emit a quad: it has exactly one endpoint inside, and P's coordinates on the
// two other axes are >= 1 and <= n - 1, so that the four cells around the edge exist
SDF_HD bool mesh_edge_quad(const MeshGrid &g, const float *D, const int P[3], int axis)
{
	const int b = (axis + 1) % 3, c = (axis + 2) % 3;
	if (P[axis] >= g.n[axis] || P[b] < 1 || P[b] > g.n[b] - 1 || P[c] < 1 || P[c] > g.n[c] - 1) return false;
	int Q[3] = {P[0], P[1], P[2]};
	Q[axis] += 1;
	return mesh_inside(g, D[mesh_point_index(g, P[0], P[1], P[2])]) != mesh_inside(g, D[mesh_point_index(g, Q[0], Q[1], Q[2])]);
}

// quads of lattice point (i, j, k): 0 .. 3, one per axis
SDF_HD uint32_t mesh_point_quads(const MeshGrid &g, const float *D, int i, int j, int k)
{
	const int P[3] = {i, j, k};
	uint32_t n = 0;
	for (int axis = 0; axis < 3; ++axis) n += mesh_edge_quad(g, D, P, axis) ? 1u : 0u;
	return n;
}

// The vertex of active cell (i, j, k): the mean of the crossings of its 12 edges, visited x edges first -- (dj, dk) = (0,0), (1,0),
// (0,1), (1,1) --, then y edges -- (di, dk) --, then z edges -- (di, dj).  An edge from lower endpoint a to upper endpoint b with
// exactly one of them inside crosses at t = s_a / (s_a - s_b): a's position with the edge axis' coordinate p_a + t * (p_b - p_a).
SDF_HD void mesh_cell_vertex(const MeshGrid &g, const float *D, int i, int j, int k, float out[3])
{
	float sum[3] = {0.f, 0.f, 0.f};
	int crossings = 0;
	const int cell[3] = {i, j, k};
	for (int axis = 0; axis < 3; ++axis)
	{
		const int b = axis == 0 ? 1 : 0, c = axis == 2 ? 1 : 2; // the two other axes, lower one first
		for (int e = 0; e < 4; ++e)
		{
			int A[3] = {cell[0], cell[1], cell[2]};
			A[b] += e & 1;
			A[c] += e >> 1;
			int B[3] = {A[0], A[1], A[2]};
			B[axis] += 1;
			const float sa = D[mesh_point_index(g, A[0], A[1], A[2])] - g.iso, sb = D[mesh_point_index(g, B[0], B[1], B[2])] - g.iso;
			if ((sa < 0.f) == (sb < 0.f)) continue;
			const float t = sa / (sa - sb);
			float p[3] = {mesh_coord(g, 0, A[0]), mesh_coord(g, 1, A[1]), mesh_coord(g, 2, A[2])};
			const float pb = mesh_coord(g, axis, B[axis]);
			p[axis] = p[axis] + t * (pb - p[axis]);
			sum[0] = sum[0] + p[0];
			sum[1] = sum[1] + p[1];
			sum[2] = sum[2] + p[2];
			++crossings;
		}
	}
	const float n = (float)crossings;
	out[0] = sum[0] / n;
	out[1] = sum[1] / n;
	out[2] = sum[2] / n;
}

// The quads of lattice point (i, j, k), axis x, y, z, as two triangles each from word `first_quad * 6` of `indices` on.  With
// (a, b, c) the cyclic axis order and C(ob, oc) the cell at P offset by ob, oc on axes b and c, the quad is the vertices of
// C(-1,-1), C(0,-1), C(0,0), C(-1,0) -- counter-clockwise seen from outside when P is inside, normal towards +a -- and the same
// four backwards when P is outside; (q0, q1, q2, q3) becomes (q0, q1, q2), (q0, q2, q3).  cell_vertex: the vertex index per cell.
SDF_HD void mesh_point_emit(const MeshGrid &g, const float *D, const uint32_t *cell_vertex, int i, int j, int k, uint32_t first_quad, uint32_t *indices)
{
	const int P[3] = {i, j, k};
	const bool p_inside = mesh_inside(g, D[mesh_point_index(g, i, j, k)]);
	size_t q = first_quad;
	for (int axis = 0; axis < 3; ++axis)
	{
		if (!mesh_edge_quad(g, D, P, axis)) continue;
		const int b = (axis + 1) % 3, c = (axis + 2) % 3;
		uint32_t v[4];
		for (int m = 0; m < 4; ++m)
		{
			int C[3] = {P[0], P[1], P[2]};
			C[b] += (m == 1 || m == 2) ? 0 : -1; // ob: -1, 0, 0, -1
			C[c] += m >= 2 ? 0 : -1;             // oc: -1, -1, 0, 0
			v[m] = cell_vertex[mesh_cell_index(g, C[0], C[1], C[2])];
		}
		if (!p_inside)
		{
			uint32_t t = v[0];
			v[0] = v[3];
			v[3] = t;
			t = v[1];
			v[1] = v[2];
			v[2] = t;
		}
		uint32_t *o = indices + q * 6;
		o[0] = v[0];
		o[1] = v[1];
		o[2] = v[2];
		o[3] = v[0];
		o[4] = v[2];
		o[5] = v[3];
		++q;
	}
}

} // namespace sdfr

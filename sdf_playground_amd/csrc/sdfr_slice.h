// sdfr_slice.h -- marching squares over a stack of plane lattices of scene distances: the stages of sdfr_slice_extract (include/sdfr.h,
// where the definition stands in full) as functions of one lattice point or one cell, scene-independent and
// host-compilable like sdfr_mesh.h.  sdfr_slice.hip runs them one lane per lattice point between exclusive prefix sums;
// tests/cpp/slice_host.cpp runs the same text sequentially on the CPU.  All arithmetic is fp32 in source order (-ffp-contract=off), so
// both give the same bits.
//
// The stack has (nu + 1)(nv + 1) * layers <= 2^30 points, point (i, j) of layer l at index i + (nu + 1) * (j + (nv + 1) * l).  Both
// count arrays are indexed by POINT: a point's vertices are those of its u-edge and its v-edge, its segments those of the cell whose
// corner c0 it is (none for a point of the last column or row) -- the order of the cells' linear index i + nu * (j + nv * l) is the
// order of their c0's point index, so one point index orders both outputs.  Those indices and both totals (at most two per point) fit
// 32 bits; an offset into a [.][3] array does not: size_t.
#pragma once
#include "sdfr_math.h"

namespace sdfr {

struct SliceGrid // sdfr_slice_grid
{
	float origin[3];
	float du[3], dv[3], dw[3];
	int32_t nu, nv, layers;
	float iso;
};

SDF_HD uint32_t slice_layer_points(const SliceGrid &g) { return (uint32_t)(g.nu + 1) * (uint32_t)(g.nv + 1); }
SDF_HD uint32_t slice_point_count(const SliceGrid &g) { return slice_layer_points(g) * (uint32_t)g.layers; }
SDF_HD uint32_t slice_point_index(const SliceGrid &g, int i, int j, int l)
{
	return (uint32_t)i + (uint32_t)(g.nu + 1) * ((uint32_t)j + (uint32_t)(g.nv + 1) * (uint32_t)l);
}
// lattice point p -> (i, j, l); p < 2^30
SDF_HD void slice_point_coords(const SliceGrid &g, uint32_t p, int &i, int &j, int &l)
{
	const uint32_t pu = (uint32_t)(g.nu + 1), pv = (uint32_t)(g.nv + 1);
	const uint32_t row = p / pu;
	i = (int)(p - row * pu);
	l = (int)(row / pv);
	j = (int)(row - (uint32_t)l * pv);
}

// component c of lattice point (i, j) of layer l: three multiplies and three adds, in this order
SDF_HD float slice_coord(const float origin[3], const float du[3], const float dv[3], const float dw[3], int c, int i, int j, int l)
{
	return ((origin[c] + (float)i * du[c]) + (float)j * dv[c]) + (float)l * dw[c];
}
SDF_HD float slice_coord(const SliceGrid &g, int c, int i, int j, int l) { return slice_coord(g.origin, g.du, g.dv, g.dw, c, i, j, l); }

// inside: s = D - iso < 0 (NaN is outside)
SDF_HD bool slice_inside(const SliceGrid &g, float d) { return d - g.iso < 0.f; }

// Does the edge of point (i, j) along u (axis 0, to (i + 1, j)) or v (axis 1, to (i, j + 1)) exist and have exactly one endpoint inside
SDF_HD bool slice_edge_vertex(const SliceGrid &g, const float *D, int i, int j, int l, int axis)
{
	if (axis == 0 ? i >= g.nu : j >= g.nv) return false;
	const float a = D[slice_point_index(g, i, j, l)], b = D[slice_point_index(g, i + (axis == 0 ? 1 : 0), j + (axis == 0 ? 0 : 1), l)];
	return slice_inside(g, a) != slice_inside(g, b);
}
// vertices of lattice point (i, j) of layer l: 0 .. 2
SDF_HD uint32_t slice_point_vertices(const SliceGrid &g, const float *D, int i, int j, int l)
{
	return (slice_edge_vertex(g, D, i, j, l, 0) ? 1u : 0u) + (slice_edge_vertex(g, D, i, j, l, 1) ? 1u : 0u);
}

// The corners of cell (i, j) of layer l, counter-clockwise in (u, v): c0 = (i, j), c1 = (i + 1, j), c2 = (i + 1, j + 1), c3 = (i, j + 1);
// s[k] = D(c_k) - iso.  -> the mask of the corners inside, bit k for c_k
SDF_HD uint32_t slice_cell_corners(const SliceGrid &g, const float *D, int i, int j, int l, float s[4])
{
	s[0] = D[slice_point_index(g, i, j, l)] - g.iso;
	s[1] = D[slice_point_index(g, i + 1, j, l)] - g.iso;
	s[2] = D[slice_point_index(g, i + 1, j + 1, l)] - g.iso;
	s[3] = D[slice_point_index(g, i, j + 1, l)] - g.iso;
	uint32_t mask = 0u;
	for (int k = 0; k < 4; ++k) mask |= s[k] < 0.f ? 1u << k : 0u;
	return mask;
}
// side k runs from c_k to c_((k + 1) % 4): OUT iff c_k is inside and the next corner is not, IN iff it is the other way round
SDF_HD bool slice_side_out(uint32_t mask, int k) { return ((mask >> k) & 1u) != 0u && ((mask >> ((k + 1) & 3)) & 1u) == 0u; }
// segments of the cell whose corner c0 is point (i, j) of layer l -- its OUT sides, 0 .. 2 --, none where there is no such cell
SDF_HD uint32_t slice_cell_segments(const SliceGrid &g, const float *D, int i, int j, int l)
{
	if (i >= g.nu || j >= g.nv) return 0u;
	float s[4];
	const uint32_t mask = slice_cell_corners(g, D, i, j, l, s);
	uint32_t n = 0u;
	for (int k = 0; k < 4; ++k) n += slice_side_out(mask, k) ? 1u : 0u;
	return n;
}

// The vertex of the edge of point (i, j) of layer l along `axis` (which slice_edge_vertex says has one): with a the lower endpoint and b
// the upper one t = s_a / (s_a - s_b), 0.5 unless 0 <= t <= 1; the position p_a + t * (p_b - p_a) per component, and the lattice
// coordinates (i + t, j) or (i, j + t)
SDF_HD void slice_vertex(const SliceGrid &g, const float *D, int i, int j, int l, int axis, float pos[3], float uv[2])
{
	const int bi = i + (axis == 0 ? 1 : 0), bj = j + (axis == 0 ? 0 : 1);
	const float sa = D[slice_point_index(g, i, j, l)] - g.iso, sb = D[slice_point_index(g, bi, bj, l)] - g.iso;
	float t = sa / (sa - sb);
	if (!(t >= 0.f && t <= 1.f)) t = 0.5f;
	for (int c = 0; c < 3; ++c)
	{
		const float pa = slice_coord(g, c, i, j, l), pb = slice_coord(g, c, bi, bj, l);
		pos[c] = pa + t * (pb - pa);
	}
	uv[0] = axis == 0 ? (float)i + t : (float)i;
	uv[1] = axis == 0 ? (float)j : (float)j + t;
}
// The vertices of point (i, j) of layer l, the u-edge's before the v-edge's, from vertex `first` on; coords: null, or [.][2]
SDF_HD void slice_point_emit(const SliceGrid &g, const float *D, int i, int j, int l, uint32_t first, float *positions, float *coords)
{
	size_t v = first;
	for (int axis = 0; axis < 2; ++axis)
	{
		if (!slice_edge_vertex(g, D, i, j, l, axis)) continue;
		float pos[3], uv[2];
		slice_vertex(g, D, i, j, l, axis, pos, uv);
		float *o = positions + v * 3;
		o[0] = pos[0];
		o[1] = pos[1];
		o[2] = pos[2];
		if (coords)
		{
			coords[v * 2] = uv[0];
			coords[v * 2 + 1] = uv[1];
		}
		++v;
	}
}

// The index of the vertex on side k of cell (i, j) of layer l, which has one.  Side 0 is the u-edge of (i, j), side 1 the v-edge of
// (i + 1, j), side 2 the u-edge of (i, j + 1), side 3 the v-edge of (i, j); a point's v-edge vertex follows its u-edge vertex.
// point_vertex: the first vertex index per point (the scanned counts)
SDF_HD uint32_t slice_side_vertex(const SliceGrid &g, const float *D, const uint32_t *point_vertex, int i, int j, int l, int k)
{
	const int pi = i + (k == 1 ? 1 : 0), pj = j + (k == 2 ? 1 : 0);
	const uint32_t first = point_vertex[slice_point_index(g, pi, pj, l)];
	if ((k & 1) == 0) return first;
	return first + (slice_edge_vertex(g, D, pi, pj, l, 0) ? 1u : 0u);
}
// The segments of cell (i, j) of layer l in the order of their OUT sides, from segment `first` on: (the vertex on the OUT side, the
// vertex on the IN side it pairs with).  One OUT side: the one IN side.  Two (two diagonal corners are inside):
// m = ((s0 + s1) + (s2 + s3)) * 0.25f; m < 0 (NaN is not): OUT side k pairs with IN side (k + 1) % 4, otherwise with (k + 3) % 4.
SDF_HD void slice_cell_emit(const SliceGrid &g, const float *D, const uint32_t *point_vertex, int i, int j, int l, uint32_t first, uint32_t *segments)
{
	float s[4];
	const uint32_t mask = slice_cell_corners(g, D, i, j, l, s);
	int outs = 0;
	for (int k = 0; k < 4; ++k) outs += slice_side_out(mask, k) ? 1 : 0;
	const float m = ((s[0] + s[1]) + (s[2] + s[3])) * 0.25f;
	size_t q = first;
	for (int k = 0; k < 4; ++k)
	{
		if (!slice_side_out(mask, k)) continue;
		int in;
		if (outs == 2) in = m < 0.f ? (k + 1) & 3 : (k + 3) & 3;
		else
		{
			in = 0;
			for (int t = 0; t < 4; ++t)
				if (((mask >> t) & 1u) == 0u && ((mask >> ((t + 1) & 3)) & 1u) != 0u) in = t;
		}
		segments[q * 2] = slice_side_vertex(g, D, point_vertex, i, j, l, k);
		segments[q * 2 + 1] = slice_side_vertex(g, D, point_vertex, i, j, l, in);
		++q;
	}
}

} // namespace sdfr

// sdfr_mesh_sharp.h -- the vertex of sdfr_mesh_extract_sharp (include/sdfr.h, where the definition stands in full):
// surface nets' topology with every vertex moved onto the planes the scene has at the cell's edge crossings, so that edges and corners
// of the scene stay edges and corners of the mesh.  Two functions of one active cell, scene-independent and host-compilable like
// sdfr_mesh.h: the crossing of one edge and its plane (five scene evaluations: four bisection samples and the point query with its
// normal), and the vertex from the twelve of them (the mass point, the normal equations, three steps of conjugate gradients, the clamp).
// The scene comes in as an evaluator with two members,
//     float distance(vec3 p) const;                     // sdfr_query_distance's distance at p
//     float distance_normal(vec3 p, vec3 &n) const;     // ... and its normal there
// which sdfr_query_kernel.h binds to the loaded scene (query_point) and tests/cpp/mesh_sharp_host.cpp to a callback.  The vertex reads
// the crossings through a getter, edge -> MeshSharpCrossing: an array on the host, shuffles from the lanes that own the edges on the
// device.  All arithmetic is fp32 in source order (-ffp-contract=off), so both give the same bits whatever the mapping.
#pragma once
#include "sdfr_mesh.h"

namespace sdfr {

enum { MESH_SHARP_CROSSES = 1u, MESH_SHARP_PLANE = 2u };
struct MeshSharpCrossing
{
	float p[3];     // the refined crossing
	float n[3];     // the scene's normal there
	float s;        // the scene's distance there - iso
	uint32_t flags; // MESH_SHARP_CROSSES: the edge has exactly one endpoint inside; MESH_SHARP_PLANE: n and s are finite and n is not 0
};

SDF_HD bool mesh_sharp_finite(float x) { return (f32_bits(x) & 0x7f800000u) != 0x7f800000u; }
SDF_HD float mesh_sharp_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// Edge `e` (0 .. 11, sdfr_mesh_extract's order: axis e / 4, the offsets on the two other axes from e % 4) of cell (i, j, k): its
// crossing, refined by four bisection steps and one linear step inside the last bracket, and the scene's plane there.  D: the lattice.
template <class Eval>
SDF_HD void mesh_sharp_crossing(const MeshGrid &g, const float *D, const Eval &scene, int i, int j, int k, int e, MeshSharpCrossing &out)
{
	out.flags = 0u;
	const int axis = e >> 2;
	const int b = axis == 0 ? 1 : 0, c = axis == 2 ? 1 : 2; // the two other axes, lower one first
	int A[3] = {i, j, k};
	A[b] += e & 1;
	A[c] += (e >> 1) & 1;
	int B[3] = {A[0], A[1], A[2]};
	B[axis] += 1;
	float s_lo = D[mesh_point_index(g, A[0], A[1], A[2])] - g.iso, s_hi = D[mesh_point_index(g, B[0], B[1], B[2])] - g.iso;
	if ((s_lo < 0.f) == (s_hi < 0.f)) return;
	float p[3] = {mesh_coord(g, 0, A[0]), mesh_coord(g, 1, A[1]), mesh_coord(g, 2, A[2])};
	const float pa = p[axis], pb = mesh_coord(g, axis, B[axis]);
	float lo = 0.f, hi = 1.f;
	for (int step = 0; step < 4; ++step)
	{
		const float mid = 0.5f * (lo + hi);
		p[axis] = pa + mid * (pb - pa);
		const float s = scene.distance(V3(p[0], p[1], p[2])) - g.iso;
		if ((s < 0.f) == (s_lo < 0.f))
		{
			lo = mid;
			s_lo = s;
		}
		else
		{
			hi = mid;
			s_hi = s;
		}
	}
	float t = lo + (s_lo / (s_lo - s_hi)) * (hi - lo);
	if (!(t >= lo && t <= hi)) t = 0.5f * (lo + hi); // (NaN too)
	p[axis] = pa + t * (pb - pa);
	vec3 n;
	const float d = scene.distance_normal(V3(p[0], p[1], p[2]), n);
	out.p[0] = p[0];
	out.p[1] = p[1];
	out.p[2] = p[2];
	out.n[0] = n.x;
	out.n[1] = n.y;
	out.n[2] = n.z;
	out.s = d - g.iso;
	out.flags = MESH_SHARP_CROSSES;
	if (mesh_sharp_finite(out.n[0]) && mesh_sharp_finite(out.n[1]) && mesh_sharp_finite(out.n[2]) && mesh_sharp_finite(out.s) &&
		!(out.n[0] == 0.f && out.n[1] == 0.f && out.n[2] == 0.f))
		out.flags |= MESH_SHARP_PLANE;
}

// The vertex of active cell (i, j, k) from its crossings, crossing(e) for e = 0 .. 11 in that order (called for every edge, twice).
template <class Get>
SDF_HD void mesh_sharp_vertex(const MeshGrid &g, int i, int j, int k, const Get &crossing, float out[3])
{
	// the mass point: surface nets' formula over the refined crossings
	float m[3] = {0.f, 0.f, 0.f};
	int crossings = 0;
	for (int e = 0; e < 12; ++e)
	{
		const MeshSharpCrossing x = crossing(e);
		if (!(x.flags & MESH_SHARP_CROSSES)) continue;
		m[0] = m[0] + x.p[0];
		m[1] = m[1] + x.p[1];
		m[2] = m[2] + x.p[2];
		++crossings;
	}
	const float count = (float)crossings;
	m[0] = m[0] / count;
	m[1] = m[1] / count;
	m[2] = m[2] / count;
	// the normal equations of the planes n_i . (x - p_i) + s_i = 0 about m: H = sum n n^T + 2^-8 c I, G = sum n b
	float H[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, G[3] = {0.f, 0.f, 0.f};
	int planes = 0;
	for (int e = 0; e < 12; ++e)
	{
		const MeshSharpCrossing x = crossing(e);
		if (!(x.flags & MESH_SHARP_PLANE)) continue;
		const float bi = ((x.n[0] * (x.p[0] - m[0]) + x.n[1] * (x.p[1] - m[1])) + x.n[2] * (x.p[2] - m[2])) - x.s;
		for (int a = 0; a < 3; ++a)
		{
			for (int b = a; b < 3; ++b) H[a][b] = H[a][b] + x.n[a] * x.n[b];
			G[a] = G[a] + x.n[a] * bi;
		}
		++planes;
	}
	const float ridge = 0x1p-8f * (float)planes;
	for (int a = 0; a < 3; ++a) H[a][a] = H[a][a] + ridge;
	H[1][0] = H[0][1];
	H[2][0] = H[0][2];
	H[2][1] = H[1][2];
	// three steps of conjugate gradients from y = 0
	float y[3] = {0.f, 0.f, 0.f}, r[3] = {G[0], G[1], G[2]}, d[3] = {G[0], G[1], G[2]};
	float rr = mesh_sharp_dot(r, r);
	for (int step = 0; step < 3 && planes != 0; ++step)
	{
		if (!(rr > 0.f)) break;
		float Hd[3];
		for (int a = 0; a < 3; ++a) Hd[a] = (H[a][0] * d[0] + H[a][1] * d[1]) + H[a][2] * d[2];
		const float dHd = mesh_sharp_dot(d, Hd);
		if (!(dHd > 0.f)) break;
		const float alpha = rr / dHd;
		for (int a = 0; a < 3; ++a) y[a] = y[a] + alpha * d[a];
		for (int a = 0; a < 3; ++a) r[a] = r[a] - alpha * Hd[a];
		const float rr2 = mesh_sharp_dot(r, r);
		const float beta = rr2 / rr;
		for (int a = 0; a < 3; ++a) d[a] = r[a] + beta * d[a];
		rr = rr2;
	}
	float x[3] = {m[0] + y[0], m[1] + y[1], m[2] + y[2]};
	if (!(mesh_sharp_finite(x[0]) && mesh_sharp_finite(x[1]) && mesh_sharp_finite(x[2])))
	{
		x[0] = m[0];
		x[1] = m[1];
		x[2] = m[2];
	}
	// never more than half a cell outside the cell
	const float h = 0.5f * g.cell;
	const int cell[3] = {i, j, k};
	for (int a = 0; a < 3; ++a)
	{
		const float lo = mesh_coord(g, a, cell[a]) - h, hi = mesh_coord(g, a, cell[a] + 1) + h;
		float v = x[a];
		v = v < lo ? lo : v; // fminf(fmaxf(v, lo), hi) of a finite v
		v = v > hi ? hi : v;
		out[a] = v;
	}
}

} // namespace sdfr

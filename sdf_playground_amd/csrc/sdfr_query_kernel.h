// sdfr_query_kernel.h -- the query kernels (sdfr_query.h), one lane per item.  Shared by the kernels compiled ahead of time
// (sdfr_query_scene.hip, a translation unit of its own so that the pixel kernels' code does not change) and by the query
// module sdfr_jit.cpp builds for a scene compiled at run time.  Device compilation only.
//
// Items are read as float3 / int2 records of consecutive lanes (coalesced), results leave as 16-byte stores; launched with
// the scene's own launch attributes (SDFR_PIXEL_KERNEL_ATTRS), in blocks of SDFR_PIXEL_BLOCK lanes.
#pragma once
#include "sdfr_pixel_kernel.h"
#include "sdfr_query.h"

namespace sdfr {

// item i's record of three floats; the offset is 64-bit: 3 * i wraps in 32 bits from i = 2^32 / 3 on, well below INT32_MAX items
SDF_HD vec3 query_load3(const float *__restrict__ p, uint32_t i)
{
	const float *r = p + (size_t)3 * i;
	return V3(r[0], r[1], r[2]);
}

template <class Scene, bool DBG>
__device__ __forceinline__ void query_points_kernel(const QueryKernelArgs &a)
{
	const FrameU &U = a.U;
	const QueryArgs &q = a.q;
	const uint32_t i = blockIdx.x * (uint32_t)SDFR_PIXEL_BLOCK + threadIdx.x;
	if (i >= (uint32_t)q.n) return;
	const vec3 p = query_load3(q.pos, i);
	vec3 n;
	const float d = query_point<Scene, DBG>(U, p, q.normals ? &n : nullptr);
	q.distance[i] = d;
	if (q.normals)
	{
		float *r = q.normals + (size_t)3 * i;
		r[0] = n.x;
		r[1] = n.y;
		r[2] = n.z;
	}
}

template <class Scene, bool DBG>
__device__ __forceinline__ void query_rays_kernel(const QueryKernelArgs &a)
{
	const FrameU &U = a.U;
	const QueryArgs &q = a.q;
	const uint32_t i = blockIdx.x * (uint32_t)SDFR_PIXEL_BLOCK + threadIdx.x;
	if (i >= (uint32_t)q.n) return;
	uint32_t rec[QUERY_HIT_WORDS];
	if (q.kind == QUERY_PICK)
	{
		const int32_t px = q.pixels[(size_t)2 * i], py = q.pixels[(size_t)2 * i + 1];
		query_pick<Scene, DBG>(U, px, py, rec);
	}
	else
		query_ray<Scene, DBG>(U, query_load3(q.pos, i), query_load3(q.dir, i), q.dist_max, V3s(0.f), V3s(0.f), rec);
	uint32_t *out = q.hits + (size_t)QUERY_HIT_WORDS * i;
	if ((reinterpret_cast<size_t>(q.hits) & 15u) == 0u) // 48-byte records of an aligned array: three 16-byte stores
	{
		uint4 *dst = reinterpret_cast<uint4 *>(out);
		dst[0] = make_uint4(rec[0], rec[1], rec[2], rec[3]);
		dst[1] = make_uint4(rec[4], rec[5], rec[6], rec[7]);
		dst[2] = make_uint4(rec[8], rec[9], rec[10], rec[11]);
	}
	else // (sdfr_hit itself only asks for 4-byte alignment)
		for (int k = 0; k < QUERY_HIT_WORDS; ++k) out[k] = rec[k];
}

// The distance query over a lattice (LatticeArgs): one wave per block, one point per lane.  A wave owns a 4 x 4 x 4 brick of points,
// so that its lanes stay within 3 cells of each other and the scenes' wave-level branches (bounding volumes, cell lookups) stay
// coherent; its stores are runs of 4 floats.  rows = 1 maps 64 consecutive points of the linear index instead (coalesced stores,
// a wave 64 cells long).  Lanes past the lattice's ragged edges leave.
template <class Scene, bool DBG>
__device__ __forceinline__ void query_lattice_kernel(const LatticeKernelArgs &a)
{
	static_assert(SDFR_PIXEL_BLOCK == 64, "one wave per block: a brick is 64 points");
	const LatticeArgs &g = a.g;
	const uint32_t px = (uint32_t)g.px, py = (uint32_t)g.py, pz = (uint32_t)g.pz, lane = threadIdx.x;
	uint32_t i, j, k;
	if (g.rows)
	{
		const uint32_t p = blockIdx.x * 64u + lane; // < 2^30 + 64
		const uint32_t row = p / px;
		i = p - row * px;
		k = row / py;
		j = row - k * py;
	}
	else
	{
		const uint32_t bx = (px + 3u) >> 2, by = (py + 3u) >> 2;
		const uint32_t brow = blockIdx.x / bx;
		const uint32_t bk = brow / by;
		i = (blockIdx.x - brow * bx) * 4u + (lane & 3u);
		j = (brow - bk * by) * 4u + ((lane >> 2) & 3u);
		k = bk * 4u + (lane >> 4);
	}
	if (i >= px || j >= py || k >= pz) return;
	const vec3 p = V3(g.origin[0] + (float)i * g.cell, g.origin[1] + (float)j * g.cell, g.origin[2] + (float)k * g.cell);
	g.out[i + px * (j + py * k)] = query_point<Scene, DBG>(a.U, p, nullptr); // (the index is < 2^30)
}

} // namespace sdfr

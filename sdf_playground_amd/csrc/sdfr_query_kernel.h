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

} // namespace sdfr

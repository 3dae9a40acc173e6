// sdfr_occlusion.h -- ambient occlusion at a point of the loaded scene (device code, host-compilable): the record of
// sdfr_query_occlusion and sdfr_hit_occlusion (sdfr_occlusion in include/sdfr.h).  From a point p and a normal n, 64
// rays leave p + bias * n along the directions of one fixed table, turned into the frame of n, and are marched to `radius` as the ray
// query marches (sdfr_query.h: query_ray_hits); the answer is the 64-bit mask of the rays that hit.  Every bit is fixed: no
// floating-point reduction, no dependence on order.  The kernel that runs it one wave per item, one lane per direction, is in
// sdfr_query_kernel.h -- only its ballot is device code --, and tests/cpp/occlusion_host.cpp compiles these functions for the CPU
// to compare them with the oracle.
#pragma once
#include "sdfr_query.h"

namespace sdfr {

enum { OCCLUSION_DIRS = 64 };

// The directions: fp32 unit vectors, cosine-distributed over the hemisphere z > 0 (tools/make_occlusion_dirs.py).  The header is
// the definition.
static constexpr float k_occlusion_dirs[OCCLUSION_DIRS][3] = {
#include "sdfr_occlusion_dirs.h"
};

// An item has an answer if its point and normal are finite and the normal is not (0, 0, 0)
SDF_HD bool occlusion_finite(float v) { return (f32_bits(v) & 0x7f800000u) != 0x7f800000u; }
SDF_HD bool occlusion_item_ok(vec3 p, vec3 n)
{
	const bool finite = occlusion_finite(p.x) && occlusion_finite(p.y) && occlusion_finite(p.z) && occlusion_finite(n.x) && occlusion_finite(n.y) &&
		occlusion_finite(n.z);
	return finite && !(n.x == 0.f && n.y == 0.f && n.z == 0.f);
}

// The frame of a normal n, used as given (the branchless basis of Duff et al., orthonormal for a unit n): every product and sum
// a separate fp32 operation, left to right as written
struct OcclusionFrame
{
	vec3 t, u, n;
};
SDF_HD OcclusionFrame occlusion_frame(vec3 n)
{
	const float s = bits_f32((f32_bits(n.z) & 0x80000000u) | 0x3f800000u); // copysignf(1, n.z)
	const float a = -1.f / (s + n.z);
	const float b = n.x * n.y * a;
	OcclusionFrame f;
	f.t = V3(1.f + s * n.x * n.x * a, s * b, -s * n.x);
	f.u = V3(b, s + n.y * n.y * a, -n.y);
	f.n = n;
	return f;
}

// World direction k: per component (t * D[k][0] + u * D[k][1]) + n * D[k][2]
SDF_HD vec3 occlusion_direction(const OcclusionFrame &f, uint32_t k)
{
	const float d0 = k_occlusion_dirs[k][0], d1 = k_occlusion_dirs[k][1], d2 = k_occlusion_dirs[k][2];
	return V3((f.t.x * d0 + f.u.x * d1) + f.n.x * d2, (f.t.y * d0 + f.u.y * d1) + f.n.y * d2, (f.t.z * d0 + f.u.z * d1) + f.n.z * d2);
}

// where every ray of an item starts: p + bias * n per component, one multiply, then one add
SDF_HD vec3 occlusion_origin(vec3 p, vec3 n, float bias)
{
	const vec3 off = bias * n;
	return p + off;
}

// Whether direction k of the item (p, n) hits within `radius`: exactly sdfr_query_rays' march of that ray with max_distance = radius
// -- no offsets, the debug plane and show_objects included (map_geometry) --, without the normal and the material of the hit.
template <class Scene, bool DBG>
SDF_HD bool occlusion_ray_hits(const FrameU &U, vec3 p, vec3 n, float bias, float radius, uint32_t k)
{
	const vec3 origin = occlusion_origin(p, n, bias);
	const vec3 dir = occlusion_direction(occlusion_frame(n), k);
	return query_ray_hits<Scene, DBG>(U, origin, dir, radius, V3s(0.f), V3s(0.f));
}

// the 4 words of sdfr_occlusion
SDF_HD void occlusion_record(uint64_t mask, uint32_t occluded, uint32_t rec[QUERY_OCCLUSION_WORDS])
{
	rec[0] = (uint32_t)mask;
	rec[1] = (uint32_t)(mask >> 32);
	rec[2] = occluded;
	rec[3] = 1u;
}
// nothing to answer (valid 0) or an invalid item (valid -1): every other word 0
SDF_HD void occlusion_none(uint32_t valid, uint32_t rec[QUERY_OCCLUSION_WORDS])
{
	rec[0] = rec[1] = rec[2] = 0u;
	rec[3] = valid;
}
// what a hit record's `hit` word makes of an item of sdfr_hit_occlusion: 1 the item is (pos, normal); 0 a miss; anything else invalid
SDF_HD uint32_t occlusion_hit_valid(uint32_t hit) { return hit <= 1u ? hit : 0xffffffffu; }

} // namespace sdfr

// sdfr_atlas.h -- the texels of an extracted mesh's texture atlas (device code, host-compilable): sdfr_atlas_texels and sdfr_atlas_bake
// of include/sdfr.h, whose "texture atlas" section is the definition restated here.  One square tile of T x T texels per quad of the
// mesh -- surface nets emits triangles 2q and 2q + 1 as (q0, q1, q2) and (q0, q2, q3) of one quad --, the quad's corners on the centres
// of the tile's corner texels.  atlas_texel maps a texel to a point of its quad and the normal there; atlas_bake_texel goes on as
// sdfr_mesh_surfaces / sdfr_mesh_lighting do with the item (P, N, reach): query_mesh_ray, one march, then the surface record's and the
// lighting record's lines.  The kernels: k_atlas_texels (sdfr_mesh.hip, scene-free) and atlas_bake_kernel (sdfr_query_kernel.h);
// tests/cpp/atlas_host.cpp compiles these functions for the CPU to compare them with the oracle.
//
// A unit that wants the scene-free part alone defines SDFR_ATLAS_GEOMETRY_ONLY first: nothing of the pixel pipeline is included then.
#pragma once
#include "sdfr_math.h"
#include "sdfr_query_args.h"
#ifndef SDFR_ATLAS_GEOMETRY_ONLY
#include "sdfr_lighting.h"
#endif

namespace sdfr {

enum { ATLAS_TEXEL_INVALID = -1, ATLAS_TEXEL_DEGENERATE = 0, ATLAS_TEXEL_VALID = 1 };

SDF_HD bool atlas_finite(float x) { return (f32_bits(x) & 0x7f800000u) != 0x7f800000u; }
SDF_HD bool atlas_finite(vec3 v) { return atlas_finite(v.x) && atlas_finite(v.y) && atlas_finite(v.z); }
SDF_HD vec3 atlas_load3(const float *p, uint32_t i)
{
	const float *r = p + (size_t)3 * i;
	return V3(r[0], r[1], r[2]);
}

// The quad of tile q: its four vertices, or ok = false -- no quad (q >= quads), triangles 2q and 2q + 1 that do not share q0 and q2,
// or an index that is no vertex, which is found out before any vertex is loaded.
struct AtlasQuad
{
	bool ok;
	vec3 p[4], n[4];
};
SDF_HD AtlasQuad atlas_load_quad(const AtlasArgs &g, uint32_t q)
{
	AtlasQuad Q;
	Q.ok = false;
	for (int k = 0; k < 4; ++k) Q.p[k] = Q.n[k] = V3s(0.f);
	if (q >= g.quads) return Q;
	const uint32_t *t = g.indices + (size_t)6 * q;
	const uint32_t i0 = t[0], i1 = t[1], i2 = t[2], i3 = t[5];
	if (t[3] != i0 || t[4] != i2) return Q;
	if (i0 >= g.vertex_count || i1 >= g.vertex_count || i2 >= g.vertex_count || i3 >= g.vertex_count) return Q;
	Q.ok = true;
	Q.p[0] = atlas_load3(g.positions, i0);
	Q.p[1] = atlas_load3(g.positions, i1);
	Q.p[2] = atlas_load3(g.positions, i2);
	Q.p[3] = atlas_load3(g.positions, i3);
	Q.n[0] = atlas_load3(g.normals, i0);
	Q.n[1] = atlas_load3(g.normals, i1);
	Q.n[2] = atlas_load3(g.normals, i2);
	Q.n[3] = atlas_load3(g.normals, i3);
	return Q;
}

// X = (A0 + s * (Aa - A0)) + t * (A2 - Aa), every operation of its own
SDF_HD vec3 atlas_mix(vec3 A0, vec3 Aa, vec3 A2, float s, float t) { return (A0 + s * (Aa - A0)) + t * (A2 - Aa); }

// Texel (a, b) of a T x T tile, 0 <= a, b < T: u = a / (T - 1), v = b / (T - 1); u >= v lies in triangle 2q = (q0, q1, q2), the rest in
// triangle 2q + 1 = (q0, q2, q3).  -> ATLAS_TEXEL_*; P and N are zero unless the texel is valid.
SDF_HD int atlas_texel(const AtlasQuad &Q, uint32_t a, uint32_t b, uint32_t T, vec3 &P, vec3 &N)
{
	P = N = V3s(0.f);
	if (!Q.ok) return ATLAS_TEXEL_INVALID;
	const float last = (float)(T - 1u);
	const float u = (float)a / last, v = (float)b / last;
	const bool first = u >= v;
	const float s = first ? u : v, t = first ? v : u;
	const vec3 X = atlas_mix(Q.p[0], first ? Q.p[1] : Q.p[3], Q.p[2], s, t);
	const vec3 M = atlas_mix(Q.n[0], first ? Q.n[1] : Q.n[3], Q.n[2], s, t);
	if (!atlas_finite(X) || !atlas_finite(M) || (M.x == 0.f && M.y == 0.f && M.z == 0.f)) return ATLAS_TEXEL_DEGENERATE;
	const float r = 1.0f / sqrt_ieee(fma1(M.z, M.z, fma1(M.y, M.y, M.x * M.x)));
	const vec3 unit = M * r;
	if (!atlas_finite(unit)) return ATLAS_TEXEL_DEGENERATE;
	P = X;
	N = unit;
	return ATLAS_TEXEL_VALID;
}

// the tile and the place in it of image texel (x, y)
SDF_HD uint32_t atlas_tile_of(const AtlasArgs &g, uint32_t x, uint32_t y) { return (y >> g.tile_log2) * (uint32_t)g.tiles_per_row + (x >> g.tile_log2); }

#ifndef SDFR_ATLAS_GEOMETRY_ONLY
// no light samples are kept (lighting_record's Samples)
struct AtlasNoSamples
{
	SDF_HD bool wanted() const { return false; }
	SDF_HD void operator()(int, const uint32_t (&)[QUERY_LIGHT_SAMPLE_WORDS]) const {}
};

// A valid texel (P, N) of a bake: the ray of sdfr_mesh_surfaces, marched once; at a hit the surface record's words give the albedo and
// normal planes and the lighting record's the lit plane, each only where `layers` asks.  -> valid: 1 hit, 0 miss (the planes stay 0).
template <class Scene, bool DBG>
SDF_HD uint32_t atlas_bake_texel(const FrameU &U, vec3 P, vec3 N, float reach, uint32_t layers, uint32_t albedo[4], uint32_t normal[4], uint32_t lit[4])
{
	for (int k = 0; k < 4; ++k) albedo[k] = normal[k] = lit[k] = 0u;
	const QueryRay ray = query_mesh_ray(P, N, reach);
	uint32_t hit[QUERY_HIT_WORDS];
	QueryHit at;
	if (!query_ray_at<Scene, DBG>(U, ray.origin, ray.dir, ray.dist_max, ray.right_off, ray.bottom_off, hit, at)) return 0u;
	if (layers & (uint32_t)(ATLAS_ALBEDO | ATLAS_NORMAL))
	{
		uint32_t srf[QUERY_SURFACE_WORDS];
		surface_record(U, at.sp, at.mat, srf);
		const bool lit_material = (srf[1] & (uint32_t)SURFACE_LIT) != 0u; // sdfr_surface.albedo, or .unlit of a material no light falls on
		albedo[0] = lit_material ? srf[4] : srf[16];
		albedo[1] = lit_material ? srf[5] : srf[17];
		albedo[2] = lit_material ? srf[6] : srf[18];
		albedo[3] = srf[7];
		normal[0] = srf[28];
		normal[1] = srf[29];
		normal[2] = srf[30];
	}
	if (layers & (uint32_t)ATLAS_LIT)
	{
		uint32_t rec[QUERY_LIGHTING_WORDS];
		lighting_record<Scene, DBG>(U, at.sp, at.mat, rec, AtlasNoSamples());
		lit[0] = rec[12];
		lit[1] = rec[13];
		lit[2] = rec[14];
		lit[3] = f32_bits(1.f);
	}
	return 1u;
}
#endif

} // namespace sdfr

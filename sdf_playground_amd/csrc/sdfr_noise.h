// sdfr_noise.h -- PCG hash, simplex noise in 2, 3 and 4 dimensions and 4-octave turbulence for the shade kernels.
//
// Same functions as the reference's Engine/shader/noise.hlsl (hash :6-16, grad4 :124-140, snoise(float2)
// :142-203, snoise(float3) :205-300, snoise(float4) :304-433, turbulence :473-476), written corner-by-corner
// in scalars so that no float4 temporaries have to stay live: the simplex corners are independent until the
// final weighted sum.  Operation order per value is the one of the HLSL source.
#pragma once
#include "sdfr_math.h"

namespace sdfr {

SDF_HD uint32_t pcg_hash(uint32_t v)
{
	uint32_t state = v * 747796405u + 2891336453u;
	uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
	return (word >> 22u) ^ word;
}
SDF_HD float pcg_hashf(uint32_t v) { return (float)pcg_hash(v) / (float)0xFFFFFFFFu; }

SDF_HD float noise_mod289(float x) { return x - floor1(x * 0.00346020761245674740484429065744f) * 289.0f; }
SDF_HD float noise_permute(float x) { return noise_mod289(x * x * 34.0f + x); }

// How snoise3 hashes a lattice point: the hash H of its gradient source (NG::Hash).  NoiseHashPlain is the definition, the text of
// noise.hlsl operation by operation; NoiseHashExact computes the same bits with fewer instructions where its precondition holds.
struct NoiseHashPlain
{
	// hashed gradient index of each of the four corners of the cell i (i1, i2: the offsets of the middle corners, components
	// 0 or 1); the "+ 0" of corner 0 is the identity because mod289 never returns -0.  Nothing to check.
	static SDF_HD vec4 corners(vec3 i, vec3 i1, vec3 i2, bool &)
	{
		i = V3(noise_mod289(i.x), noise_mod289(i.y), noise_mod289(i.z));
		float p0 = noise_permute(noise_permute(noise_permute(i.z) + i.y) + i.x);
		float p1 = noise_permute(noise_permute(noise_permute(i.z + i1.z) + i.y + i1.y) + i.x + i1.x);
		float p2 = noise_permute(noise_permute(noise_permute(i.z + i2.z) + i.y + i2.y) + i.x + i2.x);
		float p3 = noise_permute(noise_permute(noise_permute(i.z + 1.0f) + i.y + 1.0f) + i.x + 1.0f);
		return V4(p0, p1, p2, p3);
	}
	// the gradient index j = p mod 49 of a corner
	static SDF_HD float mod49(float p)
	{
		const float n_ = 0.142857142857f;
		const float ns_z = n_ * 1.0f - 0.0f;
		return p - 49.0f * floor1(p * ns_z * ns_z);
	}
};

// The same hash with a*b + c written fma(a, b, c) wherever the product a*b is exact: the fma then rounds the same real number the
// two plain operations round (the product adds no rounding of its own), once, and a correctly rounded result is unique -- zeros
// included: an exactly zero sum of nonzero terms is +0 either way, and where the product is a zero the fma adds the same signed
// zero the plain form adds (x - P is x + (-P); the fma's product is written -c * f, so it is -P).  One v_fmamk / v_fmac instead
// of a multiplication and an addition, twice per permute and once per corner.
//
// Precondition: the reduced lattice coordinates r = mod289(i) are integers in [-1, 289]; `corners` clears `ok` unless they are,
// once per snoise3, and a lane whose `ok` is cleared evaluates the noise again with NoiseHashPlain (snoise3, turbulence3), so the
// bits are the definition's whatever the input.
//   * What leaves mod289 is integer-valued or not finite: i = floor(.) is integer-valued or not finite, so is f = floor1(i * c),
//     so is the rounded product f * 289 (a product of integers is an integer; below 2^24 it is exact, and every float from 2^23
//     on is an integer), and so is the rounded difference of two integer-valued floats for the same reason.  The range test is
//     therefore all the test there is; NaN (from i = +-inf: inf - inf) fails both comparisons.  -0 cannot arrive: i = -0 gives
//     f = -0, f * 289 = -0 and -0 - -0 = +0, and any other zero difference is +0; it would pass the test and be harmless.
//   * mod289(i) is one of -1 .. 289 for every integer |i| <= 2^24 (float rounding of i * c puts a few multiples of 289 on the
//     wrong side of floor1: -1 and 289 beside 0 .. 288), hence for every input with |x| < 2^20 even in turbulence3's last octave:
//     `ok` stays set there.  The reduction of the lattice coordinates itself stays plain: fused, it differs from the definition
//     for |i| >= 2^24 (f * 289 no longer exact) with both results inside the range, so no test of r would catch it.
//   * By induction every value of the chain is then an integer of [-1, 289] and every argument x of a permute, a sum of at most two
//     of them and 0 or 1, an integer of [-2, 579].  x * x <= 335 241 is exact, 34 x^2 <= 11 398 194 < 2^24 is exact, so
//     fma(x * x, 34, x) = 34 x^2 + x =: y exactly, as the two plain operations give it, 0 <= y <= 11 398 773 < 2^24.
//     In mod289(y), f = floor1(y * c) is an integer 0 <= f <= 39 443, 289 f < 2^24 is exact, so fma(-289, f, y) is the plain
//     y - f * 289.  That result lies in [-1, 289] again for each of the 582 arguments x: tests/test_noise_fused_cpu.py goes through
//     them all (and through every x up to 702), which closes the induction.
//   * j: f = floor1(p * ns_z * ns_z) is one of -1 .. 5 for p in [-1, 289], 49 f is exact.
struct NoiseHashExact
{
	static SDF_HD bool reduced(float r) { return (r >= -1.0f) & (r <= 289.0f); }
	static SDF_HD float mod289(float y) { return fma1(-289.0f, floor1(y * 0.00346020761245674740484429065744f), y); }
	static SDF_HD float permute(float x) { return mod289(fma1(x * x, 34.0f, x)); }
	// The innermost permute of the four corners is permute(i.z + {0, i1.z, i2.z, 1}) with i1.z, i2.z 0 or 1: two permutes and
	// two selects instead of four permutes.  i.z + 0 is i.z (never -0, above) and i.z + 1 is what corner 3 adds -- the very
	// arguments of the plain text, so this part needs no precondition.
	static SDF_HD vec4 corners(vec3 i, vec3 i1, vec3 i2, bool &ok)
	{
		i = V3(noise_mod289(i.x), noise_mod289(i.y), noise_mod289(i.z));
		ok = ok & reduced(i.x) & reduced(i.y) & reduced(i.z);
		const float q0 = permute(i.z), q3 = permute(i.z + 1.0f);
		const float q1 = i1.z != 0.0f ? q3 : q0, q2 = i2.z != 0.0f ? q3 : q0;
		float p0 = permute(permute(q0 + i.y) + i.x);
		float p1 = permute(permute(q1 + i.y + i1.y) + i.x + i1.x);
		float p2 = permute(permute(q2 + i.y + i2.y) + i.x + i2.x);
		float p3 = permute(permute(q3 + i.y + 1.0f) + i.x + 1.0f);
		return V4(p0, p1, p2, p3);
	}
	static SDF_HD float mod49(float p)
	{
		const float n_ = 0.142857142857f;
		const float ns_z = n_ * 1.0f - 0.0f;
		return fma1(-49.0f, floor1(p * ns_z * ns_z), p);
	}
};

// normalised gradient number j of snoise3 (the 7 x 7 points of a square folded onto an octahedron); j = p mod 49, computed
// by the corner.  The only definition of these gradients: the table below is filled by this same function.
SDF_HD vec3 simplex_grad(float j)
{
	const float n_ = 0.142857142857f;
	const float ns_x = n_ * 2.0f - 0.0f, ns_y = n_ * 0.5f - 1.0f, ns_z = n_ * 1.0f - 0.0f;
	float xq = floor1(j * ns_z);
	float yq = floor1(j - 7.0f * xq);
	float gx = xq * ns_x + ns_y;
	float gy = yq * ns_x + ns_y;
	float h = 1.0f - abs1(gx) - abs1(gy);
	float sx = floor1(gx) * 2.0f + 1.0f;
	float sy = floor1(gy) * 2.0f + 1.0f;
	float sh = -step1(h, 0.0f);
	vec3 g = V3(gx + sx * sh, gy + sy * sh, h);
	return g * rsqrt1(dot(g, g));
}

// Where a corner gets its gradient from: the gradient source NG of snoise3 / turbulence3 and of the shading that calls them.
// NoiseGradFormula evaluates simplex_grad.  NoiseGradTable<Tab> reads simplex_grad(k), k = 0..63, from a table that Tab holds
// (Tab::at(c, k): component c of gradient k; the pixel kernel keeps it in LDS, sdfr_pixel_kernel.h) and clears `ok` unless j
// is that k -- every j the permute chain produces is an integer in 0..48 (tests/test_noise_table_cpu.py), and -0 reads entry 0,
// simplex_grad(-0) being simplex_grad(+0) bit for bit.  A lane that ends with `ok` cleared evaluates the noise once more with
// the formula (snoise3, turbulence3), so the bits are the formula's whatever the input.  The check is per lane and the
// recomputation sits after the straight-line table code, not in each corner: a branch per corner costs the register
// allocator more than the formula it skips.
struct NoiseGradFormula
{
	typedef NoiseHashPlain Hash;
	static SDF_HD vec3 grad(float j, bool &) { return simplex_grad(j); }
};
#define SDFR_NOISE_GRADS 64
template <class Tab>
struct NoiseGradTable
{
	typedef NoiseHashExact Hash; // the fallback of the table is the fallback of the hash: one `ok`, one recomputation
	static SDF_HD vec3 grad(float j, bool &ok)
	{
		// the clamp keeps the conversion defined (NaN -> the last entry) and the index inside the table whatever j is; clamped
		// from above first, which left the headline's march loops with the better register draw (tools/kernel_resources.py)
		const uint32_t k = (uint32_t)max1(min1(j, (float)(SDFR_NOISE_GRADS - 1)), 0.0f);
		ok = ok & ((float)k == j);
		return V3(Tab::at(0, k), Tab::at(1, k), Tab::at(2, k));
	}
};

// The input of that second evaluation, opaque to the compiler: shared with the table path, the corner offsets and weights
// would stay live to the end of the noise and spill.
SDF_HD vec3 noise_recompute_input(vec3 v)
{
#if defined(__HIP_DEVICE_COMPILE__)
	asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z));
#endif
	return v;
}

// gradient of one simplex corner dotted with the corner offset `xc`, times the corner's
// falloff weight: returns (m^4, dot(grad, xc)) as (x, y)
template <class NG>
SDF_HD vec2 simplex_corner(float p, vec3 xc, bool &ok)
{
	float j = NG::Hash::mod49(p);
	vec3 g = NG::grad(j, ok);
	float m = max1(0.6f - dot(xc, xc), 0.0f);
	m = m * m;
	return V2(m * m, dot(g, xc));
}

// the noise; `ok` as NG::grad leaves it
template <class NG>
SDF_HD float snoise3_grads(vec3 v, bool &ok)
{
	const float Cx = 0.166666666666666667f, Cy = 0.333333333333333333f;
	// skew to the simplex grid
	vec3 i = floor(v + dot(v, V3s(Cy)));
	vec3 x0 = v - i + dot(i, V3s(Cx));
	// rank the components to pick the traversal order of the simplex
	vec3 g = V3(step1(x0.y, x0.x), step1(x0.z, x0.y), step1(x0.x, x0.z));
	vec3 l = 1.f - g;
	vec3 lz = V3(l.z, l.x, l.y);
	vec3 i1 = min(g, lz);
	vec3 i2 = max(g, lz);
	vec3 x1 = x0 - i1 + Cx;
	vec3 x2 = x0 - i2 + Cy;
	vec3 x3 = x0 - 0.5f;

	const vec4 p = NG::Hash::corners(i, i1, i2, ok);

	vec2 c0 = simplex_corner<NG>(p.x, x0, ok);
	vec2 c1 = simplex_corner<NG>(p.y, x1, ok);
	vec2 c2 = simplex_corner<NG>(p.z, x2, ok);
	vec2 c3 = simplex_corner<NG>(p.w, x3, ok);
	return 42.0f * dot(V4(c0.x, c1.x, c2.x, c3.x), V4(c0.y, c1.y, c2.y, c3.y));
}

template <class NG = NoiseGradFormula>
SDF_HD float snoise3(vec3 v)
{
	bool ok = true;
	const float n = snoise3_grads<NG>(v, ok);
	if (ok) return n;
	return snoise3_grads<NoiseGradFormula>(noise_recompute_input(v), ok);
}

// ---- 2-D (noise.hlsl:142-203) ------------------------------------------------------------------------------
// one corner: the hashed index p picks one of 41 gradients on a diamond; returns (m^4 times the approximate
// normalisation, gradient . offset)
SDF_HD vec2 simplex2_corner(float p, float ox, float oy)
{
	float m = max1(0.5f - fma1(oy, oy, ox * ox), 0.0f);
	m = m * m;
	m = m * m;
	const float x = 2.0f * frac1(p * 0.024390243902439f) - 1.0f;
	const float h = abs1(x) - 0.5f;
	const float a0 = x - floor1(x + 0.5f);
	m = m * (1.79284291400159f - 0.85373472095314f * (a0 * a0 + h * h));
	return V2(m, a0 * ox + h * oy);
}

SDF_HD float snoise2(vec2 v)
{
	const float Cx = 0.211324865405187f, Cy = 0.366025403784439f, Cz = -0.577350269189626f;
	const float s = dot(v, V2(Cy, Cy));
	float ix = floor1(v.x + s), iy = floor1(v.y + s);
	const float t = dot(V2(ix, iy), V2(Cx, Cx));
	const float x0 = v.x - ix + t, y0 = v.y - iy + t;
	// the middle corner lies one step along the larger component
	const float sx = x0 > y0 ? 1.0f : 0.0f, sy = 1.0f - sx;
	const float x1 = x0 + Cx - sx, y1 = y0 + Cx - sy;
	const float x2 = x0 + Cz, y2 = y0 + Cz;
	ix = noise_mod289(ix);
	iy = noise_mod289(iy);
	// `iy + 0` of the first corner is the identity: mod289 never returns -0
	const float p0 = noise_permute(noise_permute(iy) + ix);
	const float p1 = noise_permute(noise_permute(iy + sy) + ix + sx);
	const float p2 = noise_permute(noise_permute(iy + 1.0f) + ix + 1.0f);
	const vec2 c0 = simplex2_corner(p0, x0, y0);
	const vec2 c1 = simplex2_corner(p1, x1, y1);
	const vec2 c2 = simplex2_corner(p2, x2, y2);
	return 130.0f * dot(V3(c0.x, c1.x, c2.x), V3(c0.y, c1.y, c2.y));
}

// ---- 4-D (noise.hlsl:124-140, 304-433) -----------------------------------------------------------------------
// gradient j of the 7 x 7 x 6 points on a cube, folded onto the 4-cross polytope (not normalised)
SDF_HD vec4 noise_grad4(float j, float ipx, float ipy, float ipz)
{
	float gx = floor1(frac1(j * ipx) * 7.0f) * ipz - 1.0f;
	float gy = floor1(frac1(j * ipy) * 7.0f) * ipz - 1.0f;
	float gz = floor1(frac1(j * ipz) * 7.0f) * ipz - 1.0f;
	const float gw = 1.5f - dot(V3(abs1(gx), abs1(gy), abs1(gz)), V3s(1.0f));
	const float below = gw < 0.f ? 1.0f : 0.0f;
	gx = gx - sign1(gx) * below;
	gy = gy - sign1(gy) * below;
	gz = gz - sign1(gz) * below;
	return V4(gx, gy, gz, gw);
}
// one corner: (falloff^4, normalised gradient . offset)
SDF_HD vec2 simplex4_corner(float j, vec4 xc)
{
	vec4 g = noise_grad4(j, 0.003401360544217687075f, 0.020408163265306122449f, 0.142857142857142857143f); // 1/294, 1/49, 1/7
	g = g * rsqrt1(dot(g, g));
	float m = max1(0.6f - dot(xc, xc), 0.0f);
	m = m * m;
	return V2(m * m, dot(g, xc));
}

SDF_HD float snoise4(vec4 v)
{
	const float G4 = 0.138196601125011f, G4x2 = 0.276393202250021f, G4x3 = 0.414589803375032f, G4x4m1 = -0.447213595499958f;
	const float s = dot(v, V4(0.309016994374947451f, 0.309016994374947451f, 0.309016994374947451f, 0.309016994374947451f));
	vec4 i = floor(v + s);
	const vec4 x0 = v - i + dot(i, V4(G4, G4, G4, G4));
	// rank of each component among the four (3 = largest; ties as step(): x >= edge counts for the earlier one)
	const float xy = step1(x0.y, x0.x), xz = step1(x0.z, x0.x), xw = step1(x0.w, x0.x);
	const float yz = step1(x0.z, x0.y), yw = step1(x0.w, x0.y), zw = step1(x0.w, x0.z);
	const vec4 rank = V4(xy + xz + xw, (1.0f - xy) + (yz + yw), ((1.0f - xz) + (1.0f - yz)) + zw, ((1.0f - xw) + (1.0f - yw)) + (1.0f - zw));
	// corner k steps along the components of rank >= 4 - k
	const vec4 i3 = V4(sat1(rank.x), sat1(rank.y), sat1(rank.z), sat1(rank.w));
	const vec4 i2 = V4(sat1(rank.x - 1.0f), sat1(rank.y - 1.0f), sat1(rank.z - 1.0f), sat1(rank.w - 1.0f));
	const vec4 i1 = V4(sat1(rank.x - 2.0f), sat1(rank.y - 2.0f), sat1(rank.z - 2.0f), sat1(rank.w - 2.0f));
	const vec4 x1 = x0 - i1 + G4;
	const vec4 x2 = x0 - i2 + G4x2;
	const vec4 x3 = x0 - i3 + G4x3;
	const vec4 x4 = x0 + G4x4m1;
	i = V4(noise_mod289(i.x), noise_mod289(i.y), noise_mod289(i.z), noise_mod289(i.w));
	const float j0 = noise_permute(noise_permute(noise_permute(noise_permute(i.w) + i.z) + i.y) + i.x);
	const float j1 = noise_permute(noise_permute(noise_permute(noise_permute(i.w + i1.w) + i.z + i1.z) + i.y + i1.y) + i.x + i1.x);
	const float j2 = noise_permute(noise_permute(noise_permute(noise_permute(i.w + i2.w) + i.z + i2.z) + i.y + i2.y) + i.x + i2.x);
	const float j3 = noise_permute(noise_permute(noise_permute(noise_permute(i.w + i3.w) + i.z + i3.z) + i.y + i3.y) + i.x + i3.x);
	const float j4 = noise_permute(noise_permute(noise_permute(noise_permute(i.w + 1.0f) + i.z + 1.0f) + i.y + 1.0f) + i.x + 1.0f);
	const vec2 c0 = simplex4_corner(j0, x0);
	const vec2 c1 = simplex4_corner(j1, x1);
	const vec2 c2 = simplex4_corner(j2, x2);
	const vec2 c3 = simplex4_corner(j3, x3);
	const vec2 c4 = simplex4_corner(j4, x4);
	return 49.0f * (dot(V3(c0.x, c1.x, c2.x), V3(c0.y, c1.y, c2.y)) + dot(V2(c3.x, c4.x), V2(c3.y, c4.y)));
}

template <class NG>
SDF_HD float turbulence3_grads(vec3 p, bool &ok)
{
	return div_c((snoise3_grads<NG>(p, ok) + snoise3_grads<NG>(p * 2.f, ok) / 2.f + snoise3_grads<NG>(p * 4.f, ok) / 4.f + snoise3_grads<NG>(p * 8.f, ok) / 8.f) * 8.f,
		15.f, 1.0f / 15.f);
}
template <class NG = NoiseGradFormula>
SDF_HD float turbulence3(vec3 p)
{
	bool ok = true;
	const float t = turbulence3_grads<NG>(p, ok);
	if (ok) return t;
	return turbulence3_grads<NoiseGradFormula>(noise_recompute_input(p), ok);
}

} // namespace sdfr

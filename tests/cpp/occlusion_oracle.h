// tests/cpp/occlusion_oracle.h -- TEST-ONLY: the occlusion record of include/sdfr.h (sdfr_query_occlusion, sdfr_hit_occlusion)
// defined with the CPU oracle's ray query (query_oracle.h: ray_turn of oracle/driver.h).  The frame and the rays are written
// here from the definition in include/sdfr.h, in plain float arithmetic (built with -ffp-contract=off), not with the library's
// sdfr_occlusion.h; only the direction table, which IS the definition, is shared.  Part of record_oracle.cpp; the product never
// loads it.
#pragma once
#include "record_oracle.h"

#include <cmath>

namespace {

const float k_table[64][3] = {
#include "sdfr_occlusion_dirs.h"
};

bool all_finite(const float *v)
{
	return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]);
}

// one item: 64 calls of the ray query, each bit its `hit`
void occlusion_item(const Entry *e, const Frame &F, const float *p, const float *n, float bias, float radius, uint32_t *out)
{
	out[0] = out[1] = out[2] = out[3] = 0u;
	if (!all_finite(p) || !all_finite(n)) return;
	if (n[0] == 0.f && n[1] == 0.f && n[2] == 0.f) return;
	const float nx = n[0], ny = n[1], nz = n[2];
	const float s = copysignf(1.f, nz);
	const float sum = s + nz;
	const float a = -1.f / sum;
	const float xy = nx * ny;
	const float b = xy * a;
	// t = (1 + s nx nx a, s b, -s nx)
	float q = s * nx;
	q = q * nx;
	q = q * a;
	const float t[3] = {1.f + q, s * b, -s * nx};
	// u = (b, s + ny ny a, -ny)
	float w = ny * ny;
	w = w * a;
	const float u[3] = {b, s + w, -ny};
	float origin[3];
	for (int c = 0; c < 3; ++c)
	{
		const float off = bias * n[c];
		origin[c] = p[c] + off;
	}
	uint64_t mask = 0;
	for (int k = 0; k < 64; ++k)
	{
		float dir[3];
		for (int c = 0; c < 3; ++c)
		{
			const float m0 = t[c] * k_table[k][0];
			const float m1 = u[c] * k_table[k][1];
			const float m2 = n[c] * k_table[k][2];
			const float s01 = m0 + m1;
			dir[c] = s01 + m2;
		}
		uint32_t rec[HIT_WORDS];
		e->rays(F, float3(origin[0], origin[1], origin[2]), float3(dir[0], dir[1], dir[2]), real(radius), no_offset, no_offset, rec);
		if (rec[10] == 1u) mask |= (uint64_t)1 << k;
	}
	out[0] = (uint32_t)(mask & 0xffffffffu);
	out[1] = (uint32_t)(mask >> 32);
	out[2] = (uint32_t)__builtin_popcountll(mask);
	out[3] = 1u;
}

} // namespace

extern "C" {

int oo_points(const char *scene, const orc_frame *f, int n, const float *points, const float *normals, float bias, float radius, uint32_t *out)
{
	const Entry *e = find(scene);
	if (!e) return -1;
	const Frame F = enter_frame(*f);
	parallel_items(64 * n, [&](int a, int b) { // (over rays: an item is 64 of them)
		for (int i = (a + 63) / 64; i < (b + 63) / 64; ++i) occlusion_item(e, F, points + 3 * i, normals + 3 * i, bias, radius, out + 4 * i);
	});
	return 0;
}

// items from hit records [n][12]: pos and normal where hit == 1, else valid = hit (anything but 0: -1)
int oo_hits(const char *scene, const orc_frame *f, int n, const uint32_t *hits, float bias, float radius, uint32_t *out)
{
	const Entry *e = find(scene);
	if (!e) return -1;
	const Frame F = enter_frame(*f);
	parallel_items(64 * n, [&](int a, int b) {
		for (int i = (a + 63) / 64; i < (b + 63) / 64; ++i)
		{
			const uint32_t *h = hits + 12 * i;
			if (h[10] != 1u)
			{
				out[4 * i] = out[4 * i + 1] = out[4 * i + 2] = 0u;
				out[4 * i + 3] = h[10] == 0u ? 0u : 0xffffffffu;
				continue;
			}
			float p[3], nr[3];
			memcpy(p, h + 2, 12);
			memcpy(nr, h + 5, 12);
			occlusion_item(e, F, p, nr, bias, radius, out + 4 * i);
		}
	});
	return 0;
}

void oo_directions(float *out) { memcpy(out, k_table, sizeof k_table); }

} // extern "C"

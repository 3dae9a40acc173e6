// tests/cpp/atlas_oracle.cpp -- TEST-ONLY: the texture atlas of a mesh as include/sdfr.h defines it ("a texture atlas of an extracted
// mesh"), written from that text alone and sharing no line with the library: the layout, the UVs and the map texel -> (state, P, N).
// Plain loops over quads and texels, divisions and remainders where the library shifts, std::fmaf / sqrtf / 1.0f / x; built with the
// tests' flags (-ffp-contract=off: nothing fuses that is not written as an fma).  The records of the texels come from the surface and
// lighting oracles applied to these P, N (tests/atlas_util.py).
#include <cmath>
#include <cstdint>

namespace {

struct Layout
{
	int64_t triangles, quads, tiles_per_row, rows;
	int tile, width, height;
};

bool layout(int64_t triangles, int tile, int width, Layout &L)
{
	if (tile != 4 && tile != 8 && tile != 16 && tile != 32) return false;
	if (width <= 0 || width > 16384 || width % 8 || width % tile) return false;
	if (triangles < 0 || triangles % 2) return false;
	L.triangles = triangles;
	L.quads = triangles / 2;
	L.tile = tile;
	L.width = width;
	L.tiles_per_row = width / tile;
	L.rows = L.quads / L.tiles_per_row + (L.quads % L.tiles_per_row ? 1 : 0);
	int64_t h = L.rows * tile;
	while (h % 8) ++h;
	if (h < 8) h = 8;
	if ((int64_t)width * h > ((int64_t)1 << 30)) return false; // the renderer's frame sizes: width * height <= 2^30
	L.height = (int)h;
	return true;
}

bool finite3(const float v[3]) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

} // namespace

extern "C" {

// out: triangles, quads, tile, width, height, tiles_per_row, rows; -1: no such atlas
int ao_layout(int64_t triangles, int tile, int width, int64_t out[7])
{
	Layout L;
	if (!layout(triangles, tile, width, L)) return -1;
	out[0] = L.triangles;
	out[1] = L.quads;
	out[2] = L.tile;
	out[3] = L.width;
	out[4] = L.height;
	out[5] = L.tiles_per_row;
	out[6] = L.rows;
	return 0;
}

// uvs [triangles][3][2]
int ao_uvs(int64_t triangles, int tile, int width, float *uvs)
{
	Layout L;
	if (!layout(triangles, tile, width, L)) return -1;
	// the quad's corners q0 .. q3 in texels of the tile, and which of them each triangle's corners are
	const int cx[4] = {0, tile - 1, tile - 1, 0}, cy[4] = {0, 0, tile - 1, tile - 1};
	const int of_triangle[2][3] = {{0, 1, 2}, {0, 2, 3}};
	for (int64_t t = 0; t < triangles; ++t)
	{
		const int64_t q = t / 2;
		const int64_t col = q % L.tiles_per_row, row = q / L.tiles_per_row;
		for (int c = 0; c < 3; ++c)
		{
			const int k = of_triangle[t % 2][c];
			const int x = (int)col * tile + cx[k], y = (int)row * tile + cy[k];
			uvs[(t * 3 + c) * 2 + 0] = ((float)x + 0.5f) / (float)L.width;
			uvs[(t * 3 + c) * 2 + 1] = ((float)y + 0.5f) / (float)L.height;
		}
	}
	return 0;
}

// P, N [H * W][3], valid [H * W]: 1, 0 degenerate, -1 invalid; zeros unless 1
int ao_texels(int64_t triangles, int tile, int width, int64_t vertex_count, const float *positions, const float *normals, const uint32_t *idx, float *P,
	float *N, int32_t *valid)
{
	Layout L;
	if (!layout(triangles, tile, width, L)) return -1;
	for (int y = 0; y < L.height; ++y)
		for (int x = 0; x < L.width; ++x)
		{
			const int64_t item = (int64_t)y * L.width + x;
			for (int c = 0; c < 3; ++c) P[3 * item + c] = N[3 * item + c] = 0.f;
			valid[item] = -1;
			const int64_t col = x / tile, row = y / tile;
			if (row >= L.rows) continue;
			const int64_t q = row * L.tiles_per_row + col;
			if (q >= L.quads) continue;
			const uint32_t *t0 = idx + 3 * (2 * q), *t1 = idx + 3 * (2 * q + 1);
			const uint32_t i[4] = {t0[0], t0[1], t0[2], t1[2]};
			if (t1[0] != i[0] || t1[1] != i[2]) continue;
			if (i[0] >= vertex_count || i[1] >= vertex_count || i[2] >= vertex_count || i[3] >= vertex_count) continue;
			valid[item] = 0;
			const int a = x % tile, b = y % tile;
			const float u = (float)a / (float)(tile - 1), v = (float)b / (float)(tile - 1);
			float X[2][3];
			const float *arrays[2] = {positions, normals};
			for (int w = 0; w < 2; ++w)
				for (int c = 0; c < 3; ++c)
				{
					const float A0 = arrays[w][3 * (int64_t)i[0] + c], A1 = arrays[w][3 * (int64_t)i[1] + c], A2 = arrays[w][3 * (int64_t)i[2] + c],
								A3 = arrays[w][3 * (int64_t)i[3] + c];
					if (u >= v)
					{
						const float e = A1 - A0, f = A2 - A1;
						const float ue = u * e, vf = v * f;
						const float s = A0 + ue;
						X[w][c] = s + vf;
					}
					else
					{
						const float e = A3 - A0, f = A2 - A3;
						const float ve = v * e, uf = u * f;
						const float s = A0 + ve;
						X[w][c] = s + uf;
					}
				}
			const float *M = X[1];
			if (!finite3(X[0]) || !finite3(M)) continue;
			if (M[0] == 0.f && M[1] == 0.f && M[2] == 0.f) continue;
			const float xx = M[0] * M[0];
			const float r = 1.0f / sqrtf(std::fmaf(M[2], M[2], std::fmaf(M[1], M[1], xx)));
			const float unit[3] = {M[0] * r, M[1] * r, M[2] * r};
			if (!finite3(unit)) continue;
			valid[item] = 1;
			for (int c = 0; c < 3; ++c)
			{
				P[3 * item + c] = X[0][c];
				N[3 * item + c] = unit[c];
			}
		}
	return 0;
}

} // extern "C"

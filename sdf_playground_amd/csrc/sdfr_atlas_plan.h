// sdfr_atlas_plan.h -- the texture atlas of an extracted mesh (sdfr_atlas_layout, sdfr_atlas_uvs, sdfr_atlas_texels, sdfr_atlas_bake in
// include/sdfr.h) as far as the host decides it: the layout of one square tile of texels per quad, the UVs, and the plan of one call --
// the argument checks in the order their errors win, the kernel's arguments, the staging sizes of a host call, the launch.  Plain host
// arithmetic, no HIP call, like sdfr_query_plan.h: sdfr_api.cpp carries the plan out, tests/test_atlas_cpu.py checks it on a machine
// without a GPU.
#pragma once
#include "sdfr_query_plan.h"

namespace sdfr {

// sdfr_atlas (include/sdfr.h), field for field
struct AtlasLayout
{
	int64_t triangles, quads;
	int32_t tile, width, height, tiles_per_row, rows, reserved;
};
enum { ATLAS_MAX_WIDTH = 16384 };

inline int atlas_tile_log2(int tile) { return tile == 4 ? 2 : tile == 8 ? 3 : tile == 16 ? 4 : tile == 32 ? 5 : -1; }

// false: the arguments allow no atlas (SDFR_ERR_INVALID_ARGUMENT); `out` is then untouched
inline bool atlas_layout(int64_t triangles, int tile, int width, AtlasLayout &out)
{
	if (atlas_tile_log2(tile) < 0) return false;
	if (width < 8 || width > ATLAS_MAX_WIDTH || width % 8 != 0 || width % tile != 0) return false;
	if (triangles < 0 || triangles % 2 != 0) return false;
	const int64_t quads = triangles / 2, tiles_per_row = width / tile;
	const int64_t rows = (quads + tiles_per_row - 1) / tiles_per_row;
	int64_t height = (rows * tile + 7) / 8 * 8;
	if (height < 8) height = 8;
	if (height > ((int64_t)1 << 30) || !frame_size_ok(width, (int)height)) return false;
	out.triangles = triangles;
	out.quads = quads;
	out.tile = tile;
	out.width = width;
	out.height = (int32_t)height;
	out.tiles_per_row = (int32_t)tiles_per_row;
	out.rows = (int32_t)rows;
	out.reserved = 0;
	return true;
}

// whether `a` is what atlas_layout makes of its own triangles, tile and width
inline bool atlas_layout_ok(const AtlasLayout &a)
{
	AtlasLayout b;
	if (!atlas_layout(a.triangles, a.tile, a.width, b)) return false;
	return a.quads == b.quads && a.height == b.height && a.tiles_per_row == b.tiles_per_row && a.rows == b.rows && a.reserved == 0;
}

// uvs [triangles][3][2]: the corner of a triangle that is its quad's corner k (q0 .. q3) lies on the centre of the tile's corner texel
// k -- (0, 0), (T - 1, 0), (T - 1, T - 1), (0, T - 1) --, origin top-left; triangle 2q is (q0, q1, q2), triangle 2q + 1 (q0, q2, q3)
inline void atlas_uvs(const AtlasLayout &a, float *uvs)
{
	static const int corner[2][3] = {{0, 1, 2}, {0, 2, 3}};
	const float W = (float)a.width, H = (float)a.height;
	for (int64_t q = 0; q < a.quads; ++q)
	{
		const int x0 = (int)(q % a.tiles_per_row) * a.tile, y0 = (int)(q / a.tiles_per_row) * a.tile;
		for (int t = 0; t < 2; ++t)
			for (int c = 0; c < 3; ++c)
			{
				const int k = corner[t][c];
				const int x = x0 + (k == 1 || k == 2 ? a.tile - 1 : 0), y = y0 + (k >= 2 ? a.tile - 1 : 0);
				float *uv = uvs + ((2 * q + t) * 3 + c) * 2;
				uv[0] = ((float)x + 0.5f) / W;
				uv[1] = ((float)y + 0.5f) / H;
			}
	}
}

// What an entry point asks for: the atlas, the mesh and the arrays as the caller gave them in a.* (a.reach and a.layers of a bake)
struct AtlasRequest
{
	const AtlasLayout *atlas;
	int64_t vertex_count;
	AtlasArgs a;
	bool bake; // sdfr_atlas_bake; else sdfr_atlas_texels
	int on_host;
};
// the arrays of a call in the order a host call stages them, as the pointer of AtlasArgs each goes through: three inputs, then the
// answers of the texels [0] or of a bake [1]
enum { ATLAS_STAGE_INPUTS = 3, ATLAS_STAGE_PIECES = 7 };
#define SDFR_A(member) offsetof(AtlasArgs, member)
static const size_t k_atlas_stage_slots[2][ATLAS_STAGE_PIECES] = {
	{SDFR_A(positions), SDFR_A(normals), SDFR_A(indices), SDFR_A(texel_positions), SDFR_A(texel_normals), SDFR_A(valid), SDFR_A(valid) /* no bytes */},
	{SDFR_A(positions), SDFR_A(normals), SDFR_A(indices), SDFR_A(albedo), SDFR_A(normal), SDFR_A(lit), SDFR_A(valid)}};
#undef SDFR_A
struct AtlasPlan
{
	int status; // QUERY_PLAN_*
	const char *error;
	AtlasArgs a;     // for the caller's arrays as device memory; a host call points them at its staging pieces
	bool needs_scene; // a bake of at least one quad; everything else runs without one
	size_t bytes[ATLAS_STAGE_PIECES]; // of the arrays of k_atlas_stage_slots[bake]; an array that is not there, and the texels' seventh: 0
	uint32_t blocks; // of QUERY_BLOCK_ITEMS threads: one per 8 x 8 square of the image (QUERY_GRID_BLOCK_PER_TILE)
};

// The checks after the handle's and before the scene's, in the order their errors win.
inline AtlasPlan plan_atlas(const AtlasRequest &c)
{
	AtlasPlan p = {};
	auto fail = [&p](const char *text) {
		p.status = QUERY_PLAN_INVALID_ARGUMENT;
		p.error = text;
		return p;
	};
	if (!c.atlas || !atlas_layout_ok(*c.atlas)) return fail("bad atlas");
	const AtlasLayout &L = *c.atlas;
	if (c.vertex_count < 0 || c.vertex_count > (int64_t)INT32_MAX) return fail("bad vertex count");
	if (!is_flag(c.on_host)) return fail("on_host must be 0 or 1");
	if (c.bake)
	{
		if (!(std::isfinite(c.a.reach) && c.a.reach > 0.f)) return fail("reach must be finite and > 0");
		if (c.a.layers == 0u || (c.a.layers & ~(uint32_t)ATLAS_LAYERS) != 0u) return fail("bad layers");
	}
	if (L.quads > 0 && !c.a.indices) return fail("null pointer");
	if (L.quads > 0 && c.vertex_count > 0 && (!c.a.positions || !c.a.normals)) return fail("null pointer");
	if (!c.a.valid) return fail("null pointer");
	if (c.bake)
	{
		if (((c.a.layers & ATLAS_ALBEDO) && !c.a.albedo) || ((c.a.layers & ATLAS_NORMAL) && !c.a.normal) || ((c.a.layers & ATLAS_LIT) && !c.a.lit))
			return fail("null pointer");
	}
	else if (!c.a.texel_positions || !c.a.texel_normals)
		return fail("null pointer");

	const size_t texels = (size_t)L.width * (size_t)L.height, V = L.quads > 0 ? (size_t)c.vertex_count : 0;
	p.a = c.a;
	p.a.vertex_count = (uint32_t)V;
	p.a.quads = (uint32_t)L.quads; // (<= 2^30 / 16 tiles)
	p.a.tile_log2 = atlas_tile_log2(L.tile);
	p.a.tiles_per_row = L.tiles_per_row;
	p.a.width = L.width;
	p.a.height = L.height;
	if (c.bake)
	{
		if (!(p.a.layers & ATLAS_ALBEDO)) p.a.albedo = nullptr;
		if (!(p.a.layers & ATLAS_NORMAL)) p.a.normal = nullptr;
		if (!(p.a.layers & ATLAS_LIT)) p.a.lit = nullptr;
		p.a.texel_positions = p.a.texel_normals = nullptr;
	}
	else
	{
		p.a.albedo = p.a.normal = p.a.lit = nullptr;
		p.a.layers = 0u;
		p.a.reach = 0.f;
	}
	p.needs_scene = c.bake && L.quads > 0;
	p.bytes[0] = p.bytes[1] = V * 12;
	p.bytes[2] = (size_t)L.triangles * 12;
	if (c.bake)
	{
		p.bytes[3] = p.a.albedo ? texels * 16 : 0;
		p.bytes[4] = p.a.normal ? texels * 16 : 0;
		p.bytes[5] = p.a.lit ? texels * 16 : 0;
		p.bytes[6] = texels * 4;
	}
	else
	{
		p.bytes[3] = p.bytes[4] = texels * 12;
		p.bytes[5] = texels * 4;
		p.bytes[6] = 0;
	}
	p.blocks = ((uint32_t)L.width / QUERY_TILE) * ((uint32_t)L.height / QUERY_TILE);
	return p;
}

} // namespace sdfr

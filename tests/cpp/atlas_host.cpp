// tests/cpp/atlas_host.cpp -- TEST-ONLY: the library's texture atlas (sdf_playground_amd/csrc/sdfr_atlas_plan.h, sdfr_atlas.h) compiled for
// the CPU, as lighting_host.cpp compiles the lighting queries, so that the CPU test tier can compare it with the oracle's definition
// (atlas_oracle.cpp and the surface and lighting oracles) bit for bit without a GPU: the host plan as the API runs it, and the texel
// map and the bake as the kernels' lanes run them -- block by block, lane by lane, a tile's quad addressed per block from T = 8 on.
// Built once for the scenes compiled ahead of time, and once per run-time scene with -DSDFR_HLSL_SCENE_FILE="<generated file>".
// The product never loads this.
#include "sdfr_hostframe.h"
#include "sdfr_atlas.h"
#include "sdfr_atlas_plan.h"
#include "host_common.h"

namespace {

// one texel of a bake as the kernel's lane does it after the texel map
typedef uint32_t (*TexelFn)(const FrameU &, vec3, vec3, float, uint32_t, uint32_t *, uint32_t *, uint32_t *);
template <class Scene, bool DBG>
uint32_t texel_of(const FrameU &U, vec3 P, vec3 N, float reach, uint32_t layers, uint32_t *albedo, uint32_t *normal, uint32_t *lit)
{
	return atlas_bake_texel<Scene, DBG>(U, P, N, reach, layers, albedo, normal, lit);
}
// the family's function for a scene and a frame, the debug or the plain instantiation: what latch hands out
struct Pick
{
	template <class Scene>
	static TexelFn of(const FrameU &U)
	{
		return frame_needs_debug(U) ? &texel_of<Scene, true> : &texel_of<Scene, false>;
	}
};

// the lanes of block `block` as the kernels map them; fn(x, y, state, P, N)
template <class F>
void block_texels(const AtlasArgs &g, uint32_t block, F fn)
{
	const uint32_t blocks_x = (uint32_t)g.width >> 3;
	const uint32_t by = block / blocks_x, bx = block - by * blocks_x;
	const uint32_t T = 1u << g.tile_log2;
	AtlasQuad uniform;
	if (g.tile_log2 >= 3) uniform = atlas_load_quad(g, atlas_tile_of(g, bx * 8u, by * 8u));
	for (uint32_t lane = 0; lane < 64u; ++lane)
	{
		const uint32_t x = bx * 8u + (lane & 7u), y = by * 8u + (lane >> 3);
		const AtlasQuad Q = g.tile_log2 >= 3 ? uniform : atlas_load_quad(g, atlas_tile_of(g, x, y));
		vec3 P, N;
		const int state = atlas_texel(Q, x & (T - 1u), y & (T - 1u), T, P, N);
		fn(x, y, state, P, N);
	}
}

} // namespace

extern "C" {

// out: triangles, quads, tile, width, height, tiles_per_row, rows; -1: no such atlas
int ah_layout(int64_t triangles, int tile, int width, int64_t out[7])
{
	AtlasLayout L;
	if (!atlas_layout(triangles, tile, width, L) || !atlas_layout_ok(L)) return -1;
	out[0] = L.triangles;
	out[1] = L.quads;
	out[2] = L.tile;
	out[3] = L.width;
	out[4] = L.height;
	out[5] = L.tiles_per_row;
	out[6] = L.rows;
	return 0;
}

int ah_uvs(int64_t triangles, int tile, int width, float *uvs)
{
	AtlasLayout L;
	if (!atlas_layout(triangles, tile, width, L)) return -1;
	atlas_uvs(L, uvs);
	return 0;
}

// The plan of a call as the API makes it.  have: bit k set = the caller gave array k of (positions, normals, indices, albedo / texel
// positions, normal / texel normals, lit, valid); the pointers themselves are never followed.  layout_damage: what is added to the
// atlas' height after the layout was made (an atlas sdfr_atlas_layout did not make).  -> status; bytes[7], blocks and needs_scene of a plan that stands
int ah_plan(int64_t triangles, int tile, int width, int layout_damage, int have_atlas, int64_t vertex_count, int bake, float reach, uint32_t layers, int have, int on_host,
	uint64_t bytes[7], uint32_t *blocks, int *needs_scene, char error[64])
{
	static float dummy[4];
	AtlasLayout L = {};
	if (!atlas_layout(triangles, tile, width, L)) L.tile = 3;
	L.height += layout_damage;
	void *p[7];
	for (int k = 0; k < 7; ++k) p[k] = (have >> k) & 1 ? dummy : nullptr;
	AtlasRequest c = {};
	c.atlas = have_atlas ? &L : nullptr;
	c.vertex_count = vertex_count;
	c.a.positions = (const float *)p[0];
	c.a.normals = (const float *)p[1];
	c.a.indices = (const uint32_t *)p[2];
	if (bake)
	{
		c.a.albedo = (float *)p[3];
		c.a.normal = (float *)p[4];
		c.a.lit = (float *)p[5];
	}
	else
	{
		c.a.texel_positions = (float *)p[3];
		c.a.texel_normals = (float *)p[4];
	}
	c.a.valid = (int32_t *)p[6];
	c.a.reach = reach;
	c.a.layers = layers;
	c.bake = bake != 0;
	c.on_host = on_host;
	const AtlasPlan plan = plan_atlas(c);
	error[0] = 0;
	if (plan.error) strncpy(error, plan.error, 63), error[63] = 0;
	if (plan.status != QUERY_PLAN_OK) return plan.status;
	for (int k = 0; k < 7; ++k) bytes[k] = plan.bytes[k];
	*blocks = plan.blocks;
	*needs_scene = plan.needs_scene ? 1 : 0;
	return 0;
}

static bool args_of(int64_t triangles, int tile, int width, int64_t vertex_count, const float *positions, const float *normals, const uint32_t *indices, AtlasArgs &g)
{
	AtlasLayout L;
	if (!atlas_layout(triangles, tile, width, L)) return false;
	g = AtlasArgs();
	g.positions = positions;
	g.normals = normals;
	g.indices = indices;
	g.vertex_count = (uint32_t)vertex_count;
	g.quads = (uint32_t)L.quads;
	g.tile_log2 = atlas_tile_log2(tile);
	g.tiles_per_row = L.tiles_per_row;
	g.width = L.width;
	g.height = L.height;
	return true;
}

// P, N [H * W][3], valid [H * W]
int ah_texels(int64_t triangles, int tile, int width, int64_t vertex_count, const float *positions, const float *normals, const uint32_t *indices, float *P,
	float *N, int32_t *valid)
{
	AtlasArgs g;
	if (!args_of(triangles, tile, width, vertex_count, positions, normals, indices, g)) return -1;
	const int blocks = (g.width / 8) * (g.height / 8);
	parallel_items(blocks, 16, [&](int lo, int hi) {
		for (int b = lo; b < hi; ++b)
			block_texels(g, (uint32_t)b, [&](uint32_t x, uint32_t y, int state, vec3 p, vec3 n) {
				const size_t i = (size_t)y * (size_t)g.width + x;
				valid[i] = state;
				P[3 * i] = p.x, P[3 * i + 1] = p.y, P[3 * i + 2] = p.z;
				N[3 * i] = n.x, N[3 * i + 1] = n.y, N[3 * i + 2] = n.z;
			});
	});
	return 0;
}

// `frame`: the inputs of a FrameU (tests/hostsim frame_from_oracle).  albedo, normal, lit: [H * W][4] words each, or null; valid [H * W]
int ah_bake(const char *scene, const FrameU *frame, int64_t triangles, int tile, int width, int64_t vertex_count, const float *positions, const float *normals,
	const uint32_t *indices, float reach, uint32_t layers, uint32_t *albedo, uint32_t *normal, uint32_t *lit, int32_t *valid)
{
	FrameU U;
	TexelFn f;
	if (!latch<Pick>(scene, frame, U, f)) return -1;
	AtlasArgs g;
	if (!args_of(triangles, tile, width, vertex_count, positions, normals, indices, g)) return -1;
	const int blocks = (g.width / 8) * (g.height / 8);
	parallel_items(blocks, 16, [&](int lo, int hi) {
		for (int b = lo; b < hi; ++b)
			block_texels(g, (uint32_t)b, [&](uint32_t x, uint32_t y, int state, vec3 p, vec3 n) {
				const size_t i = (size_t)y * (size_t)g.width + x;
				uint32_t pa[4] = {0u, 0u, 0u, 0u}, pn[4] = {0u, 0u, 0u, 0u}, pl[4] = {0u, 0u, 0u, 0u};
				uint32_t v = (uint32_t)state;
				if (state == ATLAS_TEXEL_VALID) v = f(U, p, n, reach, layers, pa, pn, pl);
				if (albedo) memcpy(albedo + 4 * i, pa, sizeof pa);
				if (normal) memcpy(normal + 4 * i, pn, sizeof pn);
				if (lit) memcpy(lit + 4 * i, pl, sizeof pl);
				valid[i] = (int32_t)v;
			});
	});
	return 0;
}
int ah_frame_size() { return (int)sizeof(FrameU); }

} // extern "C"

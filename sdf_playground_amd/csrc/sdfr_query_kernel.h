// sdfr_query_kernel.h -- the query kernels (sdfr_query.h), one lane per item (the occlusion kernel: one wave per item).  Shared by the kernels compiled ahead of time
// (sdfr_query_scene.hip, a translation unit of its own so that the pixel kernels' code does not change) and by the query
// module sdfr_jit.cpp builds for a scene compiled at run time.  Device compilation only.
//
// Items are read as float3 / int2 records of consecutive lanes (coalesced), results leave as 16-byte stores; launched with
// the scene's own launch attributes (SDFR_PIXEL_KERNEL_ATTRS), in blocks of SDFR_PIXEL_BLOCK lanes.
#pragma once
#include "sdfr_pixel_kernel.h"
#include "sdfr_query.h"
#include "sdfr_surface.h"
#include "sdfr_occlusion.h"
#include "sdfr_lighting.h"
#include "sdfr_atlas.h"
#include "sdfr_mesh_sharp.h"
#include "sdfr_slice.h"
#include "sdfr_span.h"
#include "sdfr_measure.h"

namespace sdfr {

// item i's record of three floats; the offset is 64-bit: 3 * i wraps in 32 bits from i = 2^32 / 3 on, well below INT32_MAX items
SDF_HD vec3 query_load3(const float *__restrict__ p, uint32_t i)
{
	const float *r = p + (size_t)3 * i;
	return V3(r[0], r[1], r[2]);
}

// item i's record of WORDS words (a multiple of 4) leaves from registers: 16-byte stores into an array aligned to 16 bytes, word
// stores into any other (sdfr_hit and sdfr_surface themselves only ask for 4-byte alignment)
template <int WORDS>
__device__ __forceinline__ void query_store(uint32_t *__restrict__ base, uint32_t i, const uint32_t (&rec)[WORDS])
{
	static_assert(WORDS % 4 == 0, "whole 16-byte stores");
	uint32_t *out = base + (size_t)WORDS * i;
	if ((reinterpret_cast<size_t>(base) & 15u) == 0u)
	{
		uint4 *dst = reinterpret_cast<uint4 *>(out);
#pragma unroll
		for (int k = 0; k < WORDS / 4; ++k) dst[k] = make_uint4(rec[4 * k], rec[4 * k + 1], rec[4 * k + 2], rec[4 * k + 3]);
	}
	else
	{
#pragma unroll
		for (int k = 0; k < WORDS; ++k) out[k] = rec[k];
	}
}

template <class Scene, bool DBG>
__device__ __forceinline__ void query_points_kernel(const SceneKernelArgs<QueryArgs> &a)
{
	const FrameU &U = a.U;
	const QueryArgs &q = a.a;
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
__device__ __forceinline__ void query_rays_kernel(const SceneKernelArgs<QueryArgs> &a)
{
	const FrameU &U = a.U;
	const QueryArgs &q = a.a;
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
	query_store(q.hits, i, rec); // 48-byte records: three 16-byte stores
}

// The surface queries (sdfr_surface.h): rays, picks, a whole frame or the rays towards a mesh's vertices -> `surfaces`, and `hits`
// unless null.  One wave per block.  A frame's wave takes an 8 x 8 tile of pixels, as the pixel kernel's does, so that the scenes'
// wave-level branches stay as coherent as in a render; lanes past the frame's ragged right and bottom edges leave.  Every other
// kind maps 64 consecutive items.  A record is one whole 128-byte line per lane, built in registers and written by eight 16-byte stores.
template <class Scene, bool DBG>
__device__ __forceinline__ void query_surfaces_kernel(const SceneKernelArgs<QueryArgs> &a)
{
	static_assert(SDFR_PIXEL_BLOCK == 64, "one wave per block: a tile is 64 pixels");
	const FrameU &U = a.U;
	const QueryArgs &q = a.a;
	const uint32_t lane = threadIdx.x;
	uint32_t i;
	QueryRay ray;
	bool in_frame = true;
	if (q.kind == QUERY_FRAME)
	{
		const uint32_t tiles_x = ((uint32_t)U.width + 7u) >> 3;
		const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
		const uint32_t px = tx * 8u + (lane & 7u), py = ty * 8u + (lane >> 3);
		if (px >= (uint32_t)U.width || py >= (uint32_t)U.height) return;
		i = py * (uint32_t)U.width + px; // < width * height <= 2^30
		in_frame = query_pixel_ray(U, (int)px, (int)py, ray);
	}
	else
	{
		i = blockIdx.x * 64u + lane;
		if (i >= (uint32_t)q.n) return;
		if (q.kind == QUERY_PICK)
			in_frame = query_pixel_ray(U, q.pixels[(size_t)2 * i], q.pixels[(size_t)2 * i + 1], ray);
		else if (q.kind == QUERY_MESH)
			ray = query_mesh_ray(query_load3(q.pos, i), query_load3(q.dir, i), q.reach);
		else
			ray = query_plain_ray(query_load3(q.pos, i), query_load3(q.dir, i), q.dist_max);
	}
	uint32_t hit[QUERY_HIT_WORDS], rec[QUERY_SURFACE_WORDS];
	query_surface<Scene, DBG>(U, ray, in_frame, hit, rec);
	if (q.hits) query_store(q.hits, i, hit);
	query_store(q.surfaces, i, rec);
}

// The lighting queries (sdfr_lighting.h): the surface kernel's items, mapped to lanes the same way (the lines are repeated, not shared:
// a helper of both changed the surface kernel's code) -> `lighting`, `hits` unless null, and unless `lights` is null the eight
// light samples of the item.  One lane per item: the primary ray is marched once, and the lane loops over the light slots and follows
// each shadow chain itself -- a lane per (item, light) would march the primary ray eight times, (P + S) / 8 per item against
// (P + 8 S) / 64.  A sample leaves as soon as its slot is done (five 16-byte stores, or 20 words), so that no lane holds eight of them.
struct LightSampleStore
{
	uint32_t *item; // the item's eight samples, or null
	bool aligned;
	__device__ __forceinline__ bool wanted() const { return item != nullptr; }
	__device__ __forceinline__ void operator()(int slot, const uint32_t (&s)[QUERY_LIGHT_SAMPLE_WORDS]) const
	{
		uint32_t *out = item + QUERY_LIGHT_SAMPLE_WORDS * slot;
		if (aligned)
		{
			uint4 *dst = reinterpret_cast<uint4 *>(out);
#pragma unroll
			for (int k = 0; k < QUERY_LIGHT_SAMPLE_WORDS / 4; ++k) dst[k] = make_uint4(s[4 * k], s[4 * k + 1], s[4 * k + 2], s[4 * k + 3]);
		}
		else
		{
#pragma unroll
			for (int k = 0; k < QUERY_LIGHT_SAMPLE_WORDS; ++k) out[k] = s[k];
		}
	}
};
template <class Scene, bool DBG>
__device__ __forceinline__ void query_lighting_kernel(const SceneKernelArgs<QueryArgs> &a)
{
	static_assert(QUERY_LIGHT_SLOTS == SDFR_MAX_LIGHTS && QUERY_LIGHT_SAMPLE_WORDS % 4 == 0, "eight samples of whole 16-byte pieces per item");
	static_assert(SDFR_PIXEL_BLOCK == 64, "one wave per block: a tile is 64 pixels");
	const FrameU &U = a.U;
	const QueryArgs &q = a.a;
	const uint32_t lane = threadIdx.x;
	uint32_t i;
	QueryRay ray;
	bool in_frame = true;
	if (q.kind == QUERY_FRAME)
	{
		const uint32_t tiles_x = ((uint32_t)U.width + 7u) >> 3;
		const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
		const uint32_t px = tx * 8u + (lane & 7u), py = ty * 8u + (lane >> 3);
		if (px >= (uint32_t)U.width || py >= (uint32_t)U.height) return;
		i = py * (uint32_t)U.width + px; // < width * height <= 2^30
		in_frame = query_pixel_ray(U, (int)px, (int)py, ray);
	}
	else
	{
		i = blockIdx.x * 64u + lane;
		if (i >= (uint32_t)q.n) return;
		if (q.kind == QUERY_PICK)
			in_frame = query_pixel_ray(U, q.pixels[(size_t)2 * i], q.pixels[(size_t)2 * i + 1], ray);
		else if (q.kind == QUERY_MESH)
			ray = query_mesh_ray(query_load3(q.pos, i), query_load3(q.dir, i), q.reach);
		else
			ray = query_plain_ray(query_load3(q.pos, i), query_load3(q.dir, i), q.dist_max);
	}
	LightSampleStore samples;
	samples.item = q.lights ? q.lights + (size_t)(QUERY_LIGHT_SLOTS * QUERY_LIGHT_SAMPLE_WORDS) * i : nullptr; // (n * 640 bytes: 64-bit)
	samples.aligned = (reinterpret_cast<size_t>(q.lights) & 15u) == 0u;
	uint32_t hit[QUERY_HIT_WORDS], rec[QUERY_LIGHTING_WORDS];
	query_lighting<Scene, DBG>(U, ray, in_frame, hit, rec, samples);
	if (q.hits) query_store(q.hits, i, hit);
	query_store(q.lighting, i, rec);
}

// The occlusion queries (sdfr_occlusion.h): one wave per block, one block per item, lane k marches direction k.  The item -- a point
// and a normal, or a hit record -- is addressed by the block index alone, so it is read once for the wave (scalar loads); an item
// without an answer is written by one lane and the whole wave leaves.  All 64 rays start at one origin, so the scenes' wave-level
// branches start coherent; a lane whose ray has ended waits for the slowest and does nothing else: neither the normal nor the
// material of a hit is computed.  The mask is one ballot of the hit flags, and one lane writes the 16-byte record.
template <class Scene, bool DBG>
__device__ __forceinline__ void query_occlusion_kernel(const SceneKernelArgs<QueryArgs> &a)
{
	static_assert(SDFR_PIXEL_BLOCK == 64 && OCCLUSION_DIRS == 64, "one wave per block, one lane per direction");
	const FrameU &U = a.U;
	const QueryArgs &q = a.a;
	const uint32_t i = blockIdx.x, lane = threadIdx.x; // (launch_query: q.n blocks)
	vec3 p, n;
	uint32_t valid = 1u;
	if (q.kind == QUERY_HIT_OCCLUSION)
	{
		const uint32_t *h = q.hit_items + (size_t)QUERY_HIT_WORDS * i;
		valid = occlusion_hit_valid(h[10]);
		p = V3(bits_f32(h[2]), bits_f32(h[3]), bits_f32(h[4]));
		n = V3(bits_f32(h[5]), bits_f32(h[6]), bits_f32(h[7]));
	}
	else
	{
		p = query_load3(q.pos, i);
		n = query_load3(q.dir, i);
	}
	if (valid == 1u && !occlusion_item_ok(p, n)) valid = 0u;
	uint32_t rec[QUERY_OCCLUSION_WORDS];
	if (valid != 1u)
	{
		occlusion_none(valid, rec);
		if (lane == 0u) query_store(q.occlusion, i, rec);
		return;
	}
	const bool hit = occlusion_ray_hits<Scene, DBG>(U, p, n, q.bias, q.dist_max, lane);
	const uint64_t mask = __ballot(hit);
	occlusion_record(mask, (uint32_t)__popcll(mask), rec);
	if (lane == 0u) query_store(q.occlusion, i, rec);
}

// The distance query over a lattice (LatticeArgs): one wave per block, one point per lane.  A wave owns a 4 x 4 x 4 brick of points,
// so that its lanes stay within 3 cells of each other and the scenes' wave-level branches (bounding volumes, cell lookups) stay
// coherent; its stores are runs of 4 floats.  rows = 1 maps 64 consecutive points of the linear index instead (coalesced stores,
// a wave 64 cells long).  Lanes past the lattice's ragged edges leave.
template <class Scene, bool DBG>
__device__ __forceinline__ void query_lattice_kernel(const SceneKernelArgs<LatticeArgs> &a)
{
	static_assert(SDFR_PIXEL_BLOCK == 64, "one wave per block: a brick is 64 points");
	const LatticeArgs &g = a.a;
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

// The atlas bake (sdfr_atlas.h): one wave per block, one texel per lane; a wave takes an 8 x 8 square of the IMAGE -- one quad's tile at
// T = 8, four at T = 4, part of one at T = 16 and 32.  Each lane makes its texel's ray from the mesh arrays: from a tile of 8 texels
// and more the quad is addressed by the block index alone, so its six indices and four vertices are read once for the wave (scalar
// loads); at T = 4 a lane addresses its own.  A texel that is invalid or degenerate is not marched.  Every plane that is asked for
// leaves as one 16-byte store per lane -- a wave's row of 8 texels is 128 contiguous bytes -- and `valid` as one word, at every texel
// of the image.  Nothing here is shared with the kernels above: their code stays as it was.
template <class Scene, bool DBG>
__device__ __forceinline__ void atlas_bake_kernel(const SceneKernelArgs<AtlasArgs> &a)
{
	static_assert(SDFR_PIXEL_BLOCK == 64, "one wave per block: 8 x 8 texels");
	const FrameU &U = a.U;
	const AtlasArgs &g = a.a;
	const uint32_t lane = threadIdx.x;
	const uint32_t blocks_x = (uint32_t)g.width >> 3;
	const uint32_t by = blockIdx.x / blocks_x, bx = blockIdx.x - by * blocks_x;
	const uint32_t x = bx * 8u + (lane & 7u), y = by * 8u + (lane >> 3);
	if (x >= (uint32_t)g.width || y >= (uint32_t)g.height) return; // (never: both are multiples of 8 and the grid covers them exactly)
	const uint32_t T = 1u << g.tile_log2;
	AtlasQuad Q;
	if (g.tile_log2 >= 3) Q = atlas_load_quad(g, atlas_tile_of(g, bx * 8u, by * 8u)); // wave-uniform
	else Q = atlas_load_quad(g, atlas_tile_of(g, x, y));
	vec3 P, N;
	const int state = atlas_texel(Q, x & (T - 1u), y & (T - 1u), T, P, N);
	uint32_t albedo[4] = {0u, 0u, 0u, 0u}, normal[4] = {0u, 0u, 0u, 0u}, lit[4] = {0u, 0u, 0u, 0u};
	uint32_t valid = (uint32_t)state;
	if (state == ATLAS_TEXEL_VALID) valid = atlas_bake_texel<Scene, DBG>(U, P, N, g.reach, g.layers, albedo, normal, lit);
	const uint32_t i = y * (uint32_t)g.width + x; // < width * height <= 2^30
	if (g.albedo) query_store(reinterpret_cast<uint32_t *>(g.albedo), i, albedo);
	if (g.normal) query_store(reinterpret_cast<uint32_t *>(g.normal), i, normal);
	if (g.lit) query_store(reinterpret_cast<uint32_t *>(g.lit), i, lit);
	g.valid[i] = (int32_t)valid;
}

// The sharp vertices of a mesh (sdfr_mesh_sharp.h; sdfr_mesh_extract_sharp): one wave per block, 16 lanes per vertex, so 4 vertices per
// wave.  Most cells of a grid are inactive, so the work is per vertex: sdfr_mesh.hip has left vertex v's cell index in word 3 * v of
// `positions`.  Lanes 0 .. 11 of a vertex own the cell's 12 edges: a lane whose edge crosses the surface makes its four bisection
// evaluations and the point query with its normal (a uniform trip count; the lanes without a crossing sit masked), then every lane of
// the group reads the twelve crossings in edge order through shuffles and sums them sequentially -- the bits of the sequential host
// code -- and lane 0 writes the vertex over the cell index.  A group reads and writes its own vertex's three words only.
// LANES = 1 (SDFR_MESH_SHARP_LANES, sdfr_query_args.h: a developer build, the A/B of DESIGN.md 4.12): a lane per vertex visits the 12
// edges itself, as the host code does.
template <class Scene, bool DBG>
struct MeshSharpScene
{
	const FrameU &U;
	__device__ __forceinline__ float distance(vec3 p) const { return query_point<Scene, DBG>(U, p, nullptr); }
	__device__ __forceinline__ float distance_normal(vec3 p, vec3 &n) const { return query_point<Scene, DBG>(U, p, &n); }
};
template <class Scene, bool DBG, int LANES = SDFR_MESH_SHARP_LANES>
__device__ __forceinline__ void mesh_sharp_kernel(const SceneKernelArgs<MeshSharpArgs> &a)
{
	static_assert(SDFR_PIXEL_BLOCK == 64 && (LANES == 16 || LANES == 1), "one wave per block: 4 vertices of 16 lanes, or 64 of one");
	const MeshSharpArgs &m = a.a;
	MeshGrid g;
	for (int k = 0; k < 3; ++k)
	{
		g.origin[k] = m.origin[k];
		g.n[k] = m.n[k];
	}
	g.cell = m.cell;
	g.iso = m.iso;
	const uint32_t lane = threadIdx.x, edge = lane & (uint32_t)(LANES - 1), base = lane - edge;
	const uint32_t v = blockIdx.x * (uint32_t)(64 / LANES) + lane / (uint32_t)LANES; // < 2^30 + 64
	const bool live = v < m.vertices;
	float *o = m.positions + (size_t)3 * (live ? v : 0u);
	uint32_t c = live ? f32_bits(o[0]) : 0u; // the cell's linear index, < 2^30 (read by every lane of the group before lane 0 writes)
	if (c >= mesh_cell_count(g)) c = 0u;     // (never: k_mesh_emit_cells wrote it)
	const uint32_t nx = (uint32_t)g.n[0], ny = (uint32_t)g.n[1];
	const uint32_t row = c / nx, ck = row / ny;
	const int i = (int)(c - row * nx), j = (int)(row - ck * ny), k = (int)ck;
	const MeshSharpScene<Scene, DBG> scene = {a.U};
	float x[3];
	if constexpr (LANES == 1)
	{
		if (!live) return;
		MeshSharpCrossing all[12];
		for (int e = 0; e < 12; ++e) mesh_sharp_crossing(g, m.lattice, scene, i, j, k, e, all[e]);
		mesh_sharp_vertex(g, i, j, k, [&all](int e) { return all[e]; }, x);
	}
	else
	{
		MeshSharpCrossing mine;
		mine.flags = 0u;
		mine.s = 0.f;
		for (int t = 0; t < 3; ++t) mine.p[t] = mine.n[t] = 0.f;
		if (live && edge < 12u) mesh_sharp_crossing(g, m.lattice, scene, i, j, k, (int)edge, mine);
		// (every lane of the wave is here again: the shuffles below read lanes of the reader's own group)
		mesh_sharp_vertex(g, i, j, k, [&](int e) {
			MeshSharpCrossing r;
			const int from = (int)base + e;
			for (int t = 0; t < 3; ++t)
			{
				r.p[t] = __shfl(mine.p[t], from, 64);
				r.n[t] = __shfl(mine.n[t], from, 64);
			}
			r.s = __shfl(mine.s, from, 64);
			r.flags = (uint32_t)__shfl((int)mine.flags, from, 64);
			return r;
		}, x);
	}
	if (live && edge == 0u)
	{
		o[0] = x[0];
		o[1] = x[1];
		o[2] = x[2];
	}
}

// The distance query over a stack of plane lattices (SliceArgs; sdfr_slice_extract): one wave per block, one point per lane.  A wave
// owns an 8 x 8 tile of points of ONE layer -- the layers may lie far apart, the points of a tile lie within 7 steps of each other --
// so that the scenes' wave-level branches stay coherent, as the 4 x 4 x 4 bricks do for the mesh; its stores are runs of 8 floats.
// The tile is addressed by the block index alone (scalar arithmetic).  rows = 1 maps 64 consecutive points of the linear index instead.
// Nothing is read but the kernel's arguments; every lane writes its own 4 bytes; lanes past a layer's ragged edges leave.
template <class Scene, bool DBG>
__device__ __forceinline__ void query_slices_kernel(const SceneKernelArgs<SliceArgs> &a)
{
	static_assert(SDFR_PIXEL_BLOCK == 64, "one wave per block: a tile is 64 points");
	const SliceArgs &g = a.a;
	const uint32_t pu = (uint32_t)g.pu, pv = (uint32_t)g.pv, layers = (uint32_t)g.layers, lane = threadIdx.x;
	uint32_t i, j, l;
	if (g.rows)
	{
		const uint32_t p = blockIdx.x * 64u + lane; // < 2^30 + 64
		const uint32_t row = p / pu;
		i = p - row * pu;
		l = row / pv;
		j = row - l * pv;
	}
	else
	{
		const uint32_t tu = (pu + 7u) >> 3, tv = (pv + 7u) >> 3;
		const uint32_t trow = blockIdx.x / tu;
		l = trow / tv;
		i = (blockIdx.x - trow * tu) * 8u + (lane & 7u);
		j = (trow - l * tv) * 8u + (lane >> 3);
	}
	if (i >= pu || j >= pv || l >= layers) return;
	const vec3 p = V3(slice_coord(g.origin, g.du, g.dv, g.dw, 0, (int)i, (int)j, (int)l), slice_coord(g.origin, g.du, g.dv, g.dw, 1, (int)i, (int)j, (int)l),
		slice_coord(g.origin, g.du, g.dv, g.dw, 2, (int)i, (int)j, (int)l));
	g.out[i + pu * (j + pv * l)] = query_point<Scene, DBG>(a.U, p, nullptr); // (the index is < 2^30)
}

// The span queries (sdfr_span.h; sdfr_query_ray_spans, sdfr_pick_spans, sdfr_mesh_spans): the surface kernel's items, mapped to lanes the
// same way (the lines are repeated, not shared, as in the lighting kernel) -> `summaries` and, unless max_spans is 0, `spans`.  One lane
// per item marches its ray from t = 0 to t_max with the scene's point query (query_point: the direction-free methods), whose per-ray
// set-up -- the debug flags and Scene::ray_setup for no direction -- is made once per lane, and whose evaluation stands once in the loop
// of span_item.  The lanes of a wave step independently, so a wave is as long as its longest ray.  A span leaves as one 8-byte store when
// it closes, the summary as two 16-byte stores at the end; nothing is shared between lanes: no LDS, no atomics.
// Both go through vector types of the compiler, one store instruction each from the front end on: written as an assignment of a uint4 or
// float2 struct, the aligned and the word path hold the same member stores, which the optimiser merges across the branch into word
// stores (the ISA had 21 global_store_dword and nothing wider).  query_store itself stays as it is: the other kernels' code is built on it.
typedef uint32_t span_u32x4 __attribute__((ext_vector_type(4)));
typedef float span_f32x2 __attribute__((ext_vector_type(2)));
template <class Scene, bool DBG>
struct SpanSceneDistance
{
	const FrameU &U;
	DebugFlags F;
	typename Scene::RayInv R;
	__device__ __forceinline__ float operator()(vec3 p) const
	{
		const vec3 zero = V3s(0.f);
		return scene_distance<Scene, DBG>(U, F, R, p, zero, false, 0.f, zero, zero);
	}
};
struct SpanStore
{
	float *item; // the item's max_spans slots of two floats; never used when max_spans is 0
	bool aligned;
	__device__ __forceinline__ void operator()(int k, float t_in, float t_out) const
	{
		if (aligned)
		{
			span_f32x2 v;
			v.x = t_in;
			v.y = t_out;
			reinterpret_cast<span_f32x2 *>(item)[k] = v; // one 8-byte store
		}
		else
		{
			item[2 * k] = t_in;
			item[2 * k + 1] = t_out;
		}
	}
};
template <class Scene, bool DBG>
__device__ __forceinline__ void query_spans_kernel(const SceneKernelArgs<SpanArgs> &a)
{
	static_assert(SDFR_PIXEL_BLOCK == 64, "one wave per block: a tile is 64 pixels");
	const FrameU &U = a.U;
	const SpanArgs &s = a.a;
	const uint32_t lane = threadIdx.x;
	uint32_t i;
	QueryRay ray;
	bool in_frame = true;
	if (s.kind == QUERY_FRAME)
	{
		const uint32_t tiles_x = ((uint32_t)U.width + 7u) >> 3;
		const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
		const uint32_t px = tx * 8u + (lane & 7u), py = ty * 8u + (lane >> 3);
		if (px >= (uint32_t)U.width || py >= (uint32_t)U.height) return;
		i = py * (uint32_t)U.width + px; // < width * height <= 2^30
		in_frame = query_pixel_ray(U, (int)px, (int)py, ray);
	}
	else
	{
		i = blockIdx.x * 64u + lane;
		if (i >= (uint32_t)s.n) return;
		if (s.kind == QUERY_PICK)
			in_frame = query_pixel_ray(U, s.pixels[(size_t)2 * i], s.pixels[(size_t)2 * i + 1], ray);
		else if (s.kind == QUERY_MESH)
			ray = query_mesh_ray(query_load3(s.pos, i), query_load3(s.dir, i), s.reach);
		else
			ray = query_plain_ray(query_load3(s.pos, i), query_load3(s.dir, i), s.t_max);
	}
	const SpanSceneDistance<Scene, DBG> distance = {U, debug_flags(U), Scene::ray_setup(U, V3s(0.f), query_ray_flags())};
	SpanStore store;
	store.item = s.spans + (size_t)2 * (size_t)s.max_spans * i; // (n * max_spans <= 2^30 spans of 8 bytes: 64-bit)
	store.aligned = (reinterpret_cast<size_t>(s.spans) & 7u) == 0u;
	uint32_t rec[SPAN_SUMMARY_WORDS];
	span_item(distance, store, in_frame, ray.origin, ray.dir, s.t_max, s.min_step, s.iso, s.max_steps, s.max_spans, rec);
	// 32-byte records: two 16-byte stores into an array aligned to 16 bytes, word stores into any other (query_store's rule)
	uint32_t *out = s.summaries + (size_t)SPAN_SUMMARY_WORDS * i;
	if ((reinterpret_cast<size_t>(s.summaries) & 15u) == 0u)
	{
		span_u32x4 lo, hi;
		lo.x = rec[0], lo.y = rec[1], lo.z = rec[2], lo.w = rec[3];
		hi.x = rec[4], hi.y = rec[5], hi.z = rec[6], hi.w = rec[7];
		reinterpret_cast<span_u32x4 *>(out)[0] = lo;
		reinterpret_cast<span_u32x4 *>(out)[1] = hi;
	}
	else
	{
#pragma unroll
		for (int k = 0; k < SPAN_SUMMARY_WORDS; ++k) out[k] = rec[k];
	}
}

// The measure query (sdfr_measure.h; sdfr_measure): one wave per 8 x 8 tile of columns, addressed by the block index alone, one lane per
// column, marched as the span kernel marches a ray (the same functor).  The first kernel of this unit whose lanes talk to each other: a
// lane past the grid's ragged edges does NOT leave -- it carries +0.0 into the reduction, and every lane of the wave reaches every shuffle
// and ballot below (the march's loop is the only divergent code, and it has ended).
//   moments: per component six xor-butterflies over the lane distances 1, 2, 4, 8, 16, 32.  Addition commutes, so both partners of a step
//   hold the same bits and after the six every lane holds the pairwise tree x[m] = x[2m] + x[2m + 1] over the 64 lanes, the order the
//   definition fixes.  Lane 0 stores the tile's ten doubles; k_measure_reduce (sdfr_mesh.hip) takes it from there.
//   integers: ballots and popcounts for the column counts, shuffles for the sums and bounds -- every value the whole wave's --, then lane t
//   issues the atomic of word t (MEASURE_TALLY_*; into the copy of the word that the tile's index selects) if the tile has anything for it: 64-bit atomicAdd, 32-bit atomicMin / atomicMax (agent
//   scope, HIP's default), the fp32 bounds as their order keys.  Integer atomics: the order of arrival changes nothing.
// A column's record leaves as five 8-byte stores into an array aligned to 8 bytes, as word stores into any other.
typedef uint32_t measure_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double measure_wave_tree(double v)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) v = v + __shfl_xor(v, d, 64);
	return v;
}
__device__ __forceinline__ uint32_t measure_wave_sum(uint32_t v)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
	return v;
}
__device__ __forceinline__ int measure_wave_min(int v)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1)
	{
		const int o = __shfl_xor(v, d, 64);
		v = o < v ? o : v;
	}
	return v;
}
__device__ __forceinline__ int measure_wave_max(int v)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1)
	{
		const int o = __shfl_xor(v, d, 64);
		v = o > v ? o : v;
	}
	return v;
}
template <class Scene, bool DBG>
__device__ __forceinline__ void query_measure_kernel(const SceneKernelArgs<MeasureArgs> &a)
{
	static_assert(SDFR_PIXEL_BLOCK == 64, "one wave per block: a tile is 64 columns");
	const FrameU &U = a.U;
	const MeasureArgs &g = a.a;
	const uint32_t lane = threadIdx.x;
	const uint32_t tu = ((uint32_t)g.nu + 7u) >> 3;
	const uint32_t tj = blockIdx.x / tu, ti = blockIdx.x - tj * tu;
	const int i = (int)(ti * 8u + (lane & 7u)), j = (int)(tj * 8u + (lane >> 3));
	const bool live = i < g.nu && j < g.nv;
	MeasureLane c = measure_no_column();
	if (live)
	{
		const SpanSceneDistance<Scene, DBG> distance = {U, debug_flags(U), Scene::ray_setup(U, V3s(0.f), query_ray_flags())};
		const vec3 o = V3(measure_origin(g.origin, g.du, g.dv, 0, i, j), measure_origin(g.origin, g.du, g.dv, 1, i, j), measure_origin(g.origin, g.du, g.dv, 2, i, j));
		c = measure_column(distance, o, V3(g.dw[0], g.dw[1], g.dw[2]), g.t_max, g.min_step, g.iso, g.max_steps);
		if (g.columns)
		{
			uint32_t *out = g.columns + (size_t)MEASURE_COLUMN_WORDS * ((size_t)i + (size_t)g.nu * (size_t)j); // (< 2^24 records of 40 bytes)
			const uint64_t m[3] = {(uint64_t)__double_as_longlong(c.c.m0), (uint64_t)__double_as_longlong(c.c.m1), (uint64_t)__double_as_longlong(c.c.m2)};
			const uint32_t w[MEASURE_COLUMN_WORDS] = {(uint32_t)m[0], (uint32_t)(m[0] >> 32), (uint32_t)m[1], (uint32_t)(m[1] >> 32), (uint32_t)m[2], (uint32_t)(m[2] >> 32),
				c.c.spans, c.c.steps, c.c.flags, (uint32_t)c.c.valid};
			if ((reinterpret_cast<size_t>(g.columns) & 7u) == 0u)
			{
#pragma unroll
				for (int k = 0; k < MEASURE_COLUMN_WORDS / 2; ++k)
				{
					measure_u32x2 v;
					v.x = w[2 * k];
					v.y = w[2 * k + 1];
					reinterpret_cast<measure_u32x2 *>(out)[k] = v; // one 8-byte store
				}
			}
			else
			{
#pragma unroll
				for (int k = 0; k < MEASURE_COLUMN_WORDS; ++k) out[k] = w[k];
			}
		}
	}
	// ---- from here on the whole wave, converged
	double v[MEASURE_MOMENTS];
	measure_contributions(c.c, live ? i : 0, live ? j : 0, v); // (no column, or none with an answer: m0 = m1 = m2 = +0.0, ten times +0.0)
#pragma unroll
	for (int k = 0; k < MEASURE_MOMENTS; ++k) v[k] = measure_wave_tree(v[k]);
	if (lane == 0u)
	{
		double *tile = g.partials + (size_t)MEASURE_MOMENTS * blockIdx.x;
#pragma unroll
		for (int k = 0; k < MEASURE_MOMENTS; ++k) tile[k] = v[k];
	}

	const unsigned long long hit = __ballot(c.c.spans >= 1u);
	const uint32_t n_open = (uint32_t)__popcll(__ballot((c.c.flags & (uint32_t)(SPAN_STARTS_INSIDE | SPAN_ENDS_INSIDE)) != 0u));
	const uint32_t n_out = (uint32_t)__popcll(__ballot((c.c.flags & (uint32_t)SPAN_OUT_OF_STEPS) != 0u));
	const uint32_t n_invalid = (uint32_t)__popcll(__ballot(live && c.c.valid != 1));
	const uint32_t steps = measure_wave_sum(c.c.steps); // (64 columns of at most 2^20 steps: 32 bits hold it)
	// (wave-uniform branches: `hit` is the whole wave's)
	const uint32_t spans = hit ? measure_wave_sum(c.c.spans) : 0u, crossings = steps ? measure_wave_sum(c.crossings) : 0u;
	int32_t lo[2] = {g.nu, g.nv}, hi[2] = {-1, -1};
	float t_lo = c.t_lo, t_hi = c.t_hi; // (+inf and -inf in a lane without a span; never NaN)
	if (hit)
	{
		const bool mine = c.c.spans >= 1u;
		lo[0] = measure_wave_min(mine ? i : g.nu), lo[1] = measure_wave_min(mine ? j : g.nv);
		hi[0] = measure_wave_max(mine ? i : -1), hi[1] = measure_wave_max(mine ? j : -1);
#pragma unroll
		for (int d = 1; d < 64; d <<= 1)
		{
			const float o_lo = __shfl_xor(t_lo, d, 64), o_hi = __shfl_xor(t_hi, d, 64);
			t_lo = o_lo < t_lo ? o_lo : t_lo;
			t_hi = o_hi > t_hi ? o_hi : t_hi;
		}
	}
	char *const tally = static_cast<char *>(g.tally) + (size_t)MEASURE_TALLY_STRIDE * (size_t)((uint32_t)MEASURE_TALLY_FIRST + (uint32_t)MEASURE_TALLY_COPIES * (lane < (uint32_t)MEASURE_TALLY_WORDS ? lane : 0u) +
		(blockIdx.x & (uint32_t)(MEASURE_TALLY_COPIES - 1)));
	if (lane < (uint32_t)MEASURE_TALLY_COUNTS)
	{
		const uint32_t count = lane == 0u ? (uint32_t)__popcll(hit) : lane == 1u ? n_open : lane == 2u ? n_out : lane == 3u ? n_invalid : lane == 4u ? steps : lane == 5u ? spans : crossings;
		if (count) atomicAdd(reinterpret_cast<unsigned long long *>(tally), (unsigned long long)count);
	}
	else if (lane < 11u && hit)
	{
		if (lane < 9u) atomicMin(reinterpret_cast<int32_t *>(tally), lane == 7u ? lo[0] : lo[1]);
		else atomicMax(reinterpret_cast<int32_t *>(tally), lane == 9u ? hi[0] : hi[1]);
	}
	else if (lane == 11u && hit) atomicMin(reinterpret_cast<uint32_t *>(tally), measure_order_key(t_lo));
	else if (lane == 12u && hit) atomicMax(reinterpret_cast<uint32_t *>(tally), measure_order_key(t_hi));
}

} // namespace sdfr

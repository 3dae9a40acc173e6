// sdfr_query_plan.h -- what each kind of query (sdfr_query_args.h: QUERY_*) takes, answers and launches, as one table, and the plan
// of one call made from it: the argument checks in the order their errors win, the kernel's arguments, the staging sizes of a host
// call, the kernel, the launches.  Plain host arithmetic, no HIP call: sdfr_api.cpp (query_impl) and sdfr_kernels.hip (launch_query)
// carry the plan out, tests/test_query_plan_cpu.py checks it on a machine without a GPU.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>
#include <initializer_list>

#include "sdfr_query_args.h"

namespace sdfr {

// what every entry point that takes a frame size or an "is host memory" flag accepts
inline bool frame_size_ok(int width, int height) { return width >= 1 && height >= 1 && (int64_t)width * height <= (int64_t)1 << 30; }
inline bool is_flag(int v) { return v == 0 || v == 1; }

// An array of a query: the pointer member of QueryArgs it goes through (its offset) and its bytes per item; bytes 0: no such array
struct QuerySlot
{
	size_t member, bytes;
};
enum { QUERY_REACH_RANGE, QUERY_REACH_POSITIVE }; // finite and >= 0, 0 meaning limits.range; finite and > 0
enum { QUERY_GRID_BLOCK_PER_64, QUERY_GRID_BLOCK_PER_TILE, QUERY_GRID_BLOCK_PER_ITEM };
enum { QUERY_BLOCK_ITEMS = 64, QUERY_TILE = 8 };
// a launch's threads must number below 2^32: a kind that takes a block of 64 threads per item launches at most this many items at once
static const uint32_t QUERY_ITEMS_PER_LAUNCH = 1u << 25;

struct QueryKind
{
	QuerySlot in[2];  // read, all required
	QuerySlot out[2]; // written: out[0] is required and out[1] optional -- the other way round where surfaces are asked for
	bool frame;       // takes a frame size; else the frame is 1 x 1
	bool frame_items; // ... and its items are the frame's pixels: n must be width * height
	int reach_rule;   // QUERY_REACH_* of `reach`
	const char *reach_text;
	bool bias;  // takes a bias: finite and >= 0
	int kernel; // QUERY_KERNEL_*; the ray kernel's kinds go to the surface kernel exactly when surfaces are asked for, to the lighting kernel when lighting is (query_kernel_of)
	int grid;   // QUERY_GRID_*
};
#define SDFR_Q(member, bytes) {offsetof(QueryArgs, member), bytes}
#define SDFR_Q_NONE {0, 0}
#define SDFR_Q_HITS SDFR_Q(hits, 4 * QUERY_HIT_WORDS), SDFR_Q(surfaces, 4 * QUERY_SURFACE_WORDS)
static const char *const k_query_max_distance_text = "max_distance must be finite and >= 0", *const k_query_radius_text = "radius must be finite and > 0";
static const QueryKind k_query_kinds[QUERY_KINDS] = {
	/* POINTS */ {{SDFR_Q(pos, 12), SDFR_Q_NONE}, {SDFR_Q(distance, 4), SDFR_Q(normals, 12)}, false, false, QUERY_REACH_RANGE, k_query_max_distance_text, false, QUERY_KERNEL_POINTS, QUERY_GRID_BLOCK_PER_64},
	/* RAYS   */ {{SDFR_Q(pos, 12), SDFR_Q(dir, 12)}, {SDFR_Q_HITS}, false, false, QUERY_REACH_RANGE, k_query_max_distance_text, false, QUERY_KERNEL_RAYS, QUERY_GRID_BLOCK_PER_64},
	/* PICK   */ {{SDFR_Q(pixels, 8), SDFR_Q_NONE}, {SDFR_Q_HITS}, true, false, QUERY_REACH_RANGE, k_query_max_distance_text, false, QUERY_KERNEL_RAYS, QUERY_GRID_BLOCK_PER_64},
	/* FRAME  */ {{SDFR_Q_NONE, SDFR_Q_NONE}, {SDFR_Q_HITS}, true, true, QUERY_REACH_RANGE, k_query_max_distance_text, false, QUERY_KERNEL_RAYS, QUERY_GRID_BLOCK_PER_TILE},
	/* MESH: positions, normals */ {{SDFR_Q(pos, 12), SDFR_Q(dir, 12)}, {SDFR_Q_HITS}, false, false, QUERY_REACH_POSITIVE, "reach must be finite and > 0", false, QUERY_KERNEL_RAYS, QUERY_GRID_BLOCK_PER_64},
	/* OCCLUSION: points, normals */ {{SDFR_Q(pos, 12), SDFR_Q(dir, 12)}, {SDFR_Q(occlusion, 4 * QUERY_OCCLUSION_WORDS), SDFR_Q_NONE}, false, false, QUERY_REACH_POSITIVE, k_query_radius_text, true, QUERY_KERNEL_OCCLUSION, QUERY_GRID_BLOCK_PER_ITEM},
	/* HIT_OCCLUSION */ {{SDFR_Q(hit_items, 4 * QUERY_HIT_WORDS), SDFR_Q_NONE}, {SDFR_Q(occlusion, 4 * QUERY_OCCLUSION_WORDS), SDFR_Q_NONE}, false, false, QUERY_REACH_POSITIVE, k_query_radius_text, true, QUERY_KERNEL_OCCLUSION, QUERY_GRID_BLOCK_PER_ITEM},
};
// what the lighting entries add to a ray kind's arrays: `lighting` required, `lights` optional; `hits` is then optional and `surfaces` is not taken
static const QuerySlot k_query_lighting_slots[2] = {SDFR_Q(lighting, 4 * QUERY_LIGHTING_WORDS), SDFR_Q(lights, 4 * QUERY_LIGHT_SLOTS * QUERY_LIGHT_SAMPLE_WORDS)};
#undef SDFR_Q_HITS
#undef SDFR_Q_NONE
#undef SDFR_Q

// the pointer member of `q` a slot names
inline const void *query_slot_get(const QueryArgs &q, const QuerySlot &s)
{
	const void *p;
	memcpy(&p, reinterpret_cast<const char *>(&q) + s.member, sizeof p);
	return p;
}
inline void query_slot_set(QueryArgs &q, const QuerySlot &s, const void *p) { memcpy(reinterpret_cast<char *>(&q) + s.member, &p, sizeof p); }

inline int query_kernel_of(const QueryArgs &q)
{
	const int kernel = k_query_kinds[q.kind].kernel;
	if (kernel != QUERY_KERNEL_RAYS) return kernel;
	return q.lighting ? QUERY_KERNEL_LIGHTING : q.surfaces ? QUERY_KERNEL_SURFACES : kernel;
}

// The launches of q (q.n > 0 items of a width x height frame): launch k covers the items [first, first + count) with `blocks` blocks of
// QUERY_BLOCK_ITEMS threads.  One launch, but of a block per item: QUERY_ITEMS_PER_LAUNCH items each.
struct QueryLaunch
{
	uint32_t first, count, blocks;
};
inline uint32_t query_launch_count(const QueryArgs &q)
{
	return k_query_kinds[q.kind].grid == QUERY_GRID_BLOCK_PER_ITEM ? ((uint32_t)q.n + QUERY_ITEMS_PER_LAUNCH - 1u) / QUERY_ITEMS_PER_LAUNCH : 1u;
}
inline QueryLaunch query_launch(const QueryArgs &q, int width, int height, uint32_t k)
{
	const uint32_t n = (uint32_t)q.n;
	switch (k_query_kinds[q.kind].grid)
	{
	case QUERY_GRID_BLOCK_PER_ITEM:
	{
		const uint32_t first = k * QUERY_ITEMS_PER_LAUNCH, count = n - first < QUERY_ITEMS_PER_LAUNCH ? n - first : QUERY_ITEMS_PER_LAUNCH;
		return {first, count, count};
	}
	case QUERY_GRID_BLOCK_PER_TILE:
		return {0u, n, (((uint32_t)width + QUERY_TILE - 1u) / QUERY_TILE) * (((uint32_t)height + QUERY_TILE - 1u) / QUERY_TILE)};
	default:
		return {0u, n, (n + QUERY_BLOCK_ITEMS - 1u) / QUERY_BLOCK_ITEMS};
	}
}
// q for one of its launches: the launch's items, every array of the kind advanced to the first of them (the occlusion records are 16
// bytes: the output's alignment class stays)
inline QueryArgs query_launch_args(const QueryArgs &q, const QueryLaunch &l)
{
	const QueryKind &kind = k_query_kinds[q.kind];
	QueryArgs a = q;
	a.n = (int)l.count;
	for (const QuerySlot *s : {&kind.in[0], &kind.in[1], &kind.out[0], &kind.out[1], &k_query_lighting_slots[0], &k_query_lighting_slots[1]})
		if (const void *p = s->bytes ? query_slot_get(q, *s) : nullptr) query_slot_set(a, *s, static_cast<const char *>(p) + s->bytes * (size_t)l.first);
	return a;
}

// What an entry point asks for: the kernel's arguments as the caller gave them -- q.kind, the arrays of that kind, q.reach (the
// max_distance of rays, the reach of a mesh, the radius of an occlusion query) and q.bias; everything else stays null or 0 -- and what
// only the host needs.  want_surfaces: one of the surface entries, which needs q.surfaces and takes q.hits or not.  want_lighting: one of
// the lighting entries (the kinds of the ray kernel only), which needs q.lighting and takes q.hits and q.lights or not.
struct QueryRequest
{
	QueryArgs q;
	int64_t n;
	int width, height;
	bool want_surfaces;
	int on_host;
	bool want_lighting;
};
inline QueryRequest query_request(int kind, int64_t n, int on_host)
{
	QueryRequest c = {};
	c.q.kind = kind;
	c.n = n;
	c.on_host = on_host;
	return c;
}

enum { QUERY_PLAN_OK = 0, QUERY_PLAN_INVALID_ARGUMENT = -1 }; // (SDFR_OK, SDFR_ERR_INVALID_ARGUMENT)
struct QueryPlan
{
	int status; // QUERY_PLAN_*
	const char *error;
	bool nothing_to_do; // n = 0
	QueryArgs q;        // for the caller's arrays as device memory; a host call points the slots at its staging pieces
	size_t bytes[6];    // of the arrays in the order they are staged: in[0], in[1], out[0], out[1], lighting, lights
	int width, height;  // of the frame to latch
	int kernel;         // QUERY_KERNEL_*
	uint32_t launches;  // query_launch(q, width, height, 0 .. launches - 1)
};

// The checks every query makes after the handle's and before the scene's, in the order their errors win.  range: limits.range.
inline QueryPlan plan_query(const QueryRequest &c, float range)
{
	const QueryKind &kind = k_query_kinds[c.q.kind];
	QueryPlan p = {};
	auto fail = [&p](const char *text) {
		p.status = QUERY_PLAN_INVALID_ARGUMENT;
		p.error = text;
		return p;
	};
	if (c.n < 0 || c.n > (int64_t)INT32_MAX) return fail("bad item count");
	if (!is_flag(c.on_host)) return fail("on_host must be 0 or 1");
	const float reach = c.q.reach;
	if (kind.reach_rule == QUERY_REACH_POSITIVE ? !(std::isfinite(reach) && reach > 0.f) : !std::isfinite(reach) || reach < 0.f) return fail(kind.reach_text);
	if (kind.bias && !(std::isfinite(c.q.bias) && c.q.bias >= 0.f)) return fail("bias must be finite and >= 0");
	if (kind.frame && !frame_size_ok(c.width, c.height)) return fail("bad frame size");
	p.nothing_to_do = c.n == 0;
	if (p.nothing_to_do) return p;
	if (kind.frame_items && c.n != (int64_t)c.width * c.height) return fail("without a pixel list n must be width * height");
	const bool lighting = c.want_lighting && kind.kernel == QUERY_KERNEL_RAYS;
	const QuerySlot &required = lighting ? k_query_lighting_slots[0] : kind.out[c.want_surfaces ? 1 : 0];
	for (const QuerySlot *s : {&kind.in[0], &kind.in[1], &required})
		if (s->bytes && !query_slot_get(c.q, *s)) return fail("null pointer");

	p.q = c.q;
	if (lighting) p.q.surfaces = nullptr;
	else p.q.lighting = p.q.lights = nullptr;
	p.q.n = (int)c.n;
	p.q.dist_max = reach == 0.f ? range : reach; // (a mesh's rays are marched to 2 * reach: query_mesh_ray)
	for (int k = 0; k < 2; ++k)
	{
		p.bytes[k] = (size_t)c.n * kind.in[k].bytes;
		p.bytes[2 + k] = kind.out[k].bytes && query_slot_get(p.q, kind.out[k]) ? (size_t)c.n * kind.out[k].bytes : 0;
		p.bytes[4 + k] = query_slot_get(p.q, k_query_lighting_slots[k]) ? (size_t)c.n * k_query_lighting_slots[k].bytes : 0;
	}
	p.width = kind.frame ? c.width : 1;
	p.height = kind.frame ? c.height : 1;
	p.kernel = query_kernel_of(p.q);
	p.launches = query_launch_count(p.q);
	return p;
}

} // namespace sdfr

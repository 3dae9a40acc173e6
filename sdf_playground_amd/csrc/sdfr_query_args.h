// sdfr_query_args.h -- what the host hands a query kernel, as plain structs: included by the device code (sdfr_query.h) and by the host
// code that plans a query (sdfr_query_plan.h), which includes no HIP header.  The kernels read these as kernel arguments: the layout
// below is pinned.
#pragma once
#if !defined(__HIPCC_RTC__) // hiprtc has no system headers: a run-time scene's query module gets the integer types from sdfr_math.h
#include <stdint.h>
#endif

namespace sdfr {

// One query launch.  Which members a kind reads and writes, at how many bytes per item, is the table of sdfr_query_plan.h
// (k_query_kinds); every other pointer is null, and the kernels branch on `normals`, `hits`, `surfaces` and `lights`.
enum { QUERY_POINTS = 0, QUERY_RAYS = 1, QUERY_PICK = 2, QUERY_FRAME = 3, QUERY_MESH = 4, QUERY_OCCLUSION = 5, QUERY_HIT_OCCLUSION = 6, QUERY_KINDS = 7 };
struct QueryArgs
{
	int kind;  // QUERY_*
	int n;
	const float *pos, *dir;
	const int32_t *pixels;
	float dist_max; // rays: march_ray's dist_max (picks and frames: the range; meshes: 2 * reach; occlusion: the radius)
	float reach;    // meshes
	float *distance, *normals;
	uint32_t *hits;     // 12 words per item: the layout of sdfr_hit
	uint32_t *surfaces; // 32 words per item: the layout of sdfr_surface
	// the occlusion kinds (appended: the other kernels' argument offsets stay)
	const uint32_t *hit_items; // 12 words per item, read
	uint32_t *occlusion;       // 4 words per item: the layout of sdfr_occlusion
	float bias;
	// the lighting kernel (appended likewise)
	uint32_t *lighting; // 16 words per item: the layout of sdfr_lighting
	uint32_t *lights;   // or null: 8 x 20 words per item, the layout of sdfr_light_sample[8]
};
enum { QUERY_HIT_WORDS = 12, QUERY_SURFACE_WORDS = 32, QUERY_OCCLUSION_WORDS = 4, QUERY_LIGHTING_WORDS = 16, QUERY_LIGHT_SAMPLE_WORDS = 20, QUERY_LIGHT_SLOTS = 8 };
static_assert(sizeof(QueryArgs) == 112, "QueryArgs is a kernel argument");
static_assert(__builtin_offsetof(QueryArgs, kind) == 0 && __builtin_offsetof(QueryArgs, n) == 4 && __builtin_offsetof(QueryArgs, pos) == 8 && __builtin_offsetof(QueryArgs, dir) == 16, "");
static_assert(__builtin_offsetof(QueryArgs, pixels) == 24 && __builtin_offsetof(QueryArgs, dist_max) == 32 && __builtin_offsetof(QueryArgs, reach) == 36, "");
static_assert(__builtin_offsetof(QueryArgs, distance) == 40 && __builtin_offsetof(QueryArgs, normals) == 48 && __builtin_offsetof(QueryArgs, hits) == 56, "");
static_assert(__builtin_offsetof(QueryArgs, surfaces) == 64 && __builtin_offsetof(QueryArgs, hit_items) == 72 && __builtin_offsetof(QueryArgs, occlusion) == 80, "");
static_assert(__builtin_offsetof(QueryArgs, bias) == 88 && __builtin_offsetof(QueryArgs, lighting) == 96 && __builtin_offsetof(QueryArgs, lights) == 104, "");

// A scene's query kernels by kind, the one list of them: X(kind, stem of the kernel's name, body template of sdfr_query_kernel.h, its
// arguments).  Kind QUERY_KERNEL_<kind> is the row's place in the list.  A built-in scene's unit names the kernel k_<stem>
// (sdfr_query_scene.hip), a run-time scene's query module sdfr_jit_<stem> (sdfr_jit_unit.h); both take SceneKernelArgs<arguments>
// (sdfr_frame.h).  rays: picks too; surfaces and lighting: the ray kinds when those records are asked for.  A new kind goes last.
#define SDFR_FOR_EACH_QUERY_KERNEL(X) \
	X(POINTS, query_points, query_points_kernel, QueryArgs) \
	X(RAYS, query_rays, query_rays_kernel, QueryArgs) \
	X(LATTICE, query_lattice, query_lattice_kernel, LatticeArgs) \
	X(SURFACES, query_surfaces, query_surfaces_kernel, QueryArgs) \
	X(OCCLUSION, query_occlusion, query_occlusion_kernel, QueryArgs) \
	X(LIGHTING, query_lighting, query_lighting_kernel, QueryArgs) \
	X(ATLAS, bake_atlas, atlas_bake_kernel, AtlasArgs) \
	X(MESH_SHARP, mesh_sharp, mesh_sharp_kernel, MeshSharpArgs) \
	X(SLICES, query_slices, query_slices_kernel, SliceArgs) \
	X(SPANS, query_spans, query_spans_kernel, SpanArgs) \
	X(MEASURE, query_measure, query_measure_kernel, MeasureArgs)
#define SDFR_QUERY_KERNEL_ENUM(kind, stem, body, args) QUERY_KERNEL_##kind,
enum { SDFR_FOR_EACH_QUERY_KERNEL(SDFR_QUERY_KERNEL_ENUM) QUERY_KERNEL_KINDS };
#undef SDFR_QUERY_KERNEL_ENUM

// One lattice launch (sample_lattice, sdfr_api.cpp; sdfr_mesh_extract): the distance query at the points of a regular lattice,
// computed from their indices -- point (i, j, k) is origin + (float)index * cell per axis, one multiply then one add -- into
// out[i + px * (j + py * k)].  px * py * pz <= 2^30.
struct LatticeArgs
{
	float origin[3];
	float cell;
	int32_t px, py, pz; // lattice points per axis
	int32_t rows;       // 0: a wave owns a 4 x 4 x 4 brick of points; 1: 64 consecutive points of a row (the A/B of DESIGN.md 4.6)
	float *out;
};
static_assert(sizeof(LatticeArgs) == 40 && __builtin_offsetof(LatticeArgs, px) == 16 && __builtin_offsetof(LatticeArgs, out) == 32, "LatticeArgs is a kernel argument");

// One launch of the sharp vertices (sdfr_mesh_sharp.h; sdfr_mesh_extract_sharp): the grid, field for field MeshGrid's, the lattice of its
// distances, and positions [vertices][3], whose word 3 * v holds vertex v's cell index when the kernel starts and which it overwrites.
// SDFR_MESH_SHARP_LANES lanes per vertex, 64 / SDFR_MESH_SHARP_LANES vertices per block of one wave: 16, a lane per edge of the cell, is
// what ships; 1, a lane per vertex, exists for the A/B of DESIGN.md 4.12 (a developer build: buildlib.build(extra=["-DSDFR_MESH_SHARP_LANES=1"])).
#ifndef SDFR_MESH_SHARP_LANES
#define SDFR_MESH_SHARP_LANES 16
#endif
static_assert(SDFR_MESH_SHARP_LANES == 16 || SDFR_MESH_SHARP_LANES == 1, "a lane per edge or a lane per vertex");
struct MeshSharpArgs
{
	float origin[3];
	float cell;
	int32_t n[3];
	float iso;
	const float *lattice;
	float *positions;
	uint32_t vertices;
};
static_assert(sizeof(MeshSharpArgs) == 56 && __builtin_offsetof(MeshSharpArgs, lattice) == 32 && __builtin_offsetof(MeshSharpArgs, vertices) == 48, "MeshSharpArgs is a kernel argument");

// One atlas launch (sdfr_atlas.h, sdfr_atlas_plan.h; sdfr_atlas_texels and sdfr_atlas_bake): the texels of a width x height image cut into
// square tiles of 1 << tile_log2 texels, tile q = row * tiles_per_row + col the quad of triangles 2q and 2q + 1 of `indices`.  A wave
// takes an 8 x 8 square of the image.  The scene-free kernel (k_atlas_texels) writes texel_positions, texel_normals and valid; the bake
// kernel writes the planes of `layers` that are there, and valid.
enum { ATLAS_ALBEDO = 1u, ATLAS_NORMAL = 2u, ATLAS_LIT = 4u, ATLAS_LAYERS = 7u }; // SDFR_ATLAS_*
struct AtlasArgs
{
	const float *positions, *normals; // [vertex_count][3]
	const uint32_t *indices;          // [2 * quads][3]
	uint32_t vertex_count, quads;
	int32_t tile_log2, tiles_per_row;
	int32_t width, height; // multiples of 8; width * height <= 2^30
	float reach;
	uint32_t layers;
	float *albedo, *normal, *lit; // [height * width][4] each, or null
	int32_t *valid;               // [height * width]
	float *texel_positions, *texel_normals; // [height * width][3] each
};
static_assert(sizeof(AtlasArgs) == 104 && __builtin_offsetof(AtlasArgs, vertex_count) == 24 && __builtin_offsetof(AtlasArgs, albedo) == 56 && __builtin_offsetof(AtlasArgs, valid) == 80, "AtlasArgs is a kernel argument");

// One slice launch (sdfr_slice_extract): the distance query at the points of a stack of plane lattices, computed from their indices -- point (i, j) of layer l is ((origin + (float)i * du) + (float)j * dv) + (float)l * dw per
// component, every operation separate (sdfr_slice.h: slice_coord) -- into out[i + pu * (j + pv * l)].  pu * pv * layers <= 2^30.
struct SliceArgs
{
	float origin[3];
	float du[3], dv[3], dw[3];
	int32_t pu, pv, layers; // lattice points along u and v, layers
	int32_t rows;           // 0: a wave owns an 8 x 8 tile of points of one layer; 1: 64 consecutive points of the linear index (the A/B of DESIGN.md 4.14)
	float *out;
};
static_assert(sizeof(SliceArgs) == 72 && __builtin_offsetof(SliceArgs, du) == 12 && __builtin_offsetof(SliceArgs, dw) == 36 && __builtin_offsetof(SliceArgs, pu) == 48, "");
static_assert(__builtin_offsetof(SliceArgs, rows) == 60 && __builtin_offsetof(SliceArgs, out) == 64, "SliceArgs is a kernel argument");

// One span launch (sdfr_query_ray_spans, sdfr_pick_spans, sdfr_mesh_spans): the intervals of each item's
// ray that lie inside the solid (sdfr_span.h).  kind: QUERY_RAYS (pos, dir), QUERY_PICK (pixels), QUERY_FRAME (every pixel of the frame,
// n = width * height, a wave per 8 x 8 tile) or QUERY_MESH (pos, dir = positions, normals; reach); every other input is null.
// summaries: 8 words per item, the layout of sdfr_span_summary; spans: [n][max_spans][2] floats, null if max_spans = 0.
// n * max(max_spans, 1) <= 2^30.
struct SpanArgs
{
	int32_t kind, n;
	const float *pos, *dir;
	const int32_t *pixels;
	float reach;                // meshes
	float t_max, min_step, iso; // t_max: the effective one, never the 0 that stands for limits.range
	int32_t max_steps, max_spans;
	uint32_t *summaries;
	float *spans;
};
static_assert(sizeof(SpanArgs) == 72 && __builtin_offsetof(SpanArgs, n) == 4 && __builtin_offsetof(SpanArgs, pos) == 8 && __builtin_offsetof(SpanArgs, dir) == 16, "");
static_assert(__builtin_offsetof(SpanArgs, pixels) == 24 && __builtin_offsetof(SpanArgs, reach) == 32 && __builtin_offsetof(SpanArgs, t_max) == 36, "");
static_assert(__builtin_offsetof(SpanArgs, iso) == 44 && __builtin_offsetof(SpanArgs, max_steps) == 48 && __builtin_offsetof(SpanArgs, max_spans) == 52, "");
static_assert(__builtin_offsetof(SpanArgs, summaries) == 56 && __builtin_offsetof(SpanArgs, spans) == 64, "SpanArgs is a kernel argument");

// One measure launch (sdfr_measure): the moments of the solid over nu x nv parallel columns
// (sdfr_measure.h), a wave per 8 x 8 tile of columns.  Column (i, j) starts at (origin + (float)i * du) + (float)j * dv per component and
// runs along dw.  partials: 10 doubles per tile, tiles row-major; columns: 10 words per column, the layout of sdfr_measure_column, row-major
// i + nu * j, or null; tally: the words the integer totals are counted in (MEASURE_TALLY_*).  nu, nv <= 8192, nu * nv <= 2^24.
struct MeasureArgs
{
	float origin[3];
	float du[3], dv[3], dw[3];
	int32_t nu, nv;
	float t_max, min_step, iso; // t_max: the effective one, never the 0 that stands for limits.range
	int32_t max_steps;
	double *partials;
	uint32_t *columns;
	void *tally;
};
static_assert(sizeof(MeasureArgs) == 96 && __builtin_offsetof(MeasureArgs, du) == 12 && __builtin_offsetof(MeasureArgs, dw) == 36 && __builtin_offsetof(MeasureArgs, nu) == 48, "");
static_assert(__builtin_offsetof(MeasureArgs, t_max) == 56 && __builtin_offsetof(MeasureArgs, iso) == 64 && __builtin_offsetof(MeasureArgs, max_steps) == 68, "");
static_assert(__builtin_offsetof(MeasureArgs, partials) == 72 && __builtin_offsetof(MeasureArgs, columns) == 80 && __builtin_offsetof(MeasureArgs, tally) == 88, "MeasureArgs is a kernel argument");
// The tally while it is counted: the packed result (sdfr_measure_result, 160 bytes) in the first two lines, then 16 copies of word t,
// each in a line of its own: line MEASURE_TALLY_FIRST + 16 * t + k, and tile b counts into copy k = b & 15.  (As the survey's words:
// packed into one line the atomics of all tiles queue up behind each other; and every tile has steps to add, so even a word with a line
// to itself takes its atomics one by one -- 16 384 tiles stood 170 us behind one word of `steps`)
// Words 0 .. 6: 64-bit counts -- columns hit, open, out of steps, invalid; steps, spans, crossings; 7 .. 10: hit_lo[2], hit_hi[2];
// 11, 12: the order keys of t_lo and t_hi.  k_measure_pack adds up, or takes the bounds of, the copies.
enum { MEASURE_TALLY_COUNTS = 7, MEASURE_TALLY_WORDS = 13, MEASURE_TALLY_COPIES = 16, MEASURE_TALLY_STRIDE = 128, MEASURE_TALLY_FIRST = 2,
	MEASURE_TALLY_BYTES = 128 * (2 + 13 * 16) };

} // namespace sdfr

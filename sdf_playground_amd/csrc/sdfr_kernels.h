// sdfr_kernels.h -- host-callable launchers of the gfx950 kernels (sdfr_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdfr_frame.h"
#include "sdfr_launch_plan.h"
#include "sdfr_query_args.h"

namespace sdfr {

// per-handle scratch of the wavefront schedule (allocated by the API, sized for `capacity` pixels)
struct WavefrontWorkspace
{
	size_t capacity;     // pixels
	float *ray_cur;      // [11][capacity] ray being traced for each pixel
	float *ray_queue;    // [8][capacity] pending rays, 48-byte records (GlobalRayStore)
	uint32_t *qdepth_lo; // [capacity] packed depths of slots 0-3
	uint32_t *qdepth_hi; // [capacity] packed depths of slots 4-7
	float *result;       // [8][capacity] march result: status/iter, t, d, normal xyz (+2 spare)
	float *accum;        // [4][capacity] rgb accumulator + hdr flag
	uint32_t *pstat;     // [3][capacity] per-pixel counters
	uint32_t *list_a;    // [capacity] pixels with a ray in flight (ping)
	uint32_t *list_b;    // [capacity] (pong)
	uint32_t *counters;  // [64] list sizes per round and misc
	RenderTotals *partials; // [capacity / 64 + 1] per-block counter sums of the pixel schedule
	uint32_t *tile_cursors; // [8 x 32] tile hand-out counters of the pixel kernel (TileQueue), zero between launches
};

// list entries a march wave (k_march) claims per atomic; the wavefront launcher sizes its grid by it
#define SDFR_GRAB 128

// What a scene unit (sdfr_kernels_scene.hip, one per scene of the registry) exports: its kernels by host pointer, [DBG], and
// how the scene wants them launched.  Everything that plans and launches lives in sdfr_kernels.hip, once.
struct SceneKernels
{
	const void *pixel[2], *march[2], *shade[2];
	bool persistent_tiles, square_units; // PersistentTiles, SquareUnits (sdfr_scene_traits.h)
	int retire_after, tile_w_log2;       // RetireAfter, SceneTileShape
};
// How the host names a kernel: a kernel of this library by its host pointer (`kernel`), or a function of a module loaded at run
// time (`function`, sdfr_jit.cpp).  At a launch, this field is all that differs between a built-in scene and a run-time one.
struct KernelRef
{
	const void *kernel;
	hipFunction_t function;
};
// one launch of `blocks` blocks of `threads` threads on `stream`, the kernel's parameters by address
hipError_t launch_kernel(const KernelRef &k, uint32_t blocks, uint32_t threads, void **args, hipStream_t stream);
// A scene's query kernels [kind][DBG]: a built-in scene's query unit exports them (sdfr_query_scene.hip), a run-time scene's
// query module is looked up into the same table (jit_query_kernels, sdfr_jit.h).  kind: QUERY_KERNEL_*, a row of the list of
// sdfr_query_args.h (SDFR_FOR_EACH_QUERY_KERNEL)
struct QueryKernels
{
	KernelRef k[QUERY_KERNEL_KINDS][2];
};
// One launch of a scene's query kernel of any kind for U with the kind's arguments, every pointer device memory: `blocks` blocks of one
// wave.  How many blocks is the kind's plan's to say (sdfr_mesh_plan.h, sdfr_slice_plan.h, sdfr_span_plan.h, sdfr_measure_plan.h,
// sdfr_atlas_plan.h).
template <class A>
hipError_t launch_scene_kernel(const KernelRef &k, const FrameU &U, const A &args, uint32_t blocks, hipStream_t stream)
{
	SceneKernelArgs<A> a = {U, args};
	void *params[] = {&a};
	return launch_kernel(k, blocks, SDFR_TILE_ITEMS, params, stream);
}
// a unit names its getter by its scene's index: scene_kernels_<index>(), scene_query_kernels_<index>()
#define SDFR_CAT2(a, b) a##b
#define SDFR_CAT(a, b) SDFR_CAT2(a, b)
const SceneKernels *scene_kernels(int scene); // null: not a scene of the registry
const QueryKernels *scene_query_kernels(int scene);

hipError_t launch_wavefront_schedule(int scene, const FrameU &U, const RowMap &rows, void *out, int format, uint32_t *pixel_stats,
	RenderTotals *totals, const WavefrontWorkspace &ws, hipStream_t stream, hipEvent_t *march_events, hipEvent_t *shade_events,
	int *n_rounds_out);

// one query by a scene's kernel of q's kind (sdfr_query_plan.h: query_kernel_of) for U, in the launches that header plans: q.n > 0
// items, every pointer device memory
hipError_t launch_query(const KernelRef &k, const FrameU &U, const QueryArgs &q, hipStream_t stream);

// Surface nets over a lattice of distances (sdfr_mesh.h, sdfr_mesh.hip), every pointer device memory.  launch_mesh_count: the vertex
// flag per cell and the quad count per lattice point, then their exclusive prefix sums in place -- cell_vertex [cells + 1] and
// point_quad [points + 1], whose last elements are the totals; sums: mesh_scan_sum_words(cells + 1) + mesh_scan_sum_words(points + 1)
// words of scratch.  launch_mesh_emit: positions [vertices][3] and, unless null (no quads), indices [2 * quads][3]; cells_only: instead of
// a vertex, its cell's linear index as the bits of its first word, for a scene's sharp-vertex kernel (QUERY_KERNEL_MESH_SHARP), which
// makes the vertices of sdfr_mesh_extract_sharp from them (sdfr_mesh_sharp.h).
struct MeshGrid;
size_t mesh_scan_sum_words(size_t n);
hipError_t launch_mesh_count(const MeshGrid &g, const float *lattice, uint32_t *cell_vertex, uint32_t *point_quad, uint32_t *sums, hipStream_t stream);
hipError_t launch_mesh_emit(const MeshGrid &g, const float *lattice, const uint32_t *cell_vertex, const uint32_t *point_quad, float *positions,
	uint32_t *indices, bool cells_only, hipStream_t stream);
// data [n] -> its exclusive prefix sum, in place, by the launches launch_mesh_count makes (k_mesh_scan_*); sums: mesh_scan_sum_words(n) words
void launch_mesh_scan(uint32_t *data, uint32_t n, uint32_t *sums, hipStream_t stream);
// What the lattice holds (sdfr_mesh_survey.h; sdfr_mesh_survey): out, MESH_SURVEY_WORK_BYTES of device memory, is the survey of g, near
// cells with `band`, followed by the words k_mesh_survey counted it in with integer atomics, each word in a page of its own.
struct MeshSurvey;
hipError_t launch_mesh_survey(const MeshGrid &g, const float *lattice, float band, MeshSurvey *out, hipStream_t stream);
// The parts and voids of a lattice (sdfr_components.h, sdfr_components.hip; the plan: sdfr_components_plan.h), every pointer device
// memory.  launch_components_union: parent [points] = every point's root, and scan [points + 1], the exclusive prefix sum of the root
// flags, whose last element is the number of components; sums: mesh_scan_sum_words(points + 1) words.  launch_components_tally, with
// that number in `f`: the points' labels in place of parent and into `labels` unless null, table [components], the records into `records`
// if f.fill, and the packed counts at the start of result (COMPONENT_RESULT_BYTES).
struct ComponentsPlan;
struct ComponentsFill;
struct Component;
hipError_t launch_components_union(const ComponentsPlan &p, const float *lattice, uint32_t *parent, uint32_t *scan, uint32_t *sums, hipStream_t stream);
hipError_t launch_components_tally(const ComponentsPlan &p, const ComponentsFill &f, const float *lattice, uint32_t *parent, const uint32_t *scan, uint32_t *labels,
	Component *table, Component *records, void *result, hipStream_t stream);

// Marching squares over a stack of plane lattices (sdfr_slice.h, sdfr_slice.hip; sdfr_slice_extract), every pointer device memory; the
// lattices are a scene's slice kernel's (QUERY_KERNEL_SLICES).  launch_slice_count: the vertex count and the segment count per lattice
// point, then their exclusive prefix sums in place -- point_vertex and cell_segment [points + 1], whose last elements are the totals; sums: 2 * mesh_scan_sum_words(points + 1) words of scratch -- and layer_offsets [2][layers + 1], the first vertex and the first
// segment of every layer with the totals after the last.  launch_slice_emit: positions [vertices][3], coords [vertices][2] unless null,
// and unless null (no segments) segments [segments][2].
struct SliceGrid;
hipError_t launch_slice_count(const SliceGrid &g, const float *lattice, uint32_t *point_vertex, uint32_t *cell_segment, uint32_t *sums, uint32_t *layer_offsets,
	hipStream_t stream);
hipError_t launch_slice_emit(const SliceGrid &g, const float *lattice, const uint32_t *point_vertex, const uint32_t *cell_segment, float *positions, float *coords,
	uint32_t *segments, hipStream_t stream);

// The measure (sdfr_measure.h; the plan: sdfr_measure_plan.h), every pointer device memory.  launch_measure_init: the tally's words
// (MEASURE_TALLY_BYTES) set for a grid of nu x nv columns.  Then a scene's measure kernel (QUERY_KERNEL_MEASURE), a block per 8 x 8 tile
// of columns -> MeasureArgs::partials, the tally, the columns unless null.  launch_measure_reduce: the
// passes of k_measure_reduce -- pass k reads pass_records[k] records of ten doubles from partials[k % 2] and writes a 64th as many, rounded
// up, into the other -- and then the packed result (sdfr_measure_result) at the start of the tally.
hipError_t launch_measure_init(void *tally, int32_t nu, int32_t nv, hipStream_t stream);
hipError_t launch_measure_reduce(double *const partials[2], const uint32_t *pass_records, int passes, void *tally, hipStream_t stream);

// The texture atlas of a mesh (sdfr_atlas.h; the plan: sdfr_atlas_plan.h), every pointer device memory, `blocks` blocks of one wave, one
// per 8 x 8 square of the image.  launch_atlas_texels: the scene-free kernel -- the texels' points and normals, or with g's planes
// instead the image of a bake without quads.  Any other bake is a scene's bake kernel's (QUERY_KERNEL_ATLAS).
hipError_t launch_atlas_texels(const AtlasArgs &g, uint32_t blocks, hipStream_t stream);

hipError_t launch_assemble_strips(int width, int height, int world, const void *gathered, void *out_image, int format, int priv_count,
	int priv_period, hipStream_t stream);

// HDR::process: scene16/bloom1 RGBA16F, ldr8 RGBA8, all device pointers of width*height pixels
// mid_event (optional) is recorded between the two kernels
// flags: postprocess_flag_bytes(width, height) bytes of device scratch (one per 32 pixels of a row: lit or not)
size_t postprocess_flag_bytes(int width, int height);
hipError_t launch_postprocess(int width, int height, const void *scene16, void *bloom1, void *ldr8, unsigned char *flags, hipStream_t stream,
	hipEvent_t mid_event = nullptr);

// the resolve of one pass of sdfr_render_aa (sdfr_resolve.h, sdfr_resolve.hip): every strip of the pass, all pyramid levels
struct ResolveArgs;
hipError_t launch_resolve(ResolveArgs a, hipStream_t stream);

hipError_t launch_selftest_math(int what, float c, unsigned long long *d_mismatches, hipStream_t stream);

// wavefront schedule, scene-independent start of a frame: primary rays, empty queues, round-0 list
hipError_t launch_wavefront_init(const FrameU &U, const RowMap &rm, uint32_t n_work, const WavefrontWorkspace &ws, uint32_t *pixel_stats, hipStream_t stream);

// folds the per-block partial sums of a pixel-schedule launch into `totals` and puts the tile cursors back to zero
// feedback_rows: tile rows of the launch if it was a persistent one whose rows should be re-ordered for the next frame (else 0)
hipError_t launch_reduce_totals(const RenderTotals *partials, uint32_t n_blocks, RenderTotals *totals, hipStream_t stream, uint32_t *tile_cursors,
	uint32_t feedback_rows, unsigned long long frame_pixels, uint32_t feedback_key);
int pixel_tile_cursor_words();
int scene_tile_w_log2(int scene); // the tile shape a built-in scene asks for (SceneTileShape); 3 = 8 x 8, also for run-time scenes
// A scene's pixel kernel and how the scene wants it launched.  blocks_per_cu: where the occupancy query's answer is kept between
// launches (0 = not asked yet), or null to ask on every launch.
struct PixelKernel
{
	KernelRef k;
	int *blocks_per_cu;
	PixelSceneTraits traits;
};
bool scene_pixel_kernel(int scene, bool dbg, PixelKernel &out); // of a built-in scene (a run-time scene's: jit_pixel_kernel); false: not a scene of the registry
// One launch of the pixel schedule, for built-in and run-time scenes alike: reads the developer knobs, asks how many blocks of the
// kernel stay resident, plans (plan_pixel_launch, sdfr_launch_plan.h), launches the kernel and then the fold (launch_reduce_totals).
hipError_t launch_pixel(const PixelKernel &pk, const FrameU &U, const RowMap &rm, void *out, int format, uint32_t *pixel_stats,
	RenderTotals *totals, const WavefrontWorkspace &ws, hipStream_t stream, int launch_mode);

int pixel_block_threads(); // block size of the pixel kernels (partials are sized by it)
int device_cu_count(int device);

} // namespace sdfr

// sdfr_launch_plan.h -- how a launch of the pixel kernel is laid out: what is handed out (tile rows or squares of tiles), to how
// many blocks, under which feedback key.  Plain host arithmetic over sdfr_frame.h: no HIP call, no environment -- the launcher
// (launch_pixel, sdfr_kernels.hip) asks the device and reads the developer knobs, and passes both in as values, so the policy can
// be checked on a machine without a GPU (tests/test_launch_plan_cpu.py).  One plan for the scenes compiled ahead of time and
// for the scenes compiled at run time: what differs between them is a field of PixelSceneTraits.
#pragma once
#include <stddef.h>

#include "sdfr_frame.h"

namespace sdfr {

enum { SDFR_TILE_ITEMS = 64 }; // work items of a tile: one wave, one block of the pixel kernel
#ifndef SDFR_STRIP_ROWS
#define SDFR_STRIP_ROWS 8 // include/sdfr.h; the 8-row strips of RowMap (sdfr_frame.h)
#endif

// which rows of a frame a render covers: all of them, this rank's shared strips (compact buffer), or the private strips (in place)
enum RenderMode { RENDER_FULL, RENDER_STRIPS, RENDER_PRIVATE };

// pixels of one rank's compact strip buffer (sdfr_strip_buffer_pixels_split, arguments checked): whole strips, the same on every rank
inline int64_t strip_buffer_pixels(int width, int height, int world, int priv_count, int priv_period)
{
	const int64_t strips = ((int64_t)height + SDFR_STRIP_ROWS - 1) / SDFR_STRIP_ROWS;
	const int64_t shared = strips - (int64_t)private_strip_count((uint32_t)strips, priv_count, priv_period);
	return ((shared + world - 1) / world) * SDFR_STRIP_ROWS * (int64_t)width;
}
// a row map as the API hands it to the launchers: tiles set, no hand-out units, retire_after or feedback_key -- the launcher of
// a persistent launch decides those (plan_pixel_launch)
inline RowMap api_row_map(int width, int local_rows, int rank, int world, int tile_w_log2, int priv_count, int priv_period, int direct)
{
	RowMap rm;
	rm.local_rows = local_rows;
	rm.rank = rank;
	rm.world = world;
	rm.tile_w_log2 = tile_w_log2;
	rm.priv_count = priv_count;
	rm.priv_period = priv_period;
	rm.direct = direct;
	row_map_tiles(rm, width);
	rm.unit_log2 = rm.units_x = rm.units_x_magic = rm.units = 0u;
	rm.retire_after = 0u;
	rm.feedback_key = 0u;
	return rm;
}
// The rows of one render of the API (render_impl, sdfr_api.cpp) and the pixels its output -- and the per-pixel workspace, which is
// indexed like the output -- spans.  priv_count / priv_period: the handle's strip split, which a full frame ignores.
struct FrameRows
{
	RowMap rm;
	size_t local_pixels;
};
inline FrameRows frame_rows(RenderMode mode, int width, int height, int rank, int world, int tile_w_log2, int priv_count, int priv_period)
{
	if (mode == RENDER_FULL) { priv_count = 0; priv_period = 1; }
	int local_rows = height;
	if (mode == RENDER_STRIPS) // a strip buffer keeps whole strips (rows past the frame stay zero)
		local_rows = (int)(strip_buffer_pixels(width, height, world, priv_count, priv_period) / width);
	else if (mode == RENDER_PRIVATE)
		local_rows = (int)(private_strip_count((uint32_t)((height + SDFR_STRIP_ROWS - 1) / SDFR_STRIP_ROWS), priv_count, priv_period) * SDFR_STRIP_ROWS);
	FrameRows f;
	f.rm = api_row_map(width, local_rows, rank, world, tile_w_log2, priv_count, priv_period, mode == RENDER_PRIVATE ? 1 : 0);
	f.local_pixels = mode == RENDER_PRIVATE ? (size_t)width * height : (size_t)local_rows * width;
	return f;
}
// does a strip buffer of `rm` end past the frame: its last strip is missing or cut short, and those rows are never written
inline bool strips_end_past_frame(const RowMap &rm, int height)
{
	const int last_local_strip = rm.local_rows / SDFR_STRIP_ROWS - 1;
	const long long last_row_end = last_local_strip < 0 ? 0 : ((long long)strip_local_to_global(rm, (uint32_t)last_local_strip) + 1) * SDFR_STRIP_ROWS;
	return last_row_end > height;
}

// work items (padded to whole tiles) of a launch: lists and per-pixel state are sized by this
inline uint32_t launch_work_items(int width, const RowMap &rm)
{
	const uint32_t tw_log2 = (uint32_t)rm.tile_w_log2, th_log2 = 6u - tw_log2;
	const uint32_t tiles_x = ((uint32_t)width + (1u << tw_log2) - 1u) >> tw_log2;
	const uint32_t tiles_y = ((uint32_t)rm.local_rows + (1u << th_log2) - 1u) >> th_log2;
	return tiles_x * tiles_y * 64u;
}
// cuts the frame of `rm` (tiles_x set: row_map_tiles) into squares of tiles (row_map_units) and returns the work items of those
// squares, which cover the frame with a margin; 0: no squares for this row map (a strip launch, or a frame too large)
inline uint32_t row_map_square_items(RowMap &rm)
{
	row_map_units(rm, SDFR_ROW_FEEDBACK_MAX);
	return rm.unit_log2 ? (rm.units << (2u * rm.unit_log2)) * 64u : 0u;
}
// what a handle's per-launch scratch is sized for: the work items, or -- a persistent launch hands a full frame out in squares of tiles that
// cover it with a margin (row_map_units), and launches at most one block per tile handed out -- the items of those squares
// (>= launch_work_items)
inline uint32_t launch_capacity_items(int width, const RowMap &rm)
{
	const uint32_t items = launch_work_items(width, rm);
	RowMap units = rm;
	row_map_tiles(units, width);
	const uint32_t padded = row_map_square_items(units);
	return padded > items ? padded : items;
}

// What the plan has to know of the scene.  Built-in scenes: PersistentTiles, RetireAfter, SquareUnits (sdfr_scene_traits.h) and
// 2 * index + DBG; a scene compiled at run time: one wave per tile unless asked otherwise, 8, never, and
// 0x80000000 | fnv1a(name) | DBG.
struct PixelSceneTraits
{
	bool persistent_tiles; // the launch for launch_mode 0
	int retire_after;
	bool square_units;     // persistent full-frame launches may be handed out in squares of tiles
	uint32_t feedback_key; // the scene's word of pixel_feedback_key
};
// The developer knobs as values.  SDFR_PIXEL_PERSISTENT: -1 unset, else 0 | 1; SDFR_PIXEL_BLOCKS_PER_CU: 0 unset, else the cap of
// a persistent grid; SDFR_PIXEL_RETIRE_AFTER: -1 unset, else tiles (0 = never); SDFR_PIXEL_SQUARE_UNITS: -1 unset, 0 = tile
// rows for every scene.
struct PixelLaunchKnobs
{
	int persistent, blocks_per_cu, retire_after, square_units;
};

// how the pixel kernels are launched: persistent (resident waves pull tiles from the cursors) or one wave per
// tile.  launch_mode: 0 = the scene's own default (PersistentTiles), 1 = one wave per tile, 2 = persistent;
// the developer knobs SDFR_PIXEL_PERSISTENT=0|1 and SDFR_PIXEL_BLOCKS_PER_CU=n (cap of a persistent grid) override.
// retire_after (persistent launches; SDFR_PIXEL_RETIRE_AFTER=n overrides, 0 = never): see pixel_launch_blocks.
struct PixelLaunchMode { bool persistent; int blocks_per_cu; int retire_after; };
inline PixelLaunchMode pixel_launch_mode(const PixelLaunchKnobs &knobs, int launch_mode, bool scene_default_persistent, int scene_retire_after)
{
	PixelLaunchMode m;
	m.persistent = launch_mode == 2 || (launch_mode == 0 && scene_default_persistent);
	if (knobs.persistent >= 0) m.persistent = knobs.persistent != 0;
	m.blocks_per_cu = knobs.blocks_per_cu;
	m.retire_after = knobs.retire_after >= 0 ? knobs.retire_after : scene_retire_after;
	return m;
}
// Blocks of a pixel launch.  One wave per tile: as many as tiles.  Persistent: what stays resident -- and, when waves
// retire after `retire_after` tiles, the replacements as well: tiles / retire_after, plus half a chip of waves that
// end for want of tiles before they have had their share.  Why waves retire: a SIMD serves its oldest waves first, so
// of the waves that start together the ones in its upper slots crawl for the whole frame (tools/wave_trace.py: two
// tiles against sixty), and what they hold when the queue runs dry is finished by one or two waves per SIMD while the
// rest of the chip idles -- the last 7 % of a labyrinth frame, a fifth of a fractal frame.  A wave that leaves after 8
// tiles is replaced by a younger one, the crawlers become the oldest and catch up.  Measured (ms per frame, one frame
// in flight; never / 4 / 8 / 16): labyrinth 4K 1.375 / 1.370 / 1.359 / 1.366, cube_sea 1080p 0.883 / 0.844 / 0.840 /
// 0.877, fractal 4K 1.607 / 1.470 / 1.485 / 1.549 (one wave per tile: 1.397, -, 1.482).
inline uint32_t pixel_launch_blocks(const PixelLaunchMode &mode, uint32_t tiles, uint32_t resident_blocks)
{
	if (!mode.persistent) return tiles;
	uint32_t blocks = resident_blocks;
	if (mode.retire_after > 0) blocks = resident_blocks / 2u + tiles / (uint32_t)mode.retire_after;
	if (blocks < resident_blocks) blocks = resident_blocks;
	return blocks < tiles ? blocks : tiles;
}
// RowMap::feedback_key of a launch: scene (index, or a hash of a run-time scene's name), frame width and what the row map selects,
// hashed into the upper 22 bits; the low 10 bits ARE the number of units (tile rows or squares, <= SDFR_ROW_FEEDBACK_MAX = 512) the
// order was made for: two launches with equal keys have equally long orders whatever the hash does
inline uint32_t pixel_feedback_key(uint32_t scene_key, int width, const RowMap &rm, uint32_t feedback_rows)
{
	static_assert(SDFR_ROW_FEEDBACK_MAX < 1024u, "the unit count rides in the key's low 10 bits");
	if (feedback_rows > SDFR_ROW_FEEDBACK_MAX) return 0u; // no feedback for such a launch (the kernel and the fold agree: fb_rows <= MAX)
	// FNV-1a over what a row order depends on; never 0
	uint32_t h = 2166136261u;
	const uint32_t words[] = {scene_key, (uint32_t)width, (uint32_t)rm.local_rows, (uint32_t)rm.rank, (uint32_t)rm.world, (uint32_t)rm.tile_w_log2,
		(uint32_t)rm.priv_count, (uint32_t)rm.priv_period, (uint32_t)rm.direct, rm.unit_log2};
	for (uint32_t w : words)
		for (int b = 0; b < 4; ++b) h = (h ^ ((w >> (8 * b)) & 0xffu)) * 16777619u;
	h = (h & ~1023u) | feedback_rows;
	return h ? h : 1024u;
}

// One launch of the pixel kernel and the fold that follows it.
struct PixelLaunchPlan
{
	bool fits;                // false: the workspace is too small for the launch, which is not made
	RowMap rows;              // PixelKernelArgs::rm: the caller's row map with the hand-out units, retire_after and feedback_key of this launch
	uint32_t n_work;          // work items handed out (PixelKernelArgs::n_work): the frame's, or those of the squares that cover it
	uint32_t blocks;          // grid of the pixel kernel; as many counter records for the fold
	bool tile_cursors;        // a persistent launch: the kernel gets the tile cursors (the fold gets them either way)
	uint32_t feedback_rows;   // units the fold sorts for the next frame (0: not a persistent launch)
	unsigned long long frame_pixels; // the fold's measure of "many rays per pixel"
};
// rm: as the API makes it (api_row_map); capacity: items the workspace holds (one counter record
// per block, at most one block per tile handed out); resident_blocks_per_cu: the occupancy query's answer for the kernel, >= 1
inline PixelLaunchPlan plan_pixel_launch(const PixelSceneTraits &scene, const PixelLaunchKnobs &knobs, int launch_mode, int width, const RowMap &rm,
	size_t capacity, int resident_blocks_per_cu, int cus)
{
	PixelLaunchPlan p = {};
	const uint32_t n_work = launch_work_items(width, rm);
	const uint32_t tiles_blocks = (n_work + SDFR_TILE_ITEMS - 1) / SDFR_TILE_ITEMS;
	const PixelLaunchMode mode = pixel_launch_mode(knobs, launch_mode, scene.persistent_tiles, scene.retire_after);
	uint32_t per_cu = (uint32_t)resident_blocks_per_cu;
	if (mode.blocks_per_cu > 0 && (uint32_t)mode.blocks_per_cu < per_cu) per_cu = (uint32_t)mode.blocks_per_cu;
	p.rows = rm;
	p.n_work = n_work;
	if (mode.persistent && scene.square_units && knobs.square_units != 0)
	{
		// full frames are handed out in squares of tiles, dearest square first (RowMap::unit_log2); the squares cover the frame with a margin
		const uint32_t padded = row_map_square_items(p.rows);
		if (padded) p.n_work = padded;
	}
	if ((size_t)n_work > capacity || (size_t)p.n_work > capacity) return p;
	p.fits = true;
	p.blocks = pixel_launch_blocks(mode, (p.n_work + SDFR_TILE_ITEMS - 1) / SDFR_TILE_ITEMS, (uint32_t)cus * per_cu);
	p.tile_cursors = mode.persistent;
	p.rows.retire_after = mode.persistent ? (uint32_t)mode.retire_after : 0u;
	const uint32_t tiles_x = ((uint32_t)width + (1u << rm.tile_w_log2) - 1u) >> rm.tile_w_log2;
	p.feedback_rows = !mode.persistent ? 0u : p.rows.unit_log2 ? p.rows.units : tiles_blocks / tiles_x;
	p.rows.feedback_key = mode.persistent ? pixel_feedback_key(scene.feedback_key, width, p.rows, p.feedback_rows) : 0u;
	// (the fold leaves frames with many rays per pixel in image order, SDFR_ROW_FEEDBACK_MAX_RAYS: a rule about tile ROWS -- their queue records
	// are contiguous in image order --, not about squares, which scatter them either way)
	p.frame_pixels = p.rows.unit_log2 ? ~0ull >> 8 : (unsigned long long)n_work;
	return p;
}

} // namespace sdfr

// tests/cpp/launch_plan_host.cpp -- TEST-ONLY: the pixel launch plan (sdf_playground_amd/csrc/sdfr_launch_plan.h) compiled for the
// CPU, so that tests/test_launch_plan_cpu.py can check the launch policy without a GPU.  The product never loads this.
#include "sdfr_launch_plan.h"

using namespace sdfr;

extern "C" {

struct LpIn
{
	int32_t persistent_tiles, retire_after, square_units;
	uint32_t scene_key;
	int32_t knob_persistent, knob_blocks_per_cu, knob_retire_after, knob_square_units;
	int32_t launch_mode, width;
	int32_t local_rows, rank, world, tile_w_log2, priv_count, priv_period, direct;
	int32_t resident_blocks_per_cu, cus;
	uint64_t capacity;
};
struct LpOut
{
	int32_t fits, tile_cursors;
	uint32_t tiles_x, tiles_x_magic, unit_log2, units_x, units_x_magic, units, retire_after, feedback_key;
	uint32_t n_work, blocks, feedback_rows;
	uint32_t work_items, capacity_items; // launch_work_items, launch_capacity_items of the row map
	uint64_t frame_pixels;
};

// the row map as the API makes it (api_row_map), then the plan
void lp_plan(int n, const LpIn *in, LpOut *out)
{
	for (int i = 0; i < n; ++i)
	{
		const LpIn &a = in[i];
		const RowMap rm = api_row_map(a.width, a.local_rows, a.rank, a.world, a.tile_w_log2, a.priv_count, a.priv_period, a.direct);
		const PixelSceneTraits scene = {a.persistent_tiles != 0, a.retire_after, a.square_units != 0, a.scene_key};
		const PixelLaunchKnobs knobs = {a.knob_persistent, a.knob_blocks_per_cu, a.knob_retire_after, a.knob_square_units};
		const PixelLaunchPlan p = plan_pixel_launch(scene, knobs, a.launch_mode, a.width, rm, (size_t)a.capacity, a.resident_blocks_per_cu, a.cus);
		LpOut &o = out[i];
		o.fits = p.fits ? 1 : 0;
		o.tile_cursors = p.tile_cursors ? 1 : 0;
		o.tiles_x = p.rows.tiles_x;
		o.tiles_x_magic = p.rows.tiles_x_magic;
		o.unit_log2 = p.rows.unit_log2;
		o.units_x = p.rows.units_x;
		o.units_x_magic = p.rows.units_x_magic;
		o.units = p.rows.units;
		o.retire_after = p.rows.retire_after;
		o.feedback_key = p.rows.feedback_key;
		o.n_work = p.n_work;
		o.blocks = p.blocks;
		o.feedback_rows = p.feedback_rows;
		o.work_items = launch_work_items(a.width, rm);
		o.capacity_items = launch_capacity_items(a.width, rm);
		o.frame_pixels = p.frame_pixels;
	}
}

// the rows of a render of the API: render mode, frame, rank / world, tile shape and the handle's strip split -> FrameRows
struct FrIn
{
	int32_t mode, width, height, rank, world, tile_w_log2, priv_count, priv_period;
};
static_assert(sizeof(FrameRows) == 72, "FrameRows as tests/test_launch_plan_cpu.py spells it: the 15 words of RowMap, then the pixels");
void lp_frame_rows(int n, const FrIn *in, FrameRows *out)
{
	for (int i = 0; i < n; ++i)
		out[i] = frame_rows((RenderMode)in[i].mode, in[i].width, in[i].height, in[i].rank, in[i].world, in[i].tile_w_log2, in[i].priv_count, in[i].priv_period);
}

int lp_row_feedback_max() { return (int)SDFR_ROW_FEEDBACK_MAX; }
} // extern "C"

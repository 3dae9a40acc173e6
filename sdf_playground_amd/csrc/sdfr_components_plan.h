// sdfr_components_plan.h -- sdfr_components_label and sdfr_components_label_lattice (include/sdfr.h) as far as the host decides them: the
// argument checks in the order their errors win, the grid, the lattice launch's arguments, the sizes of the workspace's pieces, the
// blocks of every launch, and once the number of components is read back the table's bytes and whether the call fills the caller's
// records.  Plain host arithmetic, no HIP call, like sdfr_mesh_plan.h: components_impl (sdfr_api.cpp) carries the plan out,
// tests/test_components_cpu.py checks it on a machine without a GPU.
#pragma once
#include "sdfr_components.h"
#include "sdfr_mesh_plan.h"

namespace sdfr {

// What the entry point was given; but for the grid's, the pointers are only compared with null here
struct ComponentsRequest
{
	const MeshGrid *grid; // sdfr_mesh_grid, field for field
	bool own_lattice;     // sdfr_components_label_lattice: the distances are the caller's `lattice`, and no scene is needed
	const void *lattice;
	int64_t capacity;
	const void *records, *labels, *counts;
	int on_host;
};
enum
{
	COMPONENTS_WORK_LATTICE, // the scene's distances (none with the caller's lattice)
	COMPONENTS_WORK_PARENT,  // parent[points]; after the numbering the points' labels
	COMPONENTS_WORK_SCAN,    // the root flags and their exclusive prefix sum [points + 1], whose last element is the number of components
	COMPONENTS_WORK_SUMS,    // ... its block sums
	COMPONENTS_WORK_RESULT,  // the 64 bytes of counts and the words they are counted in
	COMPONENTS_WORK_TABLE,   // a Component per component, behind all others: room for COMPONENTS_TABLE_FIRST at first, cut anew -- the others keep their places -- once their number is known and larger
	COMPONENTS_WORK_PIECES
};
enum { COMPONENTS_BLOCK = 256, COMPONENTS_BRICK_POINTS = 512 }; // threads of the per-point kernels, 64-lane waves; of a block of the brick stage
enum { COMPONENTS_TALLY_RUNS = 64, COMPONENTS_TALLY_GROUPS = 4, COMPONENTS_TALLY_POINTS = 64 * COMPONENTS_TALLY_RUNS }; // a wave of the tally: runs of 64 points, labels grouped per run
enum { COMPONENTS_TABLE_FIRST = 1 << 16 };                      // components the workspace has room for before they are counted (or every point's, if fewer)
struct ComponentsPlan
{
	int status; // QUERY_PLAN_*
	const char *error;
	MeshGrid g;
	LatticeArgs lattice; // but `rows` and `out`
	size_t points;
	size_t work[COMPONENTS_WORK_PIECES]; // the table's: the first guess, until plan_components_fill
	size_t lattice_bytes, label_bytes;   // of the caller's lattice and labels (not given: 0)
	// the brick stage's (8 x 8 x 8 points each); one lane per point; ... and one for the scan's last element; the tally's (COMPONENTS_TALLY_POINTS per wave)
	uint32_t brick_blocks, point_blocks, root_blocks, tally_blocks;
};

// bricks per axis and in all
inline uint32_t components_bricks(const MeshGrid &g)
{
	uint32_t n = 1;
	for (int a = 0; a < 3; ++a) n *= ((uint32_t)g.n[a] + 1u + 7u) / 8u;
	return n;
}

// The checks after the handle's and before the scene's, in the order their errors win.
inline ComponentsPlan plan_components(const ComponentsRequest &c)
{
	ComponentsPlan p = {};
	auto fail = [&p](const char *text) {
		p.status = QUERY_PLAN_INVALID_ARGUMENT;
		p.error = text;
		return p;
	};
	if (!c.grid || !c.counts || (c.own_lattice && !c.lattice)) return fail("null pointer");
	if (!is_flag(c.on_host)) return fail("on_host must be 0 or 1");
	const MeshGrid &g = *c.grid;
	if (!mesh_grid_ok(g)) return fail("bad mesh grid");
	if (c.capacity < 0) return fail("negative capacity");
	if (c.capacity > 0 && !c.records) return fail("null array with a capacity");

	p.g = g;
	p.lattice = mesh_lattice_args(g);
	p.points = mesh_point_count(g);
	p.work[COMPONENTS_WORK_LATTICE] = c.own_lattice ? 0 : p.points * 4;
	p.work[COMPONENTS_WORK_PARENT] = p.points * 4;
	p.work[COMPONENTS_WORK_SCAN] = (p.points + 1) * 4;
	p.work[COMPONENTS_WORK_SUMS] = mesh_scan_sum_words(p.points + 1) * 4;
	p.work[COMPONENTS_WORK_RESULT] = COMPONENT_RESULT_BYTES;
	p.work[COMPONENTS_WORK_TABLE] = (p.points < (size_t)COMPONENTS_TABLE_FIRST ? p.points : (size_t)COMPONENTS_TABLE_FIRST) * sizeof(Component);
	p.lattice_bytes = c.own_lattice ? p.points * 4 : 0;
	p.label_bytes = c.labels ? p.points * 4 : 0;
	p.brick_blocks = components_bricks(g);
	p.point_blocks = (uint32_t)((p.points + COMPONENTS_BLOCK - 1) / COMPONENTS_BLOCK);
	p.root_blocks = (uint32_t)(p.points / COMPONENTS_BLOCK + 1);
	const size_t per_block = (size_t)COMPONENTS_TALLY_POINTS * (COMPONENTS_BLOCK / 64);
	p.tally_blocks = (uint32_t)((p.points + per_block - 1) / per_block);
	return p;
}

// The second phase, with the number of components the device counted: the table's bytes (never fewer than the first guess), the blocks of the launch that has one lane
// per component, and whether the capacity allows the call to fill the caller's records (the mesh's rule) and with how many bytes
struct ComponentsFill
{
	int64_t components;
	bool fill;
	size_t table_bytes, record_bytes;
	uint32_t component_blocks;
};
inline ComponentsFill plan_components_fill(const ComponentsRequest &c, const ComponentsPlan &p, uint32_t components)
{
	ComponentsFill f = {};
	f.components = (int64_t)components;
	f.fill = f.components <= c.capacity;
	f.record_bytes = f.fill ? (size_t)components * sizeof(Component) : 0;
	f.table_bytes = (size_t)components * sizeof(Component);
	if (f.table_bytes < p.work[COMPONENTS_WORK_TABLE]) f.table_bytes = p.work[COMPONENTS_WORK_TABLE]; // (the first guess holds them: nothing moves)
	f.component_blocks = (components + (uint32_t)COMPONENTS_BLOCK - 1u) / (uint32_t)COMPONENTS_BLOCK;
	return f;
}

} // namespace sdfr

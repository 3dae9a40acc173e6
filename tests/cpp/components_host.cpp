// components_host.cpp -- sdfr_components_label's rules (sdf_playground_amd/csrc/sdfr_components.h) on the CPU, for tests/components_util.py:
// the union step with a plain min in place of atomicMin, run over the lattice's edges in the order the caller names, then flatten, number
// and tally as the kernels do.  Sequential: what order the unions run in is the test's to choose.
#include "sdfr_components.h"

#include <vector>

using namespace sdfr;

struct PlainMinExchange
{
	uint32_t operator()(uint32_t *word, uint32_t value) const
	{
		const uint32_t old = *word;
		if (value < old) *word = value;
		return old;
	}
};

extern "C" {

// sizeof of: 0 MeshGrid, 1 Component, 2 ComponentCounts
int cmp_sizes(int what) { return what == 0 ? (int)sizeof(MeshGrid) : what == 1 ? (int)sizeof(Component) : (int)sizeof(ComponentCounts); }

// D [points]; order [n_order]: edge slots 3 x + a (the edge from point x along axis a; no such edge: skipped), or null: every slot in
// ascending order.  records and labels: [points].  -> the number of components
int64_t cmp_label(const MeshGrid *grid, const float *D, const int64_t *order, int64_t n_order, Component *records, uint32_t *labels, ComponentCounts *counts)
{
	const MeshGrid &g = *grid;
	const uint32_t points = mesh_point_count(g), px = (uint32_t)(g.n[0] + 1), py = (uint32_t)(g.n[1] + 1);
	const uint32_t step[3] = {1u, px, px * py};
	std::vector<uint32_t> parent(points);
	for (uint32_t x = 0; x < points; ++x) parent[x] = x;
	const int64_t slots = order ? n_order : (int64_t)3 * points;
	for (int64_t e = 0; e < slots; ++e)
	{
		const int64_t slot = order ? order[e] : e;
		if (slot < 0 || slot >= (int64_t)3 * points) continue;
		const uint32_t x = (uint32_t)(slot / 3);
		const int a = (int)(slot % 3);
		const int c[3] = {(int)(x % px), (int)((x / px) % py), (int)(x / (px * py))};
		if (c[a] >= g.n[a]) continue;
		const uint32_t y = x + step[a];
		if (!component_joined(component_kind(g, D[x]), component_kind(g, D[y]))) continue;
		components_union(parent.data(), components_find(parent.data(), x), components_find(parent.data(), y), PlainMinExchange());
	}
	for (uint32_t x = 0; x < points; ++x) parent[x] = components_find(parent.data(), x);
	uint32_t n = 0;
	for (uint32_t x = 0; x < points; ++x)
		if (parent[x] == x)
		{
			labels[x] = n; // (a root comes before every other point of its component)
			records[n++] = component_empty(g, x, component_kind(g, D[x]));
		}
	for (uint32_t x = 0; x < points; ++x)
	{
		const uint32_t l = labels[parent[x]];
		labels[x] = l;
		const int c[3] = {(int)(x % px), (int)((x / px) % py), (int)(x / (px * py))};
		Component &r = records[l];
		r.points += 1;
		for (int a = 0; a < 3; ++a)
		{
			if (c[a] < r.lo[a]) r.lo[a] = c[a];
			if (c[a] > r.hi[a]) r.hi[a] = c[a];
		}
		r.flags |= component_point_faces(g, c[0], c[1], c[2]);
	}
	ComponentCounts total = {};
	for (uint32_t l = 0; l < n; ++l) component_count(total, records[l]);
	*counts = total;
	return (int64_t)n;
}

} // extern "C"

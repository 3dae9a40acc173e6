// sdfr_components.h -- the parts and enclosed voids of the solid on a lattice of scene distances: sdfr_components_label (include/sdfr.h,
// where the definition stands in full) as far as one point, one edge or one component decides it.  Scene-independent
// and host-compilable, like sdfr_mesh.h, whose grid, point index and inside test these are: sdfr_components.hip runs them one lane per
// lattice point, tests/cpp/components_host.cpp runs the same text sequentially on the CPU.  Everything is an integer, so neither the
// order of the unions nor the machine changes a result.
//
// The union is Playne and Hawick's lock-free form over parent[], in which parent[x] <= x always holds and every value ever stored in
// parent[x] is a point of x's set.  It is templated on how a word is min-ed: atomicMin on the device (LDS inside a brick, global memory
// across bricks), a plain min in the host stand-in.  max(a, b) falls strictly each turn, so the loop ends whatever other lanes do; no
// lane ever waits for another.  What the loop acts on is what the min returned -- a find through plain loads (components_find) may read
// a stale word, which is still a point of the set with an index <= x, so it is a shortcut and never what correctness rests on.
#pragma once
#include "sdfr_mesh.h"

namespace sdfr {

// 8 x 8 x 8 points per brick of the brick stage; 0: a developer build without that stage, every edge united in global memory -- the A/B of
// DESIGN.md 4.17 (buildlib.build(extra=["-DSDFR_COMPONENTS_BRICK=0"])).  The bits are the same either way.
#ifndef SDFR_COMPONENTS_BRICK
#define SDFR_COMPONENTS_BRICK 8
#endif
static_assert(SDFR_COMPONENTS_BRICK == 8 || SDFR_COMPONENTS_BRICK == 0, "bricks of 8 x 8 x 8 points, or none");

struct Component // sdfr_component, field for field
{
	uint32_t root;  // the smallest linear index of the component's points
	uint32_t flags; // COMPONENT_INSIDE, COMPONENT_FACE << face
	int64_t points;
	int32_t lo[3], hi[3]; // inclusive point indices
};
struct ComponentCounts // sdfr_component_counts, field for field
{
	int64_t components, solids, voids, closed_solids, closed_voids, inside_points, largest_solid_points, largest_void_points;
};
enum : uint32_t
{
	COMPONENT_INSIDE = 1u,
	COMPONENT_FACE = 1u << 8,         // << 0 .. 5: a point with i == 0, i == px - 1, j == 0, j == py - 1, k == 0, k == pz - 1
	COMPONENT_FACES = 0x3fu << 8,     // none of them: the component is closed
};
enum
{
	COMPONENT_COUNT_WORDS = 7,        // the words counted over the components: ComponentCounts after `components`
	COMPONENT_WORD_STRIDE = 256,      // bytes between them while they are counted: atomics on one line queue up (sdfr_mesh.hip)
	COMPONENT_RESULT_BYTES = 256 * 8, // the packed counts, then each word in a line of its own
};

// the faces of the lattice the point (i, j, k) lies on, as flag bits
SDF_HD uint32_t component_point_faces(const MeshGrid &g, int i, int j, int k)
{
	const int c[3] = {i, j, k};
	uint32_t faces = 0u;
	for (int a = 0; a < 3; ++a)
	{
		if (c[a] == 0) faces |= COMPONENT_FACE << (2 * a);
		if (c[a] == g.n[a]) faces |= COMPONENT_FACE << (2 * a + 1);
	}
	return faces;
}

// The neighbour rule: two points next to each other along a lattice axis are joined iff both are inside or both are not.  kind: 1
// inside, 0 not (NaN is not inside)
SDF_HD uint32_t component_kind(const MeshGrid &g, float d) { return mesh_inside(g, d) ? 1u : 0u; }
SDF_HD bool component_joined(uint32_t kind_a, uint32_t kind_b) { return kind_a == kind_b; }

// the root x's chain leads to, through plain loads: a shortcut only (see above)
SDF_HD uint32_t components_find(const uint32_t *parent, uint32_t x)
{
	for (uint32_t p = parent[x]; p != x; p = parent[x]) x = p;
	return x;
}

// The union step.  min_exchange(word, value): *word = min(*word, value), -> what *word held before.
template <class MinExchange>
SDF_HD void components_union(uint32_t *parent, uint32_t a, uint32_t b, MinExchange &&min_exchange)
{
	while (a != b)
	{
		if (a < b)
		{
			const uint32_t t = a;
			a = b;
			b = t;
		}
		const uint32_t old = min_exchange(parent + a, b);
		if (old == a) break; // a was a root, and now hangs below b
		a = old;             // a's set is old's: old < a, b < a
	}
}

// a component before its first point is tallied
SDF_HD Component component_empty(const MeshGrid &g, uint32_t root, uint32_t kind)
{
	Component c = {};
	c.root = root;
	c.flags = kind ? COMPONENT_INSIDE : 0u;
	for (int a = 0; a < 3; ++a)
	{
		c.lo[a] = g.n[a] + 1;
		c.hi[a] = -1;
	}
	return c;
}

// what a component adds to the counts (sequentially: the host stand-in; the device reduces the same integers in waves)
SDF_HD void component_count(ComponentCounts &n, const Component &c)
{
	const bool solid = (c.flags & COMPONENT_INSIDE) != 0u, closed = (c.flags & COMPONENT_FACES) == 0u;
	n.components += 1;
	if (solid)
	{
		n.solids += 1;
		n.closed_solids += closed ? 1 : 0;
		n.inside_points += c.points;
		if (c.points > n.largest_solid_points) n.largest_solid_points = c.points;
	}
	else
	{
		n.voids += 1;
		n.closed_voids += closed ? 1 : 0;
		if (c.points > n.largest_void_points) n.largest_void_points = c.points;
	}
}

} // namespace sdfr

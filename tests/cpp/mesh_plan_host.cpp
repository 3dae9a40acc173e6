// mesh_plan_host.cpp -- the plan of sdfr_mesh_extract (sdf_playground_amd/csrc/sdfr_mesh_plan.h) as a stand-alone host program (no HIP
// header on the include path), for tests/test_mesh_plan_cpu.py.  Every line of standard input is a request and the totals of its second phase:
//   have_grid ox oy oz cell nx ny nz iso  vertex_capacity triangle_capacity  positions normals indices counts (0: null, 1: given)  on_host  V Q
// The answer is one line: "status;error text", and for a plan that stands
//   ";origin cell iso (floats as their bits) nx ny nz;the lattice launch's origin cell (bits) px py pz;points cells;the four workspace sizes"
//   ";fill vertices triangles;the three answer sizes".
#include "sdfr_mesh_plan.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace sdfr;

static uint32_t bits(float f)
{
	uint32_t u;
	memcpy(&u, &f, 4);
	return u;
}

int main()
{
	char line[1024];
	while (fgets(line, sizeof line, stdin))
	{
		char *tok[18];
		int n = 0;
		for (char *t = strtok(line, " \n"); t && n < 18; t = strtok(nullptr, " \n")) tok[n++] = t;
		if (n != 18) return 2;
		MeshGrid g;
		for (int a = 0; a < 3; ++a) g.origin[a] = strtof(tok[1 + a], nullptr);
		g.cell = strtof(tok[4], nullptr);
		for (int a = 0; a < 3; ++a) g.n[a] = atoi(tok[5 + a]);
		g.iso = strtof(tok[8], nullptr);
		static float array[3];
		static uint32_t index_array[3];
		MeshRequest c = {};
		c.grid = atoi(tok[0]) ? &g : nullptr;
		c.vertex_capacity = strtoll(tok[9], nullptr, 10);
		c.triangle_capacity = strtoll(tok[10], nullptr, 10);
		c.positions = atoi(tok[11]) ? array : nullptr;
		c.normals = atoi(tok[12]) ? array : nullptr;
		c.indices = atoi(tok[13]) ? index_array : nullptr;
		c.counts = atoi(tok[14]) ? array : nullptr;
		c.on_host = atoi(tok[15]);

		const MeshPlan p = plan_mesh(c);
		printf("%d;%s", p.status, p.error ? p.error : "");
		if (p.status == QUERY_PLAN_OK)
		{
			printf(";%08x %08x %08x %08x %08x %d %d %d", bits(p.g.origin[0]), bits(p.g.origin[1]), bits(p.g.origin[2]), bits(p.g.cell), bits(p.g.iso), p.g.n[0], p.g.n[1], p.g.n[2]);
			printf(";%08x %08x %08x %08x %d %d %d", bits(p.lattice.origin[0]), bits(p.lattice.origin[1]), bits(p.lattice.origin[2]), bits(p.lattice.cell), p.lattice.px, p.lattice.py,
				p.lattice.pz);
			printf(";%zu %zu;%zu %zu %zu %zu", p.points, p.cells, p.work[0], p.work[1], p.work[2], p.work[3]);
			const MeshFill f = plan_mesh_fill(c, (uint32_t)strtoul(tok[16], nullptr, 10), (uint32_t)strtoul(tok[17], nullptr, 10));
			printf(";%d %" PRId64 " %" PRId64 ";%zu %zu %zu", f.fill ? 1 : 0, f.vertices, f.triangles, f.bytes[0], f.bytes[1], f.bytes[2]);
		}
		printf("\n");
	}
	return 0;
}

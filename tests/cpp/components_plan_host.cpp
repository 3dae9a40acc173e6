// components_plan_host.cpp -- the plan of sdfr_components_label (sdf_playground_amd/csrc/sdfr_components_plan.h) as a stand-alone host
// program (no HIP header on the include path), for tests/test_components_cpu.py.  Every line of standard input is a request and the number
// of components of its second phase:
//   have_grid ox oy oz cell nx ny nz iso  own_lattice lattice  capacity  records labels counts (0: null, 1: given)  on_host  C
// The answer is one line: "status;error text", and for a plan that stands
//   ";iso (its bits) nx ny nz;the lattice launch's px py pz;points;the six workspace sizes;lattice bytes, label bytes;the four block counts"
//   ";fill components;table bytes, record bytes, component blocks;the whole workspace's bytes".
#include "sdfr_components_plan.h"
#include "sdfr_stage.h"

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
		char *tok[17];
		int n = 0;
		for (char *t = strtok(line, " \n"); t && n < 17; t = strtok(nullptr, " \n")) tok[n++] = t;
		if (n != 17) return 2;
		MeshGrid g;
		for (int a = 0; a < 3; ++a) g.origin[a] = strtof(tok[1 + a], nullptr);
		g.cell = strtof(tok[4], nullptr);
		for (int a = 0; a < 3; ++a) g.n[a] = atoi(tok[5 + a]);
		g.iso = strtof(tok[8], nullptr);
		static float array[3];
		ComponentsRequest c = {};
		c.grid = atoi(tok[0]) ? &g : nullptr;
		c.own_lattice = atoi(tok[9]) != 0;
		c.lattice = atoi(tok[10]) ? array : nullptr;
		c.capacity = strtoll(tok[11], nullptr, 10);
		c.records = atoi(tok[12]) ? array : nullptr;
		c.labels = atoi(tok[13]) ? array : nullptr;
		c.counts = atoi(tok[14]) ? array : nullptr;
		c.on_host = atoi(tok[15]);

		const ComponentsPlan p = plan_components(c);
		printf("%d;%s", p.status, p.error ? p.error : "");
		if (p.status == QUERY_PLAN_OK)
		{
			printf(";%08x %d %d %d;%d %d %d;%zu;", bits(p.g.iso), p.g.n[0], p.g.n[1], p.g.n[2], p.lattice.px, p.lattice.py, p.lattice.pz, p.points);
			for (int k = 0; k < COMPONENTS_WORK_PIECES; ++k) printf("%s%zu", k ? " " : "", p.work[k]);
			printf(";%zu %zu;%u %u %u %u", p.lattice_bytes, p.label_bytes, p.brick_blocks, p.point_blocks, p.root_blocks, p.tally_blocks);
			const ComponentsFill f = plan_components_fill(c, p, (uint32_t)strtoul(tok[16], nullptr, 10));
			printf(";%d %" PRId64 ";%zu %zu %u", f.fill ? 1 : 0, f.components, f.table_bytes, f.record_bytes, f.component_blocks);
			size_t pieces[COMPONENTS_WORK_PIECES], offsets[COMPONENTS_WORK_PIECES];
			for (int k = 0; k < COMPONENTS_WORK_PIECES; ++k) pieces[k] = p.work[k];
			pieces[COMPONENTS_WORK_TABLE] = f.table_bytes;
			printf(";%zu", stage_offsets(pieces, COMPONENTS_WORK_PIECES, offsets));
		}
		printf("\n");
	}
	return 0;
}

// slice_plan_host.cpp -- the plan of sdfr_slice_extract (sdf_playground_amd/csrc/sdfr_slice_plan.h) as a stand-alone host program (no HIP
// header on the include path), for tests/test_slice_cpu.py.  Every line of standard input is a request and the totals of its second phase:
//   have_grid origin[3] du[3] dv[3] dw[3] nu nv layers iso  vertex_capacity segment_capacity  positions coords segments counts (0: null,
//   1: given)  on_host  V S
// The answer is one line: "status;error text", and for a plan that stands
//   ";the grid's 12 floats and iso (as their bits) nu nv layers;the sampling launch's 12 floats (bits) pu pv layers, its blocks in tiles
//   and in rows;points;the five workspace sizes;fill vertices segments;the three answer sizes".
#include "sdfr_slice_plan.h"

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
	char line[2048];
	while (fgets(line, sizeof line, stdin))
	{
		char *tok[26];
		int n = 0;
		for (char *t = strtok(line, " \n"); t && n < 26; t = strtok(nullptr, " \n")) tok[n++] = t;
		if (n != 26) return 2;
		SliceGrid g;
		for (int a = 0; a < 3; ++a)
		{
			g.origin[a] = strtof(tok[1 + a], nullptr);
			g.du[a] = strtof(tok[4 + a], nullptr);
			g.dv[a] = strtof(tok[7 + a], nullptr);
			g.dw[a] = strtof(tok[10 + a], nullptr);
		}
		g.nu = atoi(tok[13]);
		g.nv = atoi(tok[14]);
		g.layers = atoi(tok[15]);
		g.iso = strtof(tok[16], nullptr);
		static float array[3];
		static uint32_t index_array[3];
		SliceRequest c = {};
		c.grid = atoi(tok[0]) ? &g : nullptr;
		c.vertex_capacity = strtoll(tok[17], nullptr, 10);
		c.segment_capacity = strtoll(tok[18], nullptr, 10);
		c.positions = atoi(tok[19]) ? array : nullptr;
		c.coords = atoi(tok[20]) ? array : nullptr;
		c.segments = atoi(tok[21]) ? index_array : nullptr;
		c.counts = atoi(tok[22]) ? array : nullptr;
		c.on_host = atoi(tok[23]);

		const SlicePlan p = plan_slice(c);
		printf("%d;%s", p.status, p.error ? p.error : "");
		if (p.status == QUERY_PLAN_OK)
		{
			printf(";");
			for (int a = 0; a < 3; ++a) printf("%08x ", bits(p.g.origin[a]));
			for (int a = 0; a < 3; ++a) printf("%08x ", bits(p.g.du[a]));
			for (int a = 0; a < 3; ++a) printf("%08x ", bits(p.g.dv[a]));
			for (int a = 0; a < 3; ++a) printf("%08x ", bits(p.g.dw[a]));
			printf("%08x %d %d %d;", bits(p.g.iso), p.g.nu, p.g.nv, p.g.layers);
			for (int a = 0; a < 3; ++a) printf("%08x ", bits(p.sample.origin[a]));
			for (int a = 0; a < 3; ++a) printf("%08x ", bits(p.sample.du[a]));
			for (int a = 0; a < 3; ++a) printf("%08x ", bits(p.sample.dv[a]));
			for (int a = 0; a < 3; ++a) printf("%08x ", bits(p.sample.dw[a]));
			SliceArgs rows = p.sample;
			rows.rows = 1;
			printf("%d %d %d %u %u", p.sample.pu, p.sample.pv, p.sample.layers, slice_sample_blocks(p.sample), slice_sample_blocks(rows));
			printf(";%zu;%zu %zu %zu %zu %zu", p.points, p.work[0], p.work[1], p.work[2], p.work[3], p.work[4]);
			const SliceFill f = plan_slice_fill(c, (uint32_t)strtoul(tok[24], nullptr, 10), (uint32_t)strtoul(tok[25], nullptr, 10));
			printf(";%d %" PRId64 " %" PRId64 ";%zu %zu %zu", f.fill ? 1 : 0, f.vertices, f.segments, f.bytes[0], f.bytes[1], f.bytes[2]);
		}
		printf("\n");
	}
	return 0;
}

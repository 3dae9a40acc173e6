// query_plan_host.cpp -- the query table and plan of sdf_playground_amd/csrc/sdfr_query_plan.h as a stand-alone host program (no HIP header
// on the include path), for tests/test_query_plan_cpu.py.  Every line of standard input is a request:
//   kind n on_host reach bias width height want_surfaces range  pos dir pixels distance normals hits surfaces hit_items occlusion
// the nine arrays as 0 (null) or 1 .. 6 (an address that stands for itself: code << 44, far apart enough for any offset).  The answer is
// one line: "status;error text", and for a plan that has something to do
//   ";kernel;width height;the four staging sizes;kind n dist_max reach bias (floats as their bits);the nine pointers" and per launch
//   ";first count blocks n, the nine pointers of that launch".
#include "sdfr_query_plan.h"

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
static void print_pointers(const QueryArgs &q)
{
	const void *p[9] = {q.pos, q.dir, q.pixels, q.distance, q.normals, q.hits, q.surfaces, q.hit_items, q.occlusion};
	for (const void *v : p) printf(" %" PRIxPTR, (uintptr_t)v);
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
		QueryRequest c = query_request(atoi(tok[0]), strtoll(tok[1], nullptr, 10), atoi(tok[2]));
		c.q.reach = strtof(tok[3], nullptr);
		c.q.bias = strtof(tok[4], nullptr);
		c.width = atoi(tok[5]);
		c.height = atoi(tok[6]);
		c.want_surfaces = atoi(tok[7]) != 0;
		const float range = strtof(tok[8], nullptr);
		uintptr_t a[9];
		for (int k = 0; k < 9; ++k) a[k] = (uintptr_t)strtoull(tok[9 + k], nullptr, 10) << 44;
		c.q.pos = (const float *)a[0];
		c.q.dir = (const float *)a[1];
		c.q.pixels = (const int32_t *)a[2];
		c.q.distance = (float *)a[3];
		c.q.normals = (float *)a[4];
		c.q.hits = (uint32_t *)a[5];
		c.q.surfaces = (uint32_t *)a[6];
		c.q.hit_items = (const uint32_t *)a[7];
		c.q.occlusion = (uint32_t *)a[8];

		const QueryPlan p = plan_query(c, range);
		printf("%d;%s", p.status, p.error ? p.error : "");
		if (p.status == QUERY_PLAN_OK && !p.nothing_to_do)
		{
			printf(";%d;%d %d;%zu %zu %zu %zu;%d %d %08x %08x %08x;", p.kernel, p.width, p.height, p.bytes[0], p.bytes[1], p.bytes[2], p.bytes[3], p.q.kind, p.q.n,
				bits(p.q.dist_max), bits(p.q.reach), bits(p.q.bias));
			print_pointers(p.q);
			for (uint32_t k = 0; k < p.launches; ++k)
			{
				const QueryLaunch l = query_launch(p.q, p.width, p.height, k);
				const QueryArgs q = query_launch_args(p.q, l);
				printf(";%u %u %u %d", l.first, l.count, l.blocks, q.n);
				print_pointers(q);
			}
		}
		printf("\n");
	}
	return 0;
}

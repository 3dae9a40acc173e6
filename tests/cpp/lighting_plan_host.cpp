// lighting_plan_host.cpp -- the plan of the lighting entries (sdf_playground_amd/csrc/sdfr_query_plan.h: QueryRequest::want_lighting) as a
// stand-alone host program (no HIP header on the include path), for tests/test_lighting_plan_cpu.py; query_plan_host.cpp covers the
// requests that existed before.  Every line of standard input is a request:
//   kind n on_host reach width height range  pos dir pixels hits surfaces lighting lights
// the seven arrays as 0 (null) or 1 .. 7 (an address that stands for itself: code << 44).  The answer is one line: "status;error text",
// and for a plan that has something to do ";kernel;width height;the six staging sizes;n dist_max (bits);the seven pointers" and per launch
// ";first count blocks n, the seven pointers of that launch".
#include "sdfr_query_plan.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace sdfr;

static void print_pointers(const QueryArgs &q)
{
	const void *p[7] = {q.pos, q.dir, q.pixels, q.hits, q.surfaces, q.lighting, q.lights};
	for (const void *v : p) printf(" %" PRIxPTR, (uintptr_t)v);
}

int main()
{
	char line[1024];
	while (fgets(line, sizeof line, stdin))
	{
		char *tok[14];
		int n = 0;
		for (char *t = strtok(line, " \n"); t && n < 14; t = strtok(nullptr, " \n")) tok[n++] = t;
		if (n != 14) return 2;
		QueryRequest c = query_request(atoi(tok[0]), strtoll(tok[1], nullptr, 10), atoi(tok[2]));
		c.q.reach = strtof(tok[3], nullptr);
		c.width = atoi(tok[4]);
		c.height = atoi(tok[5]);
		c.want_lighting = true;
		const float range = strtof(tok[6], nullptr);
		uintptr_t a[7];
		for (int k = 0; k < 7; ++k) a[k] = (uintptr_t)strtoull(tok[7 + k], nullptr, 10) << 44;
		c.q.pos = (const float *)a[0];
		c.q.dir = (const float *)a[1];
		c.q.pixels = (const int32_t *)a[2];
		c.q.hits = (uint32_t *)a[3];
		c.q.surfaces = (uint32_t *)a[4];
		c.q.lighting = (uint32_t *)a[5];
		c.q.lights = (uint32_t *)a[6];

		const QueryPlan p = plan_query(c, range);
		printf("%d;%s", p.status, p.error ? p.error : "");
		if (p.status == QUERY_PLAN_OK && !p.nothing_to_do)
		{
			uint32_t dist_max;
			memcpy(&dist_max, &p.q.dist_max, 4);
			printf(";%d;%d %d;%zu %zu %zu %zu %zu %zu;%d %08x;", p.kernel, p.width, p.height, p.bytes[0], p.bytes[1], p.bytes[2], p.bytes[3], p.bytes[4], p.bytes[5],
				p.q.n, dist_max);
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

// span_plan_host.cpp -- the plan of the span queries (sdf_playground_amd/csrc/sdfr_span_plan.h) as a stand-alone host program (no HIP header
// on the include path), for tests/test_span_cpu.py.  Every line of standard input is a request:
//   kind (1 rays, 2 pick, 4 mesh)  n  in0 in1 (0: null, 1: given)  width height  reach  params (0: null, 1: given)  t_max min_step iso
//   max_steps max_spans  summaries spans (0: null, 1: given)  on_host  range
// The answer is one line: "status;error text", and for a plan that stands ";nothing_to_do", and for one with something to do
//   ";kind n, which of pos dir pixels summaries spans are there (0 / 1), reach t_max min_step iso (as their bits), max_steps max_spans;
//   the four staging sizes;width height;blocks".
#include "sdfr_span_plan.h"

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
		static float array[3];
		SpanParams sp;
		sp.t_max = strtof(tok[8], nullptr);
		sp.min_step = strtof(tok[9], nullptr);
		sp.iso = strtof(tok[10], nullptr);
		sp.max_steps = atoi(tok[11]);
		sp.max_spans = atoi(tok[12]);
		SpanRequest c = {};
		c.kind = atoi(tok[0]);
		c.n = strtoll(tok[1], nullptr, 10);
		c.in0 = atoi(tok[2]) ? array : nullptr;
		c.in1 = atoi(tok[3]) ? array : nullptr;
		c.width = atoi(tok[4]);
		c.height = atoi(tok[5]);
		c.reach = strtof(tok[6], nullptr);
		c.params = atoi(tok[7]) ? &sp : nullptr;
		c.summaries = atoi(tok[13]) ? array : nullptr;
		c.spans = atoi(tok[14]) ? array : nullptr;
		c.on_host = atoi(tok[15]);

		const SpanPlan p = plan_spans(c, strtof(tok[16], nullptr));
		printf("%d;%s", p.status, p.error ? p.error : "");
		if (p.status == QUERY_PLAN_OK)
		{
			printf(";%d", p.nothing_to_do ? 1 : 0);
			if (!p.nothing_to_do)
			{
				const SpanArgs &a = p.a;
				printf(";%d %d %d %d %d %d %d %08x %08x %08x %08x %d %d", a.kind, a.n, a.pos ? 1 : 0, a.dir ? 1 : 0, a.pixels ? 1 : 0, a.summaries ? 1 : 0, a.spans ? 1 : 0,
					bits(a.reach), bits(a.t_max), bits(a.min_step), bits(a.iso), a.max_steps, a.max_spans);
				printf(";%zu %zu %zu %zu;%d %d;%u", p.bytes[0], p.bytes[1], p.bytes[2], p.bytes[3], p.width, p.height, p.blocks);
			}
		}
		printf("\n");
	}
	return 0;
}

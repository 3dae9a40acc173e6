// measure_plan_host.cpp -- the plan of sdfr_measure (sdf_playground_amd/csrc/sdfr_measure_plan.h) as a stand-alone host program (no HIP
// header on the include path), for tests/test_measure_cpu.py.  Every line of standard input is a request:
//   grid (0: null, 1: given)  origin[3] du[3] dv[3] dw[3]  nu nv  params (0: null, 1: given)  t_max min_step iso max_steps max_spans
//   out columns (0: null, 1: given)  on_host  range
// The answer is one line: "status;error text", and for a plan that stands
//   ";nu nv, t_max min_step iso (as their bits), max_steps, whether columns is there;blocks;passes, the records each pass reads;
//   result_in;the three workspace sizes;the bytes of columns".
#include "sdfr_measure_plan.h"

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
		char *tok[25];
		int n = 0;
		for (char *t = strtok(line, " \n"); t && n < 25; t = strtok(nullptr, " \n")) tok[n++] = t;
		if (n != 25) return 2;
		static double array[5];
		MeasureGrid g;
		for (int k = 0; k < 3; ++k)
		{
			g.origin[k] = strtof(tok[1 + k], nullptr);
			g.du[k] = strtof(tok[4 + k], nullptr);
			g.dv[k] = strtof(tok[7 + k], nullptr);
			g.dw[k] = strtof(tok[10 + k], nullptr);
		}
		g.nu = atoi(tok[13]);
		g.nv = atoi(tok[14]);
		SpanParams sp;
		sp.t_max = strtof(tok[16], nullptr);
		sp.min_step = strtof(tok[17], nullptr);
		sp.iso = strtof(tok[18], nullptr);
		sp.max_steps = atoi(tok[19]);
		sp.max_spans = atoi(tok[20]);
		MeasureRequest c = {};
		c.grid = atoi(tok[0]) ? &g : nullptr;
		c.params = atoi(tok[15]) ? &sp : nullptr;
		c.out = atoi(tok[21]) ? array : nullptr;
		c.columns = atoi(tok[22]) ? array : nullptr;
		c.on_host = atoi(tok[23]);

		const MeasurePlan p = plan_measure(c, strtof(tok[24], nullptr));
		printf("%d;%s", p.status, p.error ? p.error : "");
		if (p.status == QUERY_PLAN_OK)
		{
			const MeasureArgs &a = p.a;
			bool same = !a.partials && !a.tally;
			for (int k = 0; k < 3; ++k)
				same = same && bits(a.origin[k]) == bits(g.origin[k]) && bits(a.du[k]) == bits(g.du[k]) && bits(a.dv[k]) == bits(g.dv[k]) && bits(a.dw[k]) == bits(g.dw[k]);
			if (!same) return 3;
			printf(";%d %d %08x %08x %08x %d %d;%u;%d", a.nu, a.nv, bits(a.t_max), bits(a.min_step), bits(a.iso), a.max_steps, a.columns ? 1 : 0, p.blocks, p.passes);
			for (int k = 0; k < p.passes; ++k) printf(" %u", p.pass_records[k]);
			printf(";%d;%zu %zu %zu;%zu", p.result_in, p.work[0], p.work[1], p.work[2], p.column_bytes);
		}
		printf("\n");
	}
	return 0;
}

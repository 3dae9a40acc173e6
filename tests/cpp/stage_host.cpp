// stage_host.cpp -- the carving arithmetic of sdf_playground_amd/csrc/sdfr_stage.h as a stand-alone host program (no HIP header on
// the include path), for tests/test_stage_cpu.py.  Every line of standard input is a list of byte counts; the answer is a line with
// the offset of every piece, then the total.
#include "sdfr_stage.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main()
{
	char line[1024];
	while (fgets(line, sizeof line, stdin))
	{
		size_t bytes[sdfr::SDFR_STAGE_MAX_PIECES], offsets[sdfr::SDFR_STAGE_MAX_PIECES];
		int n = 0;
		for (char *tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n"))
		{
			if (n == sdfr::SDFR_STAGE_MAX_PIECES) return 2; // more pieces than any caller names
			bytes[n++] = (size_t)strtoull(tok, nullptr, 10);
		}
		const size_t total = sdfr::stage_offsets(bytes, n, offsets);
		for (int k = 0; k < n; ++k) printf("%zu ", offsets[k]);
		printf("%zu\n", total);
	}
	return 0;
}

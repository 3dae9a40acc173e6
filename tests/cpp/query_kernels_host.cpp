// query_kernels_host.cpp -- the list of query kernel kinds (sdf_playground_amd/csrc/sdfr_query_args.h) and the translation units of a run-time
// scene (sdfr_jit_unit.h) as a stand-alone host program (no HIP header on the include path), for tests/test_query_kernels_cpu.py.
// Standard input is a scene's text.  The answer:
//   "kinds <QUERY_KERNEL_KINDS>", "frame <sizeof(FrameU)>", and per kind of the list
//   "kind <QUERY_KERNEL_*> <name> <stem> <body> <arguments> <sizeof and alignof the kernel's argument>", the texts as sdfr_jit_unit.h has them;
//   then "query <line>" and "pixel <line>" for every kernel line of the scene's query unit and of its pixel unit -- or, with the
//   argument "units", both units whole.
#include "sdfr_frame.h"
#include "sdfr_jit_unit.h"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <iterator>
#include <regex>

using namespace sdfr;

// the names of the scene's VAR_ tags in the order they first appear: the slots the library gives them
static std::vector<std::string> var_slots(const std::string &text)
{
	std::vector<std::string> slots;
	const std::regex tag("VAR_(\\w+)\\s*\\(");
	for (std::sregex_iterator m(text.begin(), text.end(), tag), end; m != end; ++m)
	{
		bool known = false;
		for (const std::string &s : slots) known = known || s == (*m)[1].str();
		if (!known) slots.push_back((*m)[1].str());
	}
	return slots;
}

static void print_kernel_lines(const char *what, const std::string &unit)
{
	const std::string mark = "#line 1 \"sdfr_jit_kernels\"\n";
	size_t at = unit.find(mark);
	if (at == std::string::npos) return;
	for (at += mark.size(); at < unit.size();)
	{
		const size_t end = unit.find('\n', at);
		const std::string line = unit.substr(at, end - at);
		if (line.find("__global__") != std::string::npos) printf("%s %s\n", what, line.c_str());
		if (end == std::string::npos) break;
		at = end + 1;
	}
}

int main(int argc, char **argv)
{
	const std::string scene((std::istreambuf_iterator<char>(std::cin)), std::istreambuf_iterator<char>());
	const std::vector<std::string> slots = var_slots(scene);
	if (argc > 1 && !strcmp(argv[1], "units"))
	{
		printf("%s---- pixel ----\n%s", jit_translation_unit(scene, slots, true).c_str(), jit_translation_unit(scene, slots, false).c_str());
		return 0;
	}
	printf("kinds %d\nframe %zu\n", (int)QUERY_KERNEL_KINDS, sizeof(FrameU));
#define PRINT_KIND(KIND, STEM, BODY, ARGS) \
	{ \
		const QueryKernelRow &row = k_query_kernel_rows[QUERY_KERNEL_##KIND]; \
		printf("kind %d %s %s %s %s %zu %zu\n", (int)QUERY_KERNEL_##KIND, row.kind, row.stem, row.body, row.args, sizeof(SceneKernelArgs<ARGS>), alignof(SceneKernelArgs<ARGS>)); \
	}
	SDFR_FOR_EACH_QUERY_KERNEL(PRINT_KIND)
#undef PRINT_KIND
	print_kernel_lines("query", jit_translation_unit(scene, slots, true));
	print_kernel_lines("pixel", jit_translation_unit(scene, slots, false));
	return 0;
}

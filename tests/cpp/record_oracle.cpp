// tests/cpp/record_oracle.cpp -- TEST-ONLY: the one library of the record oracles: the qo_ (query_oracle.h), so_ (surface_oracle.h),
// lo_ (lighting_oracle.h) and oo_ (occlusion_oracle.h) entry points, and the table of scenes they look up, generated from
// oracle/scene_list.h.  Built by tests/query_util.py (build_oracle_lib); the product never loads it.
#include "query_oracle.h"
#include "surface_oracle.h"
#include "lighting_oracle.h"
#include "occlusion_oracle.h"

namespace {

#define X(name, S) {name, &point_query<S>, &ray_query<S>, &pick_query<S>, &surface_query<S>, &surface_pick<S>, &lighting_query<S>, &lighting_pick<S>},
const Entry k_scenes[] = {ORC_REFERENCE_SCENES(X) ORC_TEST_SCENES(X)};
#undef X

const Entry *find(const char *name)
{
	for (const Entry &e : k_scenes)
		if (strcmp(e.name, name) == 0) return &e;
	return nullptr;
}

} // namespace

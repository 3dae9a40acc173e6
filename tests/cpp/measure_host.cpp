// tests/cpp/measure_host.cpp -- TEST-ONLY: the stage functions of sdfr_measure (sdf_playground_amd/csrc/sdfr_measure.h) and the
// properties (sdfr_measure_plan.h) compiled for the CPU and run column by column over two analytic fields, the way k_query_measure runs
// them one lane per column over a scene, then reduced by the header's host restatement of the two reductions, so that the CPU test tier
// can compare every bit with the definition restated in numpy (tests/measure_util.py) without a GPU.  Built with -ffp-contract=off, as
// the library.  The product never loads this.
#include "sdfr_measure_plan.h"

#include <cmath>
#include <limits>
#include <vector>

using namespace sdfr;

namespace {

// the fields of tests/cpp/span_host.cpp, line for line
struct SlabLadder
{
	int n;
	const float *c, *r;
	float nan_lo, nan_hi;
	float operator()(vec3 p) const
	{
		float D = std::numeric_limits<float>::infinity();
		for (int k = 0; k < n; ++k)
		{
			const float v = fabsf(p.x - c[k]) - r[k];
			D = v < D ? v : D;
		}
		return p.x >= nan_lo && p.x <= nan_hi ? std::numeric_limits<float>::quiet_NaN() : D;
	}
};
struct Sphere
{
	float c[3], radius;
	float operator()(vec3 p) const
	{
		const float x = p.x - c[0], y = p.y - c[1], z = p.z - c[2];
		return sqrtf(x * x + y * y + z * z) - radius;
	}
};

// every column of the grid, then the reduction; extras: [nu * nv][3] words -- crossings and the bits of t_lo and t_hi
template <class Field>
int measure_all(const MeasureGrid &g, const SpanParams &p, const Field &field, MeasureColumn *columns, uint32_t *extras, MeasureResult *out)
{
	std::vector<MeasureLane> lanes((size_t)g.nu * g.nv);
	for (int j = 0; j < g.nv; ++j)
		for (int i = 0; i < g.nu; ++i)
		{
			const vec3 o = V3(measure_origin(g.origin, g.du, g.dv, 0, i, j), measure_origin(g.origin, g.du, g.dv, 1, i, j), measure_origin(g.origin, g.du, g.dv, 2, i, j));
			const size_t at = (size_t)i + (size_t)g.nu * j;
			lanes[at] = measure_column(field, o, V3(g.dw[0], g.dw[1], g.dw[2]), p.t_max, p.min_step, p.iso, p.max_steps);
			columns[at] = lanes[at].c;
			extras[3 * at] = lanes[at].crossings;
			extras[3 * at + 1] = f32_bits(lanes[at].t_lo);
			extras[3 * at + 2] = f32_bits(lanes[at].t_hi);
		}
	std::vector<double> tiles((size_t)measure_tiles(g.nu) * measure_tiles(g.nv) * MEASURE_MOMENTS);
	measure_reduce_host(lanes.data(), g.nu, g.nv, tiles.data(), *out);
	return 0;
}

} // namespace

extern "C" {

int msh_measure_slabs(const MeasureGrid *g, const SpanParams *p, int slabs, const float *c, const float *r, float nan_lo, float nan_hi, MeasureColumn *columns,
	uint32_t *extras, MeasureResult *out)
{
	const SlabLadder field = {slabs, c, r, nan_lo, nan_hi};
	return measure_all(*g, *p, field, columns, extras, out);
}
int msh_measure_sphere(const MeasureGrid *g, const SpanParams *p, const float *centre, float radius, MeasureColumn *columns, uint32_t *extras, MeasureResult *out)
{
	const Sphere field = {{centre[0], centre[1], centre[2]}, radius};
	return measure_all(*g, *p, field, columns, extras, out);
}
// `n` records of ten doubles, reduced in place into the first; -> the passes
int msh_reduce_records(double *records, int64_t n) { return measure_reduce_records(records, (size_t)n); }
void msh_properties(const MeasureGrid *g, const MeasureResult *res, double density, SolidProperties *out) { measure_properties(*g, *res, density, *out); }
uint32_t msh_order_key(float f) { return measure_order_key(f); }
float msh_order_value(uint32_t k) { return measure_order_value(k); }
int msh_sizes(int what)
{
	const int sizes[] = {(int)sizeof(MeasureGrid), (int)sizeof(MeasureColumn), (int)sizeof(MeasureResult), (int)sizeof(SolidProperties), (int)sizeof(MeasureArgs),
		(int)MEASURE_TALLY_BYTES, (int)offsetof(MeasureResult, columns_hit), (int)offsetof(MeasureResult, hit_lo), (int)offsetof(MeasureResult, t_lo)};
	return what >= 0 && what < (int)(sizeof sizes / sizeof sizes[0]) ? sizes[what] : -1;
}

} // extern "C"

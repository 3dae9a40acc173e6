// sdfr_span.h -- the intervals of a ray that lie inside the solid: the stage function of the span queries (sdfr_query_ray_spans,
// sdfr_pick_spans, sdfr_mesh_spans in include/sdfr.h, where the definition stands in full), templated on a distance functor,
// scene-independent and host-compilable like sdfr_slice.h.  k_query_spans (sdfr_query_kernel.h) runs it one lane per ray over the loaded
// scene's point query; tests/cpp/span_host.cpp runs the same text over analytic fields on the CPU.  All arithmetic is fp32 in source order
// (-ffp-contract=off), so both give the same bits.
//
// The march samples s(t) = D(origin + t * dir) - iso from t = 0 and steps by max(|s|, min_step) up to t_max: where |D - iso| never
// overestimates the distance to the level set, outside and inside, a sign change can only fall into a step of min_step.  Each sign
// change is located by linear interpolation between the two samples around it.
#pragma once
#include "sdfr_math.h"

namespace sdfr {

struct SpanParams // sdfr_span_params
{
	float t_max, min_step, iso;
	int32_t max_steps, max_spans;
};
enum { SPAN_STARTS_INSIDE = 1, SPAN_ENDS_INSIDE = 2, SPAN_OUT_OF_STEPS = 4 }; // SDFR_SPAN_*
enum { SPAN_SUMMARY_WORDS = 8, SPAN_MAX_SPANS = 64, SPAN_MAX_STEPS = 1 << 20 };

// An item has an answer if its origin and direction are finite and the direction is not (0, 0, 0)
SDF_HD bool span_finite(float v) { return (f32_bits(v) & 0x7f800000u) != 0x7f800000u; }
SDF_HD bool span_item_ok(vec3 o, vec3 d)
{
	const bool finite = span_finite(o.x) && span_finite(o.y) && span_finite(o.z) && span_finite(d.x) && span_finite(d.y) && span_finite(d.z);
	return finite && !(d.x == 0.f && d.y == 0.f && d.z == 0.f);
}

// The answer of one item: rec, the 8 words of sdfr_span_summary, and through store(k, t_in, t_out) every one of its max_spans span slots
// -- span k when it closes, and zeros for the slots no span fills.  is_ray false: the item is no ray at all (a pixel outside the frame),
// valid = -1; a ray that is not span_item_ok: valid = 0; neither evaluates the scene.  distance(p) is D at p.
// The loop has ONE evaluation site: the sample at t = 0 is its first trip.
template <class Distance, class Store>
SDF_HD void span_item(const Distance &distance, const Store &store, bool is_ray, vec3 o, vec3 d, float t_max, float min_step, float iso, int32_t max_steps,
	int32_t max_spans, uint32_t rec[SPAN_SUMMARY_WORDS])
{
	uint32_t crossings = 0u, spans = 0u, steps = 0u, flags = 0u;
	int32_t valid = is_ray ? 0 : -1;
	float length = 0.f, t = 0.f;
	if (is_ray && span_item_ok(o, d))
	{
		valid = 1;
		float t_prev = 0.f, s_prev = 0.f, t_in = 0.f;
		bool inside_prev = false, open = false;
		for (;;)
		{
			const vec3 p = V3(o.x + t * d.x, o.y + t * d.y, o.z + t * d.z); // one multiply, then one add
			const float s = distance(p) - iso;
			const bool inside = s < 0.f; // NaN is outside
			if (steps != 0u ? inside != inside_prev : inside)
			{
				// a crossing between the samples at t_prev and t; or, at t = 0, a ray that starts inside
				float tc = 0.f;
				if (steps != 0u)
				{
					float u = s_prev / (s_prev - s);
					if (!(u >= 0.f && u <= 1.f)) u = 0.5f;
					tc = t_prev + u * (t - t_prev);
					++crossings;
				}
				else
					flags |= (uint32_t)SPAN_STARTS_INSIDE;
				if (inside)
				{
					open = true;
					t_in = tc;
					++spans;
				}
				else
				{
					open = false;
					if (spans <= (uint32_t)max_spans) store((int)(spans - 1u), t_in, tc);
					length = length + (tc - t_in);
				}
			}
			++steps;
			if (!(t < t_max)) break; // that was the sample at t_max
			if (steps == (uint32_t)max_steps)
			{
				flags |= (uint32_t)SPAN_OUT_OF_STEPS;
				break;
			}
			const float a = abs1(s);
			const float h = a > min_step ? a : min_step; // NaN steps by min_step
			const float t_next = t + h;
			t_prev = t;
			s_prev = s;
			inside_prev = inside;
			t = t_next < t_max ? t_next : t_max;
		}
		if (open)
		{
			flags |= (uint32_t)SPAN_ENDS_INSIDE;
			if (spans <= (uint32_t)max_spans) store((int)(spans - 1u), t_in, t);
			length = length + (t - t_in);
		}
	}
	for (int32_t k = spans < (uint32_t)max_spans ? (int32_t)spans : max_spans; k < max_spans; ++k) store((int)k, 0.f, 0.f);
	rec[0] = crossings;
	rec[1] = spans;
	rec[2] = steps;
	rec[3] = (uint32_t)valid;
	rec[4] = f32_bits(length);
	rec[5] = f32_bits(t);
	rec[6] = flags;
	rec[7] = 0u;
}

} // namespace sdfr

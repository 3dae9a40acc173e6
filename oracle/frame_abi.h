// oracle/frame_abi.h -- TEST INFRASTRUCTURE (CPU oracle), not product code.
//
// The one C layout of a frame (pyoracle.OrcFrame mirrors it) and its way into the oracle: what orc_render (oracle_api.cpp) and
// the record oracles (tests/cpp/record_oracle.cpp) take from their callers.
#pragma once
#include "sdf_lib.h"

extern "C" {

struct orc_frame
{
	float eye[3], front[3], right[3], top[3];
	float stime;
	int width, height;
	int iter_count, bounce_count, ray_count, light_count;
	float range;
	int max_cost_default;
	float debug_nx, debug_ny, debug_nz, debug_scale, debug_x, debug_y, debug_z, show_objects;
	float scene_var[8];
	int extension_lights; // 0..7, extension (SURVEY.md 8d cfg 5)
	float extension_marble_reflection; // 0 = reference, extension (SURVEY.md 8d cfg 3 as worded)
	float dist_eps, grad_eps, reflect_eps, refract_eps, shadow_eps; // pshader_sdf.hlsl:31-35
};

} // extern "C"

namespace orc {

inline Frame to_frame(const orc_frame &f)
{
	Frame F;
	F.eye = float3(f.eye[0], f.eye[1], f.eye[2]);
	F.front_vec = float3(f.front[0], f.front[1], f.front[2]);
	F.right_vec = float3(f.right[0], f.right[1], f.right[2]);
	F.top_vec = float3(f.top[0], f.top[1], f.top[2]);
	F.stime = f.stime;
	F.width = f.width;
	F.height = f.height;
	F.iter_count = f.iter_count;
	F.bounce_count = f.bounce_count;
	F.ray_count = f.ray_count;
	F.light_count = f.light_count;
	F.range = f.range;
	F.max_cost_default = (uint)f.max_cost_default;
	F.debug_nx = f.debug_nx;
	F.debug_ny = f.debug_ny;
	F.debug_nz = f.debug_nz;
	F.debug_scale = f.debug_scale;
	F.debug_x = f.debug_x;
	F.debug_y = f.debug_y;
	F.debug_z = f.debug_z;
	F.show_objects = f.show_objects;
	for (int i = 0; i < MAX_SCENE_VARS; ++i)
		F.scene_var[i] = f.scene_var[i];
	F.extension_lights = f.extension_lights < 0 ? 0 : (f.extension_lights > 7 ? 7 : f.extension_lights);
	F.extension_marble_reflection = f.extension_marble_reflection;
	F.dist_eps = f.dist_eps;
	F.grad_eps = f.grad_eps;
	F.reflect_eps = f.reflect_eps;
	F.refract_eps = f.refract_eps;
	F.shadow_eps = f.shadow_eps;
	return F;
}

// The frame a call works on: to_frame, and the driver's epsilons (sdf_lib.h) set from it -- before the call starts its threads
inline Frame enter_frame(const orc_frame &f)
{
	const Frame F = to_frame(f);
	dist_eps = F.dist_eps;
	grad_eps = F.grad_eps;
	reflect_eps = F.reflect_eps;
	refract_eps = F.refract_eps;
	shadow_eps = F.shadow_eps;
	return F;
}

} // namespace orc

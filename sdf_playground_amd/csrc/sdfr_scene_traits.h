// sdfr_scene_traits.h -- what a scene MAY declare beside its mandatory members (name, variables, prepare, RayInv, ray_setup, dist, material,
// light, ambient, background: sdfr_scenes.h), and how the kernels find out (device code, host-compilable, hiprtc-compilable).
//
// Constants are `static constexpr` members, functions `static SDF_HD`; a scene without the member gets the default and pays nothing.
// Readers: P = the pixel pipeline (render_pixel / shade_hit / shade_miss: the pixel kernel, scenes compiled at run time, tests/hostsim),
// W = the wavefront kernels (k_march, k_shade), Q = the queries (sdfr_query.h, sdfr_lighting.h), L = the launch (k_pixel's attributes,
// SceneKernels -> sdfr_launch_plan.h).  "Never DBG": the debug-plane build (DBG = true) ignores the member and keeps the reference's path.
//
// member                                              | absent  | read by | what the scene promises by declaring it
// ----------------------------------------------------+---------+---------+-------------------------------------------------------------------
// bool geometry_reads_march_state                     | false   | P Q     | `dist` takes a sixth argument, `const GeoStep &`: the sample's running
//   (SceneReadsMarchState)                            |         |         | camera_distance and the pixel's ray offsets, the reference's whole GeometryInput
//                                                     |         |         | (pshader_sdf.hlsl:187-218, 297-302).  No scene of the reference reads them; scenes
//                                                     |         |         | in its dialect declare it (sdfr_hlsl.h).  k_march calls the five-argument form.
// void normal(const FrameU &U, const SurfacePoint &sp,| none    | P W Q   | map_normal (pshader_sdf.hlsl:318-330; sdf_structs.hlsl:39-52): called once per hit,
//   NormalOut &no)               (SceneNormal::call)  |         |         | `no` preloaded {grad_eps, 0, false}, sp.normal 0.  It may hand back the normal
//                                                     |         |         | (no.use_normal = true: the three forward differences are not taken) and / or change
//                                                     |         |         | no.sample_dist, which also offsets the shadow rays (:520).
// void lights(const FrameU &U, const SurfacePoint &sp,| none    | P W Q   | map_light in the reference's own shape (pshader_sdf.hlsl:505-516), ONE call per lit
//   Light L[SDFR_MAX_LIGHTS],                         |         |         | hit with `used` all false, the lights zeroed and `ambient` 0.075.  It replaces
//   bool used[SDFR_MAX_LIGHTS], float &ambient)       |         |         | light(U, i, L) and ambient(), which such a scene need not have (SceneLightSlot,
//                                (SceneLights::call)  |         |         | SceneAmbient).
// bool ray_escapes(const FrameU &U, const RayInv &R,  | false   | P Q     | True only if NOTHING of the scene lies on the ray from p onwards: the ray is a miss
//   vec3 p, vec3 dir)            (RayEscapes::test)   |         |         | already (an escaped shadow ray delivers its light, any other sees the background,
//                                                     |         |         | whose colour must not depend on the step count), and the march stops.  Only with
//                                                     |         |         | FrameU::step_shortcuts, outside rays, never DBG (the plane is an extra object).
// float escapes_from(const FrameU &U, vec3 start,     | 3e38    | P Q     | Once per ray: the distance along it from which on nothing of the scene lies between
//   vec3 dir, float range)       (EscapesFrom::get)   |         |         | the march and `range`, where the ray is out of range anyway -- 3e38 if there is none.
//                                                     |         |         | A sample beyond it is a miss; one comparison per step.  Conditions as ray_escapes.
// void ray_bounds(const FrameU &U, RayInv &R,         | no-op   | P       | Once per ray, right after ray_setup, with the start and the range marched to: the
//   vec3 start, vec3 dir, float range)                |         |         | scene may strengthen R with facts that hold for every sample with t <= range, and
//                                (RayBounds::apply)   |         |         | ray_escapes may then call the ray gone although the scene goes on beyond `range`.
//                                                     |         |         | Licence: escapes_from's -- a hit needs m.t <= dist_max (march_advance), and a miss
//                                                     |         |         | is the same result whatever ended it.  Only render_pixel calls it, only with step
//                                                     |         |         | shortcuts on: the wavefront march, the ray queries and the light loop's shadow
//                                                     |         |         | probe keep ray_setup alone.
// bool shadow_hits_need_normal                        | true    | P Q     | false: material() never reads sp.normal, so the three normal samples of a shadow
//   (ShadowHitsNeedNormal)                            |         |         | ray's hit, which only the material could see, are skipped.
// bool shadow_hits_need_material                      | true    | P       | false: material() is a pure function that never lowers the alpha below 1, so a
//   (ShadowHitsNeedMaterial)                          |         |         | shadow ray's hit adds 0, pushes nothing and leaves the tone-map flag alone: it is
//                                                     |         |         | counted without shade_hit.  Never DBG.
// bool peel_unrelaxed_samples                         | false   | P       | Nothing about the scene: a ray's first three samples, which never rewind, become
//   (PeelUnrelaxedSamples)                            |         |         | straight-line code in front of the march loop (march_advance_unrelaxed) -- the same
//                                                     |         |         | samples, states and counters.  Another register draw for the whole kernel: opt in
//                                                     |         |         | with a measurement.  Never DBG.
// vec3 frame_sun_dir(const FrameU &U)                 | none    | P W     | light() puts a directional light into slot 0 in EVERY frame, and this is its
//                                (FrameSunDir::get)   |         |         | L.pos / (length(L.pos) + U.dist_eps), made once by prepare(): the light loop does
//                                                     |         |         | not form the quotients per hit.  (Extension lights take slots 1 and above.)
// bool inline_escaped_shadows                         | false   | P       | Counts only with ray_escapes.  A shadow ray that escapes where it starts is not
//   (InlineEscapedShadows)                            |         |         | queued but delivers its light from the light loop, when that keeps the order of the
//                                                     |         |         | pixel's sums: the queue is empty, the hit's own colour has been added, the ray
//                                                     |         |         | budget reaches it; from the first ray that is queued on, all are.  Never DBG.
// template <class NG> vec3 background(const FrameU &U,| plain   | P W     | The background's noise takes its gradients from NG (sdfr_noise.h): the same values
//   vec3 dir, uint32_t iter) (SceneBackground::get)   | form    |         | from the formula or the LDS table.
// bool noise_grad_table       (PixelNoiseGrads)       | false   | L       | The shading's turbulence3 runs in most waves: k_pixel fills 768 B of LDS with the
//                                                     |         |         | simplex gradients and reads them there.  Elsewhere it only costs.  Never DBG.
// int waves_per_simd          (PixelWavesPerSimd)     | 7       | L       | amdgpu_waves_per_eu of k_pixel: very long evaluations prefer fewer waves with more
//                                                     |         |         | registers (tree: 5), a march loop that fits 64 registers can ask for 8.
// bool persistent_tiles       (PersistentTiles)       | false   | L       | The default launch mode is the persistent one (resident waves pull tiles): wins
//                                                     |         |         | where tiles are dear and uneven, loses where they are cheap
//                                                     |         |         | (profiles/r02_launch_modes.txt).
// bool square_units           (SquareUnits)           | false   | L P     | Persistent full-frame launches hand the tiles out in squares, dearest first by the
//                                                     |         |         | last frame's cost: for an object in the middle of the picture.  The kernel carries
//                                                     |         |         | the code (another register draw).
// int tile_w_log2             (SceneTileShape)        | 3       | L       | A wave's pixels are a (1 << n) x (64 >> n) tile, n = 3 .. 6 (8 x 8 by default;
//                                                     |         |         | profiles/r03_launch_experiments.txt).
// int retire_after            (RetireAfter)           | 8       | L       | Tiles a wave of the persistent launch renders before it makes room for a younger
//                                                     |         |         | one (pixel_launch_blocks); 0 = never.
//
// Every trait answers `Trait<Scene>::value`: the constant, or whether the function is there.  A function trait also forwards the
// call (the name in brackets above) and does what the "absent" column says for a scene without the member, for the call sites
// that are not under `if constexpr`.
#pragma once
#include "sdfr_frame.h"
#include "sdfr_lib.h"

namespace sdfr {

// what `dist` gets as its sixth argument in a scene with geometry_reads_march_state
struct GeoStep
{
	float camera_distance;       // geometry.camera_distance at this sample (the hit's, for the normal's samples)
	vec3 right_off, bottom_off;  // geometry.right_ray_offset / bottom_ray_offset: the pixel's, for every ray of the pixel
};

template <class...>
struct VoidT { typedef void type; };

#define SDFR_SCENE_CONSTANT(Trait, type_, member, absent) \
	template <class Scene, class = void> struct Trait { static constexpr type_ value = absent; }; \
	template <class Scene> struct Trait<Scene, typename VoidT<decltype(Scene::member)>::type> { static constexpr type_ value = Scene::member; };
// params / args: the forwarding function's parameter list and the member's argument list, each in its brackets; R is the scene's RayInv
// (`available` is what a function trait's `value` was called before this header: kept for sources written against that name, which
// the library's own code no longer uses)
#define SDFR_SCENE_FUNCTION(Trait, member, ret, absent, forward, params, args) \
	template <class Scene, class = void> struct Trait \
	{ \
		static constexpr bool value = false, available = false; \
		template <class R = void> static SDF_HD ret forward params { return absent; } \
	}; \
	template <class Scene> struct Trait<Scene, typename VoidT<decltype(&Scene::member)>::type> \
	{ \
		static constexpr bool value = true, available = true; \
		template <class R = void> static SDF_HD ret forward params { return Scene::member args; } \
	};

SDFR_SCENE_CONSTANT(SceneReadsMarchState, bool, geometry_reads_march_state, false)
SDFR_SCENE_CONSTANT(ShadowHitsNeedNormal, bool, shadow_hits_need_normal, true)
SDFR_SCENE_CONSTANT(ShadowHitsNeedMaterial, bool, shadow_hits_need_material, true)
SDFR_SCENE_CONSTANT(PeelUnrelaxedSamples, bool, peel_unrelaxed_samples, false)
SDFR_SCENE_CONSTANT(DeclaresInlineEscapedShadows, bool, inline_escaped_shadows, false)
SDFR_SCENE_CONSTANT(PixelNoiseGrads, bool, noise_grad_table, false)
SDFR_SCENE_CONSTANT(PersistentTiles, bool, persistent_tiles, false)
SDFR_SCENE_CONSTANT(SquareUnits, bool, square_units, false)
SDFR_SCENE_CONSTANT(SceneTileShape, int, tile_w_log2, 3)
SDFR_SCENE_CONSTANT(RetireAfter, int, retire_after, 8)
#ifndef SDFR_PIXEL_WAVES_PER_EU
#define SDFR_PIXEL_WAVES_PER_EU 7 // why 7: sdfr_pixel_kernel.h
#endif
#ifdef SDFR_PIXEL_WAVES_FIXED // developer builds that sweep SDFR_PIXEL_WAVES_PER_EU override the scenes' own choice
template <class Scene> struct PixelWavesPerSimd { static constexpr int value = SDFR_PIXEL_WAVES_PER_EU; };
#else
SDFR_SCENE_CONSTANT(PixelWavesPerSimd, int, waves_per_simd, SDFR_PIXEL_WAVES_PER_EU)
#endif

SDFR_SCENE_FUNCTION(SceneNormal, normal, void, void(), call, (const FrameU &U, const SurfacePoint &sp, NormalOut &no), (U, sp, no))
SDFR_SCENE_FUNCTION(SceneLights, lights, void, void(), call, (const FrameU &U, const SurfacePoint &sp, Light *L, bool *used, float &ambient), (U, sp, L, used, ambient))
SDFR_SCENE_FUNCTION(RayEscapes, ray_escapes, bool, false, test, (const FrameU &U, const R &r, vec3 p, vec3 dir), (U, r, p, dir))
SDFR_SCENE_FUNCTION(EscapesFrom, escapes_from, float, 3e38f, get, (const FrameU &U, vec3 start, vec3 dir, float range), (U, start, dir, range))
SDFR_SCENE_FUNCTION(RayBounds, ray_bounds, void, void(), apply, (const FrameU &U, R &r, vec3 start, vec3 dir, float range), (U, r, start, dir, range))
SDFR_SCENE_FUNCTION(FrameSunDir, frame_sun_dir, vec3, V3s(0.f), get, (const FrameU &U), (U))

// background<NG> where the scene's takes a gradient source (the shared sky), else as it is
template <class Scene, class NG, class = void>
struct SceneBackground
{
	static constexpr bool value = false;
	static SDF_HD vec3 get(const FrameU &U, vec3 dir, uint32_t iter) { return Scene::background(U, dir, iter); }
};
template <class Scene, class NG>
struct SceneBackground<Scene, NG, typename VoidT<decltype(Scene::template background<NG>(*(const FrameU *)0, V3s(0.f), 0u))>::type>
{
	static constexpr bool value = true;
	static SDF_HD vec3 get(const FrameU &U, vec3 dir, uint32_t iter) { return Scene::template background<NG>(U, dir, iter); }
};

// inline_escaped_shadows counts only with ray_escapes
template <class Scene>
struct InlineEscapedShadows { static constexpr bool value = DeclaresInlineEscapedShadows<Scene>::value && RayEscapes<Scene>::value; };

// a scene with lights() need not have ambient() and light(): the default ambient, every slot from the table lights() filled
template <class Scene, bool HasLights = SceneLights<Scene>::value>
struct SceneAmbient { static SDF_HD float get() { return Scene::ambient(); } };
template <class Scene>
struct SceneAmbient<Scene, true> { static SDF_HD float get() { return 0.075f; } };
template <class Scene, bool HasLights = SceneLights<Scene>::value>
struct SceneLightSlot { static SDF_HD bool get(const FrameU &U, int i, Light &L) { return Scene::light(U, i, L); } };
template <class Scene>
struct SceneLightSlot<Scene, true> { static SDF_HD bool get(const FrameU &, int, Light &) { return false; } };

#undef SDFR_SCENE_CONSTANT
#undef SDFR_SCENE_FUNCTION

} // namespace sdfr

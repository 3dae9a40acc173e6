// tests/cpp/scene_traits.cpp -- TEST-ONLY host translation unit: the scene contract of sdf_playground_amd/csrc/sdfr_scene_traits.h, as static_asserts.
// A scene with the mandatory members alone gets every default of the header's table; a scene that declares everything gets what it declared;
// inline_escaped_shadows counts only with ray_escapes; and each built-in scene that opts into something is seen to (read from the scene headers).
// Built and run by tests/test_scene_traits_cpu.py: that it compiles is the test.
#include "sdfr_scene_traits.h"
#include "sdfr_scenes.h"
#include "sdfr_scenes2.h"
#include "sdfr_scenes3.h"
#include "sdfr_scenes4.h"
#include "sdfr_scene_debug.h"

using namespace sdfr;

namespace {

struct Bare
{
	struct RayInv {};
	static RayInv ray_setup(const FrameU &, vec3, const RayFlags &) { return RayInv(); }
	static float dist(const FrameU &, const RayInv &, vec3, vec3, bool) { return 1.f; }
	static void material(const FrameU &, const SurfacePoint &, Material &) {}
	static bool light(const FrameU &, int, Light &) { return false; }
	static float ambient() { return 0.5f; }
	static vec3 background(const FrameU &, vec3, uint32_t) { return V3s(0.f); }
};

struct Full : Bare
{
	static constexpr bool geometry_reads_march_state = true;
	static float dist(const FrameU &, const RayInv &, vec3, vec3, bool, const GeoStep &) { return 1.f; }
	static void normal(const FrameU &, const SurfacePoint &, NormalOut &) {}
	static void lights(const FrameU &, const SurfacePoint &, Light *, bool *, float &) {}
	static bool ray_escapes(const FrameU &, const RayInv &, vec3, vec3) { return true; }
	static float escapes_from(const FrameU &, vec3, vec3, float) { return 2.f; }
	static void ray_bounds(const FrameU &, RayInv &, vec3, vec3, float) {}
	static constexpr bool shadow_hits_need_normal = false;
	static constexpr bool shadow_hits_need_material = false;
	static constexpr bool peel_unrelaxed_samples = true;
	static vec3 frame_sun_dir(const FrameU &) { return V3s(1.f); }
	static constexpr bool inline_escaped_shadows = true;
	template <class NG>
	static vec3 background(const FrameU &, vec3, uint32_t) { return V3s(0.f); }
	static constexpr bool noise_grad_table = true;
	static constexpr int waves_per_simd = 5;
	static constexpr bool persistent_tiles = true;
	static constexpr bool square_units = true;
	static constexpr int tile_w_log2 = 5;
	static constexpr int retire_after = 2;
};

// the declaration without the rule it rests on
struct InlineWithoutEscapes : Bare
{
	static constexpr bool inline_escaped_shadows = true;
};

// ---- the defaults of the table ----------------------------------------------------------------------------------------------------
static_assert(!SceneReadsMarchState<Bare>::value && !SceneNormal<Bare>::value && !SceneLights<Bare>::value, "absent: false");
static_assert(!RayEscapes<Bare>::value && !EscapesFrom<Bare>::value && !RayBounds<Bare>::value && !FrameSunDir<Bare>::value, "absent: false");
static_assert(ShadowHitsNeedNormal<Bare>::value && ShadowHitsNeedMaterial<Bare>::value, "the reference's behaviour unless the scene vouches");
static_assert(!PeelUnrelaxedSamples<Bare>::value && !InlineEscapedShadows<Bare>::value && !SceneBackground<Bare, NoiseGradFormula>::value, "absent: false");
static_assert(!PixelNoiseGrads<Bare>::value && !PersistentTiles<Bare>::value && !SquareUnits<Bare>::value, "absent: false");
static_assert(PixelWavesPerSimd<Bare>::value == 7 && SceneTileShape<Bare>::value == 3 && RetireAfter<Bare>::value == 8, "the launch defaults");

// ---- everything declared ---------------------------------------------------------------------------------------------------------------
static_assert(SceneReadsMarchState<Full>::value && SceneNormal<Full>::value && SceneLights<Full>::value, "declared");
static_assert(RayEscapes<Full>::value && EscapesFrom<Full>::value && RayBounds<Full>::value && FrameSunDir<Full>::value, "declared");
static_assert(!ShadowHitsNeedNormal<Full>::value && !ShadowHitsNeedMaterial<Full>::value, "declared false");
static_assert(PeelUnrelaxedSamples<Full>::value && InlineEscapedShadows<Full>::value && SceneBackground<Full, NoiseGradFormula>::value, "declared");
static_assert(PixelNoiseGrads<Full>::value && PersistentTiles<Full>::value && SquareUnits<Full>::value, "declared");
static_assert(PixelWavesPerSimd<Full>::value == 5 && SceneTileShape<Full>::value == 5 && RetireAfter<Full>::value == 2, "declared");

// ---- the earlier spelling of a function trait's value, kept for sources written against it --------------------------------------------------
static_assert(RayEscapes<Full>::available && EscapesFrom<Full>::available && RayBounds<Full>::available && SceneNormal<Full>::available, "as value");
static_assert(!RayEscapes<Bare>::available && !EscapesFrom<Bare>::available && !RayBounds<Bare>::available && !SceneNormal<Bare>::available, "as value");

// ---- the composite rule ----------------------------------------------------------------------------------------------------------------
static_assert(!InlineEscapedShadows<InlineWithoutEscapes>::value, "inline_escaped_shadows counts only with ray_escapes");

// ---- what the built-in scenes opt into today -------------------------------------------------------------------------------------------
static_assert(RayBounds<SceneLabyrinth>::value && PeelUnrelaxedSamples<SceneLabyrinth>::value && FrameSunDir<SceneLabyrinth>::value, "labyrinth");
static_assert(!ShadowHitsNeedMaterial<SceneLabyrinth>::value && !ShadowHitsNeedNormal<SceneLabyrinth>::value && PixelNoiseGrads<SceneLabyrinth>::value, "labyrinth");
static_assert(RayEscapes<SceneLabyrinth>::value && !InlineEscapedShadows<SceneLabyrinth>::value && PersistentTiles<SceneLabyrinth>::value, "labyrinth");
static_assert(PixelWavesPerSimd<SceneLabyrinth>::value == 7 && RetireAfter<SceneLabyrinth>::value == 4 && SceneTileShape<SceneLabyrinth>::value == 3, "labyrinth");
static_assert(InlineEscapedShadows<SceneGems>::value && SquareUnits<SceneGems>::value && PersistentTiles<SceneGems>::value, "gems");
static_assert(SceneTileShape<SceneGems>::value == 4 && RetireAfter<SceneGems>::value == 1 && PixelWavesPerSimd<SceneGems>::value == 7, "gems");
static_assert(SquareUnits<SceneFractal>::value && RetireAfter<SceneFractal>::value == 1 && InlineEscapedShadows<SceneFractal>::value, "fractal");
static_assert(EscapesFrom<SceneLense>::value && SceneTileShape<SceneLense>::value == 4 && PixelWavesPerSimd<SceneLense>::value == 8, "lense");
static_assert(PersistentTiles<SceneCubeSea>::value && RetireAfter<SceneCubeSea>::value == 4 && RayEscapes<SceneCubeSea>::value, "cube_sea");
static_assert(PersistentTiles<SceneLightShadows>::value && RayEscapes<SceneLightShadows>::value && !InlineEscapedShadows<SceneLightShadows>::value, "light_shadows");
static_assert(InlineEscapedShadows<SceneFastSphere>::value && !PersistentTiles<SceneFastSphere>::value && !ShadowHitsNeedNormal<SceneFastSphere>::value, "fast_sphere");
static_assert(PixelWavesPerSimd<SceneDistortion>::value == 8 && SceneTileShape<SceneNeon>::value == 4, "distortion, neon");
static_assert(PixelWavesPerSimd<SceneTree>::value == 5 && PersistentTiles<SceneTree>::value && RetireAfter<SceneTree>::value == 4, "tree");
static_assert(ShadowHitsNeedNormal<SceneCoordinateMaterial>::value, "coordinate_material's materials read the normal of a shadow hit");
static_assert(SceneNormal<SceneNormalTest>::value && !SceneNormal<SceneLabyrinth>::value, "normal_test is the one scene with a map_normal");
static_assert(SceneBackground<SceneFastSphere, NoiseGradFormula>::value && SceneBackground<SceneLabyrinth, NoiseGradFormula>::value, "the shared sky takes a gradient source");
static_assert(!SceneReadsMarchState<SceneLabyrinth>::value && !SceneLights<SceneLabyrinth>::value, "no scene compiled ahead of time reads the march state or fills a light table");

} // namespace

int main() { return 0; }

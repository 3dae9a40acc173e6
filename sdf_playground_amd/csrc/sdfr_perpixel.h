// sdfr_perpixel.h -- the per-pixel pipeline (sdfr_render_pixel.h) together with every scene
// compiled ahead of time, and the registry that numbers them.
#pragma once
#include "sdfr_render_pixel.h"
#include "sdfr_scenes.h"
#include "sdfr_scenes2.h"
#include "sdfr_scenes3.h"
#include "sdfr_scenes4.h"
#include "sdfr_scene_debug.h"

namespace sdfr {

// scene registry: X(index, SceneType)
#define SDFR_FOR_EACH_SCENE(X) \
	X(0, SceneFastSphere) X(1, SceneCubeSea) X(2, SceneLabyrinth) X(3, SceneFractal) X(4, SceneLense) X(5, SceneGems) X(6, SceneLightShadows) \
	X(7, SceneCube) X(8, SceneGyroid) X(9, SceneBasicTransparency) X(10, SceneBasicClouds) X(11, SceneCoordinateMaterial) \
	X(12, SceneDistortion) X(13, SceneTable) X(14, SceneSierpinski) X(15, SceneNeon) \
	X(16, SceneFractal2) X(17, SceneShell) X(18, SceneSpiral) X(19, SceneTerrain) X(20, SceneTiling) X(21, SceneTree) \
	X(22, SceneDebugMaterials) X(23, SceneNormalTest)
// the first SDFR_PUBLIC_SCENE_COUNT are the reference's scenes (what sdfr_scene_count / sdfr_scene_name list);
// the rest are the library's own diagnostic scenes, loaded by name only (sdfr_scene_debug.h)
#define SDFR_COUNT_SCENE(I, S) +1
enum { SDFR_PUBLIC_SCENE_COUNT = 22, SDFR_SCENE_COUNT = 0 SDFR_FOR_EACH_SCENE(SDFR_COUNT_SCENE) };
#undef SDFR_COUNT_SCENE

// the scene type of a registry index: each scene's kernels are a compile unit of their own, built with -DSDFR_SCENE=<index>
// (sdfr_kernels_scene.hip, sdfr_query_scene.hip; sdf_playground_amd/buildlib.py gives single scenes options of their own, SCENE_FLAGS)
template <int I>
struct SceneAt;
#define SDFR_SCENE_AT(I, S) template <> struct SceneAt<I> { using type = S; };
SDFR_FOR_EACH_SCENE(SDFR_SCENE_AT)
#undef SDFR_SCENE_AT

} // namespace sdfr

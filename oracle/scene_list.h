// oracle/scene_list.h -- TEST INFRASTRUCTURE (CPU oracle), not product code.
//
// The one list of the oracle's scenes, as (name, scene type): oracle_api.cpp's table and the record oracles' entry table
// (tests/cpp/record_oracle.cpp) are generated from it with X(name, Scene).
#pragma once
#include "scenes.h"
#include "scenes2.h"
#include "scenes3.h"
#include "scenes4.h"
#include "test_scenes.h"

// the reference's scenes, in the order orc_scene_name counts them
#define ORC_REFERENCE_SCENES(X) \
	X("fast_sphere", SceneFastSphere) \
	X("cube_sea", SceneCubeSea) \
	X("labyrinth", SceneLabyrinth) \
	X("fractal", SceneFractal) \
	X("lense", SceneLense) \
	X("gems", SceneGems) \
	X("light_shadows", SceneLightShadows) \
	X("cube", SceneCube) \
	X("gyroid", SceneGyroid) \
	X("basic_transparency", SceneBasicTransparency) \
	X("basic_clouds", SceneBasicClouds) \
	X("coordinate_material", SceneCoordinateMaterial) \
	X("distortion", SceneDistortion) \
	X("table", SceneTable) \
	X("sierpinski", SceneSierpinski) \
	X("neon", SceneNeon) \
	X("fractal2", SceneFractal2) \
	X("shell", SceneShell) \
	X("spiral", SceneSpiral) \
	X("terrain", SceneTerrain) \
	X("tiling", SceneTiling) \
	X("tree", SceneTree)

// scenes that exist for tests only (test_scenes.h; light_shadows_backwards: scenes.h, for Images/multi-lights.png only): found by
// name, not part of the reference's list
#define ORC_TEST_SCENES(X) \
	X("debug_materials", SceneDebugMaterials) \
	X("light_shadows_backwards", SceneLightShadowsT<true>) \
	X("normal_test", SceneNormalTest) \
	X("noise_lod", SceneNoiseLod) \
	X("dialect_tour", SceneDialectTour)

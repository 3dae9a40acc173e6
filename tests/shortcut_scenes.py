"""The built-in scenes that declare step-shortcut rules (sdf_playground_amd/csrc/sdfr_pixel.h), written down once for the tests that
cover each rule.  tests/test_scene_bounds_cpu.py checks these sets against what the functors declare (hostsim_scene_rules), so a rule
added to or removed from a scene fails the CPU tier until the tests know of it; the GPU tier reads the sets from here."""

# every built-in scene, in the library's order (sdfr_scene_name)
ALL_SCENES = ("fast_sphere", "cube_sea", "labyrinth", "fractal", "lense", "gems", "light_shadows", "cube", "gyroid", "basic_transparency",
              "basic_clouds", "coordinate_material", "distortion", "table", "sierpinski", "neon", "fractal2", "shell", "spiral", "terrain",
              "tiling", "tree")

# Scene::ray_escapes: a ray from p along dir meets nothing more of the scene
RAY_ESCAPES = frozenset([
    "fast_sphere", "cube_sea", "labyrinth", "fractal", "gems", "light_shadows", "cube", "gyroid", "basic_transparency", "basic_clouds",
    "coordinate_material", "distortion", "table", "sierpinski", "neon", "fractal2", "shell", "spiral", "terrain", "tiling", "tree",
])

# Scene::escapes_from: the distance along a ray from which on it meets nothing up to its range
ESCAPES_FROM = frozenset(["lense"])

# Scene::inline_escaped_shadows in effect (declared, with a ray_escapes for it to act on): a shadow ray that escapes where it starts is
# delivered from the light loop instead of being queued
INLINE_ESCAPED_SHADOWS = frozenset([
    "fast_sphere", "fractal", "gems", "cube", "basic_transparency", "basic_clouds", "coordinate_material", "distortion", "table",
    "sierpinski", "neon", "fractal2", "shell", "spiral",
])

# The shortcut-heavy hunt (tools/fuzz_parity.py) sized to what found the last lense bug -- a rule that took the direction of a shadow ray
# towards a directional light for a unit vector, seen in 32 of 6 000 lense cases, all with dist_eps = 1e-3 -- run by the GPU tier on the
# HIP kernels (tests/test_gpu_fuzz.py) and by the CPU tier on the host build of the same pipeline (tests/test_hunt_cpu.py), case for case
HUNT_SIZE = (64, 48)
HUNT_OPTIONS = dict(shortcut_heavy=True, eps_max_share=0.4, wide_cameras=True, full_range_vars=True)
LENSE_HUNT_SEEDS = (401, 402, 403)  # 500 cases each
LENSE_HUNT_CASES = 500
RULE_HUNT_SCENES = ("cube_sea", "labyrinth", "fractal", "gems")  # the bench's other scenes with a rule
RULE_HUNT_SEED = 404
RULE_HUNT_CASES = 300

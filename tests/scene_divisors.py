"""The constants the scene code divides by through div_c (sdf_playground_amd/csrc/sdfr_math.h): the list tests/test_gpu_math.py verifies
div_c for exhaustively on the GPU, and the constants of the `_c` probes (tests/probe_scenes.py).  No GPU needed to import this."""
import numpy as np

# every divisor handed to div_c / op_rep_inf_c / op_pipe_c / turbulence3 by the scene code
SCENE_DIVISORS = [
    20.0,                                              # labyrinth cell size
    3.0, 10.0,                                         # lense background cells
    15.0,                                              # turbulence3 normalisation
    float(np.float32(6.28318530717958647)),            # op_rep_angle: angle * count / tau
    float(np.float32(0.001)), float(np.float32(0.05)), float(np.float32(0.025)), float(np.float32(0.01)),   # smooth min / max widths (gems, table, tree)
    float(np.float32(np.float32(np.float32(1.41421356237309504) * np.float32(0.1)) / np.float32(4.0))),  # op_pipe period (labyrinth vase)
]
# tree: the branch generations' scales 1.4^-i, formed like the scene does (repeated fp32 division)
_scale = np.float32(1.0)
for _i in range(8):
    _scale = np.float32(_scale / np.float32(1.4))
    SCENE_DIVISORS.append(float(_scale))
SCENE_DIVISORS += [float(np.float32(2.2)), 11.0]                  # tree: lattice spacing, hop period (10 is in the list already)
SCENE_DIVISORS += [float(3 ** i) for i in range(2, 8)]   # fractal: level scales 9 .. 2187 (3 is in the list already)

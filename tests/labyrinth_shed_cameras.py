"""The labyrinth eyes of the tests of the work the pixel kernel shed (tests/test_labyrinth_shed_cpu.py on the host build,
tests/test_gpu_labyrinth_shed.py on the kernels).  What each eye is for is said beside it.  The folded cell (SceneLabyrinth::fold): wall 1
is the box x 2..5, z 2..4, wall 2 the box x 4..10, z 4..6, both y 0..4; the vases stand at (7 | 9, 0, 3), the torch's flame about
(5.3, 3.1..3.6, 3)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FOVY = np.float32(60.0) * np.float32(3.14159265358979) / np.float32(180.0)
VIEW = (0.6, -0.3, 0.7)  # the direction of every eye that has none of its own

# eyes near enough to a vase or the torch that the object passes its cull test and is the nearest thing
NEAR_OBJECTS = [
    ("near_vase_bowl", (7.55, 1.89, 3.0)),    # 0.05 off the bowl of the vase at x = 7
    ("near_vase_foot", (9.0, 0.2, 3.45)),     # 0.05 off the foot of the mirrored vase
    ("near_torch_flame", (5.5, 3.3, 3.0)),    # 0.07 off the flame cone
    ("near_torch_wood", (5.25, 2.58, 3.0)),   # beside the middle of the tilted stick
]
# eyes in the box of the combined cull test where the balls' own tests decide, and eyes in a corridor far from both objects
CORRIDOR = [
    ("corridor_far", (1.0, 1.5, 1.0)),        # the combined test skips both objects
    ("corridor_mid", (6.0, 3.0, 2.5)),        # inside the combined box, between vase and torch
    ("corridor_low", (8.0, 0.5, 1.2)),
    ("corridor_top", (7.0, 3.9, 3.0)),        # above the vase, below the wall tops
]
OTHERS = [
    ("inside_wall1", (3.5, 2.0, 3.0)),        # negative distance: every primary ray is a hit at its first sample
    ("inside_wall2", (-7.0, 1.0, 25.0)),      # ... through the mirror and a cell further
    ("below_floor", (3.0, -1.0, -5.0)),
    ("far_pp", (1e4 + 3.25, 5.0, 1e4 - 6.5)),  # cells far from the origin
    ("far_nn", (-1e4 - 8.75, 2.0, -1e4 + 2.5)),
    ("far_vase", (1e4 + 7.5, 1.875, 1e4 + 3.0)),  # 10000 = 500 cells: the vase's place in that cell
]
ZEROS = [("zero_%s_%s" % ("xyz"[axis], "plus" if sign > 0 else "minus"), tuple(np.copysign(0.0, sign) if i == axis else v for i, v in enumerate((3.0, 2.5, 5.5))))
         for axis in range(3) for sign in (1, -1)]


def sweep_eyes():
    import bench

    out = []
    for k in range(16):
        kind, eye, target, stime = bench.CONFIGS["3"]["camera"](k)
        out.append(("sweep%d" % k, kind, tuple(float(x) for x in eye), tuple(float(x) for x in target), float(stime)))
    return out


def cameras():
    """[(name, kind, eye, direction or look-at, stime)]: the sixteen sweep eyes of bench.py with their own views, then the eyes above"""
    cams = sweep_eyes()
    for k, (name, eye) in enumerate(NEAR_OBJECTS + CORRIDOR + OTHERS + ZEROS):
        cams.append((name, "dir", eye, VIEW if k % 2 == 0 else (-0.5, 0.2, -0.8), 0.1 * (k + 1)))
    return cams


def oracle_frame(oracle, cam, W, H, **limits):
    _name, kind, eye, target, stime = cam
    basis = (oracle.camera_lookat if kind == "lookat" else oracle.camera_direction)(eye, target, FOVY, np.float32(W) / np.float32(H))
    for i in range(3):
        assert np.float32(basis[0][i]).view(np.uint32) == np.float32(eye[i]).view(np.uint32)  # the eye reaches the frame as it is, the sign of a zero too
    f = oracle.default_frame("labyrinth", W, H, basis=basis, stime=stime)
    f.iter_count = 256
    for k, v in limits.items():
        setattr(f, k, v)
    return f, basis

"""The labyrinth cameras of the march-step tests (tests/test_labyrinth_step_cpu.py on the host build, tests/test_gpu_labyrinth_step.py on
the kernels), each rendered against the oracle at 64 x 40 with iter_count 256.  What each is for is said beside it; the CPU
tier asserts of the oracle's own frames that the cameras above the floor show hits and misses, so no case passes by seeing nothing."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H = 64, 40
FOVY = np.float32(60.0) * np.float32(3.14159265358979) / np.float32(180.0)
FAR = 524288.0  # 2^19: cell indices of 26214, coordinates with 1/16 between neighbours


def cameras():
    """[(name, kind, eye, direction or look-at, stime)]"""
    import bench

    cams = []
    for k in (0, 5, 11):
        kind, eye, target, stime = bench.CONFIGS["3"]["camera"](k)
        cams.append(("sweep%d" % k, kind, eye, target, stime))
    cams += [
        # the floor's height is a zero whose sign p.x and p.z decide when p.y = -0 (SceneLabyrinth::floor_dist): every primary ray of these
        # cameras starts at y = -0; looking down it keeps it (fma(dir.y < 0, +0, -0) = -0), looking up its first sample is at +0
        ("minus0_pp_down", "dir", (3.0, -0.0, 5.5), (0.6, -0.3, 0.7), 0.1),
        ("minus0_pp_up", "dir", (3.0, -0.0, 5.5), (0.6, 0.3, 0.7), 0.1),
        ("minus0_nn_down", "dir", (-3.0, -0.0, -5.5), (0.6, -0.3, 0.7), 0.2),
        ("minus0_nn_up", "dir", (-3.0, -0.0, -5.5), (0.6, 0.3, 0.7), 0.2),
        ("minus0_pn_level", "dir", (3.0, -0.0, -5.5), (-0.6, 0.0, 0.7), 0.3),
        ("minus0_np_level", "dir", (-3.0, -0.0, 5.5), (0.6, -0.0, -0.7), 0.3),
        # on the floor and below it: the fast plane is <= 0 from there (tests/test_shortcuts_cpu.py)
        ("on_floor", "lookat", (0.5, 0.0, -1.0), (5.0, 0.6, 4.0), 0.4),
        ("below_floor", "lookat", (3.0, -1.0, -5.0), (0.0, 1.0, 0.0), 0.5),
    ]
    # large cell indices and both signs of the fold: one camera per quadrant, off the cell grid by different amounts
    for name, sx, sz, dx, dz in (("far_pp", 1, 1, 0.8, 0.6), ("far_np", -1, 1, 0.5, -0.85), ("far_nn", -1, -1, -0.7, 0.7), ("far_pn", 1, -1, -0.3, -0.95)):
        cams.append((name, "dir", (sx * (FAR + 11.25), 5.0, sz * (FAR - 6.5)), (dx, -0.3, dz), 0.6))
    return cams


def oracle_frame(oracle, cam, **limits):
    _name, kind, eye, target, stime = cam
    basis = (oracle.camera_lookat if kind == "lookat" else oracle.camera_direction)(eye, target, FOVY, np.float32(W) / np.float32(H))
    if eye[1] == 0 and np.signbit(np.float32(eye[1])):
        assert np.signbit(basis[0][1])  # the eye's -0 reaches the frame
    f = oracle.default_frame("labyrinth", W, H, basis=basis, stime=stime)
    f.iter_count = 256
    for k, v in limits.items():
        setattr(f, k, v)
    return f, basis

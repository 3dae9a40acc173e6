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


FAR22 = 4194304.0  # 2^22: the marble's last octaves reach lattice coordinates of 2^24 .. 2^26
LATE = 369098752.0  # 11 * 2^25: the fire's scrolled coordinate, 3 * stime, is beyond 2^30 in every octave


def fallback_cameras():
    """[(name, kind, eye, direction or look-at, stime)]: frames in which some noise evaluations, and not all, leave the gradient table's
    straight-line path (sdfr_noise.h: a lane whose `ok` is cleared evaluates the noise again with the formula) -- which needs a
    lattice coordinate i whose noise_mod289 leaves [-1, 289].  For positive i that happens from 2^24 on, at a rate of 2e-3 and more.  For
    negative i it happens only for the 850 values -17957882 - 1156 k, down to -18939326, where it gives 290 (an exhaustive sweep of
    the even integers of [-2^25, -2^24]; none in the next three binades).  tests/test_labyrinth_fallback_cpu.py counts, on the host
    build with the table, what falls back in each of these frames; directions, offsets and LATE were chosen by those counts.
      * late*: bench sweep cameras that show a torch, at a time so late that the fire's scrolled coordinate falls back in every flame pixel;
      * far22_pp, _np, _pn: one camera per quadrant at +-2^22; where x or z is positive, walls and vases fall back in a few pixels;
      * far22_nn: the quadrant where both are negative.  With |x| = |z| = 2^22 the walls' lattice coordinates are about -7.0e6 times
        the octave (1, 2, 4, 8) and -2.8e6 times it for y, the vases' three times that: none of them meets the band above, and of 6000
        random cameras within 2000 units of (-2^22, -2^22) none had a pixel fall back.  The camera therefore stands at 1.3 * 2^22, where
        the walls' second octave (about -1.84e7) lies in the band; it was the second of the first 25 random cameras there with a count."""
    import bench

    cams = []
    for k in (3, 15):
        kind, eye, target, _stime = bench.CONFIGS["3"]["camera"](k)
        cams.append(("late%d" % k, kind, eye, target, LATE))
    cams += [
        ("far22_pp", "dir", (FAR22 + 11.25, 5.0, FAR22 - 6.5), (-0.7, -0.3, 0.7), 0.6),
        ("far22_np", "dir", (-(FAR22 - 8.5), 6.5, FAR22 + 14.0), (-0.3, -0.3, -0.95), 0.6),
        ("far22_pn", "dir", (FAR22 + 11.25, 5.0, -(FAR22 - 6.5)), (-0.9, -0.3, -0.4), 0.6),
        ("far22_nn", "dir", (-5596275.0, 6.5, -5419721.0), (0.39, -0.3, 0.92), 0.6),
    ]
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

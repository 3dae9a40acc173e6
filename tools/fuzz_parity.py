"""Randomised parity hunt (GPU box): random cameras, times, variable values and limits for every
built-in scene, HIP kernels against the CPU oracle, bit for bit (pixels and per-pixel counters).
The fixed-camera tests cannot find a culling bound or a fast-math domain that only fails from
some other viewpoint; this can.  Prints every mismatch; exit status 1 if there was one.
draw_cases() hands the same cases to any other renderer (tests/test_hunt_cpu.py: the host build).

    python tools/fuzz_parity.py --cases 40 --seed 1
    python tools/fuzz_parity.py --cases 500 --seed 401 --scenes lense --shortcut-heavy --eps-max-share 0.4 --wide-cameras --full-range-vars"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import sdf_playground_amd as sp
from oracle import pyoracle as po


FOVY = np.float32(60.0) * np.float32(3.14159265358979) / np.float32(180.0)


def draw_case(rng, scene, W, H, c, table=None, shortcut_heavy=False, eps_max_share=None, wide_cameras=False, full_range_vars=False):
    """Case c of a scene: its oracle frame `f` and what the renderer needs to render the same (camera, limits, variables, schedule,
    launch mode, step shortcuts).  The options beyond shortcut_heavy are off by default and then draw nothing: a seed gives the cases
    it always gave.
      eps_max_share    that share of the cases runs dist_eps at its largest, 1e-3, the other four epsilons anywhere in their ranges
                       (the length of a shadow ray's direction towards a directional light is |L| / (|L| + dist_eps))
      wide_cameras     one case in two from between the lense's blob fields, from above its upper field looking down through the
                       gaps (y up to 12), or from below its lower field
      full_range_vars  every variable drawn, one in four at an end of its range"""
    asp = np.float32(W) / np.float32(H)
    if table is None:
        table = po.var_table(scene)
    # camera: somewhere in a box around the origin, looking roughly at the scene's middle
    eye = (float(rng.uniform(-9, 9)), float(rng.uniform(0.2, 8)), float(rng.uniform(-9, 9)))
    tgt = (float(rng.uniform(-2, 2)), float(rng.uniform(0, 3)), float(rng.uniform(-2, 2)))
    if c % 5 == 4:  # sometimes from far away / from below the canopy / grazing the floor
        eye = (float(rng.uniform(-40, 40)), float(rng.choice([0.05, 0.5, 25.0])), float(rng.uniform(-40, 40)))
    if c % 7 == 6:  # under the floor, exactly on it, a hair above it (the fast plane divides the height by 1e-20)
        eye = (eye[0], float(rng.choice([-1.0, -0.05, 0.0, 1e-22, 1e-6])), eye[2])
    if wide_cameras and rng.random() < 0.5:
        kind = int(rng.integers(0, 3))
        xz = (float(rng.uniform(-15, 15)), float(rng.uniform(-15, 15)))
        if kind == 0:  # between the blob fields (|y| < 3.9), looking anywhere in the slab
            eye = (xz[0], float(rng.uniform(-3.8, 3.8)), xz[1])
            tgt = (float(rng.uniform(-8, 8)), float(rng.uniform(-4, 4)), float(rng.uniform(-8, 8)))
        elif kind == 1:  # above the upper field, looking down through its gaps
            eye = (xz[0], float(rng.uniform(6.2, 12)), xz[1])
            tgt = (xz[0] + float(rng.uniform(-6, 6)), float(rng.uniform(-5, 3)), xz[1] + float(rng.uniform(-6, 6)))
        else:  # below the lower field, looking up
            eye = (xz[0], float(rng.uniform(-12, -6.2)), xz[1])
            tgt = (xz[0] + float(rng.uniform(-6, 6)), float(rng.uniform(-3, 6)), xz[1] + float(rng.uniform(-6, 6)))
    stime = float(np.float32(rng.uniform(0, 30)))
    basis = po.camera_lookat(eye, tgt, FOVY, asp)
    f = po.default_frame(scene, W, H, basis=basis, stime=stime)
    limits = dict(iter_count=int(rng.choice([100, 100, 256, 37])), max_cost_default=int(rng.choice([7, 7, 9, 4])),
                  ray_count=int(rng.choice([8, 8, 3])), bounce_count=int(rng.choice([16, 16, 5])),
                  light_count=8, range=100.0, extension_lights=int(rng.choice([0, 0, 0, 7])),
                  extension_marble_reflection=float(rng.choice([0.0, 0.0, 0.0, 0.25])))
    others = lambda: dict(grad_eps=float(np.float32(rng.choice([1e-5, 1e-3, 2e-2]))), reflect_eps=float(np.float32(rng.choice([0.0, 1e-4, 1e-2]))),
                          refract_eps=float(np.float32(rng.choice([0.0, 1e-4, 1e-2]))), shadow_eps=float(np.float32(rng.choice([0.0, 1e-4, 5e-3]))))
    # the driver's epsilons: the reference's, or (one case in four) all five somewhere in their accepted ranges
    if eps_max_share is not None and rng.random() < eps_max_share:
        limits.update(dist_eps=float(np.float32(1e-3)), **others())
    elif rng.random() < 0.25:
        dist_eps = float(np.float32(rng.choice([1e-5, 3e-4, 1e-3])))
        limits.update(dist_eps=dist_eps, **others())
    else:
        limits.update(dist_eps=0.0001, grad_eps=0.0001, reflect_eps=0.001, refract_eps=0.001, shadow_eps=0.0003)
    values = {}
    for name, mn, mx, start, _st, _v, slot in table:
        if slot < 0:
            continue
        if full_range_vars:
            v = float(np.float32(rng.choice([mn, mx]) if rng.random() < 0.25 else rng.uniform(mn, mx)))
        elif rng.random() < 0.7:
            v = float(np.float32(rng.uniform(mn, mx)))
        else:
            continue
        values[name] = v
        f.scene_var[slot] = v
    schedule = int(rng.integers(0, 2))
    if shortcut_heavy:  # the pixel schedule with step shortcuts on, eight lights in half of the cases: what the escape rules and the delivered shadow rays see
        schedule = 1
        limits["extension_lights"] = int(rng.choice([0, 7]))
        if rng.random() < 0.5:  # any ray budget and queue length: the delivered shadow rays have to respect both
            limits["bounce_count"] = int(rng.integers(1, 17))
            limits["ray_count"] = int(rng.integers(1, 9))
    for k, v in limits.items():
        setattr(f, k, v)
    launch = int(rng.choice([sp.LAUNCH_AUTO, sp.LAUNCH_PER_TILE, sp.LAUNCH_PERSISTENT]))  # pixel schedule: how the tiles reach the waves
    shortcuts = (bool(rng.integers(0, 2)) or shortcut_heavy) and schedule == 1  # step shortcuts: same pixels, rays and hits; fewer steps counted
    return dict(f=f, eye=eye, tgt=tgt, stime=stime, limits=limits, values=values, schedule=schedule, launch=launch, shortcuts=shortcuts)


def draw_cases(cases, seed, size, scenes=None, **options):
    """(scene, c, case) for `cases` cases of every scene, in the order run() renders them (options: draw_case)"""
    rng = np.random.default_rng(seed)
    W, H = size
    for scene in (scenes or sp.scene_names()):
        table = po.var_table(scene)
        for c in range(cases):
            yield scene, c, draw_case(rng, scene, W, H, c, table, **options)


def same_as_oracle(img, st, ref, rst, shortcuts):
    """pixels, rays and hits bit for bit; the step counters too, or with step shortcuts never above the oracle's"""
    stats_same = np.array_equal(st, rst) if not shortcuts else (np.array_equal(st[..., 0], rst[..., 0]) and np.array_equal(st[..., 2], rst[..., 2]) and bool((st[..., 1] <= rst[..., 1]).all()))
    same = np.array_equal(img.view(np.uint32), ref.view(np.uint32)) and stats_same
    if not same:
        # NaN payloads may differ in sign/payload bits: compare values with NaN == NaN as well
        same = np.array_equal(img, ref, equal_nan=True) and stats_same
    return same


def run(cases, seed, size, scenes=None, verbose=False, shortcut_heavy=False, **options):
    W, H = size
    r = sp.SDFRenderer(0)
    bad = []
    n = 0
    current = None
    for scene, c, case in draw_cases(cases, seed, size, scenes, shortcut_heavy=shortcut_heavy, **options):
        if scene != current:
            if current is not None:
                print("%-20s %d cases done, %d mismatches so far" % (current, cases, len(bad)), flush=True)
            r.initShader(scene)
            current = scene
        f, limits, values, schedule = case["f"], case["limits"], case["values"], case["schedule"]
        r.setLimits(**limits)
        r.setParameters(case["stime"])
        cam = sp.Camera()
        cam.SetEye(case["eye"])
        cam.SetLookat(case["tgt"])
        cam.SetFOVY(float(FOVY))
        cam.SetAspect(float(np.float32(W) / np.float32(H)))
        r.resetVariables()
        for name, v in values.items():
            r.setValue(name, v)
        r.setSchedule(schedule)
        r.setLaunchMode(case["launch"])
        r.setStepShortcuts(case["shortcuts"])
        img, st = r.render(cam, W, H, pixel_stats=True)
        ref, rst, _ = po.render(scene, f, stats=True)
        n += 1
        if not same_as_oracle(img, st, ref, rst, case["shortcuts"]):
            diff = int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum())
            bad.append((scene, c, case["eye"], case["tgt"], case["stime"], limits, values, schedule, diff))
            print("MISMATCH", bad[-1], flush=True)
        elif verbose:
            print("ok", scene, c, flush=True)
    if current is not None:
        print("%-20s %d cases done, %d mismatches so far" % (current, cases, len(bad)), flush=True)
    r.setStepShortcuts(False)
    r.close()
    return n, bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--size", default="64x48")
    ap.add_argument("--scenes", default="")
    ap.add_argument("--shortcut-heavy", action="store_true", help="every case on the pixel schedule with step shortcuts, half of them with eight lights")
    ap.add_argument("--eps-max-share", type=float, default=None, help="that share of the cases with dist_eps = 1e-3, the other epsilons random")
    ap.add_argument("--wide-cameras", action="store_true", help="half of the cameras between, above or below the lense's blob fields")
    ap.add_argument("--full-range-vars", action="store_true", help="every variable drawn, one in four at an end of its range")
    a = ap.parse_args()
    w, h = (int(x) for x in a.size.split("x"))
    n, bad = run(a.cases, a.seed, (w, h), [s for s in a.scenes.split(",") if s] or None, shortcut_heavy=a.shortcut_heavy,
                 eps_max_share=a.eps_max_share, wide_cameras=a.wide_cameras, full_range_vars=a.full_range_vars)
    print("%d cases, %d mismatches" % (n, len(bad)))
    sys.exit(1 if bad else 0)

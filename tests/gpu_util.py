"""The scaffold of the GPU tier (tests/test_gpu_*.py): the one copy of what every family's file needs to put a renderer handle into
the state of an oracle frame, to move arrays to the device and back, and to check that a family's calls leave rendering alone; the
camera set-up and comparison of the parity tests; and what the handle-sequence tests do to a handle.  torch and sdf_playground_amd
are imported inside functions, so the module imports on a machine without a GPU (tests/test_gpu_scaffold_cpu.py pins it there).
Test infrastructure: the product never imports this.  Test modules import from here and from their family's *_util module, never
from each other."""
import contextlib
import math
import os

import numpy as np
import pytest

import handle_sequences as hs
import query_util as qu
from handle_sequences import DEFAULT_LIMITS  # noqa: F401  (the one literal; re-exported)


@pytest.fixture(scope="module")
def renderer():
    """one handle per test module: `from gpu_util import renderer  # noqa: F401` registers the fixture in the importing module"""
    import sdf_playground_amd as sp

    r = sp.SDFRenderer(0)
    yield r
    r.close()


# ---- the handle's state ---------------------------------------------------------------------------------------------------------------
def load(r, scene):
    if scene in qu.HLSL:
        r.initShaderHlsl(scene, os.path.join(qu.SCENES_DIR, scene + ".hlsl"))
    else:
        r.initShader(scene)


_load = load  # (setup's `load` argument hides the name)


def setup(r, scene, of, variables=None, limits=None, shortcuts=False, load=True):
    """the handle's state = the oracle frame `of`; limits: what differs from DEFAULT_LIMITS; load=False: the scene is loaded already"""
    if load:
        _load(r, scene)
    r.setParameters(of.stime)
    r.setCameraBasis(of.eye, of.front, of.right, of.top)
    r.setLimits(**dict(DEFAULT_LIMITS, **(limits or {})))
    r.setStepShortcuts(shortcuts)
    for name, v in (variables or {}).items():
        assert r.setValue(name, v)


def stats(r):
    s = r.getStats()
    return (s.pixels, s.rays, s.march_evals, s.hits, s.march_launches, s.shade_launches)


def raw(r):
    """-> (the library, the handle), for calls through the raw C ABI"""
    import sdf_playground_amd as sp

    return sp.load_library(), r._h


# ---- arrays ----------------------------------------------------------------------------------------------------------------------------
def to_device(a, dtype=None):
    """numpy -> a contiguous CUDA tensor (uint32 words as int32)"""
    import torch

    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def to_host(x, sync=True):
    """a tensor, a tuple of tensors or numpy (handed back as it is) -> numpy, after torch.cuda.synchronize() unless sync=False"""
    if sync:
        import torch

        torch.cuda.synchronize()
    if isinstance(x, tuple):
        return tuple(to_host(t, sync=False) for t in x)
    return x.cpu().numpy() if hasattr(x, "data_ptr") else x


@contextlib.contextmanager
def with_size(of, w, h):
    """the oracle frame `of` at w x h for the block, its own size after it"""
    size = of.width, of.height
    of.width, of.height = w, h
    try:
        yield of
    finally:
        of.width, of.height = size


# ---- "leaves rendering alone" --------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def rendering_untouched(r, w, h):
    """Renders w x h with pixel_stats, runs the block, and asserts that the block changed neither getStats() nor getTimings() and that
    a second render gives the same image bits, per-pixel counters and getStats().  Yields (the first image, its stats tuple)."""
    img0, st0 = r.render(None, w, h, pixel_stats=True)
    s0, t0 = stats(r), r.getTimings()
    yield img0, s0
    assert stats(r) == s0 and r.getTimings() == t0
    img1, st1 = r.render(None, w, h, pixel_stats=True)
    assert np.array_equal(img0.view(np.uint32), img1.view(np.uint32)) and np.array_equal(st0, st1) and stats(r) == s0


# ---- the parity tests' cameras, set-up and comparison (test_gpu_parity, test_gpu_jit, test_gpu_shortcuts, test_gpu_aa) ---------------
PARITY_TOL = 1e-4
PARITY_W, PARITY_H = 240, 160
TH = 0.3
FOVY = np.float32(60.0) * np.float32(3.14159265358979) / np.float32(180.0)


def parity_cameras():
    """-> ({scene: (kind, eye, target)}, fovy, aspect) of the PARITY_W x PARITY_H frames"""
    asp = np.float32(PARITY_W) / np.float32(PARITY_H)
    return {
        "fast_sphere": ("lookat", (0, 2, -3), (0, 1, 0)),
        "cube_sea": ("dir", (3 * math.cos(TH), 4.5, 3 * math.sin(TH)), (math.cos(TH + 0.6), -0.45, math.sin(TH + 0.6))),
        "labyrinth": ("dir", (1.5 * math.cos(TH), 5.0, 1.5 * math.sin(TH)), (math.cos(TH), -0.35, math.sin(TH))),
        "fractal": ("lookat", (2.2 * math.cos(TH), 1.6, 2.2 * math.sin(TH)), (0, 1, 0)),
        "lense": ("lookat", (7 * math.sin(-0.3), 0.5, 7 * math.cos(-0.3)), (0, 0, 0)),
        "gems": ("lookat", (2.5 * math.cos(TH), 2, 2.5 * math.sin(TH)), (0, 1, 0)),
        "light_shadows": ("lookat", (0, 5, -9), (0, 1, 0)),
        "cube": ("lookat", (2.5, 2.5, -3), (0, 1, 0)),
        "gyroid": ("lookat", (1.8, 1.6, -2.2), (0, 0, 0)),
        "basic_transparency": ("lookat", (2.0, 2.5, -4), (0, 2, 0)),
        "basic_clouds": ("lookat", (0, 2, -8), (0, 4, 0)),
        "coordinate_material": ("lookat", (3, 4, -5), (0, 2, 0)),
        "distortion": ("lookat", (0.8, 1.8, -2.5), (0, 1.5, 0)),
        "table": ("lookat", (2, 2, -3), (0, 1, 0)),
        "sierpinski": ("lookat", (1.2, 1.6, -2.2), (0, 1.2, 0)),
        "neon": ("lookat", (-2, 2.5, -3.5), (0, 2, 1)),
        "fractal2": ("lookat", (1.8, 1.8, -2.0), (0, 1, 0)),
        "shell": ("lookat", (-2.2, 1.8, -2.0), (0, 1, 0)),
        "spiral": ("lookat", (0, 4, -12), (0, 3, 0)),
        "terrain": ("lookat", (6, 5, -8), (0, 0, 0)),
        "tiling": ("lookat", (0, 4.5, -9), (0, 4, 0)),
        "tree": ("lookat", (0, 2.2, -4), (0, 1, 1)),
    }, FOVY, asp


def parity_setup(renderer, oracle, scene, stime, limits=None, variables=None):
    """the handle and an oracle frame in the same state, the camera through the C++ host camera -> the frame"""
    import sdf_playground_amd as sp

    cams, fovy, asp = parity_cameras()
    kind, eye, tgt = cams[scene]
    basis = (oracle.camera_lookat if kind == "lookat" else oracle.camera_direction)(eye, tgt, fovy, asp)
    f = oracle.default_frame(scene, PARITY_W, PARITY_H, basis=basis, stime=stime)
    renderer.initShader(scene)
    renderer.setParameters(stime)
    cam = sp.Camera()
    cam.SetEye(eye)
    (cam.SetLookat if kind == "lookat" else cam.SetDirection)(tgt)
    cam.SetFOVY(float(fovy))
    cam.SetAspect(float(asp))
    renderer.setCamera(cam)
    # the C++ host camera must reproduce the oracle's (and the reference's) basis bit for bit
    assert np.array_equal(renderer.getCameraBasis().view(np.uint32), basis.view(np.uint32))
    renderer.setLimits(**DEFAULT_LIMITS)
    if limits:
        renderer.setLimits(**limits)
        for k, v in limits.items():
            setattr(f, k, v)
    if variables:
        table = {r[0]: r for r in oracle.var_table(scene)}
        for k, v in variables.items():
            assert renderer.setValue(k, v)
            slot = table[k][6]
            if slot >= 0:
                f.scene_var[slot] = v
            else:
                setattr(f, k, v)
    return f


def parity_compare(renderer, oracle, scene, f, schedule):
    """-> whether the frame is the oracle's bit for bit, after asserting the tolerance and the counters"""
    renderer.setSchedule(schedule)
    img, st = renderer.render(None, PARITY_W, PARITY_H, pixel_stats=True)
    ref, rst, tot = oracle.render(scene, f, stats=True)
    assert not np.isnan(img).any()
    diff = np.abs(img.astype(np.float64) - ref.astype(np.float64)).max()
    assert diff <= PARITY_TOL, "%s: L-inf %g" % (scene, diff)
    assert np.array_equal(st, rst), "%s: per-pixel ray/eval/hit counters differ" % scene
    s = renderer.getStats()
    assert (s.pixels, s.rays, s.march_evals, s.hits) == tuple(int(x) for x in tot)
    return np.array_equal(img.view(np.uint32), ref.view(np.uint32))


# ---- the handle sequences (test_gpu_handle_state, test_gpu_handle_mixed): what a step does to the handle -----------------------------
def totals(s):
    return (int(s.pixels), int(s.rays), int(s.march_evals), int(s.hits))


def orbit_camera(r, scene, t, w, h):
    """the handle's camera = handle_sequences.camera(scene, t) for a w x h frame"""
    import sdf_playground_amd as sp

    kind, eye, target = hs.camera(scene, t)
    cam = sp.Camera()
    cam.SetEye(eye)
    (cam.SetLookat if kind == "lookat" else cam.SetDirection)(target)
    cam.SetFOVY(float(FOVY))
    cam.SetAspect(float(np.float32(w) / np.float32(h)))
    r.setCamera(cam)


def apply_changes(r, changes):
    """the settings a step changes, in the order a host would make them (a scene load resets the variables first)"""
    if "scene" in changes:
        load(r, changes["scene"])
    if "fif" in changes:
        r.setFramesInFlight(changes["fif"])
    if "schedule" in changes:
        r.setSchedule(hs.SCHEDULE[changes["schedule"]])
    if "launch" in changes:
        r.setLaunchMode(hs.LAUNCH[changes["launch"]])
    if "shortcuts" in changes:
        r.setStepShortcuts(changes["shortcuts"])
    if "limits" in changes:
        r.setLimits(**hs.limits(changes["limits"]))
    if "var" in changes:
        assert r.setValue(*changes["var"])
    if "stime" in changes:
        r.setParameters(changes["stime"])
    if "split" in changes:
        r.setStripSplit(*changes["split"])

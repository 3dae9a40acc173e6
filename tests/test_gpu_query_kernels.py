"""GPU tier: every kind of query kernel (sdf_playground_amd/csrc/sdfr_query_args.h: SDFR_FOR_EACH_QUERY_KERNEL) through both of its tables.
fast_sphere answers every kind as the built-in scene -- the kernels of its unit, sdfr_query_scene.hip -- and as its own text loaded as a
run-time scene -- the kernels of the query module, sdfr_jit_unit.h --, in a plain frame and in a debug-plane frame, so that both [kind][DBG]
columns of both tables are launched.  Both sides instantiate the same bodies with the same code-generation options, so the answers must be
the same bits; a kernel looked up under another kind's name, or launched with another kind's arguments, is not.
Shapes: the smallest that reach a second block and a ragged last one."""
import ctypes

import numpy as np
import pytest

import jit_util

pytestmark = pytest.mark.gpu

N = 65           # items: one full block of 64 and one more
W = H = 9        # a frame of 2 x 2 tiles, ragged on both sides
ORIGIN, CELL, DIMS = (-0.875, 0.3, -0.525), 0.35, (5, 4, 3)  # a lattice around the sphere (radius 0.5 about (0, 1, 0))
FRAMES = {"plain": {}, "debug": {"debug_ny": 1.0, "debug_y": 0.4}}
SPANS = dict(min_step=0.02, max_steps=64, max_spans=2)


def _inputs():
    rng = np.random.default_rng(20261)
    unit = rng.normal(size=(N, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    centre = np.array([0.0, 1.0, 0.0])
    return dict(points=(centre + rng.uniform(-1.0, 1.0, size=(N, 3))).astype(np.float32),
                origins=(centre + 3.0 * unit + rng.uniform(-0.3, 0.3, size=(N, 3))).astype(np.float32),  # towards the sphere, some past it
                dirs=(-unit).astype(np.float32),
                on_sphere=(centre + 0.5 * unit).astype(np.float32), normals=unit.astype(np.float32),
                pixels=rng.integers(-1, W + 1, size=(N, 2)).astype(np.int32))  # some outside the frame


def _words(a):
    """an answer as its bytes"""
    if isinstance(a, ctypes.Structure):
        return np.frombuffer(bytes(a), np.uint8)
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _answers(r, sp, x):
    """{kind: [arrays]} of the scene loaded into r, for the variables and camera it has"""
    out = {}
    out["points"] = r.queryDistance(x["points"], normals=True)
    hits = r.queryRays(x["origins"], x["dirs"])
    out["rays"] = [hits]
    out["picks"] = [r.pick(x["pixels"], W, H)]
    out["ray surfaces"] = r.queryRaySurfaces(x["origins"], x["dirs"], hits=True)
    out["mesh rays"] = r.meshSurfaces(x["on_sphere"], x["normals"], 0.1, hits=True)
    out["occlusion"] = [r.queryOcclusion(x["on_sphere"], x["normals"], 0.01, 1.5)]
    out["hit occlusion"] = [r.hitOcclusion(hits, 0.01, 1.5)]
    out["lighting"] = r.queryRayLighting(x["origins"], x["dirs"], hits=True, lights=True)
    out["spans"] = r.querySpans(x["origins"], x["dirs"], **SPANS)
    out["frame surfaces"] = r.pickSurfaces(None, W, H, hits=True)
    out["frame spans"] = r.pickSpans(None, W, H, **SPANS)
    pos, nrm, idx = r.extractMesh(ORIGIN, CELL, DIMS)
    assert len(pos) > 4 and len(pos) % 4 and len(idx) > 0  # several blocks of the sharp kernel's 4 vertices, and a ragged last one
    out["mesh"] = [pos, nrm, idx]
    out["sharp mesh"] = list(r.extractMesh(ORIGIN, CELL, DIMS, sharp=True))
    baked = r.bakeAtlas(pos, nrm, idx, tile=8, reach=2.0 * CELL, layers=("albedo", "normal", "lit"))
    assert baked["valid"].shape[0] > 8 or baked["valid"].shape[1] > 8
    out["atlas"] = [baked[k] for k in ("albedo", "normal", "lit", "valid")]
    out["slices"] = [a for a in r.extractSlices((-0.9, 0.8, -0.9), (0.2, 0.0, 0.0), (0.0, 0.0, 0.2), (0.0, 0.3, 0.0), dims=(W, H), layers=2) if a is not None]
    grid, depth = sp.measureGrid((-0.9, 0.4, -0.9), (0.9, 1.6, 0.9), 0.2, axis="y")
    assert (grid.nu, grid.nv) == (W, H)
    out["measure"] = r.measure(grid, 0.05, t_max=depth, max_steps=64, columns=True)
    return out


KINDS = ("points", "rays", "picks", "ray surfaces", "mesh rays", "occlusion", "hit occlusion", "lighting", "spans", "frame surfaces", "frame spans",
         "mesh", "sharp mesh", "atlas", "slices", "measure")


@pytest.fixture(scope="module")
def answers():
    """{(side, frame): {kind: [arrays]}}: one handle per side, host arrays"""
    import sdf_playground_amd as sp

    x = _inputs()
    cam = sp.Camera()
    cam.SetEye((1.5, 2.5, -5.0))
    cam.SetLookat((0.0, 1.0, 0.0))
    cam.SetAspect(W / H)
    got = {}
    for side in ("built in", "run time"):
        r = sp.SDFRenderer(0)
        try:
            if side == "built in":
                r.initShader("fast_sphere")
            else:
                r.initShaderSource("fast_sphere_rt", jit_util.aot_scene_source("SceneFastSphere"))
            r.setParameters(0.75)
            r.setCamera(cam)
            for frame, variables in FRAMES.items():
                r.resetVariables()
                for name, v in variables.items():
                    assert r.setValue(name, v)
                got[side, frame] = _answers(r, sp, x)
        finally:
            r.close()
    return got


def test_every_kind_is_asked(answers):
    for key, got in answers.items():
        assert tuple(got) == KINDS, key
    # the frames differ: the debug plane is in the debug frame's answers
    assert any(not np.array_equal(_words(a), _words(b)) for a, b in zip(answers["built in", "plain"]["rays"], answers["built in", "debug"]["rays"]))
    # and the rays hit something: the comparison below is not one of misses
    assert int((answers["built in", "plain"]["rays"][0]["hit"] == 1).sum()) > 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_built_in_and_run_time_kernels_answer_the_same_bits(answers, frame, kind):
    a, b = answers["built in", frame][kind], answers["run time", frame][kind]
    assert len(a) == len(b) > 0
    for k, (u, v) in enumerate(zip(a, b)):
        wu, wv = _words(u), _words(v)
        assert wu.size == wv.size > 0, (kind, k)
        differing = np.flatnonzero(wu != wv)
        assert differing.size == 0, "%s, %s frame, answer %d: %d of %d bytes differ, the first at %d" % (kind, frame, k, differing.size, wu.size, differing[0])

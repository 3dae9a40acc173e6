"""Shared by the query tests (test_query_cpu.py, test_gpu_query.py): the oracle's definitions of the three scene queries
(tests/cpp/query_oracle.h), the library's query functions built for the CPU (tests/cpp/query_host.cpp), the frames and the
seeded sample sets, and the bit comparison.  Test infrastructure: the product never imports this."""
import ctypes
import glob
import os
import sys

import numpy as np

import cppbuild
from cppbuild import BUILD, CSRC, HERE, ORACLE, ROOT

SCENES_DIR = os.path.join(ROOT, "sdf_playground_amd", "scenes")
for _d in (ROOT, HERE):
    if _d not in sys.path:
        sys.path.insert(0, _d)

from oracle import pyoracle as po  # noqa: E402

# the scenes compiled ahead of time: the 22 public ones and the two diagnostic scenes
BUILTIN = ["fast_sphere", "cube_sea", "labyrinth", "fractal", "lense", "gems", "light_shadows", "cube", "gyroid", "basic_transparency", "basic_clouds",
           "coordinate_material", "distortion", "table", "sierpinski", "neon", "fractal2", "shell", "spiral", "terrain", "tiling", "tree",
           "debug_materials", "normal_test"]
# run-time scenes in the reference's dialect that have an oracle twin (oracle/test_scenes.h)
HLSL = ["noise_lod", "dialect_tour"]
TIMES = [0.0, 1.25]
# the slider scenes, with values off their defaults
MOVED_VARS = {"lense": {"xpos": 0.7, "zpos": 6.5, "mixing": 0.35}, "cube": {"size": 1.4, "ypos": 0.3, "red": 0.2},
              "neon": {"r1": 1.3, "spacing": 0.05}, "tiling": {"m1": 2.0, "width": 0.25, "truchet_width": 0.1},
              "fractal2": {"slider": 1.7}, "terrain": {"levels": 5.0}}
FLAGS = cppbuild.EXACT_FLAGS + ["-w", "-pthread"]
HIT_WORDS = 12


_libs = {}


def build_lib(name, source, flags=(), deps=()):
    """tests/cpp/_build/lib<name>.so from tests/cpp/<source> with FLAGS and `flags`, stale when the source or one of `deps` is newer -> its path"""
    return cppbuild.compile(os.path.join(BUILD, "lib%s.so" % name), [os.path.join(HERE, "cpp", source)], deps, FLAGS + list(flags))


def build_oracle_lib():
    """librecord_oracle.so, the one library of the oracle's definitions (the qo_, so_, lo_ and oo_ entry points): tests/cpp/record_oracle.cpp
    over its headers, the oracle's and the library's direction table; stale when one of them is newer"""
    name = "record_oracle"
    if name not in _libs:
        deps = sorted(glob.glob(os.path.join(HERE, "cpp", "*_oracle.h"))) + [os.path.join(CSRC, "sdfr_occlusion_dirs.h")] + cppbuild.oracle_headers()
        _libs[name] = ctypes.CDLL(build_lib(name, name + ".cpp", ["-I" + ORACLE, "-I" + CSRC], deps))
        assert _libs[name].qo_frame_size() == ctypes.sizeof(po.OrcFrame)
    return _libs[name]


def build_host_lib(name, source, scene, text=None):
    """lib<name>_<key>.so of the library's own functions for the CPU, from tests/cpp/<source> over csrc: one build ("builtin") for the
    built-in scenes, one per run-time scene -- a scene of HLSL, or any name with its dialect `text` -- translated by the library as
    sdfr_load_scene_hlsl translates it"""
    key = scene if scene in HLSL or text is not None else "builtin"
    if (name, key) not in _libs:
        deps = [os.path.join(HERE, "cpp", "host_common.h")] + cppbuild.csrc_headers()
        flags = ["-I" + CSRC]
        if key != "builtin":
            import sdf_playground_amd as sp

            if text is None:
                text = open(os.path.join(SCENES_DIR, scene + ".hlsl")).read()
            gen = os.path.join(BUILD, scene + ".scene.inc")
            cppbuild.scene_include(gen, text, sp.translate_scene_hlsl)
            deps.append(gen)
            flags.append('-DSDFR_HLSL_SCENE_FILE="%s"' % gen)
        _libs[name, key] = ctypes.CDLL(build_lib("%s_%s" % (name, key), source, flags, deps))
    return _libs[name, key]


def oracle_lib():
    L = build_oracle_lib()
    vp = ctypes.c_void_p
    L.qo_points.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, vp, vp, vp]
    L.qo_rays.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, vp, vp, ctypes.c_float, vp]
    L.qo_pick.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, vp, vp]
    return L


def host_lib(scene):
    """The library's query functions for the CPU"""
    L = build_host_lib("query_host", "query_host.cpp", scene)
    vp = ctypes.c_void_p
    L.qh_points.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, vp, vp, vp]
    L.qh_rays.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, vp, vp, ctypes.c_float, vp]
    L.qh_pick.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]
    return L


# ---- frames ---------------------------------------------------------------------------------------------------------------------
def frame(scene, stime, width=64, height=48, variables=None):
    """pyoracle.default_frame (the start-up camera, the reference's limits and variable defaults), variables moved as given."""
    f = po.default_frame(scene, width, height, stime=stime)
    if variables:
        table = {row[0]: row[6] for row in po.var_table(scene)}
        for name, v in variables.items():
            slot = table[name]
            if slot >= 0:
                f.scene_var[slot] = v
            else:
                setattr(f, name, v)
    return f


def host_frame(of, shortcuts=False):
    from hostsim import frame_from_oracle

    U = frame_from_oracle(of)
    U.step_shortcuts = 1 if shortcuts else 0
    return U


# ---- the three definitions ------------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def oracle_points(scene, of, pts, normals=True):
    pts = np.ascontiguousarray(pts, np.float32)
    d = np.empty(len(pts), np.float32)
    n = np.empty((len(pts), 3), np.float32) if normals else None
    assert oracle_lib().qo_points(scene.encode(), ctypes.byref(of), len(pts), _p(pts), _p(d), _p(n) if normals else None) == 0
    return d, n


def oracle_rays(scene, of, origins, dirs, max_distance=0.0):
    o, d = np.ascontiguousarray(origins, np.float32), np.ascontiguousarray(dirs, np.float32)
    h = np.empty((len(o), HIT_WORDS), np.uint32)
    assert oracle_lib().qo_rays(scene.encode(), ctypes.byref(of), len(o), _p(o), _p(d), max_distance, _p(h)) == 0
    return h


def oracle_pick(scene, of, pixels):
    px = np.ascontiguousarray(pixels, np.int32)
    h = np.empty((len(px), HIT_WORDS), np.uint32)
    assert oracle_lib().qo_pick(scene.encode(), ctypes.byref(of), len(px), _p(px), _p(h)) == 0
    return h


def host_points(scene, U, pts, normals=True):
    pts = np.ascontiguousarray(pts, np.float32)
    d = np.empty(len(pts), np.float32)
    n = np.empty((len(pts), 3), np.float32) if normals else None
    assert host_lib(scene).qh_points(scene.encode(), ctypes.byref(U), len(pts), _p(pts), _p(d), _p(n) if normals else None) == 0
    return d, n


def host_rays(scene, U, origins, dirs, max_distance=0.0):
    o, d = np.ascontiguousarray(origins, np.float32), np.ascontiguousarray(dirs, np.float32)
    h = np.empty((len(o), HIT_WORDS), np.uint32)
    assert host_lib(scene).qh_rays(scene.encode(), ctypes.byref(U), len(o), _p(o), _p(d), max_distance, _p(h)) == 0
    return h


def host_pick(scene, U, width, height, pixels):
    px = np.ascontiguousarray(pixels, np.int32)
    h = np.empty((len(px), HIT_WORDS), np.uint32)
    assert host_lib(scene).qh_pick(scene.encode(), ctypes.byref(U), width, height, len(px), _p(px), _p(h)) == 0
    return h


# ---- samples --------------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def ray_samples(of, seed, n):
    """Rays from the camera's eye into its view cone, from random points of a box around it (some inside solids), and directions of
    length 0.25 .. 4 (used as given)."""
    rng = np.random.default_rng(seed)
    eye = np.array(of.eye, np.float64)
    front, right, top = (np.array(getattr(of, k), np.float64) for k in ("front", "right", "top"))
    k = n // 2
    sx, sy = rng.uniform(-1, 1, k), rng.uniform(-1, 1, k)
    d0 = front[None] + sx[:, None] * right[None] + sy[:, None] * top[None]
    d0 /= np.linalg.norm(d0, axis=1, keepdims=True)
    o0 = np.repeat(eye[None], k, 0)
    o1 = eye[None] + rng.uniform(-4, 4, (n - k, 3)) * np.array([1.0, 0.6, 1.0]) + np.array([0.0, 0.0, 3.0])
    d1 = _unit(rng, n - k)
    dirs = np.concatenate([d0, d1]) * np.exp(rng.uniform(np.log(0.25), np.log(4.0), (n, 1)))
    dirs[: n // 8] = np.concatenate([d0, d1])[: n // 8]  # some exactly as made: unit length up to rounding
    return np.concatenate([o0, o1]).astype(np.float32), dirs.astype(np.float32)


def point_samples(scene, of, seed, n):
    """Four seeded sets: a box around the camera, far points (|p| up to 1e3), points within +-4 dist_eps of the oracle's ray hits,
    exact zeros and denormal coordinates."""
    rng = np.random.default_rng(seed)
    eye = np.array(of.eye, np.float64)
    q = n // 4
    box = eye[None] + rng.uniform(-5, 5, (q, 3)) + np.array([0.0, -1.0, 3.0])
    far = _unit(rng, q) * (10.0 ** rng.uniform(0, 3, (q, 1)))
    o, d = ray_samples(of, seed + 1, 2 * q)
    hits = oracle_rays(scene, of, o, d)
    pos = hits[:, 2:5].view(np.float32)
    pos = pos[(hits[:, 10] == 1) & np.isfinite(pos).all(1)]
    if len(pos) == 0:
        pos = box[:1]
    near = pos[rng.integers(0, len(pos), q)] + rng.uniform(-4, 4, (q, 3)) * of.dist_eps
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 1.1754942e-38], np.float32)
    special = tiny[rng.integers(0, len(tiny), (n - 3 * q, 3))].astype(np.float64)
    special[::3, 1] = rng.uniform(-1, 3, len(special[::3]))  # denormal x/z over the floor and objects
    return np.concatenate([box, far, near, special]).astype(np.float32)


def pick_grid(width, height):
    """every pixel of the frame, and a few outside it"""
    ys, xs = np.mgrid[0:height, 0:width]
    inside = np.stack([xs.ravel(), ys.ravel()], 1)
    outside = np.array([[-1, 0], [0, -1], [width, 0], [0, height], [-7, height + 3], [2 ** 31 - 1, 5], [-2 ** 31, -2 ** 31]])
    return np.concatenate([inside, outside]).astype(np.int32)


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """element-wise: equal bit patterns, or both NaN"""
    a32, b32 = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    af, bf = a32.view(np.float32), b32.view(np.float32)
    return (a32 == b32) | (np.isnan(af) & np.isnan(bf))


def assert_same(what, got, want):
    ok = same_bits(got, want)
    if not ok.all():
        bad = np.argwhere(~ok)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d words differ; first at %s: got %r want %r" % (what, len(bad), ok.size, i, got[i[0]], want[i[0]]))


def hits_array(h):
    """HIT_DTYPE records or [n, 12] 32-bit words -> [n, 12] uint32"""
    h = np.ascontiguousarray(h)
    return h.view(np.uint32).reshape(-1, HIT_WORDS)

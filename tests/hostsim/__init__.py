"""tests/hostsim -- TEST-ONLY CPU build of the product's per-pixel pipeline stages
(sdf_playground_amd/csrc/*.h).  It lets the CPU test tier bit-compare the stage arithmetic
of the HIP kernels with the oracle without a GPU.  The product never loads this library."""
import ctypes
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(_HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(_HERE))

import cppbuild  # noqa: E402

_FLAGS = cppbuild.EXACT_FLAGS + ["-pthread", "-I" + cppbuild.CSRC]


class FrameU(ctypes.Structure):
    """Mirror of sdfr::FrameU (sdf_playground_amd/csrc/sdfr_frame.h)."""

    _fields_ = [
        ("eye", ctypes.c_float * 3), ("front", ctypes.c_float * 3), ("right", ctypes.c_float * 3), ("top", ctypes.c_float * 3),
        ("stime", ctypes.c_float),
        ("width", ctypes.c_int), ("height", ctypes.c_int),
        ("iter_count", ctypes.c_int), ("bounce_count", ctypes.c_int), ("ray_count", ctypes.c_int), ("light_count", ctypes.c_int),
        ("range", ctypes.c_float), ("max_cost_default", ctypes.c_uint),
        ("debug_nx", ctypes.c_float), ("debug_ny", ctypes.c_float), ("debug_nz", ctypes.c_float), ("debug_scale", ctypes.c_float),
        ("debug_x", ctypes.c_float), ("debug_y", ctypes.c_float), ("debug_z", ctypes.c_float), ("show_objects", ctypes.c_float),
        ("scene_var", ctypes.c_float * 8),
        ("debug_normal", ctypes.c_float * 3), ("debug_plane_on", ctypes.c_int), ("show_on", ctypes.c_int),
        ("ddx", ctypes.c_float), ("ddy", ctypes.c_float), ("sky_s", ctypes.c_float), ("sky_c", ctypes.c_float),
        ("su", ctypes.c_float * 48),
        ("extension_lights", ctypes.c_int), ("ext_light", (ctypes.c_float * 6) * 7), ("extension_marble_reflection", ctypes.c_float),
        ("step_shortcuts", ctypes.c_int),
        ("dist_eps", ctypes.c_float), ("grad_eps", ctypes.c_float), ("reflect_eps", ctypes.c_float), ("refract_eps", ctypes.c_float),
        ("shadow_eps", ctypes.c_float),
        ("widthf", ctypes.c_float), ("heightf", ctypes.c_float),
    ]


_lib = None


def lib():
    global _lib
    if _lib is None:
        so = cppbuild.compile(os.path.join(_HERE, "libhostsim.so"), [os.path.join(_HERE, "hostsim.cpp")],
                              [os.path.join(_HERE, "render_rows.h")] + cppbuild.csrc_headers(), _FLAGS)
        _lib = ctypes.CDLL(so)
        _lib.hostsim_math.restype = ctypes.c_float
        _lib.hostsim_math.argtypes = [ctypes.c_int, ctypes.c_float, ctypes.c_float]
        assert _lib.hostsim_frame_size() == ctypes.sizeof(FrameU)
    return _lib


def frame_from_oracle(of):
    """Copy the inputs of an oracle OrcFrame into a product FrameU."""
    f = FrameU()
    lib().hostsim_frame_defaults(ctypes.byref(f))
    for name in ("stime", "width", "height", "iter_count", "bounce_count", "ray_count", "light_count", "range", "max_cost_default",
                 "debug_nx", "debug_ny", "debug_nz", "debug_scale", "debug_x", "debug_y", "debug_z", "show_objects", "extension_lights", "extension_marble_reflection",
                 "dist_eps", "grad_eps", "reflect_eps", "refract_eps", "shadow_eps"):
        setattr(f, name, getattr(of, name))
    for i in range(3):
        f.eye[i], f.front[i], f.right[i], f.top[i] = of.eye[i], of.front[i], of.right[i], of.top[i]
    for i in range(8):
        f.scene_var[i] = of.scene_var[i]
    return f


def render(scene, frame, stats=True, nthreads=None):
    W, H = frame.width, frame.height
    out = np.zeros((H, W, 4), np.float32)
    st = np.zeros((H, W, 3), np.uint32) if stats else None
    rc = lib().hostsim_render(scene.encode(), ctypes.byref(frame), out.ctypes.data_as(ctypes.c_void_p),
                              st.ctypes.data_as(ctypes.c_void_p) if stats else None, nthreads or cppbuild.default_threads())
    if rc != 0:
        raise ValueError("hostsim_render failed: %d" % rc)
    return out, st


# ---- scenes in the reference's dialect (sdfr_load_scene_hlsl), built for the CPU -----------------------------------------
_HLSL_DIR = os.path.join(_HERE, "_hlsl")


def build_hlsl(name, text, cpp=False):
    """Compiles a run-time scene with g++ around the product's per-pixel pipeline (hlsl_host.cpp) and returns the loaded library and
    the scene's variable slots.  `text` is in the reference's dialect and translated by the library (sdfr_translate_scene_hlsl), or,
    cpp=True, in the library's C++ form (`struct Scene`, sdf_playground_amd/scenes/README.md), which may have a prepare()."""
    translate = None
    if not cpp:
        if cppbuild.ROOT not in sys.path:
            sys.path.insert(0, cppbuild.ROOT)
        import sdf_playground_amd as sp

        translate = sp.translate_scene_hlsl
    gen = os.path.join(_HLSL_DIR, name + ".scene.inc")
    slots = cppbuild.scene_include(gen, text, translate)
    flags = _FLAGS + ["-w", '-DSDFR_HLSL_SCENE_FILE="%s"' % gen] + (["-DSDFR_SCENE_HAS_PREPARE=1"] if cpp else [])
    so = cppbuild.compile(os.path.join(_HLSL_DIR, "lib%s.so" % name), [os.path.join(_HERE, "hlsl_host.cpp")],
                          [gen, os.path.join(_HERE, "render_rows.h")] + cppbuild.csrc_headers(), flags)
    L = ctypes.CDLL(so)
    assert L.hlslsim_frame_size() == ctypes.sizeof(FrameU)
    return L, slots


def render_hlsl(L, frame, stats=True, nthreads=None):
    W, H = frame.width, frame.height
    out = np.zeros((H, W, 4), np.float32)
    st = np.zeros((H, W, 3), np.uint32) if stats else None
    rc = L.hlslsim_render(ctypes.byref(frame), out.ctypes.data_as(ctypes.c_void_p), st.ctypes.data_as(ctypes.c_void_p) if stats else None,
                          nthreads or cppbuild.default_threads())
    assert rc == 0
    return out, st


render_scene_source = render_hlsl

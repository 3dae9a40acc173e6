"""Shared by the surface tests (test_surface_cpu.py, test_gpu_surface.py): the oracle's definition of the surface record
(tests/cpp/surface_oracle.h), the library's surface functions built for the CPU (tests/cpp/surface_host.cpp), and the host-made
rays towards mesh vertices.  Frames, samples and the bit comparison are query_util's.  Test infrastructure: the product never
imports this."""
import ctypes

import numpy as np

import query_util as qu

HIT_WORDS = qu.HIT_WORDS
SURFACE_WORDS = 32

def oracle_lib():
    L = qu.build_oracle_lib()
    vp = ctypes.c_void_p
    L.so_rays.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, vp, vp, ctypes.c_float, vp, vp]
    L.so_pick.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, vp, vp, vp]
    return L


def host_lib(scene):
    """The library's surface functions for the CPU"""
    L = qu.build_host_lib("surface_host", "surface_host.cpp", scene)
    vp = ctypes.c_void_p
    L.sh_rays.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_float, vp, vp]
    L.sh_pick.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp]
    return L


def _out(n):
    return np.empty((n, HIT_WORDS), np.uint32), np.empty((n, SURFACE_WORDS), np.uint32)


def oracle_rays(scene, of, origins, dirs, max_distance=0.0):
    """(hits [n, 12], surfaces [n, 32]) as uint32 words"""
    o, d = np.ascontiguousarray(origins, np.float32), np.ascontiguousarray(dirs, np.float32)
    h, s = _out(len(o))
    assert oracle_lib().so_rays(scene.encode(), ctypes.byref(of), len(o), qu._p(o), qu._p(d), max_distance, qu._p(h), qu._p(s)) == 0
    return h, s


def oracle_pick(scene, of, pixels):
    px = np.ascontiguousarray(pixels, np.int32)
    h, s = _out(len(px))
    assert oracle_lib().so_pick(scene.encode(), ctypes.byref(of), len(px), qu._p(px), qu._p(h), qu._p(s)) == 0
    return h, s


def mesh_rays(positions, normals, reach):
    """The rays sdfr_mesh_surfaces defines, made on the host in fp32: origin = position + reach * normal (one multiply, then one add),
    dir = -normal, max_distance = 2 * reach."""
    p, n = np.ascontiguousarray(positions, np.float32), np.ascontiguousarray(normals, np.float32)
    r = np.float32(reach)
    off = (n * r).astype(np.float32)
    return (p + off).astype(np.float32), (-n).astype(np.float32), float(np.float32(2.0) * r)


def oracle_mesh(scene, of, positions, normals, reach):
    o, d, reach2 = mesh_rays(positions, normals, reach)
    return oracle_rays(scene, of, o, d, reach2)


def host_rays(scene, U, origins, dirs, max_distance=0.0):
    o, d = np.ascontiguousarray(origins, np.float32), np.ascontiguousarray(dirs, np.float32)
    h, s = _out(len(o))
    assert host_lib(scene).sh_rays(scene.encode(), ctypes.byref(U), 0, len(o), qu._p(o), qu._p(d), max_distance, qu._p(h), qu._p(s)) == 0
    return h, s


def host_mesh(scene, U, positions, normals, reach):
    p, n = np.ascontiguousarray(positions, np.float32), np.ascontiguousarray(normals, np.float32)
    h, s = _out(len(p))
    assert host_lib(scene).sh_rays(scene.encode(), ctypes.byref(U), 1, len(p), qu._p(p), qu._p(n), reach, qu._p(h), qu._p(s)) == 0
    return h, s


def host_pick(scene, U, width, height, pixels):
    px = np.ascontiguousarray(pixels, np.int32)
    h, s = _out(len(px))
    assert host_lib(scene).sh_pick(scene.encode(), ctypes.byref(U), width, height, len(px), qu._p(px), qu._p(h), qu._p(s)) == 0
    return h, s


def frame_pixels(width, height):
    """every pixel of the frame in row-major order: item y * width + x"""
    ys, xs = np.mgrid[0:height, 0:width]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)


def surfaces_array(s):
    """SURFACE_DTYPE records, a device tensor's copy or [n, 32] 32-bit words -> [n, 32] uint32"""
    return np.ascontiguousarray(s).view(np.uint32).reshape(-1, SURFACE_WORDS)


def assert_same(what, got, want):
    """(hits, surfaces) pairs, or single arrays"""
    if isinstance(got, tuple):
        qu.assert_same(what + ": hits", qu.hits_array(got[0]), want[0])
        qu.assert_same(what + ": surfaces", surfaces_array(got[1]), want[1])
    else:
        qu.assert_same(what, got, want)

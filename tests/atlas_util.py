"""Shared by the atlas tests (test_atlas_cpu.py, test_gpu_atlas.py): the oracle's definition of the texture atlas
(tests/cpp/atlas_oracle.cpp: layout, UVs, texel -> point and normal) with the surface and lighting oracles applied to its texels, the
library's atlas code built for the CPU (tests/cpp/atlas_host.cpp), the two test meshes and the hand-made one.  Frames and the bit
comparison are query_util's.  Test infrastructure: the product never imports this."""
import ctypes
import functools

import numpy as np

import lighting_util as lu
import mesh_util as mu
import query_util as qu
import surface_util as su

ALBEDO, NORMAL, LIT = 1, 2, 4
LAYER_NAMES = {ALBEDO: "albedo", NORMAL: "normal", LIT: "lit"}
ONE = np.float32(1.0).view(np.uint32)
# the meshes of the lighting tests, built as tests/test_lighting_cpu.py builds them: stime, origin, cell, dims
MESHES = lu.MESHES
W, H = 64, 48

_oracle = []


def oracle_lib():
    if not _oracle:
        L = ctypes.CDLL(qu.build_lib("atlas_oracle", "atlas_oracle.cpp"))  # no header but the standard library's
        vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
        L.ao_layout.argtypes = [i64, ci, ci, vp]
        L.ao_uvs.argtypes = [i64, ci, ci, vp]
        L.ao_texels.argtypes = [i64, ci, ci, i64, vp, vp, vp, vp, vp, vp]
        _oracle.append(L)
    return _oracle[0]


def host_lib(scene="fast_sphere"):
    """The library's atlas plan, texel map and bake for the CPU"""
    L = qu.build_host_lib("atlas_host", "atlas_host.cpp", scene)
    vp, i64, ci, cf, u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_uint32
    L.ah_layout.argtypes = [i64, ci, ci, vp]
    L.ah_uvs.argtypes = [i64, ci, ci, vp]
    L.ah_plan.argtypes = [i64, ci, ci, ci, ci, i64, ci, cf, u32, ci, ci, vp, vp, vp, ctypes.c_char_p]
    L.ah_texels.argtypes = [i64, ci, ci, i64, vp, vp, vp, vp, vp, vp]
    L.ah_bake.argtypes = [ctypes.c_char_p, vp, i64, ci, ci, i64, vp, vp, vp, cf, u32, vp, vp, vp, vp]
    return L


FIELDS = ("triangles", "quads", "tile", "width", "height", "tiles_per_row", "rows")


def _layout(fn, triangles, tile, width):
    out = np.zeros(7, np.int64)
    return dict(zip(FIELDS, out.tolist())) if fn(triangles, tile, width, qu._p(out)) == 0 else None


def oracle_layout(triangles, tile, width):
    return _layout(oracle_lib().ao_layout, triangles, tile, width)


def host_layout(triangles, tile, width):
    return _layout(host_lib().ah_layout, triangles, tile, width)


def oracle_uvs(triangles, tile, width):
    uvs = np.full((triangles, 3, 2), np.nan, np.float32)
    assert oracle_lib().ao_uvs(triangles, tile, width, qu._p(uvs)) == 0
    return uvs


def host_uvs(triangles, tile, width):
    uvs = np.full((triangles, 3, 2), np.nan, np.float32)
    assert host_lib().ah_uvs(triangles, tile, width, qu._p(uvs)) == 0
    return uvs


def _mesh(pos, nrm, idx):
    return np.ascontiguousarray(pos, np.float32).reshape(-1, 3), np.ascontiguousarray(nrm, np.float32).reshape(-1, 3), np.ascontiguousarray(idx, np.uint32).reshape(-1, 3)


def _texels(fn, pos, nrm, idx, tile, width, vertex_count):
    pos, nrm, idx = _mesh(pos, nrm, idx)
    lay = oracle_layout(len(idx), tile, width)
    h, w = lay["height"], lay["width"]
    P, N, valid = np.full((h, w, 3), np.nan, np.float32), np.full((h, w, 3), np.nan, np.float32), np.full((h, w), 77, np.int32)
    assert fn(len(idx), tile, width, len(pos) if vertex_count is None else vertex_count, qu._p(pos), qu._p(nrm), qu._p(idx), qu._p(P), qu._p(N), qu._p(valid)) == 0
    return P, N, valid


def oracle_texels(pos, nrm, idx, tile, width, vertex_count=None):
    """(P [H, W, 3], N [H, W, 3], valid [H, W]) of the definition"""
    return _texels(oracle_lib().ao_texels, pos, nrm, idx, tile, width, vertex_count)


def host_texels(pos, nrm, idx, tile, width, vertex_count=None):
    return _texels(host_lib().ah_texels, pos, nrm, idx, tile, width, vertex_count)


def oracle_bake(scene, of, pos, nrm, idx, tile, width, reach, layers=ALBEDO | NORMAL | LIT, vertex_count=None):
    """The planes of sdfr_atlas_bake from the definition: the oracle's texels, and for those with valid = 1 the oracle's surface and
    lighting records of the item (P, N, reach).  -> {"albedo", "normal", "lit": [H, W, 4] uint32 words, "valid": [H, W] int32, "tile":
    [H, W] bool, the texels of well-formed tiles}; all three planes whatever `layers` (which only saves the lighting oracle's time)."""
    P, N, state = oracle_texels(pos, nrm, idx, tile, width, vertex_count)
    h, w = state.shape
    out = {k: np.zeros((h, w, 4), np.uint32) for k in ("albedo", "normal", "lit")}
    valid = state.copy()
    live = state == 1
    if live.any():
        _hits, srf = su.oracle_mesh(scene, of, P[live], N[live], reach)
        hit = srf[:, 3] == 1
        lit_material = (srf[:, 1] & 2) != 0
        albedo = np.zeros((len(srf), 4), np.uint32)
        albedo[:, :3] = np.where(lit_material[:, None], srf[:, 4:7], srf[:, 16:19])
        albedo[:, 3] = srf[:, 7]
        normal = np.zeros((len(srf), 4), np.uint32)
        normal[:, :3] = srf[:, 28:31]
        albedo[~hit] = 0
        normal[~hit] = 0
        out["albedo"][live], out["normal"][live] = albedo, normal
        valid[live] = srf[:, 3].view(np.int32)
        if layers & LIT:
            _h, g, _s = lu.oracle_mesh(scene, of, P[live], N[live], reach, lights=False)
            assert np.array_equal(g[:, 0], srf[:, 3])
            lit = np.zeros((len(g), 4), np.uint32)
            lit[:, :3] = g[:, 12:15]
            lit[:, 3] = ONE
            lit[~hit] = 0
            out["lit"][live] = lit
    out["valid"] = valid
    out["tile"] = state != -1
    return out


def host_bake(scene, U, pos, nrm, idx, tile, width, reach, layers=ALBEDO | NORMAL | LIT, vertex_count=None):
    pos, nrm, idx = _mesh(pos, nrm, idx)
    lay = oracle_layout(len(idx), tile, width)
    h, w = lay["height"], lay["width"]
    planes = {k: np.full((h, w, 4), 0xdeadbeef, np.uint32) if layers & bit else None for bit, k in LAYER_NAMES.items()}
    valid = np.full((h, w), 77, np.int32)
    ptr = lambda a: qu._p(a) if a is not None else None  # noqa: E731
    assert host_lib(scene).ah_bake(scene.encode(), ctypes.byref(U), len(idx), tile, width, len(pos) if vertex_count is None else vertex_count, qu._p(pos),
                                   qu._p(nrm), qu._p(idx), reach, layers, ptr(planes["albedo"]), ptr(planes["normal"]), ptr(planes["lit"]), qu._p(valid)) == 0
    planes["valid"] = valid
    return planes


def assert_bake(what, got, want, layers=ALBEDO | NORMAL | LIT):
    """the requested planes and valid, bit for bit"""
    assert np.array_equal(np.asarray(got["valid"]).astype(np.int32), want["valid"]), what + ": valid"
    for bit, k in LAYER_NAMES.items():
        if layers & bit:
            g = np.ascontiguousarray(got[k]).view(np.uint32).reshape(-1, 4)
            qu.assert_same("%s: %s" % (what, k), g, want[k].reshape(-1, 4))


def assert_condition(want):
    """the oracle's own output reaches the surface: valid == 1 on at least 99 % of the texels of well-formed tiles (without this a
    comparison could pass on planes of zeros)"""
    tiles = want["tile"]
    assert tiles.sum() > 0 and (want["valid"][tiles] == 1).mean() >= 0.99, ((want["valid"][tiles] == 1).mean(), int(tiles.sum()))


@functools.lru_cache(None)
def mesh(scene):
    """(frame, positions, normals, indices, cell) as tests/test_lighting_cpu.py::test_mesh_vertices makes them"""
    stime, origin, cell, dims = MESHES[scene]
    of = qu.frame(scene, stime, W, H)
    D = qu.oracle_points(scene, of, mu.lattice_points(origin, cell, dims), normals=False)[0]
    pos, idx = mu.host_extract(D, origin, cell, dims, 0.0)
    _d, nrm = qu.oracle_points(scene, of, pos)
    return of, pos, nrm, np.ascontiguousarray(idx, np.uint32), cell


def handmade():
    """Three quads of the fast_sphere mesh on twelve vertices of their own, then damaged.  Quad 0: normals n0 = n2 = 0 and n3 = -n1, so M
    is (u - v) n1 -- 0 on the diagonal, n1's direction above it --, and q3's position NaN, so every texel below the diagonal is
    degenerate.  Quad 1: its second triangle does not start at q0.  Quad 2: one index == vertex_count.  -> positions, normals, indices"""
    _of, pos, nrm, idx, _cell = mesh("fast_sphere")
    P, N, I = [], [], []
    for q in range(3):
        quad = [idx[2 * q][0], idx[2 * q][1], idx[2 * q][2], idx[2 * q + 1][2]]
        P += [pos[i] for i in quad]
        N += [nrm[i] for i in quad]
        b = 4 * q
        I += [[b, b + 1, b + 2], [b, b + 2, b + 3]]
    P, N, I = np.array(P, np.float32), np.array(N, np.float32), np.array(I, np.uint32)
    N[0] = N[2] = 0.0
    N[3] = -N[1]
    P[3, 0] = np.nan
    I[3, 0] = 5
    I[4, 1] = 12
    return P, N, I


@functools.lru_cache(None)
def reference(scene, tile, width, reach_key, extension_lights=0):
    """the oracle's bake of a test mesh, computed once and shared; reach_key: "2cell" or a number"""
    of, pos, nrm, idx, cell = mesh(scene)
    of = frame_with(scene, extension_lights)
    reach = 2 * cell if reach_key == "2cell" else float(reach_key)
    return oracle_bake(scene, of, pos, nrm, idx, tile, width, reach), reach


def frame_with(scene, extension_lights=0):
    of = qu.frame(scene, MESHES[scene][0], W, H)
    of.extension_lights = extension_lights
    return of

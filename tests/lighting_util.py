"""Shared by the lighting tests (test_lighting_cpu.py, test_gpu_lighting.py): the oracle's definition of the lighting records
(tests/cpp/lighting_oracle.h), the library's lighting functions built for the CPU (tests/cpp/lighting_host.cpp), the conditions
under which `lit` is the renderer's pixel, and the sums recomputed from the light samples.  Frames, samples and the bit comparison
are query_util's, the mesh rays surface_util's.  Test infrastructure: the product never imports this."""
import ctypes

import numpy as np

import query_util as qu
import surface_util as su

HIT_WORDS = qu.HIT_WORDS
LIGHTING_WORDS = 16
SAMPLE_WORDS = 20
SLOTS = 8
UNUSED, NO_CHAIN, BLOCKED, ESCAPED = 0, 1, 2, 3


def oracle_lib():
    L = qu.build_oracle_lib()
    vp = ctypes.c_void_p
    L.lo_rays.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, vp, vp, ctypes.c_float, vp, vp, vp]
    L.lo_pick.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, vp, vp, vp, vp]
    return L


def host_lib(scene):
    """The library's lighting functions for the CPU"""
    L = qu.build_host_lib("lighting_host", "lighting_host.cpp", scene)
    vp = ctypes.c_void_p
    L.lh_rays.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_float, vp, vp, vp]
    L.lh_pick.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    return L


def _out(n, lights=True):
    """(hits [n, 12], lighting [n, 16], light samples [n, 8, 20] or None) as uint32 words, filled with a pattern nothing writes"""
    return (np.full((n, HIT_WORDS), 0xdeadbeef, np.uint32), np.full((n, LIGHTING_WORDS), 0xdeadbeef, np.uint32),
            np.full((n, SLOTS, SAMPLE_WORDS), 0xdeadbeef, np.uint32) if lights else None)


def _pl(a):
    return qu._p(a) if a is not None else None


def oracle_rays(scene, of, origins, dirs, max_distance=0.0, lights=True):
    o, d = np.ascontiguousarray(origins, np.float32), np.ascontiguousarray(dirs, np.float32)
    h, g, s = _out(len(o), lights)
    assert oracle_lib().lo_rays(scene.encode(), ctypes.byref(of), len(o), qu._p(o), qu._p(d), max_distance, qu._p(h), qu._p(g), _pl(s)) == 0
    return h, g, s


def oracle_pick(scene, of, pixels, lights=True):
    px = np.ascontiguousarray(pixels, np.int32)
    h, g, s = _out(len(px), lights)
    assert oracle_lib().lo_pick(scene.encode(), ctypes.byref(of), len(px), qu._p(px), qu._p(h), qu._p(g), _pl(s)) == 0
    return h, g, s


def oracle_mesh(scene, of, positions, normals, reach, lights=True):
    o, d, reach2 = su.mesh_rays(positions, normals, reach)
    return oracle_rays(scene, of, o, d, reach2, lights)


def host_rays(scene, U, origins, dirs, max_distance=0.0, lights=True):
    o, d = np.ascontiguousarray(origins, np.float32), np.ascontiguousarray(dirs, np.float32)
    h, g, s = _out(len(o), lights)
    assert host_lib(scene).lh_rays(scene.encode(), ctypes.byref(U), 0, len(o), qu._p(o), qu._p(d), max_distance, qu._p(h), qu._p(g), _pl(s)) == 0
    return h, g, s


def host_mesh(scene, U, positions, normals, reach, lights=True):
    p, n = np.ascontiguousarray(positions, np.float32), np.ascontiguousarray(normals, np.float32)
    h, g, s = _out(len(p), lights)
    assert host_lib(scene).lh_rays(scene.encode(), ctypes.byref(U), 1, len(p), qu._p(p), qu._p(n), reach, qu._p(h), qu._p(g), _pl(s)) == 0
    return h, g, s


def host_pick(scene, U, width, height, pixels, lights=True):
    px = np.ascontiguousarray(pixels, np.int32)
    h, g, s = _out(len(px), lights)
    assert host_lib(scene).lh_pick(scene.encode(), ctypes.byref(U), width, height, len(px), qu._p(px), qu._p(h), qu._p(g), _pl(s)) == 0
    return h, g, s


def lighting_array(g):
    """LIGHTING_DTYPE records, a device tensor's copy or [n, 16] 32-bit words -> [n, 16] uint32"""
    return np.ascontiguousarray(g).view(np.uint32).reshape(-1, LIGHTING_WORDS)


def samples_array(s):
    """LIGHT_SAMPLE_DTYPE records [n, 8], a device tensor's copy [n, 160] or words -> [n, 8, 20] uint32"""
    return np.ascontiguousarray(s).view(np.uint32).reshape(-1, SLOTS, SAMPLE_WORDS)


def assert_same(what, got, want):
    """(hits, lighting, samples) triples; a None on either side is not compared"""
    for name, conv, a, b in (("hits", qu.hits_array, got[0], want[0]), ("lighting", lighting_array, got[1], want[1]),
                             ("light samples", lambda s: samples_array(s).reshape(-1, SLOTS * SAMPLE_WORDS), got[2], want[2])):
        if a is not None and b is not None:
            qu.assert_same("%s: %s" % (what, name), conv(a), conv(b))


def f32(words):
    return np.ascontiguousarray(words).view(np.float32)


def popcount(m):
    return np.array([bin(int(v)).count("1") for v in m], np.int64)


def well_formed(hits, g, s, light_count):
    """what the records promise whatever the scene"""
    valid = g[:, 0].view(np.int32)
    assert np.array_equal(valid, hits[:, 10].view(np.int32))
    assert not g[valid != 1][:, 1:].any() and not g[:, 15].any()
    used, traced, visible = g[:, 1], g[:, 2], g[:, 3]
    assert not (visible & ~traced).any() and not (traced & ~used).any()
    assert not (used >> np.uint32(max(light_count, 0))).any() if light_count < 32 else True
    if s is None:
        return
    state = s[:, :, 0].view(np.int32)
    assert ((state >= 0) & (state <= 3)).all()
    assert not s[valid != 1].any() and not s[state == UNUSED].any() and not s[:, :, [3, 19]].any()
    bit = np.uint32(1) << np.arange(SLOTS, dtype=np.uint32)[None, :]
    assert np.array_equal((used[:, None] & bit) != 0, state != UNUSED)
    assert np.array_equal((traced[:, None] & bit) != 0, state >= BLOCKED)
    assert np.array_equal((visible[:, None] & bit) != 0, state == ESCAPED)
    assert not s[state != ESCAPED][:, 16:19].any()
    assert np.array_equal(s[:, :, 2].sum(1, dtype=np.uint32), g[:, 11])
    assert ((s[:, :, 2] >= 1) == (state >= BLOCKED)).all()
    # direct and lit from the delivered light in slot order, fp32
    own, delivered = f32(g[:, 4:7]), f32(s[:, :, 16:19])
    direct = np.zeros_like(own)
    lit = (np.float32(0.0) + own).astype(np.float32)
    with np.errstate(all="ignore"):
        for i in range(SLOTS):
            esc = (state[:, i] == ESCAPED)[:, None]
            direct = np.where(esc, (direct + delivered[:, i]).astype(np.float32), direct)
            lit = np.where(esc, (lit + delivered[:, i]).astype(np.float32), lit)
    hit = valid == 1
    qu.assert_same("direct from delivered", direct[hit], f32(g[:, 8:11])[hit])
    qu.assert_same("lit from delivered", lit[hit], f32(g[:, 12:15])[hit])


def spawns_nothing_else(surfaces, g):
    """Per item: a hit whose primary ray spawns nothing but shadow rays in the driver: no reflection, no refraction, no continuation
    through a see-through hit (which the driver starts before it looks at use_light).  surfaces: the [n, 32] surface records."""
    valid = g[:, 0].view(np.int32) == 1
    max_cost = surfaces[:, 2].astype(np.int64)
    reflects = f32(surfaces[:, 20:23]).astype(bool).any(1) & (3 < max_cost)
    refracts = f32(surfaces[:, 24:27]).astype(bool).any(1) & (4 < max_cost)
    see_through = (f32(surfaces[:, 7]) < 1) & (2 < max_cost)
    return valid & ~reflects & ~refracts & ~see_through


def pixel_conditions(surfaces, g, bounce_count, ray_count):
    """Per item: whether sdfr_lighting.lit is the renderer's pixel (include/sdfr.h): nothing else spawned, chains of one segment each,
    and the driver's budgets not reached"""
    traced = popcount(g[:, 2])
    one_segment = g[:, 11].astype(np.int64) == traced
    budget = (1 + traced <= bounce_count) & (1 + traced <= ray_count)
    return spawns_nothing_else(surfaces, g) & one_segment & budget


# ---- the cases the CPU and the GPU tier share --------------------------------------------------------------------------------------
W, H = 64, 48
# the meshes of tests/test_gpu_surface.py: stime, origin, cell, dims
MESHES = {"fast_sphere": (0.0, (-1.55, -0.3, -1.55), 0.13, (24, 23, 25)), "debug_materials": (0.4, (-2.05, -0.3, -1.55), 0.17, (24, 23, 25))}


def frame_limits(of):
    """the limits the lighting and atlas tests move, as the oracle frame `of` has them: gpu_util.setup's `limits`"""
    return dict(light_count=of.light_count, max_cost_default=of.max_cost_default, extension_lights=of.extension_lights,
                extension_marble_reflection=of.extension_marble_reflection)


# the frames on which `lit` is pinned against the driver itself (orc::ps_main's rgb on the CPU, the renderer's pixel on the GPU):
# scene, stime, frame changes, camera (eye, look-at; None: the start-up camera) -- chosen on the oracle alone.  With all seven extension
# lights a lit hit starts eight chains, one more than the driver's eight ray slots leave room for beside the primary ray: six here.
PIXEL_FRAMES = {
    "basic_transparency": ("basic_transparency", 0.5, {}, ((-5.0, 6.0, 2.0), (0.0, 0.0, 0.0))),
    "light_shadows": ("light_shadows", 0.5, {}, None),
    "gems, extension lights": ("gems", 0.5, {"extension_lights": 6}, None),
    "labyrinth, extension lights": ("labyrinth", 0.5, {"extension_lights": 3}, None),
}


def pixel_frame(key):
    scene, stime, changes, camera = PIXEL_FRAMES[key]
    of = qu.frame(scene, stime, W, H)
    if camera:
        fovy = np.float32(60.0) * np.float32(3.14159265358979) / np.float32(180.0)
        basis = qu.po.camera_lookat(camera[0], camera[1], fovy, np.float32(W) / np.float32(H))
        for i in range(3):
            of.eye[i], of.front[i], of.right[i], of.top[i] = basis[0][i], basis[1][i], basis[2][i], basis[3][i]
    for k, v in changes.items():
        setattr(of, k, v)
    return scene, of


def pixel_classes(scene, of, g, srf):
    """(qualifies: the three conditions of include/sdfr.h; single: one chain of any length within the bounce budget, which the driver
    sums in the same order whatever its length; lit hits)"""
    ok = pixel_conditions(srf, g, of.bounce_count, of.ray_count)
    lit_hits = (g[:, 0] == 1) & ((srf[:, 1] & 2) != 0)
    # the header's wording of the see-through condition and the driver's coincide on these frames: no unlit see-through hit
    assert not ((srf[:, 3] == 1) & ((srf[:, 1] & 2) == 0) & (f32(srf[:, 7]) < 1)).any()
    single = spawns_nothing_else(srf, g) & (popcount(g[:, 2]) == 1) & (1 + g[:, 11].astype(np.int64) <= of.bounce_count)
    return ok, single, lit_hits

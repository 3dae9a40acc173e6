"""GPU tier of the lighting queries (sdfr_query_ray_lighting, sdfr_pick_lighting, sdfr_mesh_lighting) through libsdfr.so: bit for
bit against the oracle's definition of the records (tests/cpp/lighting_oracle.h) for every scene compiled ahead of time and the
run-time scenes with an oracle twin, host and device memory; their hit records against the ray query's and the pick's; the whole
frame (no pixel list, 8 x 8 tiles) against the pixel list; step shortcuts on against off; small and awkward sizes, the word-store
path, with and without the light samples, argument checks; no side effects on rendering; one handle across scene changes; the mesh
with lighting; and the renderer's own pixels where `lit` is defined to be the pixel."""
import ctypes
import zlib

import numpy as np
import pytest

import gpu_util as gu
import lighting_util as lu
import query_util as qu
import surface_util as su
from gpu_util import DEFAULT_LIMITS
from gpu_util import renderer  # noqa: F401
from lighting_util import MESHES, PIXEL_FRAMES, pixel_classes, pixel_frame

pytestmark = pytest.mark.gpu

N_RAYS = 2000
W, H = 64, 48
FW, FH = 61, 45  # the whole frame: ragged 8 x 8 tiles on both edges


def _setup(r, scene, of, variables=None, shortcuts=False):
    """the handle's state = the oracle frame `of`, with the four limits the tests move taken from it"""
    gu.setup(r, scene, of, variables, lu.frame_limits(of), shortcuts)


def _frame_oracle(scene, of, w, h):
    with gu.with_size(of, w, h):
        return lu.oracle_pick(scene, of, su.frame_pixels(w, h))


def _check_all(r, scene, of, seed, device=True, n_rays=N_RAYS):
    o, dirs = qu.ray_samples(of, seed + 7, n_rays)
    px = qu.pick_grid(W, H)
    ray_ref, pick_ref, frame_ref = lu.oracle_rays(scene, of, o, dirs), lu.oracle_pick(scene, of, px), _frame_oracle(scene, of, FW, FH)
    rays = r.queryRayLighting(o, dirs, hits=True, lights=True)
    picks = r.pickLighting(px, W, H, hits=True, lights=True)
    frame = r.pickLighting(None, FW, FH, hits=True, lights=True)
    lu.assert_same("%s rays (host)" % scene, rays, ray_ref)
    lu.assert_same("%s pick (host)" % scene, picks, pick_ref)
    lu.assert_same("%s frame (host)" % scene, frame, frame_ref)
    # the hit records are the ray query's and the pick's
    qu.assert_same("%s hits against sdfr_query_rays" % scene, qu.hits_array(rays[0]), qu.hits_array(r.queryRays(o, dirs)))
    qu.assert_same("%s hits against sdfr_pick" % scene, qu.hits_array(picks[0]), qu.hits_array(r.pick(px, W, H)))
    # hits = NULL, lights = NULL: the same lighting
    qu.assert_same("%s rays, hits = lights = NULL" % scene, lu.lighting_array(r.queryRayLighting(o, dirs)), ray_ref[1])
    qu.assert_same("%s frame, lights = NULL" % scene, lu.lighting_array(r.pickLighting(None, FW, FH, hits=True)[1]), frame_ref[1])
    # step shortcuts: every lighting record and sample the same (misses end early: their hit records may differ)
    r.setStepShortcuts(True)
    lu.assert_same("%s rays, shortcuts" % scene, (None,) + r.queryRayLighting(o, dirs, lights=True), ray_ref)
    lu.assert_same("%s frame, shortcuts" % scene, (None,) + r.pickLighting(None, FW, FH, lights=True), frame_ref)
    r.setStepShortcuts(False)
    if device:
        lu.assert_same("%s rays (device)" % scene, gu.to_host(r.queryRayLighting(gu.to_device(o), gu.to_device(dirs), hits=True, lights=True)), ray_ref)
        lu.assert_same("%s pick (device)" % scene, gu.to_host(r.pickLighting(gu.to_device(px), W, H, hits=True, lights=True)), pick_ref)
        lu.assert_same("%s frame (device)" % scene, gu.to_host(r.pickLighting(None, FW, FH, hits=True, lights=True, device=True)), frame_ref)
    return ray_ref, pick_ref


@pytest.mark.parametrize("scene", qu.BUILTIN + qu.HLSL)
def test_lighting_equals_oracle(renderer, scene):
    of = qu.frame(scene, 1.25 if scene in qu.BUILTIN else 0.5, W, H)
    _setup(renderer, scene, of)
    _check_all(renderer, scene, of, seed=zlib.crc32(scene.encode()) & 0xffff)


@pytest.mark.parametrize("scene", ["lense", "tiling"])
def test_lighting_with_moved_variables(renderer, scene):
    of = qu.frame(scene, 0.5, W, H, qu.MOVED_VARS[scene])
    _setup(renderer, scene, of, qu.MOVED_VARS[scene])
    _check_all(renderer, scene, of, seed=11, device=False, n_rays=600)
    renderer.resetVariables()


@pytest.mark.parametrize("what", ["light_count 0", "light_count 1", "extension_lights 7", "max_cost_default 2", "marble extension", "debug plane"])
def test_limits_and_extensions(renderer, what):
    scene, variables = {"extension_lights 7": "gems", "max_cost_default 2": "light_shadows"}.get(what, "labyrinth"), None
    if what == "debug plane":
        variables = {"debug_nx": 0.3, "debug_ny": 1.0, "debug_y": 0.4}
    of = qu.frame(scene, 0.5, W, H, variables)
    if what.startswith("light_count"):
        of.light_count = int(what.split()[1])
    elif what == "extension_lights 7":
        of.extension_lights = 7
    elif what == "max_cost_default 2":
        of.max_cost_default = 2
    elif what == "marble extension":
        of.extension_marble_reflection = 0.25
    _setup(renderer, scene, of, variables)
    _rays, (ph, pg, ps) = _check_all(renderer, scene, of, seed=31, device=False, n_rays=600)
    if what == "extension_lights 7":
        assert (lu.popcount(pg[:, 2]) == 8).any()  # eight chains from one lane
    if what == "max_cost_default 2":
        assert (pg[:, 1] != 0).any() and not pg[:, 2].any()
    renderer.resetVariables()
    renderer.setLimits(**DEFAULT_LIMITS)


def test_whole_frame_equals_the_pixel_list(renderer):
    scene = "light_shadows"
    _setup(renderer, scene, qu.frame(scene, 0.6, W, H))
    for w, h in ((FW, FH), (1, 1), (9, 1), (8, 8), (3, 17)):
        listed = renderer.pickLighting(su.frame_pixels(w, h), w, h, hits=True, lights=True)
        assert len(listed[1]) == w * h
        lu.assert_same("%d x %d" % (w, h), renderer.pickLighting(None, w, h, hits=True, lights=True), listed)
        lu.assert_same("%d x %d (device)" % (w, h), gu.to_host(renderer.pickLighting(None, w, h, hits=True, lights=True, device=True)), listed)


@pytest.mark.parametrize("scene", sorted(MESHES))
def test_mesh_with_lighting(renderer, scene):
    import sdf_playground_amd as sp

    stime, origin, cell, dims = MESHES[scene]
    of = qu.frame(scene, stime, W, H)
    _setup(renderer, scene, of)
    pos, nrm, idx, lit = renderer.extractMesh(origin, cell, dims, lighting=True)
    plain = renderer.extractMesh(origin, cell, dims)
    for a, b in zip((pos, nrm, idx), plain):  # the mesh itself is sdfr_mesh_extract's
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert len(pos) > 500 and lit.dtype == sp.LIGHTING_DTYPE
    reach = 2.0 * cell
    ref = lu.oracle_mesh(scene, of, pos, nrm, reach)
    mesh = renderer.meshLighting(pos, nrm, reach, hits=True, lights=True)
    lu.assert_same("%s meshLighting (host)" % scene, mesh, ref)
    qu.assert_same("%s extractMesh(lighting=True) against meshLighting on its arrays" % scene, lu.lighting_array(lit), lu.lighting_array(mesh[1]))
    o, d, reach2 = su.mesh_rays(pos, nrm, reach)
    qu.assert_same("%s mesh hits against sdfr_query_rays" % scene, qu.hits_array(mesh[0]), qu.hits_array(renderer.queryRays(o, d, reach2)))
    # with the surfaces and the occlusion: the lighting is the last element; another reach, on the device
    out = renderer.extractMesh(origin, cell, dims, surfaces=True, occlusion=True, lighting=True, reach=0.2, device=True)
    assert len(out) == 6
    (dlit,) = gu.to_host((out[-1],))
    qu.assert_same("%s mesh lighting, reach 0.2 (device)" % scene, lu.lighting_array(dlit), lu.oracle_mesh(scene, of, pos, nrm, 0.2)[1])


def test_small_and_awkward_sizes(renderer):
    import torch

    scene = "light_shadows"
    of = qu.frame(scene, 0.3, W, H)
    _setup(renderer, scene, of)
    L, h = gu.raw(renderer)
    o, dirs = qu.ray_samples(of, 5, 65)
    ref = lu.oracle_rays(scene, of, o, dirs)
    assert (ref[1][:, 2] != 0).any()
    for n in (0, 1, 63, 64, 65):
        want = tuple(a[:n] for a in ref)
        lu.assert_same("n = %d" % n, renderer.queryRayLighting(o[:n], dirs[:n], hits=True, lights=True), want)
        dev = gu.to_host(renderer.queryRayLighting(gu.to_device(o[:n].reshape(-1, 3)), gu.to_device(dirs[:n].reshape(-1, 3)), hits=True, lights=True))
        lu.assert_same("n = %d (device)" % n, dev, want)
    # records that start 4 bytes past a 16-byte boundary: the word stores; the words around them stay
    n = 65
    sentinel = 0x7fc12345
    bufs = [torch.full((words * n + 8,), sentinel, dtype=torch.int32, device="cuda") for words in (12, 16, 160)]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    do, dd = gu.to_device(o), gu.to_device(dirs)
    vp = ctypes.c_void_p
    assert L.sdfr_query_ray_lighting(h, n, vp(do.data_ptr()), vp(dd.data_ptr()), 0.0, *[vp(b.data_ptr() + 4) for b in bufs], 0) == 0
    renderer.sync()
    for what, b, words, want in zip(("hits", "lighting", "lights"), bufs, (12, 16, 160), ref):
        a = b.cpu().numpy().view(np.uint32)
        qu.assert_same("offset " + what, a[1:1 + words * n].reshape(n, words), want.reshape(n, words))
        assert a[0] == sentinel and (a[1 + words * n:] == sentinel).all()
    # a pixel outside the frame: valid = -1 and zeros
    hits, g, s = renderer.pickLighting(np.array([[-1, 0], [W, 0], [0, H], [3, 4]], np.int32), W, H, hits=True, lights=True)
    assert list(g["valid"][:3]) == [-1, -1, -1] and list(hits["hit"][:3]) == [-1, -1, -1] and g["valid"][3] in (0, 1)
    assert not lu.lighting_array(g)[:3, 1:].any() and not lu.samples_array(s)[:3].any()


def test_arguments(renderer):
    import sdf_playground_amd as sp

    scene = "fast_sphere"
    _setup(renderer, scene, qu.frame(scene, 0.0, W, H))
    L, h = gu.raw(renderer)
    buf = np.zeros(64, np.float32)
    out, hit, smp = np.full(W * H * 16, 7, np.uint32), np.full(W * H * 12, 7, np.uint32), np.full(W * H * 160, 7, np.uint32)  # what no call below may touch
    p, g, hp, sp_ = (a.ctypes.data_as(ctypes.c_void_p) for a in (buf, out, hit, smp))
    INVALID, NO_SCENE = -1, -4
    assert L.sdfr_query_ray_lighting(h, 0, None, None, 0.0, None, None, None, 1) == 0
    assert L.sdfr_pick_lighting(h, W, H, 0, None, None, None, None, 0) == 0
    assert L.sdfr_mesh_lighting(h, 0, None, None, 0.5, None, None, None, 1) == 0
    # NULL lighting, NULL inputs
    assert L.sdfr_query_ray_lighting(h, 1, p, p, 0.0, hp, None, sp_, 1) == INVALID
    assert L.sdfr_pick_lighting(h, W, H, 1, p, hp, None, sp_, 1) == INVALID
    assert L.sdfr_pick_lighting(h, W, H, W * H, None, hp, None, sp_, 1) == INVALID
    assert L.sdfr_mesh_lighting(h, 1, p, p, 0.5, hp, None, sp_, 1) == INVALID
    assert L.sdfr_query_ray_lighting(h, 1, p, None, 0.0, hp, g, sp_, 1) == INVALID
    assert L.sdfr_mesh_lighting(h, 1, None, p, 0.5, hp, g, sp_, 1) == INVALID
    # the whole frame: n must be width * height
    for n in (1, W * H - 1, W * H + 1):
        assert L.sdfr_pick_lighting(h, W, H, n, None, hp, g, sp_, 1) == INVALID
    assert L.sdfr_pick_lighting(h, 0, H, 1, p, hp, g, sp_, 1) == INVALID
    # reach, max_distance
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert L.sdfr_mesh_lighting(h, 1, p, p, bad, hp, g, sp_, 1) == INVALID
    for bad in (-1.0, float("inf"), float("nan")):
        assert L.sdfr_query_ray_lighting(h, 1, p, p, bad, hp, g, sp_, 1) == INVALID
    # n, on_host, the handle
    for n in (-1, 2 ** 31):
        assert L.sdfr_query_ray_lighting(h, n, p, p, 0.0, hp, g, sp_, 1) == INVALID
        assert L.sdfr_pick_lighting(h, W, H, n, p, hp, g, sp_, 1) == INVALID
        assert L.sdfr_mesh_lighting(h, n, p, p, 0.5, hp, g, sp_, 1) == INVALID
    for bad in (2, -1):
        assert L.sdfr_query_ray_lighting(h, 1, p, p, 0.0, hp, g, sp_, bad) == INVALID
        assert L.sdfr_pick_lighting(h, W, H, W * H, None, hp, g, sp_, bad) == INVALID
        assert L.sdfr_mesh_lighting(h, 1, p, p, 0.5, hp, g, sp_, bad) == INVALID
    assert L.sdfr_query_ray_lighting(None, 1, p, p, 0.0, hp, g, sp_, 1) == INVALID
    fresh = sp.SDFRenderer(0)
    try:
        assert L.sdfr_query_ray_lighting(fresh._h, 1, p, p, 0.0, hp, g, sp_, 1) == NO_SCENE
        assert L.sdfr_pick_lighting(fresh._h, W, H, W * H, None, hp, g, sp_, 1) == NO_SCENE
        assert L.sdfr_mesh_lighting(fresh._h, 1, p, p, 0.5, hp, g, sp_, 1) == NO_SCENE
    finally:
        fresh.close()
    assert (out == 7).all() and (hit == 7).all() and (smp == 7).all()
    # and the same buffers are written by a good call
    assert L.sdfr_pick_lighting(h, W, H, W * H, None, hp, g, sp_, 1) == 0
    assert set(out.reshape(-1, 16)[:, 0]) <= {0, 1} and set(hit.reshape(-1, 12)[:, 10]) <= {0, 1} and set(smp.reshape(-1, 20)[:, 0]) <= {0, 1, 2, 3}


def test_lighting_queries_leave_rendering_alone(renderer):
    scene = "labyrinth"
    of = qu.frame(scene, 0.4, 96, 64)
    _setup(renderer, scene, of)
    o, dirs = qu.ray_samples(of, 71, 500)
    with gu.rendering_untouched(renderer, 96, 64):
        renderer.queryRayLighting(o, dirs, hits=True, lights=True)
        renderer.pickLighting(qu.pick_grid(32, 16), 32, 16)
        renderer.pickLighting(None, 33, 17, hits=True)
        renderer.meshLighting(o, dirs, 0.25, lights=True)
        renderer.extractMesh((-5.35, -0.3, -2.55), 0.25, (5, 4, 3), lighting=True)


def test_one_handle_across_scene_changes():
    # built-in scene -> run-time scene (its lazily compiled query module has the lighting kernel) -> the same built-in scene
    import sdf_playground_amd as sp

    n, w, h = 130, 24, 17
    r = sp.SDFRenderer(0)
    try:
        rounds = []
        for scene in ("labyrinth", qu.HLSL[0], "labyrinth"):
            of = qu.frame(scene, 0.5, W, H)
            _setup(r, scene, of)
            o, dirs = qu.ray_samples(of, 92, n)
            refs = (lu.oracle_rays(scene, of, o, dirs), _frame_oracle(scene, of, w, h), lu.oracle_mesh(scene, of, o, dirs, 0.3))
            got = [r.queryRayLighting(o, dirs, hits=True, lights=True), r.pickLighting(None, w, h, hits=True, lights=True),
                   r.meshLighting(o, dirs, 0.3, hits=True, lights=True)]
            for what, g, want in zip(("rays", "frame", "mesh"), got, refs):
                lu.assert_same("%s %s" % (scene, what), g, want)
            rounds.append(got)
        for a, b in zip(rounds[0], rounds[2]):
            lu.assert_same("first and third round", a, b)
    finally:
        r.close()


@pytest.mark.parametrize("key", sorted(PIXEL_FRAMES))
def test_lit_is_the_renderer_s_pixel(renderer, key):
    # the frames and the caps of the CPU test, which checks the same classes against the oracle's driver
    scene, of = pixel_frame(key)
    _setup(renderer, scene, of)
    img, st = renderer.render(None, W, H, pixel_stats=True)
    _h, g, s = (f(a) for f, a in zip((qu.hits_array, lu.lighting_array, lu.samples_array), renderer.pickLighting(None, W, H, hits=True, lights=True)))
    srf = su.surfaces_array(renderer.pickSurfaces(None, W, H))
    img = img.reshape(-1, 4)
    ok, single, lit_hits = pixel_classes(scene, of, g, srf)
    assert lit_hits.sum() > 200 and ok.sum() >= 0.5 * lit_hits.sum(), (int(ok.sum()), int(lit_hits.sum()))
    qu.assert_same("%s: lit against the rendered pixels" % key, lu.f32(g[:, 12:15])[ok], np.ascontiguousarray(img[ok, :3]))
    qu.assert_same("%s: lit against the rendered pixels, single chains" % key, lu.f32(g[:, 12:15])[single], np.ascontiguousarray(img[single, :3]))
    # the renderer traced what the record says: the primary ray and one ray per chain
    rays = st.reshape(-1, 3)[:, 0].astype(np.int64)
    assert np.array_equal(rays[ok], 1 + lu.popcount(g[ok, 2]))
    if key == "basic_transparency":
        assert (single & (g[:, 11] >= 2) & (g[:, 3] != 0)).any()
    else:
        assert (ok & (g[:, 3] != g[:, 2])).any() and (ok & (lu.popcount(g[:, 1]) >= 2)).any()

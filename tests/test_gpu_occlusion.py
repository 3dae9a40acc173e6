"""GPU tier of the occlusion queries (sdfr_query_occlusion, sdfr_hit_occlusion) through libsdfr.so: bit for bit against the oracle's
definition of the record (tests/cpp/occlusion_oracle.h) for every scene compiled ahead of time and two run-time scenes, host and
device memory, both entries, the hits of sdfr_pick and sdfr_pick_surfaces fed back on the device; small sizes, the word-store path
and a hit array off 16-byte alignment; the debug kernel variant; step shortcuts; a scene whose answer is known without the oracle;
the mesh with occlusion; argument checks; no side effects on rendering; one handle across scene changes; two frames in flight."""
import ctypes
import zlib

import numpy as np
import pytest

import gpu_util as gu
import occlusion_util as ou
import query_util as qu
from gpu_util import DEFAULT_LIMITS
from gpu_util import renderer  # noqa: F401

pytestmark = pytest.mark.gpu

N_ITEMS = 150
W, H = 64, 48
PW, PH = 9, 7  # the frame whose picks are fed back
BIAS, RADIUS = ou.BIAS, ou.RADIUS
# the meshes: about 24^3 cells, no axis a multiple of the lattice kernel's brick
MESHES = {"fast_sphere": (0.0, (-1.55, -0.3, -1.55), 0.13, (24, 23, 25)), "labyrinth": (0.5, (-5.35, -0.3, -2.55), 0.11, (25, 23, 24))}


def _hits_to_device(hits):
    """HIT_DTYPE records or [n, 12] words -> an [n, 12] int32 device tensor"""
    return gu.to_device(qu.hits_array(hits).view(np.int32))


def _check_all(r, scene, of, seed, device=True, n=N_ITEMS):
    hits = ou.hit_items(scene, of, seed, n)
    ref = ou.oracle_hits(scene, of, hits, BIAS, RADIUS)
    p, nr, is_item = ou.points_of_hits(hits)
    pref = ou.oracle_points(scene, of, p, nr, BIAS, RADIUS)  # (the misses' zeros as points: no answer either)
    qu.assert_same("%s hits (host)" % scene, ou.occlusion_array(r.hitOcclusion(hits, BIAS, RADIUS)), ref)
    qu.assert_same("%s points (host)" % scene, ou.occlusion_array(r.queryOcclusion(p, nr, BIAS, RADIUS)), pref)
    qu.assert_same("%s points against hits" % scene, pref[is_item], ref[is_item])
    if device:
        qu.assert_same("%s hits (device)" % scene, ou.occlusion_array(gu.to_host(r.hitOcclusion(_hits_to_device(hits), BIAS, RADIUS))), ref)
        qu.assert_same("%s points (device)" % scene, ou.occlusion_array(gu.to_host(r.queryOcclusion(gu.to_device(p), gu.to_device(nr), BIAS, RADIUS))), pref)
    ou.well_formed(ref)
    return hits, ref


def _check_picks(r, scene, of):
    """sdfr_hit_occlusion fed by sdfr_pick's and sdfr_pick_surfaces' device hits of a 9 x 7 frame, nothing leaving the device in between"""
    px = qu.pick_grid(PW, PH)  # every pixel, and a few outside the frame: hit = -1
    with gu.with_size(of, PW, PH):
        want = ou.oracle_hits(scene, of, qu.oracle_pick(scene, of, px), BIAS, RADIUS)
    picked = r.pick(gu.to_device(px), PW, PH)
    qu.assert_same("%s occlusion of sdfr_pick's hits" % scene, ou.occlusion_array(gu.to_host(r.hitOcclusion(picked, BIAS, RADIUS))), want)
    frame_hits, _srf = r.pickSurfaces(None, PW, PH, hits=True, device=True)
    qu.assert_same("%s occlusion of the G-buffer's hits" % scene, ou.occlusion_array(gu.to_host(r.hitOcclusion(frame_hits, BIAS, RADIUS))), want[:PW * PH])
    assert (want[PW * PH:, 3] == 0xffffffff).all() and not want[PW * PH:, :3].any()


@pytest.mark.parametrize("scene", qu.BUILTIN + qu.HLSL)
def test_occlusion_equals_oracle(renderer, scene):
    of = qu.frame(scene, 1.25 if scene in qu.BUILTIN else 0.5, W, H)
    gu.setup(renderer, scene, of)
    _check_all(renderer, scene, of, seed=zlib.crc32(scene.encode()) & 0xffff)
    _check_picks(renderer, scene, of)


def test_small_sizes_and_alignment(renderer):
    import torch

    scene = "labyrinth"
    of = qu.frame(scene, 0.3, W, H)
    gu.setup(renderer, scene, of)
    L, h = gu.raw(renderer)
    hits = ou.hit_items(scene, of, 5, 65)
    ref = ou.oracle_hits(scene, of, hits, BIAS, RADIUS)
    p, nr, _is = ou.points_of_hits(hits)
    pref = ou.oracle_points(scene, of, p, nr, BIAS, RADIUS)
    assert (ref[:, 2] > 0).any()
    for n in (0, 1, 2, 65):
        qu.assert_same("n = %d" % n, ou.occlusion_array(renderer.hitOcclusion(hits[:n], BIAS, RADIUS)), ref[:n])
        qu.assert_same("n = %d points" % n, ou.occlusion_array(renderer.queryOcclusion(p[:n], nr[:n], BIAS, RADIUS)), pref[:n])
        qu.assert_same("n = %d (device)" % n, ou.occlusion_array(gu.to_host(renderer.hitOcclusion(_hits_to_device(hits[:n]), BIAS, RADIUS))), ref[:n])
        dev = renderer.queryOcclusion(gu.to_device(p[:n].reshape(-1, 3)), gu.to_device(nr[:n].reshape(-1, 3)), BIAS, RADIUS)
        qu.assert_same("n = %d points (device)" % n, ou.occlusion_array(gu.to_host(dev)), pref[:n])
    # records that start 4 bytes past a 16-byte boundary: the word stores; the words around them stay.  The hits likewise off by 4 bytes
    n = 65
    sentinel = 0x7fc12345
    obuf = torch.full((4 * n + 8,), sentinel, dtype=torch.int32, device="cuda")
    hbuf = torch.zeros((12 * n + 4,), dtype=torch.int32, device="cuda")
    hbuf[1:1 + 12 * n] = _hits_to_device(hits).reshape(-1)
    assert obuf.data_ptr() % 16 == 0 and hbuf.data_ptr() % 16 == 0
    vp = ctypes.c_void_p
    assert L.sdfr_hit_occlusion(h, n, vp(hbuf.data_ptr() + 4), BIAS, RADIUS, vp(obuf.data_ptr() + 4), 0) == 0
    renderer.sync()
    o = obuf.cpu().numpy().view(np.uint32)
    qu.assert_same("offset records", o[1:1 + 4 * n].reshape(n, 4), ref)
    assert o[0] == sentinel and (o[1 + 4 * n:] == sentinel).all()
    obuf.fill_(sentinel)
    dp, dn = gu.to_device(p), gu.to_device(nr)
    assert L.sdfr_query_occlusion(h, n, vp(dp.data_ptr()), vp(dn.data_ptr()), BIAS, RADIUS, vp(obuf.data_ptr() + 4), 0) == 0
    renderer.sync()
    o = obuf.cpu().numpy().view(np.uint32)
    qu.assert_same("offset records (points)", o[1:1 + 4 * n].reshape(n, 4), pref)
    assert o[0] == sentinel and (o[1 + 4 * n:] == sentinel).all()


def test_degenerate_items(renderer):
    scene = "labyrinth"
    of = qu.frame(scene, 0.5, W, H)
    gu.setup(renderer, scene, of)
    hits = ou.hit_items(scene, of, 51, 200)
    p, _n, is_item = ou.points_of_hits(hits)
    p = p[is_item][:9].copy()
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    nr = np.array([[0, 0, 0], [nan, 1, 0], [0, 1, 0], [0, 0, -1], [0.6, 0.8, -0.0], [0, 2.5, 0], [0.3, 1.7, -0.9], [0, -0.0, 0], [0, inf, 0]], np.float32)
    p[2] = (p[2][0], inf, p[2][2])
    ref = ou.oracle_points(scene, of, p, nr, BIAS, RADIUS)
    got = renderer.queryOcclusion(p, nr, BIAS, RADIUS)
    qu.assert_same("degenerate items", ou.occlusion_array(got), ref)
    assert got["valid"].tolist() == [0, 0, 0, 1, 1, 1, 1, 0, 0]
    rec = hits[is_item][:4].copy()
    rec[1, 10], rec[2, 10], rec[3, 10] = 0, 0xffffffff, 7
    got = renderer.hitOcclusion(rec, BIAS, RADIUS)
    qu.assert_same("hit words", ou.occlusion_array(got), ou.oracle_hits(scene, of, rec, BIAS, RADIUS))
    assert got["valid"].tolist() == [1, 0, -1, -1]


def test_debug_plane(renderer):
    # the DBG kernel variant
    v = {"debug_nx": 0.3, "debug_ny": 1.0, "debug_y": 0.4}
    for scene in ("labyrinth", "dialect_tour"):
        of = qu.frame(scene, 0.75, W, H, v)
        gu.setup(renderer, scene, of, v)
        hits, ref = _check_all(renderer, scene, of, seed=21, device=False)
        assert (hits[:, 9] == 5).any() and ref[:, 2].any()  # MATERIAL_DISTANCE_PLANE among the items
        v2 = {"show_objects": 0.0, "debug_ny": 1.0}
        renderer.resetVariables()
        of = qu.frame(scene, 0.75, W, H, v2)
        gu.setup(renderer, scene, of, v2)
        _check_all(renderer, scene, of, seed=22, device=False)
        renderer.resetVariables()


@pytest.mark.parametrize("scene", ["labyrinth", "cube_sea", "tree"])
def test_step_shortcuts_do_not_change_the_mask(renderer, scene):
    of = qu.frame(scene, 0.6, W, H)
    hits = ou.hit_items(scene, of, 33, N_ITEMS)
    ref = ou.oracle_hits(scene, of, hits, BIAS, RADIUS)
    gu.setup(renderer, scene, of, shortcuts=True)
    on = ou.occlusion_array(renderer.hitOcclusion(hits, BIAS, RADIUS))
    renderer.setStepShortcuts(False)
    off = ou.occlusion_array(renderer.hitOcclusion(hits, BIAS, RADIUS))
    qu.assert_same("%s shortcuts on against off" % scene, on, off)
    qu.assert_same("%s against the oracle" % scene, on, ref)
    assert ou.partial_share(ref) >= 0.10


def test_floor_and_wall_is_known_without_the_oracle(renderer):
    import sdf_playground_amd as sp

    table = sp.occlusionDirections()
    assert np.array_equal(table.view(np.uint32), ou.host_directions().view(np.uint32))
    want, compared = ou.wall_expectation(table)
    assert want.sum() == 12 and (~compared).sum() <= 2
    renderer.initShaderHlsl("floor_and_wall", ou.FLOOR_AND_WALL)
    renderer.setLimits(**DEFAULT_LIMITS)
    renderer.setStepShortcuts(False)
    for rec in (renderer.queryOcclusion(*ou.WALL_ITEM, 0.01, 1.0), gu.to_host(renderer.queryOcclusion(gu.to_device(ou.WALL_ITEM[0]), gu.to_device(ou.WALL_ITEM[1]), 0.01, 1.0))):
        rec = ou.occlusion_array(rec)
        assert rec[0, 3] == 1
        bits = ou.mask_bits(rec)[0]
        assert np.array_equal(bits[compared], want[compared])
        assert want[compared].sum() <= rec[0, 2] <= want[compared].sum() + (~compared).sum()


@pytest.mark.parametrize("scene", sorted(MESHES))
def test_mesh_with_occlusion(renderer, scene):
    import sdf_playground_amd as sp

    stime, origin, cell, dims = MESHES[scene]
    of = qu.frame(scene, stime, W, H)
    gu.setup(renderer, scene, of)
    pos, nrm, idx, occ = renderer.extractMesh(origin, cell, dims, occlusion=True)
    plain = renderer.extractMesh(origin, cell, dims)
    for a, b in zip((pos, nrm, idx), plain):  # the mesh itself is sdfr_mesh_extract's
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert len(pos) > 500 and occ.dtype == sp.OCCLUSION_DTYPE and len(occ) == len(pos)
    # the defaults: bias one cell, radius eight
    ref = ou.oracle_points(scene, of, pos, nrm, cell, 8.0 * cell)
    qu.assert_same("%s mesh occlusion against the oracle" % scene, ou.occlusion_array(occ), ref)
    qu.assert_same("%s mesh occlusion against queryOcclusion" % scene, ou.occlusion_array(renderer.queryOcclusion(pos, nrm, cell, 8.0 * cell)), ref)
    ou.well_formed(ref)
    share = ou.partial_share(ref)
    print("%s: %d vertices, %.3f valid, %.3f of them partly occluded" % (scene, len(pos), (ref[:, 3] == 1).mean(), share))
    assert (ref[:, 3] == 1).mean() >= 0.99
    # with the surfaces too, other parameters, everything left on the device
    dpos, dnrm, _didx, dsrf, docc = renderer.extractMesh(origin, cell, dims, surfaces=True, occlusion=True, ao_radius=0.3, ao_bias=0.05, device=True)
    assert tuple(dsrf.shape) == (len(pos), 32)
    qu.assert_same("%s mesh occlusion, radius 0.3 (device)" % scene, ou.occlusion_array(gu.to_host(docc)), ou.oracle_points(scene, of, pos, nrm, 0.05, 0.3))


def test_arguments(renderer):
    import sdf_playground_amd as sp

    scene = "fast_sphere"
    gu.setup(renderer, scene, qu.frame(scene, 0.0, W, H))
    L, h = gu.raw(renderer)
    buf = np.zeros(64, np.float32)
    hit = np.zeros(4, sp.HIT_DTYPE)
    out = np.full(16, 7, np.uint32)  # what no failing call below may touch
    p, hp, o = (a.ctypes.data_as(ctypes.c_void_p) for a in (buf, hit, out))
    INVALID, NO_SCENE = -1, -4
    assert L.sdfr_occlusion_directions(None) == INVALID
    assert L.sdfr_query_occlusion(h, 0, None, None, 0.0, 1.0, None, 1) == 0
    assert L.sdfr_hit_occlusion(h, 0, None, 0.0, 1.0, None, 0) == 0
    # NULL pointers
    assert L.sdfr_query_occlusion(h, 1, None, p, 0.0, 1.0, o, 1) == INVALID
    assert L.sdfr_query_occlusion(h, 1, p, None, 0.0, 1.0, o, 1) == INVALID
    assert L.sdfr_query_occlusion(h, 1, p, p, 0.0, 1.0, None, 1) == INVALID
    assert L.sdfr_hit_occlusion(h, 1, None, 0.0, 1.0, o, 1) == INVALID
    assert L.sdfr_hit_occlusion(h, 1, hp, 0.0, 1.0, None, 1) == INVALID
    # bias: finite and >= 0; radius: finite and > 0 -- also with n = 0
    for bad in (-0.5, float("inf"), float("nan")):
        assert L.sdfr_query_occlusion(h, 1, p, p, bad, 1.0, o, 1) == INVALID
        assert L.sdfr_hit_occlusion(h, 1, hp, bad, 1.0, o, 1) == INVALID
        assert L.sdfr_hit_occlusion(h, 0, hp, bad, 1.0, o, 1) == INVALID
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert L.sdfr_query_occlusion(h, 1, p, p, 0.0, bad, o, 1) == INVALID
        assert L.sdfr_hit_occlusion(h, 1, hp, 0.0, bad, o, 1) == INVALID
        assert L.sdfr_query_occlusion(h, 0, p, p, 0.0, bad, o, 1) == INVALID
    # n, on_host, the handle
    for n in (-1, 2 ** 31):
        assert L.sdfr_query_occlusion(h, n, p, p, 0.0, 1.0, o, 1) == INVALID
        assert L.sdfr_hit_occlusion(h, n, hp, 0.0, 1.0, o, 1) == INVALID
    for bad in (2, -1):
        assert L.sdfr_query_occlusion(h, 1, p, p, 0.0, 1.0, o, bad) == INVALID
        assert L.sdfr_hit_occlusion(h, 1, hp, 0.0, 1.0, o, bad) == INVALID
    assert L.sdfr_query_occlusion(None, 1, p, p, 0.0, 1.0, o, 1) == INVALID
    assert L.sdfr_hit_occlusion(None, 1, hp, 0.0, 1.0, o, 1) == INVALID
    fresh = sp.SDFRenderer(0)
    try:
        assert L.sdfr_query_occlusion(fresh._h, 1, p, p, 0.0, 1.0, o, 1) == NO_SCENE
        assert L.sdfr_hit_occlusion(fresh._h, 1, hp, 0.0, 1.0, o, 1) == NO_SCENE
    finally:
        fresh.close()
    assert (out == 7).all()
    # and the same buffer is written by a good call: four misses
    assert L.sdfr_hit_occlusion(h, 4, hp, 0.0, 1.0, o, 1) == 0
    assert not out.any()


def test_occlusion_queries_leave_rendering_alone(renderer):
    scene = "labyrinth"
    of = qu.frame(scene, 0.4, 96, 64)
    gu.setup(renderer, scene, of)
    hits = ou.hit_items(scene, of, 71, 100)
    p, nr, _is = ou.points_of_hits(hits)
    with gu.rendering_untouched(renderer, 96, 64):
        renderer.hitOcclusion(hits, BIAS, RADIUS)
        renderer.queryOcclusion(p, nr, BIAS, RADIUS)
        renderer.hitOcclusion(renderer.pick(gu.to_device(qu.pick_grid(PW, PH)), PW, PH), BIAS, RADIUS)
        renderer.extractMesh((-5.35, -0.3, -2.55), 0.25, (5, 4, 3), occlusion=True)


def test_one_handle_across_scene_changes():
    # built-in scene -> run-time scene (its lazily compiled query module has the occlusion kernel) -> the same built-in scene
    import sdf_playground_amd as sp

    r = sp.SDFRenderer(0)
    try:
        rounds = []
        for scene in ("labyrinth", qu.HLSL[0], "labyrinth"):
            of = qu.frame(scene, 0.5, W, H)
            gu.setup(r, scene, of)
            hits = ou.hit_items(scene, of, 92, 70)
            ref = ou.oracle_hits(scene, of, hits, BIAS, RADIUS)
            got = ou.occlusion_array(r.hitOcclusion(hits, BIAS, RADIUS))
            qu.assert_same("%s hits" % scene, got, ref)
            qu.assert_same("%s hits (device)" % scene, ou.occlusion_array(gu.to_host(r.hitOcclusion(_hits_to_device(hits), BIAS, RADIUS))), ref)
            rounds.append(got)
        assert np.array_equal(rounds[0], rounds[2]) and rounds[0][:, 2].any()
    finally:
        r.close()


def test_two_frames_in_flight(renderer):
    # with two frames in flight a query runs on the lane of the frame submitted last; sdfr_sync before reading
    import torch

    scene, w, h = "labyrinth", 128, 72
    of = qu.frame(scene, 0.4, W, H)
    gu.setup(renderer, scene, of)
    hits = ou.hit_items(scene, of, 13, 70)
    ref = ou.oracle_hits(scene, of, hits, BIAS, RADIUS)
    img_ref = renderer.render(None, w, h)
    renderer.setFramesInFlight(2)
    try:
        imgs = [torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        dh = _hits_to_device(hits)
        got = []
        for k in range(4):
            renderer.render(None, w, h, out=imgs[k % 2])
            got.append(ou.occlusion_array(renderer.hitOcclusion(hits, BIAS, RADIUS)))
            dev = renderer.hitOcclusion(dh, BIAS, RADIUS)
            renderer.waitFrame(torch.cuda.current_stream().cuda_stream)
            renderer.sync()
            got.append(ou.occlusion_array(dev.cpu().numpy()))
            assert np.array_equal(imgs[k % 2].cpu().numpy().view(np.uint32), img_ref.view(np.uint32))
        for g in got:
            qu.assert_same("two frames in flight", g, ref)
    finally:
        renderer.setFramesInFlight(1)

"""GPU tier of the scene queries (sdfr_query_distance, sdfr_query_rays, sdfr_pick) through libsdfr.so: bit for bit against the
oracle's definitions (tests/cpp/query_oracle.h) for every scene compiled ahead of time and the run-time scenes with an oracle
twin, host and device memory; the run-time scenes' lazily compiled query module; one handle going from a built-in scene to a
run-time one and back through every entry point that launches the loaded scene; step shortcuts; agreement with the renderer's own
primary rays; no side effects on rendering; sizes and argument checks."""
import os
import zlib

import numpy as np
import pytest

import gpu_util as gu
import query_util as qu
from gpu_util import renderer  # noqa: F401

pytestmark = pytest.mark.gpu

N_POINTS = 20000
N_RAYS = 2000
W, H = 64, 48
SCENES_DIR = qu.SCENES_DIR


def _check_all(r, scene, of, seed, device=True):
    import torch

    pts = qu.point_samples(scene, of, seed, N_POINTS)
    d_ref, n_ref = qu.oracle_points(scene, of, pts)
    d, n = r.queryDistance(pts, normals=True)
    qu.assert_same("%s distance (host)" % scene, d, d_ref)
    qu.assert_same("%s normal (host)" % scene, n, n_ref)
    o, dirs = qu.ray_samples(of, seed + 7, N_RAYS)
    h_ref = qu.oracle_rays(scene, of, o, dirs)
    qu.assert_same("%s rays (host)" % scene, qu.hits_array(r.queryRays(o, dirs)), h_ref)
    px = qu.pick_grid(W, H)
    p_ref = qu.oracle_pick(scene, of, px)
    qu.assert_same("%s pick (host)" % scene, qu.hits_array(r.pick(px, W, H)), p_ref)
    if device:
        dd = r.queryDistance(gu.to_device(pts))  # without normals
        hd = r.queryRays(gu.to_device(o), gu.to_device(dirs))
        pd = r.pick(gu.to_device(px), W, H)
        torch.cuda.synchronize()
        qu.assert_same("%s distance (device)" % scene, dd.cpu().numpy(), d_ref)
        qu.assert_same("%s rays (device)" % scene, qu.hits_array(hd.cpu().numpy()), h_ref)
        qu.assert_same("%s pick (device)" % scene, qu.hits_array(pd.cpu().numpy()), p_ref)
        dn, nn = r.queryDistance(gu.to_device(pts), normals=True)
        torch.cuda.synchronize()
        qu.assert_same("%s normal (device)" % scene, nn.cpu().numpy(), n_ref)
    return h_ref, p_ref


@pytest.mark.parametrize("scene", qu.BUILTIN)
def test_builtin_queries_equal_oracle(renderer, scene):
    of = qu.frame(scene, 1.25, W, H)
    gu.setup(renderer, scene, of)
    _check_all(renderer, scene, of, seed=zlib.crc32(scene.encode()) & 0xffff)


@pytest.mark.parametrize("scene", sorted(qu.MOVED_VARS))
def test_queries_with_moved_variables(renderer, scene):
    of = qu.frame(scene, 0.5, W, H, qu.MOVED_VARS[scene])
    gu.setup(renderer, scene, of, qu.MOVED_VARS[scene])
    _check_all(renderer, scene, of, seed=11, device=False)


def test_debug_plane_and_hidden_objects(renderer):
    v = {"debug_nx": 0.3, "debug_ny": 1.0, "debug_y": 0.4}
    of = qu.frame("labyrinth", 0.75, W, H, v)
    gu.setup(renderer, "labyrinth", of, v)
    _check_all(renderer, "labyrinth", of, seed=21, device=False)
    renderer.resetVariables()


@pytest.mark.parametrize("scene", qu.HLSL)
def test_runtime_scenes_equal_oracle(renderer, scene):
    of = qu.frame(scene, 0.5, W, H)
    gu.setup(renderer, scene, of)
    _check_all(renderer, scene, of, seed=31)


def test_pendulum_hlsl_equals_its_cpp_twin():
    import sdf_playground_amd as sp

    of = qu.frame("fast_sphere", 0.8, W, H)  # (only the camera and limits: the pendulum has no oracle twin)
    px = qu.pick_grid(W, H)
    o, dirs = qu.ray_samples(of, 41, N_RAYS)
    pts = np.concatenate([o + dirs * t for t in (0.5, 1.5, 3.0)])
    out = []
    for how in ("hlsl", "cpp"):
        r = sp.SDFRenderer(0)
        try:
            if how == "hlsl":
                r.initShaderHlsl("pendulum_hlsl", os.path.join(SCENES_DIR, "pendulum.hlsl"))
            else:
                r.initShaderSource("pendulum_cpp", os.path.join(SCENES_DIR, "pendulum.scene.h"))
            gu.setup(r, None, of, load=False)
            d, n = r.queryDistance(pts, normals=True)
            out.append((d, n, qu.hits_array(r.queryRays(o, dirs)), qu.hits_array(r.pick(px, W, H))))
        finally:
            r.close()
    (a, b) = out
    for k, what in enumerate(("distance", "normal", "rays", "pick")):
        qu.assert_same("pendulum " + what, a[k], b[k])
    assert (a[2][:, 10] == 1).any()


def test_runtime_query_module_follows_the_scene(renderer):
    # a built-in scene after a run-time one uses the built-in kernels; a second run-time scene gets its own query module
    of = qu.frame("labyrinth", 0.3, W, H)
    gu.setup(renderer, "noise_lod", qu.frame("noise_lod", 0.3, W, H))
    renderer.queryDistance(np.zeros((4, 3), np.float32))
    gu.setup(renderer, "labyrinth", of)
    _check_all(renderer, "labyrinth", of, seed=51, device=False)
    for scene in ("noise_lod", "dialect_tour"):
        of = qu.frame(scene, 0.3, W, H)
        gu.setup(renderer, scene, of)
        _check_all(renderer, scene, of, seed=52, device=False)


# ---- one handle, built-in scene -> run-time scene -> the same built-in scene: every launch of the loaded scene -------------------------
# 130 items: two full waves and a partial one; a pick list with one pixel outside the frame; 5 x 4 x 3 cells: a 6 x 5 x 4 lattice, no
# axis a multiple of the lattice kernel's 4-point brick; a 24 x 17 frame: ragged against the 8 x 8 tile
SW_N, SW_W, SW_H = 130, 24, 17
SW_GRID = ((-5.35, -0.3, -2.55), 0.25, (5, 4, 3))  # over the floor, and in the labyrinth over a wall's corner
_switch_refs = {}


def _switch_reference(scene):
    """the inputs of a round and the oracle's answers to them, in the order _switch_answers gives the library's (computed once)"""
    if scene not in _switch_refs:
        import mesh_util as mu

        of = qu.frame(scene, 0.5, SW_W, SW_H)
        pts = qu.point_samples(scene, of, 91, SW_N)
        o, dirs = qu.ray_samples(of, 92, SW_N)
        px = np.concatenate([qu.pick_grid(SW_W, SW_H)[:3 * (SW_N - 1):3], [[SW_W, 3]]]).astype(np.int32)
        assert len(pts) == len(o) == len(px) == SW_N
        D, _ = qu.oracle_points(scene, of, mu.lattice_points(*SW_GRID), normals=False)
        pos, idx = mu.surface_nets(D, *SW_GRID, 0.0)
        assert len(pos) > 0 and len(idx) > 0
        img, st, _ = qu.po.render(scene, of, stats=True)
        want = list(qu.oracle_points(scene, of, pts)) + [qu.oracle_rays(scene, of, o, dirs), qu.oracle_pick(scene, of, px), pos,
                                                          qu.oracle_points(scene, of, pos)[1], idx, img, st]
        _switch_refs[scene] = (of, (pts, o, dirs, px), want)
    return _switch_refs[scene]


SWITCH_ANSWERS = ("distance", "normal", "rays", "pick", "mesh positions", "mesh normals", "mesh indices", "image", "pixel_stats")


def _switch_answers(r, inputs, device):
    """a point query with normals, a ray query, a pick, a mesh extraction with normals and a render with pixel_stats"""
    import torch

    pts, o, dirs, px = (gu.to_device(a) for a in inputs) if device else inputs
    d, n = r.queryDistance(pts, normals=True)
    rays, picks = r.queryRays(o, dirs), r.pick(px, SW_W, SW_H)
    pos, nrm, idx = r.extractMesh(*SW_GRID, device=device)
    if device:
        img = torch.empty((SW_H, SW_W, 4), dtype=torch.float32, device="cuda")
        st = torch.empty((SW_H, SW_W, 3), dtype=torch.int32, device="cuda")
        r.render(None, SW_W, SW_H, out=img, pixel_stats=st)
        r.sync()
        torch.cuda.synchronize()
        d, n, rays, picks, pos, nrm, idx, img, st = (t.cpu().numpy() for t in (d, n, rays, picks, pos, nrm, idx, img, st))
    else:
        img, st = r.render(None, SW_W, SW_H, pixel_stats=True)
    return [d, n, qu.hits_array(rays), qu.hits_array(picks), pos, nrm, idx.view(np.uint32), img, st.view(np.uint32)]


def test_one_handle_from_a_builtin_scene_to_a_runtime_scene_and_back():
    import sdf_playground_amd as sp

    r = sp.SDFRenderer(0)
    try:
        rounds = []
        for scene in ("labyrinth", qu.HLSL[0], "labyrinth"):
            of, inputs, want = _switch_reference(scene)
            gu.setup(r, scene, of)
            rounds.append([])
            for device in (False, True):
                got = _switch_answers(r, inputs, device)
                rounds[-1] += got
                for what, g, w in zip(SWITCH_ANSWERS, got, want):
                    assert g.shape == w.shape, (scene, what, device, g.shape, w.shape)
                    qu.assert_same("%s %s (%s)" % (scene, what, "device" if device else "host"), g, w)
        assert (rounds[0][3][-1, 10], rounds[1][3][-1, 10]) == (0xffffffff, 0xffffffff)  # the pixel outside the frame: hit = -1
        for a, b in zip(rounds[0], rounds[2]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        r.close()


@pytest.mark.parametrize("scene", ["labyrinth", "lense", "cube_sea"])
def test_step_shortcuts_keep_hits(renderer, scene):
    of = qu.frame(scene, 0.25, W, H)
    gu.setup(renderer, scene, of)
    o, dirs = qu.ray_samples(of, 61, N_RAYS)
    px = qu.pick_grid(W, H)
    exact = qu.hits_array(renderer.queryRays(o, dirs))
    pexact = qu.hits_array(renderer.pick(px, W, H))
    renderer.setStepShortcuts(True)
    short = qu.hits_array(renderer.queryRays(o, dirs))
    pshort = qu.hits_array(renderer.pick(px, W, H))
    renderer.setStepShortcuts(False)
    for e, s in ((exact, short), (pexact, pshort)):
        hit = e[:, 10] == 1
        assert np.array_equal(s[:, 10], e[:, 10])
        assert np.array_equal(s[hit], e[hit])
        assert (s[~hit, 8] <= e[~hit, 8]).all()


@pytest.mark.parametrize("scene", ["labyrinth", "lense", "noise_lod"])
def test_pick_misses_where_the_render_does(renderer, scene):
    w, h = 160, 96
    of = qu.frame(scene, 0.6, w, h)
    gu.setup(renderer, scene, of)
    _, st = renderer.render(None, w, h, pixel_stats=True)
    hits = renderer.pick(qu.pick_grid(w, h)[: w * h], w, h)
    assert np.array_equal((hits["hit"] == 0).reshape(h, w), st[..., 2] == 0)


def test_queries_leave_rendering_alone(renderer):
    scene = "labyrinth"
    of = qu.frame(scene, 0.4, 96, 64)
    gu.setup(renderer, scene, of)
    o, dirs = qu.ray_samples(of, 71, 500)
    with gu.rendering_untouched(renderer, 96, 64):
        renderer.queryRays(o, dirs)
        renderer.pick(qu.pick_grid(32, 16), 32, 16)
        renderer.queryDistance(o, normals=True)


def test_two_frames_in_flight(renderer):
    import torch

    scene = "lense"
    of = qu.frame(scene, 0.9, W, H)
    gu.setup(renderer, scene, of)
    o, dirs = qu.ray_samples(of, 81, 1000)
    ref = qu.hits_array(renderer.queryRays(o, dirs))
    img_ref = renderer.render(None, 128, 72)
    renderer.setFramesInFlight(2)
    try:
        imgs = [torch.empty((72, 128, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        got = []
        for k in range(4):
            renderer.render(None, 128, 72, out=imgs[k % 2])
            got.append(qu.hits_array(renderer.queryRays(o, dirs)))
            dev = renderer.queryRays(gu.to_device(o), gu.to_device(dirs))
            renderer.waitFrame(torch.cuda.current_stream().cuda_stream)
            renderer.sync()
            got.append(qu.hits_array(dev.cpu().numpy()))
            assert np.array_equal(imgs[k % 2].cpu().numpy().view(np.uint32), img_ref.view(np.uint32))
        for g in got:
            assert np.array_equal(g, ref)
    finally:
        renderer.setFramesInFlight(1)


def test_sizes_and_arguments(renderer):
    import ctypes

    import sdf_playground_amd as sp
    import torch

    L = sp.load_library()
    scene = "fast_sphere"
    of = qu.frame(scene, 0.0, W, H)
    gu.setup(renderer, scene, of)
    h = renderer._h
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.sdfr_query_distance(h, 0, None, None, None, 1) == 0
    assert L.sdfr_query_rays(h, 0, None, None, 0.0, None, 0) == 0
    assert L.sdfr_pick(h, W, H, 0, None, None, 1) == 0
    assert L.sdfr_query_distance(h, -1, p, p, None, 1) == -1
    assert L.sdfr_query_distance(h, 2 ** 31, p, p, None, 1) == -1
    assert L.sdfr_query_distance(h, 1, None, p, None, 1) == -1
    assert L.sdfr_query_distance(h, 1, p, None, None, 1) == -1
    assert L.sdfr_query_distance(h, 1, p, p, None, 2) == -1
    assert L.sdfr_query_rays(h, 1, p, None, 0.0, p, 1) == -1
    for bad in (-1.0, float("inf"), float("nan")):
        assert L.sdfr_query_rays(h, 1, p, p, bad, p, 1) == -1
    assert L.sdfr_pick(h, 0, H, 1, p, p, 1) == -1
    assert L.sdfr_pick(h, W, H, 1, None, p, 1) == -1
    assert L.sdfr_query_distance(None, 1, p, p, None, 1) == -1
    fresh = sp.SDFRenderer(0)
    try:
        assert L.sdfr_query_distance(fresh._h, 1, p, p, None, 1) == -4
        assert L.sdfr_pick(fresh._h, W, H, 1, p, p, 1) == -4
    finally:
        fresh.close()
    # picks outside the frame
    hits = renderer.pick(np.array([[-1, 0], [W, 0], [0, H], [3, 4]], np.int32), W, H)
    assert list(hits["hit"][:3]) == [-1, -1, -1] and hits["hit"][3] in (0, 1)
    # a count that is no multiple of any block, on the device
    n = 2 ** 22 + 17
    rng = np.random.default_rng(5)
    pts = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    d = renderer.queryDistance(gu.to_device(pts))
    torch.cuda.synchronize()
    d = d.cpu().numpy()
    k = np.r_[0:300, n - 300:n]
    d_ref, _ = qu.oracle_points(scene, of, pts[k], normals=False)
    qu.assert_same("large n", d[k], d_ref)
    dirs = np.repeat(np.array([[0.0, -1.0, 0.3]], np.float32), n, 0)
    hd = renderer.queryRays(gu.to_device(pts), gu.to_device(dirs))
    torch.cuda.synchronize()
    hd = qu.hits_array(hd.cpu().numpy())
    qu.assert_same("large n rays", hd[k], qu.oracle_rays(scene, of, pts[k], dirs[k]))


def test_item_offsets_past_32_bits(renderer):
    # past item 2^32 / 3 the offset of a float3 record (3 * i) no longer fits 32 bits: the last items must still read their own
    # point and write their own normal
    import torch

    scene = "fast_sphere"
    of = qu.frame(scene, 0.0, W, H)
    gu.setup(renderer, scene, of)
    n = (1 << 32) // 3 + 1000
    tail = np.random.default_rng(9).uniform(-3, 3, (1000, 3)).astype(np.float32)
    pts = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    pts[n - 1000:] = torch.from_numpy(tail).cuda()
    d, nr = renderer.queryDistance(pts, normals=True)
    torch.cuda.synchronize()
    d_ref, n_ref = qu.oracle_points(scene, of, tail)
    qu.assert_same("distance past 2^32 / 3 items", d[n - 1000:].cpu().numpy(), d_ref)
    qu.assert_same("normal past 2^32 / 3 items", nr[n - 1000:].cpu().numpy(), n_ref)
    zero_d, zero_n = qu.oracle_points(scene, of, np.zeros((1, 3), np.float32))
    qu.assert_same("distance of the first items", d[:1000].cpu().numpy(), np.repeat(zero_d, 1000))
    qu.assert_same("normal of the first items", nr[:1000].cpu().numpy(), np.repeat(zero_n, 1000, 0))
    del pts, d, nr
    torch.cuda.empty_cache()


def test_device_tensors_are_checked(renderer):
    import torch

    gu.setup(renderer, "fast_sphere", qu.frame("fast_sphere", 0.0, W, H))
    pts = torch.zeros((8, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(TypeError):
        renderer.queryDistance(pts.to(torch.int32))
    with pytest.raises(TypeError):
        renderer.pick(torch.zeros((8, 2), dtype=torch.float32, device="cuda"), W, H)
    with pytest.raises(TypeError):
        renderer.queryRays(pts, pts.t().contiguous().t())  # not contiguous
    with pytest.raises(ValueError):
        renderer.queryDistance(pts, out=torch.empty(7, dtype=torch.float32, device="cuda"))
    out = torch.empty((8, 12), dtype=torch.int32, device="cuda")  # hit records may be int32 as well
    renderer.queryRays(pts, pts + 1.0, out=out)
    torch.cuda.synchronize()
    assert set(out[:, 10].cpu().tolist()) <= {0, 1}

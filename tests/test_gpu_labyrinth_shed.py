"""GPU tier: the labyrinth's pixel kernel after it shed work a frame or a result already fixes -- the walls' clamps as sums, no
material for the hits of shadow rays, the sun's direction per frame (SceneLabyrinth, sdfr_scenes.h; ShadowHitsNeedMaterial,
FrameSunDir, sdfr_scene_traits.h) -- against the oracle, bit for bit:
pixels, rays and hits per pixel, and the evaluations, exactly where every step is marched and as an upper bound with step shortcuts.
100 x 60 pixels: 13 x 8 tiles, the right and the bottom ones partial.  The eyes are those of the CPU tier
(tests/labyrinth_shed_cameras.py)."""
import functools

import numpy as np
import pytest

import labyrinth_shed_cameras as cams

pytestmark = pytest.mark.gpu

W, H = 100, 60
LIMITS = dict(iter_count=256, bounce_count=16, ray_count=8, light_count=8, range=100.0, max_cost_default=7, extension_lights=0, extension_marble_reflection=0.0,
              dist_eps=0.0001, grad_eps=0.0001, reflect_eps=0.001, refract_eps=0.001, shadow_eps=0.0003)
CAMERAS = {c[0]: c for c in cams.cameras()}
# one sweep eye, an eye in a corridor beside a vase, an eye inside a wall, eyes with a -0 component (from y = -0 every ray ends on the floor at once)
EYES = ["sweep5", "near_vase_bowl", "inside_wall1", "zero_x_minus", "zero_y_minus"]


@functools.lru_cache(maxsize=None)
def _reference(name, limits=(), variables=(), size=(W, H)):
    """the oracle's frame from camera `name`: (basis, image, stats, totals), computed once and read-only"""
    from oracle import pyoracle as po

    f, basis = cams.oracle_frame(po, CAMERAS[name], size[0], size[1], **dict(limits))
    for k, v in variables:
        setattr(f, k, v)
    img, st, tot = po.render("labyrinth", f, stats=True)
    for a in (img, st, tot):
        a.setflags(write=False)
    return basis, img, st, tot


def _aim(r, name, basis, **limits):
    r.setLimits(**LIMITS)
    if limits:
        r.setLimits(**limits)
    r.setParameters(CAMERAS[name][4])
    r.setCameraBasis(*[[float(x) for x in row] for row in basis])  # the oracle's own basis: a -0 of the eye arrives as it is
    assert np.array_equal(r.getCameraBasis().view(np.uint32), basis.view(np.uint32))


def _fresh():
    import sdf_playground_amd as sp

    r = sp.SDFRenderer(0)
    r.initShader("labyrinth")
    r.setSchedule(sp.SCHEDULE_PIXEL)
    return r


@pytest.fixture(scope="module")
def renderer():
    r = _fresh()
    yield r
    r.close()


def _bits(a):
    return a.view(np.uint32)


def _check(r, name, where, ref, rst, tot, shortcuts):
    img, st = r.render(None, W, H, pixel_stats=True)
    assert np.array_equal(_bits(img), _bits(ref)), where + (int((_bits(img) != _bits(ref)).any(axis=2).sum()),)
    assert np.array_equal(st[..., 0], rst[..., 0]) and np.array_equal(st[..., 2], rst[..., 2]), where
    s = r.getStats()
    assert (int(s.pixels), int(s.rays), int(s.hits)) == (int(tot[0]), int(tot[1]), int(tot[3])), where
    if shortcuts:
        assert (st[..., 1] <= rst[..., 1]).all(), where
    else:
        assert np.array_equal(st[..., 1], rst[..., 1]) and int(s.march_evals) == int(tot[2]), where


@pytest.mark.parametrize("launch", ["per_tile", "persistent"])
@pytest.mark.parametrize("name", EYES)
def test_frames_match_the_oracle(renderer, name, launch):
    import sdf_playground_amd as sp

    basis, ref, rst, tot = _reference(name)
    if name == "inside_wall1":
        assert int((rst[..., 1] == 1).sum()) == W * H  # every primary ray ends on its first sample
    else:
        assert 0 < int((rst[..., 2] >= 2).sum())  # shadow rays that hit (hits beyond the first)
    _aim(renderer, name, basis)
    renderer.setLaunchMode(sp.LAUNCH_PER_TILE if launch == "per_tile" else sp.LAUNCH_PERSISTENT)
    try:
        for shortcuts in (False, True):
            renderer.setStepShortcuts(shortcuts)
            _check(renderer, name, (name, launch, shortcuts), ref, rst, tot, shortcuts)
    finally:
        renderer.setStepShortcuts(False)
        renderer.setLaunchMode(sp.LAUNCH_AUTO)


@pytest.mark.parametrize("name", ["sweep5", "near_vase_bowl"])
def test_debug_plane_takes_the_unchanged_kernel(renderer, name):
    """the debug build keeps the reference's path: every sample through map_geometry, every hit through shade_hit"""
    variables = (("debug_ny", 1.0), ("debug_y", 1.5), ("debug_scale", 0.5))
    basis, ref, rst, tot = _reference(name, variables=variables)
    assert not np.array_equal(_bits(ref), _bits(_reference(name)[1]))  # the plane shows
    _aim(renderer, name, basis)
    try:
        for k, v in variables:
            assert renderer.setValue(k, v)
        _check(renderer, name, (name, "debug plane"), ref, rst, tot, False)
    finally:
        renderer.resetVariables()
    basis, ref, rst, tot = _reference(name)
    _check(renderer, name, (name, "plane off again"), ref, rst, tot, False)


@pytest.mark.parametrize("name", ["sweep5", "near_vase_bowl"])
def test_reflective_marble_and_seven_more_lights(renderer, name):
    """the reflective-marble extension (its reflected rays' shadow rays hit as well), and seven extension lights with a cost limit of
    9: slots 1 to 7 take the generic light path beside the sun's per-frame direction in slot 0"""
    for limits in ((("extension_marble_reflection", 0.25),), (("extension_lights", 7), ("max_cost_default", 9))):
        basis, ref, rst, tot = _reference(name, limits=limits)
        assert int(tot[1]) > int(_reference(name)[3][1])  # more rays than the plain frame
        _aim(renderer, name, basis, **dict(limits))
        try:
            for shortcuts in (False, True):
                renderer.setStepShortcuts(shortcuts)
                _check(renderer, name, (name, limits, shortcuts), ref, rst, tot, shortcuts)
        finally:
            renderer.setStepShortcuts(False)
            renderer.setLimits(**LIMITS)


def test_a_handle_takes_each_frame_s_own_eye(renderer):
    """three frames in a row from three eyes, then two frames in flight from two: each equals the frame of a fresh handle (and the
    oracle's).  A per-frame constant left over from the frame before would show."""
    import torch

    order = ["near_vase_bowl", "inside_wall1", "sweep5"]
    fresh = {}
    for name in order:
        r = _fresh()
        try:
            _aim(r, name, _reference(name)[0])
            fresh[name] = r.render(None, W, H, pixel_stats=True)
        finally:
            r.close()
        assert np.array_equal(_bits(fresh[name][0]), _bits(_reference(name)[1])), name
    for name in order:
        _aim(renderer, name, _reference(name)[0])
        img, st = renderer.render(None, W, H, pixel_stats=True)
        assert np.array_equal(_bits(img), _bits(fresh[name][0])) and np.array_equal(st, fresh[name][1]), name
    renderer.setFramesInFlight(2)
    try:
        outs = []
        for name in ("zero_y_minus", "near_vase_bowl", "sweep5", "inside_wall1"):
            _aim(renderer, name, _reference(name)[0])
            outs.append((name, torch.empty((H, W, 4), dtype=torch.float32, device="cuda")))
            renderer.render(None, W, H, out=outs[-1][1])
        renderer.sync()
        for name, out in outs:
            assert np.array_equal(_bits(out.cpu().numpy()), _bits(_reference(name)[1])), name
    finally:
        renderer.setFramesInFlight(1)


def test_strips_and_anti_aliased_frames_are_today_s(renderer):
    """compared the way tests/test_gpu_parity.py and tests/test_gpu_aa.py compare theirs: the strips of three ranks assemble to the handle's
    full frame, and the anti-aliased frame is the pyramid of the handle's own render of the supersampled frame; both frames are the
    oracle's"""
    import torch
    import sdf_playground_amd as sp
    import aa_util as au

    name = "near_vase_bowl"
    basis, ref, _rst, _tot = _reference(name)
    _aim(renderer, name, basis)
    full = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    renderer.render(None, W, H, out=full)
    world = 3
    n = sp.strip_buffer_pixels(W, H, world)
    gathered = torch.empty((world, n, 4), dtype=torch.float32, device="cuda")
    for rank in range(world):
        renderer.renderStrips(W, H, rank, world, gathered[rank])
    out = torch.empty_like(full)
    renderer.assembleStrips(W, H, world, gathered, out)
    renderer.sync()
    assert torch.equal(out, full)
    assert np.array_equal(_bits(full.cpu().numpy()), _bits(ref))

    factor, w, h = 2, W // 2, H // 2
    basis2, ref2, rst2, _tot2 = _reference(name, size=(w * factor, h * factor))
    _aim(renderer, name, basis2)
    img, st = renderer.renderAA(None, w, h, factor, pixel_stats=True)
    s, sst = renderer.render(None, w * factor, h * factor, pixel_stats=True)
    assert au.same_bits(img, au.pyramid(s, factor)) and np.array_equal(st, au.sum_stats(sst, factor))
    assert np.array_equal(_bits(s), _bits(ref2)) and np.array_equal(sst, rst2)

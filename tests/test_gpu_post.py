"""GPU tier: the bloom + tone-map kernels (sdfr_post.hip) through the C ABI against the
oracle's restatement of HDR::process: byte-exact LDR image and bit-exact bloom buffer."""
import math

import numpy as np
import pytest

from gpu_util import renderer  # noqa: F401

pytestmark = pytest.mark.gpu


def _check(renderer, oracle, scene16):
    import torch
    import sdf_playground_amd as sp

    H, W, _ = scene16.shape
    hdr = sp.HDR(renderer)
    hdr.init(W, H)
    hdr.getRenderTarget().copy_(torch.from_numpy(scene16))
    ldr = hdr.process().cpu().numpy()
    renderer.sync()
    b1, b2, ref = oracle.postprocess(scene16)
    assert np.array_equal(hdr._bloom.cpu().numpy().view(np.uint16), b1.view(np.uint16))
    assert np.array_equal(ldr, ref)


@pytest.mark.parametrize("size", [(64, 64), (300, 77), (33, 65), (257, 31), (1, 1), (513, 97)])
def test_postprocess_random_images(renderer, oracle, size):
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    img = (rng.random((h, w, 4)) ** 3 * 6).astype(np.float16)
    img[..., 3] = rng.integers(0, 2, (h, w))
    img[rng.random((h, w)) < 0.02] = [60000, 0, 1e-7, 1]  # large and subnormal halves
    _check(renderer, oracle, img)


@pytest.mark.parametrize("size", [(700, 230), (256, 96), (289, 129)])
def test_postprocess_mostly_dark_images(renderer, oracle, size):
    """blocks whose staged tile is all zeros skip the taps (sdfr_post.hip): a few bright texels placed on and around
    the block and halo boundaries of both passes (256-wide row segments +- 32; 32x32 tiles +- 32 rows), dark texels
    of both signs of zero and small values the bright-pass removes"""
    w, h = size
    rng = np.random.default_rng(w + h)
    img = np.zeros((h, w, 4), np.float16)
    img[..., :3] = (rng.random((h, w, 3)) * 0.2).astype(np.float16)  # dark: the bright-pass factor is 0
    img[rng.random((h, w)) < 0.3] = np.float16(-0.0)
    img[..., 3] = rng.integers(0, 2, (h, w))
    for x in (0, 31, 32, 223, 224, 255, 256, 287, 288, 289, 511, 512, 543, 544, w - 1):
        for y in (0, 31, 32, 63, 64, 95, 96, 127, 128, h - 1):
            if x < w and y < h and rng.random() < 0.25:
                img[y, x] = [float(rng.uniform(1, 40)), float(rng.uniform(0.5, 9)), float(rng.uniform(0, 3)), float(rng.integers(0, 2))]
    _check(renderer, oracle, img)
    # and one lone light in the middle of nothing, every other block is skipped
    img[..., :3] = 0
    img[h // 2, w // 2] = [30, 20, 10, 1]
    _check(renderer, oracle, img)
    img[...] = 0
    _check(renderer, oracle, img)


@pytest.mark.parametrize("dark", [True, False])
def test_postprocess_unusual_texels(renderer, oracle, dark):
    """what the tone map's short cuts must not change (sdfr_post.hip, tone_map): negative colours, infinities, NaN,
    colours past the exponential's underflow, alpha that is not the renderer's 0 / 1 flag (fractions, negative, NaN,
    inf, -0) -- in tiles without any bloom (dark) and in tiles that blur a bright neighbourhood"""
    w, h = 200, 136
    rng = np.random.default_rng(77 + dark)
    img = np.zeros((h, w, 4), np.float16)
    img[..., :3] = (rng.random((h, w, 3)) * (0.3 if dark else 4.0)).astype(np.float16)
    img[..., 3] = rng.integers(0, 2, (h, w))
    specials = [float("inf"), float("-inf"), float("nan"), -0.0, -1.5, -300.0, 88.0, 90.0, 200.0, 65504.0, 6e-8, -6e-8, 0.5, 2.0]
    for k in range(900):
        x, y, c = int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(0, 4))
        img[y, x, c] = specials[int(rng.integers(0, len(specials)))]
    if dark:  # keep the bright-pass shut: no texel brighter than 0.75 (NaN / inf colours would light the tile)
        rgb = img[..., :3].astype(np.float32)
        bad = ~np.isfinite(rgb).all(axis=2) | (rgb.max(axis=2) > 0.7)
        img[bad, :3] = np.float16(-2.0)
    _check(renderer, oracle, img)


def test_postprocess_of_rendered_frame(renderer, oracle):
    """render (RGBA16F target) -> process, as Application::render does (Application.cpp:274-284)."""
    import torch
    import sdf_playground_amd as sp

    W, H = 320, 180
    renderer.initShader("light_shadows")  # emissive spheres: plenty of bloom
    renderer.setParameters(0.5)
    renderer.setLimits(iter_count=100, bounce_count=16, ray_count=8, light_count=8, range=100.0, max_cost_default=7)
    cam = sp.Camera()
    cam.SetEye((0, 5, -9))
    cam.SetLookat((0, 1, 0))
    cam.SetAspect(W / H)
    hdr = sp.HDR(renderer)
    hdr.init(W, H)
    renderer.render(cam, W, H, out=hdr.getRenderTarget(), fmt=sp.RGBA16F)
    ldr = hdr.process().cpu().numpy()
    scene16 = hdr.getRenderTarget().cpu().numpy()
    _, _, ref = oracle.postprocess(scene16)
    assert np.array_equal(ldr, ref)
    assert (ldr[..., :3].max(axis=2) > 200).mean() > 0.002  # something bright is in the picture


def test_named_timings_follow_the_reference_frame():
    """GPUProfiler names of one frame (SDFRenderer.cpp:100-104, Postprocessing.cpp:147-171)."""
    import sdf_playground_amd as sp
    import torch

    r = sp.SDFRenderer(0)
    r.initShader("labyrinth")
    assert r.getTimings() == {}
    hdr = sp.HDR(r)
    hdr.init(320, 200)
    r.render(sp.Camera(), 320, 200, out=hdr.getRenderTarget(), fmt=sp.RGBA16F)
    assert list(r.getTimings()) == ["setup", "draw"]
    hdr.process()
    t = r.getTimings()
    assert list(t) == ["setup", "draw", "Bloom 1", "Bloom 2 + HDR"]
    assert all(v >= 0.0 for v in t.values()) and t["draw"] > 0.0 and t["Bloom 1"] > 0.0
    assert abs(t["draw"] - r.getStats().ms_gpu) < 1e-6
    r.setSchedule(sp.SCHEDULE_WAVEFRONT)
    r.setProfiling(True)
    r.render(sp.Camera(), 320, 200, out=hdr.getRenderTarget(), fmt=sp.RGBA16F)
    names = list(r.getTimings())
    assert names[:4] == ["setup", "draw", "draw: march 0", "draw: shade 0"] and names[-2:] == ["Bloom 1", "Bloom 2 + HDR"]
    r.close()

"""GPU tier: the benchmark's frames as bench.py renders them -- each configuration whose scene has a step-shortcut rule, all
bench.SWEEP frames of its camera sweep, the renderer set up as bench.py's make_renderer does (pixel schedule, the default launch
mode, step shortcuts on).  Every frame equals, bit for bit, the same frame with every step marched, with the same pixel, ray and hit
totals; a stride-12 sample of it, at a phase that moves from frame to frame, carries the oracle's pixels, rays and hits; and the
bench's second pass (two frames in flight) gives the same bits again."""
import numpy as np
import pytest

from gpu_util import DEFAULT_LIMITS
from gpu_util import renderer  # noqa: F401

pytestmark = pytest.mark.gpu

STRIDE = 12


def _phase(k):
    # 37 is prime to 144: the sweep's frames sample 16 different phases of the 12 x 12 grid
    j = (37 * k + 5) % (STRIDE * STRIDE)
    return j % STRIDE, j // STRIDE


@pytest.mark.parametrize("config", ["2", "3", "3r", "4", "5", "5g"])
def test_bench_sweep_with_shortcuts(renderer, oracle, config):
    import torch
    import bench
    import sdf_playground_amd as sp

    assert len({_phase(k) for k in range(bench.SWEEP)}) == bench.SWEEP
    cfg = bench.CONFIGS[config]
    scene, w, h = cfg["scene"], cfg["width"], cfg["height"]
    r = renderer
    r.initShader(scene)
    r.resetVariables()
    r.setLimits(**DEFAULT_LIMITS)
    r.setLimits(**cfg["limits"])
    r.setSchedule(sp.SCHEDULE_PIXEL)
    r.setLaunchMode(sp.LAUNCH_AUTO)
    frames = []
    try:
        img_off = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        img_st = torch.empty_like(img_off)
        pst = torch.empty((h, w, 3), dtype=torch.int32, device="cuda")
        saved = 0
        for k in range(bench.SWEEP):
            cam, stime = bench.make_camera(k, w, h, config)
            r.setParameters(stime)
            # the bench's frame: shortcuts on, no per-pixel counters
            r.setStepShortcuts(True)
            img = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
            r.render(cam, w, h, out=img)
            on = r.getStats()
            # the same with the per-pixel counters, then with every step marched
            r.render(cam, w, h, out=img_st, pixel_stats=pst)
            st = r.getStats()
            r.setStepShortcuts(False)
            r.render(cam, w, h, out=img_off)
            off = r.getStats()
            bits = img.view(torch.int32)
            assert torch.equal(bits, img_off.view(torch.int32)), (config, k, "shortcuts on / off")
            assert torch.equal(bits, img_st.view(torch.int32)), (config, k, "with per-pixel counters")
            assert (on.pixels, on.rays, on.hits) == (off.pixels, off.rays, off.hits) == (st.pixels, st.rays, st.hits), (config, k)
            assert on.pixels == w * h and on.march_evals == st.march_evals <= off.march_evals, (config, k, on.march_evals, off.march_evals)
            sums = pst.view(-1, 3).sum(dim=0, dtype=torch.int64).tolist()
            assert sums == [st.rays, st.march_evals, st.hits], (config, k, sums)
            saved += off.march_evals - on.march_evals
            # a stride-12 sample against the oracle, at this frame's own phase of the grid
            ox, oy = _phase(k)
            f = bench.oracle_frame(oracle, k, w, h, config)
            ref, rst, _ = oracle.render(scene, f, region=(ox, oy, w, h), step=(STRIDE, STRIDE), stats=True)
            got = img[oy::STRIDE, ox::STRIDE].cpu().numpy()
            gst = pst[oy::STRIDE, ox::STRIDE].cpu().numpy().view(np.uint32)
            ref, rst = ref[oy::STRIDE, ox::STRIDE], rst[oy::STRIDE, ox::STRIDE]
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (config, k, int((got.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum()))
            assert np.array_equal(gst[..., 0], rst[..., 0]) and np.array_equal(gst[..., 2], rst[..., 2]), (config, k)
            assert (gst[..., 1] <= rst[..., 1]).all(), (config, k)
            frames.append((img, (on.pixels, on.rays, on.hits)))
        assert saved > 0, config

        # the bench's second pass: two frames in flight on the one handle, rendered into two images in turn.  Each frame is compared on a
        # side stream that waits for it on the device; a frame's image is rendered into again only once its comparison is done.
        r.sync()
        r.setStepShortcuts(True)
        r.setFramesInFlight(2)
        pair = [torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        side = torch.cuda.Stream()
        equal, done = [], []
        for k in range(bench.SWEEP):
            if k >= 2:
                done[k - 2].synchronize()
            cam, stime = bench.make_camera(k, w, h, config)
            r.setParameters(stime)
            r.setCamera(cam)
            r.render(None, w, h, out=pair[k & 1])
            r.waitFrame(side.cuda_stream)
            with torch.cuda.stream(side):
                equal.append((pair[k & 1].view(torch.int32) == frames[k][0].view(torch.int32)).all())
                ev = torch.cuda.Event()
                ev.record(side)
                done.append(ev)
        r.sync()
        side.synchronize()
        last = r.getStats()
        assert [bool(e) for e in equal] == [True] * bench.SWEEP, (config, [bool(e) for e in equal])
        assert (last.pixels, last.rays, last.hits) == frames[-1][1], config
    finally:
        r.setFramesInFlight(1)
        r.setStepShortcuts(False)
        r.setLimits(**DEFAULT_LIMITS)

"""GPU tier: the labyrinth's pixel kernel with its once-per-ray rule (SceneLabyrinth::ray_bounds; RayBounds, sdfr_scene_traits.h: a descending ray still
above the wall tops where its range ends is a miss before its first evaluation) against the oracle, bit for bit: pixels, rays and hits per
pixel, and the evaluations, exactly where every step is marched and as an upper bound with step shortcuts.  The frames are those of the CPU
tier (tests/range_clear_cases.py; tests/test_range_clear_pipeline_cpu.py asserts what they contain), one wave per tile and the persistent
launch; then the band of the real workload: sweep frame 0 of the benchmark's headline configuration at its full size, rows 416 to 463."""
import numpy as np
import pytest

import range_clear_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderer():
    import sdf_playground_amd as sp

    r = sp.SDFRenderer(0)
    r.initShader("labyrinth")
    r.setSchedule(sp.SCHEDULE_PIXEL)
    yield r
    r.close()


def _bits(a):
    return a.view(np.uint32)


@pytest.mark.parametrize("launch", ["per_tile", "persistent"])
@pytest.mark.parametrize("case", list(rc.CASES))
def test_frames_match_the_oracle(renderer, case, launch):
    import sdf_playground_amd as sp

    renderer.setLaunchMode(sp.LAUNCH_PER_TILE if launch == "per_tile" else sp.LAUNCH_PERSISTENT)
    inside = rc.masks(case)[0]
    try:
        for iter_count in rc.ITER_COUNTS:
            basis, ref, rst, tot = rc.reference(case, iter_count)
            renderer.setLimits(**rc.limits_of(case, iter_count))
            renderer.setParameters(rc.CASES[case][0][4])
            renderer.setCameraBasis(*[[float(x) for x in row] for row in basis])  # the oracle's own basis: the eye arrives as it is
            assert np.array_equal(_bits(renderer.getCameraBasis()), _bits(basis))
            for shortcuts in (False, True):
                renderer.setStepShortcuts(shortcuts)
                where = (case, launch, iter_count, shortcuts)
                img, st = renderer.render(None, rc.W, rc.H, pixel_stats=True)
                assert np.array_equal(_bits(img), _bits(ref)), where + (int((_bits(img) != _bits(ref)).any(axis=2).sum()),)
                assert np.array_equal(st[..., 0], rst[..., 0]) and np.array_equal(st[..., 2], rst[..., 2]), where
                s = renderer.getStats()
                assert (int(s.pixels), int(s.rays), int(s.hits)) == (int(tot[0]), int(tot[1]), int(tot[3])), where
                if shortcuts:
                    assert (st[..., 1] <= rst[..., 1]).all(), where
                    assert (st[..., 1][inside] == 0).all() and (rst[..., 1][inside] > 0).all(), where  # the band does not march
                else:
                    assert np.array_equal(st[..., 1], rst[..., 1]) and int(s.march_evals) == int(tot[2]), where
    finally:
        renderer.setStepShortcuts(False)
        renderer.setLaunchMode(sp.LAUNCH_AUTO)
        renderer.setLimits(**dict(rc.mp.LIMITS, iter_count=100))


def test_the_band_of_the_headline_frame(renderer, oracle):
    """sweep frame 0 at 3840 x 2160 with the iteration limit 256, as bench.py renders it: rows 416 to 463 (the band is rows 425 to 453), every
    fourth column, against the oracle's region, step shortcuts on and off"""
    import torch
    import bench
    import sdf_playground_amd as sp

    cfg = bench.CONFIGS["3"]
    w, h = cfg["width"], cfg["height"]
    y0, y1, stride = 416, 464, 4
    f = bench.oracle_frame(oracle, 0, w, h, "3")
    ref, rst, _ = oracle.render("labyrinth", f, region=(0, y0, w, y1), step=(stride, 1), stats=True)
    ref, rst = ref[y0:y1, ::stride], rst[y0:y1, ::stride]
    ys, xs = np.mgrid[y0:y1, 0:w:stride]
    basis = [f.eye, f.front, f.right, f.top]
    inside = rc.band_masks([[float(v[i]) for i in range(3)] for v in basis], w, h, xs, ys, float(f.range))[0]
    assert int(inside.sum()) >= 20000 and (rst[..., 1][inside] > 0).all() and (rst[..., 2][inside] == 0).all()  # 91 722 pixels of the frame, a quarter sampled

    r = renderer
    r.resetVariables()
    r.setLimits(**dict(rc.mp.LIMITS, iter_count=100))
    r.setLimits(**cfg["limits"])
    r.setLaunchMode(sp.LAUNCH_AUTO)
    cam, stime = bench.make_camera(0, w, h, "3")
    r.setParameters(stime)
    img = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    pst = torch.empty((h, w, 3), dtype=torch.int32, device="cuda")
    try:
        for shortcuts in (True, False):
            r.setStepShortcuts(shortcuts)
            r.render(cam, w, h, out=img, pixel_stats=pst)
            got = img[y0:y1, ::stride].cpu().numpy()
            gst = pst[y0:y1, ::stride].cpu().numpy().view(np.uint32)
            assert np.array_equal(_bits(got), _bits(ref)), (shortcuts, int((_bits(got) != _bits(ref)).any(axis=2).sum()))
            assert np.array_equal(gst[..., 0], rst[..., 0]) and np.array_equal(gst[..., 2], rst[..., 2]), shortcuts
            if shortcuts:
                assert (gst[..., 1] <= rst[..., 1]).all()
                assert (gst[..., 1][inside] == 0).all()
            else:
                assert np.array_equal(gst[..., 1], rst[..., 1])
    finally:
        r.setStepShortcuts(False)
        r.setLimits(**dict(rc.mp.LIMITS, iter_count=100))

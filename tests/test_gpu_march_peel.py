"""GPU tier: the labyrinth's pixel kernel with its peeled march -- a ray's first three samples as straight-line code, the factor once, the march
loop without march_pre (PeelUnrelaxedSamples, sdfr_scene_traits.h; render_pixel) -- against the oracle, bit for bit: pixels, rays and hits per pixel,
and the evaluations, exactly where every step is marched and as an upper bound with step shortcuts.  The frames are those of the CPU tier
(tests/march_peel_cases.py, which also says what they have to contain; tests/test_march_peel_pipeline_cpu.py asserts it and holds the control:
tests/test_march_peel_cpu.py shows that the factor one sample early is seen): 96 x 54 pixels, 12 x 7 tiles, the bottom ones partial; every
iteration limit from 1 to 5, 100 and 256; one wave per tile and the persistent launch."""
import numpy as np
import pytest

import march_peel_cases as mp

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
@pytest.mark.parametrize("case", list(mp.CASES))
def test_frames_match_the_oracle(renderer, case, launch):
    import sdf_playground_amd as sp

    renderer.setLaunchMode(sp.LAUNCH_PER_TILE if launch == "per_tile" else sp.LAUNCH_PERSISTENT)
    try:
        for iter_count in mp.ITER_COUNTS:
            basis, ref, rst, tot = mp.reference(case, iter_count)
            renderer.setLimits(**mp.limits_of(case, iter_count))
            renderer.setParameters(mp.CASES[case][0][4])
            renderer.setCameraBasis(*[[float(x) for x in row] for row in basis])  # the oracle's own basis: the eye arrives as it is
            assert np.array_equal(_bits(renderer.getCameraBasis()), _bits(basis))
            for shortcuts in (False, True):
                renderer.setStepShortcuts(shortcuts)
                where = (case, launch, iter_count, shortcuts)
                img, st = renderer.render(None, mp.W, mp.H, pixel_stats=True)
                assert np.array_equal(_bits(img), _bits(ref)), where + (int((_bits(img) != _bits(ref)).any(axis=2).sum()),)
                assert np.array_equal(st[..., 0], rst[..., 0]) and np.array_equal(st[..., 2], rst[..., 2]), where
                s = renderer.getStats()
                assert (int(s.pixels), int(s.rays), int(s.hits)) == (int(tot[0]), int(tot[1]), int(tot[3])), where
                if shortcuts:
                    assert (st[..., 1] <= rst[..., 1]).all(), where
                else:
                    assert np.array_equal(st[..., 1], rst[..., 1]) and int(s.march_evals) == int(tot[2]), where
    finally:
        renderer.setStepShortcuts(False)
        renderer.setLaunchMode(sp.LAUNCH_AUTO)


def test_the_cases_end_rays_in_every_peeled_pass():
    seen = mp.classify()
    for key, pixels in seen.items():
        assert pixels >= 50, (key, seen)

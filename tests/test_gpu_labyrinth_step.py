"""GPU tier: the labyrinth's kernels after the exact rewrites of the march step (SceneLabyrinth::rep20 / fold / floor_dist, sdfr_scenes.h)
against the oracle, bit for bit: pixels, rays and hits, and the step counters where every step is marched.  64 x 40 pixels are 40 tiles,
enough for the persistent hand-out and its row feedback; the cameras are those of the CPU tier (tests/labyrinth_step_cameras.py, what
each is for is said there; tests/test_labyrinth_step_cpu.py asserts that the oracle's frames show hits and misses)."""
import numpy as np
import pytest

import labyrinth_step_cameras as lsc

pytestmark = pytest.mark.gpu

CAMERAS = lsc.cameras()
LIMITS = dict(iter_count=256, bounce_count=16, ray_count=8, light_count=8, range=100.0, max_cost_default=7, extension_lights=0, extension_marble_reflection=0.0,
              dist_eps=0.0001, grad_eps=0.0001, reflect_eps=0.001, refract_eps=0.001, shadow_eps=0.0003)


@pytest.fixture(scope="module")
def renderer():
    import sdf_playground_amd as sp

    r = sp.SDFRenderer(0)
    r.initShader("labyrinth")
    yield r
    r.close()


def _compare(renderer, oracle, cam, schedules, **limits):
    import sdf_playground_amd as sp

    f, basis = lsc.oracle_frame(oracle, cam, **limits)
    ref, rst, _ = oracle.render("labyrinth", f, stats=True)
    renderer.setLimits(**LIMITS)
    if limits:
        renderer.setLimits(**limits)
    renderer.setParameters(cam[4])
    renderer.setCameraBasis(*[[float(x) for x in row] for row in basis])  # the oracle's own basis: an eye at y = -0 arrives as it is
    assert np.array_equal(renderer.getCameraBasis().view(np.uint32), basis.view(np.uint32))
    try:
        for schedule in schedules:
            renderer.setSchedule(schedule)
            for shortcuts in (False, True):
                renderer.setStepShortcuts(shortcuts)
                img, st = renderer.render(None, lsc.W, lsc.H, pixel_stats=True)
                where = (cam[0], schedule, shortcuts)
                assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), where + (int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum()),)
                assert np.array_equal(st[..., 0], rst[..., 0]) and np.array_equal(st[..., 2], rst[..., 2]), where
                if shortcuts:
                    assert (st[..., 1] <= rst[..., 1]).all(), where
                else:
                    assert np.array_equal(st[..., 1], rst[..., 1]), where
    finally:
        renderer.setStepShortcuts(False)
        renderer.setSchedule(sp.SCHEDULE_PIXEL)
        renderer.setLimits(**LIMITS)


@pytest.mark.parametrize("name", [c[0] for c in CAMERAS])
def test_labyrinth_matches_the_oracle(renderer, oracle, name):
    import sdf_playground_amd as sp

    cam = next(c for c in CAMERAS if c[0] == name)
    _compare(renderer, oracle, cam, [sp.SCHEDULE_PIXEL])


def test_reflective_marble_matches_the_oracle(renderer, oracle):
    """configuration 3r's path: walls and vases reflect"""
    import sdf_playground_amd as sp

    _compare(renderer, oracle, CAMERAS[1], [sp.SCHEDULE_PIXEL], extension_marble_reflection=0.25)


@pytest.mark.parametrize("name", ["sweep11", "minus0_pp_down", "far_np"])
def test_wavefront_schedule_matches_the_oracle(renderer, oracle, name):
    """the wavefront kernels evaluate the same SceneLabyrinth::dist"""
    import sdf_playground_amd as sp

    cam = next(c for c in CAMERAS if c[0] == name)
    _compare(renderer, oracle, cam, [sp.SCHEDULE_WAVEFRONT])


# ---- the gradient table's second pass -----------------------------------------------------------------------------------
# Frames in which some lanes of the pixel kernel, and not all, find their lattice coordinates outside the table path's domain and
# evaluate the noise again with the formula, divergently (sdfr_noise.h: snoise3 / turbulence3 with NoiseGradTable); no camera above
# reaches that.  tests/test_labyrinth_fallback_cpu.py counts the pixels that do, per frame, on the host build with the table.
FALLBACK_CAMERAS = lsc.fallback_cameras()


@pytest.mark.parametrize("name", [c[0] for c in FALLBACK_CAMERAS])
def test_table_fallback_frames_match_the_oracle(renderer, oracle, name):
    import sdf_playground_amd as sp

    cam = next(c for c in FALLBACK_CAMERAS if c[0] == name)
    _compare(renderer, oracle, cam, [sp.SCHEDULE_PIXEL])


def test_table_fallback_frame_matches_the_oracle_on_the_wavefront_schedule(renderer, oracle):
    """the wavefront kernels shade with the formula: the same frame, the other gradient source"""
    import sdf_playground_amd as sp

    _compare(renderer, oracle, next(c for c in FALLBACK_CAMERAS if c[0] == "far22_pn"), [sp.SCHEDULE_WAVEFRONT])

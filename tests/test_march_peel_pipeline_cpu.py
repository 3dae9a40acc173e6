"""CPU tier: the whole pipeline with the labyrinth's peeled march -- the host build of the product's headers (tests/hostsim: render_pixel with a
ray's first three samples as straight-line code, the factor once, the loop without march_pre; PeelUnrelaxedSamples, sdfr_scene_traits.h) against the
oracle: pixels, rays and hits per pixel bit for bit, the evaluations equal where every step is marched and no more than the oracle's with step
shortcuts.  The frames and what they have to contain: tests/march_peel_cases.py; every case with the iteration limits 1, 2, 3, 4, 5, 100, 256."""
import numpy as np
import pytest

import march_peel_cases as mp


def _bits(a):
    return a.view(np.uint32)


@pytest.mark.parametrize("case", list(mp.CASES))
def test_host_pipeline_matches_the_oracle(case):
    import hostsim

    for iter_count in mp.ITER_COUNTS:
        _basis, ref, rst, _tot = mp.reference(case, iter_count)
        hf = hostsim.frame_from_oracle(mp.oracle_frame(case, iter_count)[0])
        for shortcuts in (0, 1):
            hf.step_shortcuts = shortcuts
            img, st = hostsim.render("labyrinth", hf)
            where = (case, iter_count, shortcuts)
            assert np.array_equal(_bits(img), _bits(ref)), where + (int((_bits(img) != _bits(ref)).any(axis=2).sum()),)
            assert np.array_equal(st[..., 0], rst[..., 0]) and np.array_equal(st[..., 2], rst[..., 2]), where
            if shortcuts:
                assert (st[..., 1] <= rst[..., 1]).all(), where
            else:
                assert np.array_equal(st[..., 1], rst[..., 1]), where


def test_the_cases_end_rays_in_every_peeled_pass():
    """no case passes by seeing nothing, on the oracle alone: primary rays that end at sample 1, 2, 3 and 4, each by a hit, by the range and by the
    iteration limit, and rays that rewind after the fourth"""
    seen = mp.classify()
    for key, pixels in seen.items():
        assert pixels >= 50, (key, seen)


def test_the_other_cases_show_what_they_are_for():
    """the eye above the walls: with step shortcuts its rising rays end before any evaluation; the full frames: shadow rays that hit"""
    import hostsim

    _basis, _ref, rst, _tot = mp.reference("above_looking_up", 256)
    hf = hostsim.frame_from_oracle(mp.oracle_frame("above_looking_up", 256)[0])
    hf.step_shortcuts = 1
    _img, st = hostsim.render("labyrinth", hf)
    assert int(((st[..., 1] == 0) & (rst[..., 1] > 0)).sum()) > mp.W * mp.H // 2
    for case in ("sweep0", "sweep5", "sweep11", "near_wall"):
        assert int((mp.reference(case, 256)[2][..., 2] >= 2).sum()) > 100, case
    for case in ("on_floor", "below_floor", "inside_wall"):
        st = mp.reference(case, 256)[2]
        assert int((st[..., 2] >= 1).sum()) == mp.W * mp.H  # every primary ray is a hit

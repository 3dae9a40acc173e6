"""CPU tier: the whole pipeline with the labyrinth's once-per-ray rule (SceneLabyrinth::ray_bounds; RayBounds, sdfr_scene_traits.h) -- the host build of
the product's headers (tests/hostsim) against the oracle: pixels, rays and hits per pixel bit for bit, the evaluations equal where every step is
marched and no more than the oracle's with step shortcuts.  The frames: tests/range_clear_cases.py, every case with the iteration limits 1, 3,
100 and 256.  Then, on the oracle and the host build alone, what the cases are for: the band's pixels march in the oracle and not in the product,
and the descending misses under the band still march."""
import numpy as np
import pytest

import range_clear_cases as rc


def _bits(a):
    return a.view(np.uint32)


def _host(case, iter_count, shortcuts):
    import hostsim

    hf = hostsim.frame_from_oracle(rc.oracle_frame(case, iter_count)[0])
    hf.step_shortcuts = shortcuts
    return hostsim.render("labyrinth", hf)


@pytest.mark.parametrize("case", list(rc.CASES))
def test_host_pipeline_matches_the_oracle(case):
    for iter_count in rc.ITER_COUNTS:
        _basis, ref, rst, _tot = rc.reference(case, iter_count)
        for shortcuts in (0, 1):
            img, st = _host(case, iter_count, shortcuts)
            where = (case, iter_count, shortcuts)
            assert np.array_equal(_bits(img), _bits(ref)), where + (int((_bits(img) != _bits(ref)).any(axis=2).sum()),)
            assert np.array_equal(st[..., 0], rst[..., 0]) and np.array_equal(st[..., 2], rst[..., 2]), where
            if shortcuts:
                assert (st[..., 1] <= rst[..., 1]).all(), where
            else:
                assert np.array_equal(st[..., 1], rst[..., 1]), where


def test_the_wide_cases_hold_a_band_and_marching_misses_under_it():
    """per wide case at least 200 pixels in the band, which march in the oracle and not in the product; under the band, descending primary
    misses that still march, step for step as the oracle does: at least 200 over the wide cases together, some in each (from 30 high with a
    range of 100 a ray under the band misses only down to dir.y = -0.3, where it reaches the floor: two rows of the frame, 192 pixels)"""
    for iter_count in rc.ITER_COUNTS:
        marching = {}
        for case in [c for c in rc.CASES if rc.CASES[c][2]]:
            inside, _below, _maybe, just_below = rc.masks(case)
            rst = rc.reference(case, iter_count)[2]
            _img, st = _host(case, iter_count, 1)
            miss = (rst[..., 0] == 1) & (rst[..., 2] == 0)  # the primary ray alone, and no hit
            band = inside & (rst[..., 1] > 0)
            assert int(inside.sum()) >= 200 and np.array_equal(band, inside), (case, iter_count, int(inside.sum()), int(band.sum()))
            assert miss[inside].all() and (st[..., 1][inside] == 0).all(), (case, iter_count)
            marching[case] = int((just_below & miss & (st[..., 1] > 0)).sum())
            # no rule speaks for them
            assert np.array_equal(st[..., 1][just_below & miss], rst[..., 1][just_below & miss]), (case, iter_count)
        print(iter_count, marching)
        assert sum(marching.values()) >= 200 and min(marching.values()) > 0, (iter_count, marching)


def test_the_narrow_cases():
    """the benchmark's geometry with one row in the band, ended before its first evaluation, and with the band between two rows; between
    the walls: no band, and every descending primary miss marches as the oracle does"""
    inside, _below, _maybe, _just = rc.masks("bench_geometry_row")
    rst = rc.reference("bench_geometry_row", 256)[2]
    _img, st = _host("bench_geometry_row", 256, 1)
    assert int(inside.sum()) >= rc.W // 2, int(inside.sum())
    assert (rst[..., 1][inside] > 0).all() and (rst[..., 2][inside] == 0).all() and (st[..., 1][inside] == 0).all()
    assert not rc.masks("bench_geometry")[2].any()

    _inside, below, maybe, _just = rc.masks("between_walls")
    assert not maybe.any()
    rst = rc.reference("between_walls", 256)[2]
    _img, st = _host("between_walls", 256, 1)
    miss = below & (rst[..., 0] == 1) & (rst[..., 2] == 0)
    assert np.array_equal(st[..., 1][miss], rst[..., 1][miss])

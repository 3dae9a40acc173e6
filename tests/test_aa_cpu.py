"""CPU tier of sdfr_render_aa: the stage functions of sdfr_resolve.h, built for the host (tests/cpp/resolve_host.cpp) and run
sequentially over compact strip buffers, against the definition of include/sdfr.h restated in numpy (aa_util.pyramid) bit for bit --
on oracle-rendered supersampled frames and on a random buffer with denormals, infinities and NaN --, the half conversion against the
oracle's, the counter sums; the pass planner of sdfr_aa_plan.h over a sweep of heights, factors and budgets; the command line's --aa."""
import numpy as np
import pytest

import aa_util as au

SCENES = {"fast_sphere": 0.0, "labyrinth": 1.25}  # scene: time


def _budgets(factor, strips):
    """one strip per pass, two (the passes do not divide the strips evenly), everything in one pass"""
    return [au.budget_for(au.W, factor, n) for n in (1, 2, strips)]


@pytest.mark.parametrize("factor", au.FACTORS)
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_stage_functions_equal_the_definition(oracle, scene, factor):
    s, st, _tot = au.oracle_s(oracle, scene, SCENES[scene], au.W, au.H, factor)
    want = au.pyramid(s, factor)
    want_st = au.sum_stats(st, factor)
    assert want.shape == (au.H, au.W, 4) and np.isfinite(want).all()
    # the picture has edges: some pixels are neither all hit nor all miss, so the filter is doing something
    assert len(np.unique(want_st[..., 2])) > 2, "a flat picture: the case would show nothing"
    strips = au.plan(au.W, au.H, factor, 1)[0]
    for budget in _budgets(factor, strips):
        img, got_st = au.host_resolve(s, st, au.W, au.H, factor, budget, 0)
        assert au.same_bits(img, want), "%s x%d budget %d" % (scene, factor, budget)
        assert np.array_equal(got_st, want_st)
        img16, _ = au.host_resolve(s, None, au.W, au.H, factor, budget, 1)
        assert np.array_equal(img16.view(np.uint16), oracle.float_to_half(want)), "the 16F image is the fp32 result converted once"


def _random_frame(factor, seed):
    rng = np.random.default_rng(seed)
    h, w = au.H * factor, au.W * factor
    s = (rng.standard_normal((h, w, 4)) * np.exp(rng.uniform(-30, 30, (h, w, 4)))).astype(np.float32)
    u = s.view(np.uint32)
    pick = rng.random((h, w, 4))
    u[pick < 0.05] = rng.integers(1, 1 << 23, int((pick < 0.05).sum()), dtype=np.uint32)  # denormals
    u[(pick >= 0.05) & (pick < 0.06)] = 0x7F800000  # +inf
    u[(pick >= 0.06) & (pick < 0.07)] = 0xFF800000  # -inf
    u[(pick >= 0.07) & (pick < 0.08)] = 0x7FC00000  # NaN
    u[(pick >= 0.08) & (pick < 0.10)] = rng.integers(0x47000000, 0x47900000, int(((pick >= 0.08) & (pick < 0.10)).sum()), dtype=np.uint32)  # around the largest half
    u[(pick >= 0.10) & (pick < 0.14)] = rng.integers(0x32000000, 0x39000000, int(((pick >= 0.10) & (pick < 0.14)).sum()), dtype=np.uint32)  # halves' denormal range
    st = rng.integers(0, 1 << 20, (h, w, 3), dtype=np.uint32)
    return s, st


@pytest.mark.parametrize("factor", au.FACTORS)
def test_stage_functions_on_unusual_values(oracle, factor):
    s, st = _random_frame(factor, 20 + factor)
    want = au.pyramid(s, factor)
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
    strips = au.plan(au.W, au.H, factor, 1)[0]
    for budget in _budgets(factor, strips):
        img, got_st = au.host_resolve(s, st, au.W, au.H, factor, budget, 0)
        assert au.same_bits_or_nan(img, want)  # (bit for bit; only a NaN may be another NaN: aa_util.same_bits_or_nan says why)
        assert np.array_equal(got_st, au.sum_stats(st, factor))
        img16, _ = au.host_resolve(s, None, au.W, au.H, factor, budget, 1)
        assert au.same_bits_or_nan(img16, oracle.float_to_half(want).view(np.float16))


def test_half_conversion_equals_the_oracles(oracle):
    rng = np.random.default_rng(5)
    u = np.concatenate([rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32),
                        np.arange(0x32F00000, 0x33100000, 4099, dtype=np.uint32),  # around half the smallest denormal half
                        np.arange(0x387F0000, 0x38810000, 257, dtype=np.uint32),   # around the smallest normal half
                        np.arange(0x477F0000, 0x47810000, 61, dtype=np.uint32),    # around the largest half
                        np.array([0, 0x80000000, 0x33000000, 0x33000001, 0x477FEFFF, 0x477FF000, 0x7F800000, 0xFF800000, 0x7F800001, 0xFFC12345], np.uint32)])
    # ties: exactly between two neighbouring halves of both parities, normal (2^0 ..) and denormal (2^-20 ..)
    ties = np.concatenate([0x3F800000 + (np.arange(64, dtype=np.uint32) << 13) + 0x1000, 0x35800000 + (np.arange(8, dtype=np.uint32) << 20) + 0x80000])
    u = np.concatenate([u, ties.astype(np.uint32), ties.astype(np.uint32) | 0x80000000])
    f = u.view(np.float32)
    got, want = au.host_half(f), oracle.float_to_half(f)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%d differ, first: %08x -> %04x, oracle %04x" % (len(bad), u[bad[0]], got[bad[0]], want[bad[0]])
    assert (want[-len(ties):] & 0x7FFF != 0).all()


def test_planner_covers_every_row_once_with_the_fewest_passes():
    width = 5
    checked = 0
    for factor in (1, 2, 4, 8):
        per_strip = au.STRIP_ROWS // factor
        for height in range(1, 41):
            strips = -(-factor * height // au.STRIP_ROWS)
            for n in sorted({1, 2, 3, 5, strips - 1, strips, strips + 3} - {0, -1}):
                for slack in (0, 7):  # a budget between two strip counts holds the lower one
                    budget = au.budget_for(width, factor, n) + slack
                    p = au.host_plan(width, height, factor, budget)
                    want_strips, want_passes, want_spp = au.plan(width, height, factor, budget)
                    assert (p["strips"], p["passes"], p["strips_per_pass"]) == (want_strips, want_passes, want_spp), (factor, height, n)
                    assert p["s_width"] == factor * width and p["s_height"] == factor * height and p["rows_per_strip"] == per_strip
                    assert p["pass_pixels"] == p["strips_per_pass"] * au.STRIP_ROWS * p["s_width"]
                    # P is minimal: the buffer fits the budget (or is the one strip a pass must hold), and with one pass fewer it would not
                    strip_bytes = au.STRIP_ROWS * p["s_width"] * 16
                    assert p["strips_per_pass"] * strip_bytes <= budget or p["strips_per_pass"] == 1
                    if p["passes"] > 1:
                        assert -(-strips // (p["passes"] - 1)) * strip_bytes > budget
                    produced = np.zeros(height, np.int32)
                    total_strips = 0
                    for pass_ in range(p["passes"]):
                        count, rows = au.host_pass_rows(width, height, factor, budget, pass_, p["strips_per_pass"])
                        total_strips += count
                        for l, (row0, n_rows) in enumerate(rows):
                            assert 0 <= n_rows <= per_strip and row0 + n_rows <= height  # no row >= H
                            assert (n_rows > 0) == (l < count)
                            if n_rows:
                                assert row0 == (l * p["passes"] + pass_) * per_strip
                            produced[row0:row0 + n_rows] += 1
                    assert total_strips == strips and (produced == 1).all(), (factor, height, n)
                    checked += 1
    assert checked > 1500
    # the sizes that matter in practice: 3840 x 2160 at 4 x 4 under 256 MiB and under the default, 1 GiB
    p = au.host_plan(3840, 2160, 4, 256 << 20)
    assert (p["strips"], p["passes"], p["strips_per_pass"]) == (1080, 8, 135)
    p = au.host_plan(3840, 2160, 4, 1 << 30)
    assert (p["strips"], p["passes"], p["strips_per_pass"]) == (1080, 2, 540)


def test_cli_aa_option():
    from sdf_playground_amd import cli

    ap = cli.make_parser()
    with pytest.raises(SystemExit):
        ap.parse_args(["--scene", "lense", "--aa", "3"])
    assert ap.parse_args(["--scene", "lense"]).aa == 1
    assert [ap.parse_args(["--scene", "lense", "--aa", str(k)]).aa for k in (1, 2, 4, 8)] == [1, 2, 4, 8]

    class Recorder:
        def __init__(self):
            self.calls = []

        def render(self, *a, **kw):
            self.calls.append(("render", a, kw))

        def renderAA(self, *a, **kw):
            self.calls.append(("renderAA", a, kw))

    r = Recorder()
    assert cli.render_call(r, 1) == r.render  # --aa 1 is today's path: render itself, not renderAA with a factor of 1
    cli.render_call(r, 4)("cam", 64, 40, fmt=1)
    assert r.calls == [("renderAA", ("cam", 64, 40), {"factor": 4, "fmt": 1})]

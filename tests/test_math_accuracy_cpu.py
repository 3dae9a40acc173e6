"""CPU tier: the deterministic elementary functions against true values.  Every frame test is "kernels = oracle, bit for bit"; this
file says how far that shared arithmetic (sdf_playground_amd/csrc/sdfr_math.h, host build; oracle/detmath.h bit-equal beside it) is
from sin, cos, atan2, exp2, log2 and pow themselves.  tests/cpp/math_accuracy_host.cpp sweeps the functions against libm in double
(tests/math_accuracy_util.py lists the ranges); tests/golden/math_accuracy.json records, per binade of the argument, the largest
error in ulps of the true value, the largest absolute error and the largest |result|, each with its argument.  The figures are
written as measured; the two stated conditions -- on |x| <= 2^16 sin1 and cos1 stay within [-1, 1] and within 3e-7 of the truth --
are asserted on every float of that domain.  The recorded worst cases are checked against mpmath at 60 digits, so libm, the
yardstick, is itself checked."""
import numpy as np
import pytest

import math_accuracy_util as mau


@pytest.fixture(scope="module")
def swept():
    return mau.sweep()


@pytest.fixture(scope="module")
def table():
    return mau.load()


def test_no_binade_exceeds_its_recorded_figure(swept, table):
    assert table["sweep"]["stride"] == mau.STRIDE and table["sweep"]["far_stride"] == mau.FAR_STRIDE
    failed = []
    for f in mau.ROW_FUNCTIONS:
        recorded = table["functions"][f]["rows"]
        assert sorted(swept[f]) == sorted(recorded), f
        for key, row in swept[f].items():
            rec = recorded[key]
            assert row["n"] == rec["n"], (f, key)  # the same arguments
            ok = (row["ulp"] <= rec["ulp"] + mau.ULP_SLACK and row["abs"] <= rec["abs"] + 2.0 ** -52 * max(1.0, rec["max_abs_result"]) and
                  row["max_abs_result"] <= rec["max_abs_result"] and row["nonfinite"] <= rec["nonfinite"] and row["tiny"] == rec["tiny"])
            if not ok:
                failed.append("%s %s: measured %r, recorded %r" % (f, key, row, rec))
    for f, top in mau.summary(swept).items():
        print("%-28s %s" % (f, ", ".join("%s %.9g" % kv for kv in top.items())))
    assert not failed, "\n".join(failed[:10])


def test_identities_hold_bit_for_bit_on_the_whole_sweep(swept):
    """sincos1 = (sin1, cos1), sin1(-x) = -sin1(x), cos1(-x) = cos1(x), sincos1_small = sincos1 on |x| <= 0.75, atan21(-y, 1) = -atan21(y, 1),
    atan1(y) = atan21(y, 1): counted by the sweep at every argument it visits; and oracle/detmath.h gives the product's bits on every
    251st of them, so the table describes both sides"""
    for f in mau.ROW_FUNCTIONS:
        assert sum(r["broken"] for r in swept[f].values()) == 0, f
        assert sum(r["differ"] for r in swept[f].values()) == 0, f
        assert sum(r["compared"] for r in swept[f].values()) > 60000, f
    # the one argument the sweep leaves out of sin's symmetry: sin1(-0) is +0 (the reduction's fma(-k, c, x) gives +0 for k = x = -0)
    z = np.array([0.0, -0.0], np.float32)
    assert mau.bits(mau.evaluate("sin1", z)).tolist() == [0, 0] and mau.bits(mau.evaluate("sincos1_small.x", z)).tolist() == [0, 0]
    assert mau.bits(mau.evaluate("cos1", z)).tolist() == [0x3F800000] * 2


def test_stated_domain_of_sin_and_cos(swept):
    """|x| <= 2^16: |result| <= 1 and absolute error < 3e-7, on every float of [2^-14, 2^16] and the edges and samples below"""
    for f in ("sin1", "cos1"):
        rows = [r for k, r in swept[f].items() if mau.in_domain(k)]
        assert sum(r["n"] for r in rows) > 30 * 2 ** 23
        assert max(r["max_abs_result"] for r in rows) <= 1.0, f
        assert max(r["abs"] for r in rows) < mau.ABS_BOUND, f
        assert all(r["nonfinite"] == 0 for r in rows), f
        edge = np.array([mau.SINCOS_DOMAIN, -mau.SINCOS_DOMAIN], np.float32)  # the domain's last float lies in the first binade beyond
        v = mau.evaluate(f, edge)
        assert (np.abs(v) <= 1).all() and (np.abs(v - mau.truth(f, edge)) < mau.ABS_BOUND).all()


def test_beyond_2_to_the_24_the_reduction_no_longer_reduces():
    """what DESIGN.md 8 says of arguments far outside the domain: results outside [-1, 1], infinities and NaN for finite arguments"""
    x = np.array([1e10, 1e20, 3e38], np.float32)
    s, c = mau.evaluate("sin1", x), mau.evaluate("cos1", x)
    assert abs(s[0]) > 1e15 and np.isinf(s[1]) and np.isnan(c[2])


def test_recorded_worst_cases_agree_with_mpmath(table):
    """each row's worst argument, recomputed against mpmath at 60 digits, gives the recorded ulp figure to 0.01 ulp (and the
    absolute figure of sin1 and cos1, which the stated condition rests on, to one part in 10^6 and the rounding of a double truth)"""
    import mpmath as mp

    mp.mp.dps = 60
    fns = {"sin1": lambda a: mp.sin(a[0]), "cos1": lambda a: mp.cos(a[0]), "atan21": lambda a: mp.atan2(a[0], a[1]), "atan21_pairs": lambda a: mp.atan2(a[0], a[1]),
           "exp21": lambda a: mp.power(2, a[0]), "log21": lambda a: mp.log(a[0], 2), "pow1": lambda a: mp.power(a[0], a[1])}
    checked = 0
    for f in mau.ROW_FUNCTIONS:
        what = f.replace("_pairs", "")
        for key, row in table["functions"][f]["rows"].items():
            for figure, at in (("ulp", "ulp_at"), ("abs", "abs_at")):
                if row[figure] == 0 or (figure == "abs" and f not in ("sin1", "cos1")):
                    continue
                args = mau.from_hex(row[at])
                v = mau.evaluate(what, args[:1], args[1:] or None)[0]
                t = fns[f]([mp.mpf(float(a)) for a in args])
                d = abs(mp.mpf(float(v)) - t)
                if figure == "ulp":
                    got = d / mp.ldexp(1, mp.frexp(abs(t))[1] - 1 - 23)
                    assert abs(got - row["ulp"]) < 0.01, (f, key, row[at], float(got), row["ulp"])
                else:
                    assert abs(d - row["abs"]) <= 1e-6 * row["abs"] + 2.0 ** -52 * abs(t), (f, key, row[at], float(d), row["abs"])  # (the double truth's own rounding)
                checked += 1
    assert checked > 300


def _specials():
    u = np.array([0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x7F7FFFFF, 0x7F800000], np.uint32)  # 0, denormals, FLT_MIN, 1, FLT_MAX, inf
    return np.concatenate([u, u | np.uint32(0x80000000)]).view(np.float32)


def test_atan21_on_the_axes_zeros_denormals_and_infinities(table):
    """every pair of +-{0, denormals, FLT_MIN, 1, FLT_MAX, inf}: the product's bits are the oracle's, and the value is atan2's within the
    recorded figure, but for what atan21 defines otherwise: atan21(+-0, +-0) = +0; a zero y counts as +0 (the result is +0 or +pi, never
    -0 or -pi); an infinity over an infinity is NaN"""
    s = _specials()
    y, x = [a.ravel() for a in np.meshgrid(s, s, indexing="ij")]
    v, t = mau.evaluate("atan21", y, x), mau.truth("atan21", y, x)
    assert np.array_equal(mau.bits(v), mau.bits(mau.evaluate(102, y, x)))
    both_inf = np.isinf(y) & np.isinf(x)
    assert np.isnan(v[both_inf]).all() and not np.isnan(v[~both_inf]).any()
    zero_y = y == 0
    want = np.where(np.signbit(x) & (x != 0), np.float32(np.pi), np.float32(0.0))[zero_y]
    assert np.array_equal(mau.bits(v[zero_y]), mau.bits(want))
    rest = ~both_inf & ~zero_y
    ulps, _, scored = mau.errors(v[rest], t[rest])
    worst = max(r["ulp"] for r in table["functions"]["atan21_pairs"]["rows"].values())
    assert scored.all() and np.nanmax(ulps) <= worst and (np.signbit(v[rest]) == np.signbit(t[rest])).all()


def test_exp21_and_log21_at_their_thresholds():
    f32 = np.float32
    x = np.array([0.0, -0.0, 128.0, np.nextafter(f32(128), f32(0)), -126.0, np.nextafter(f32(-126), f32(-200)), -149.0, -150.0, np.inf, -np.inf, np.nan], f32)
    v = mau.evaluate("exp21", x)
    assert np.array_equal(mau.bits(v[:-1]), mau.bits(mau.evaluate(103, x[:-1]))) and np.isnan(v[-1])
    assert v[0] == 1 and v[1] == 1 and np.isinf(v[2]) and v[3] < np.inf and abs(float(v[3]) / 2.0 ** float(x[3]) - 1) < 2.0 ** -22
    assert v[4] == f32(2.0 ** -126)  # the last argument with a result: below -126 exp21 is 0, where exp2 is a denormal (absolute error <= 2^-126)
    assert (v[5:8] == 0).all() and np.isinf(v[8]) and v[9] == 0
    x = np.array([0.0, -0.0, -1.0, np.inf, np.nan, 1.0], f32)
    v = mau.evaluate("log21", x)
    assert v[0] == -np.inf and v[1] == -np.inf and np.isnan(v[2]) and v[3] == np.inf and np.isnan(v[4]) and mau.bits(v[5:])[0] == 0
    assert mau.same(v, mau.evaluate(104, x)).all()


# ---- the GPU tier's scene, points and checks, run on the CPU first (tests/test_gpu_math_accuracy.py runs them on the device) --------
MODES = [False, True]


@pytest.mark.parametrize("fast_math", MODES, ids=["ieee", "fast"])
def test_accuracy_scene_compiles_for_gfx950(fast_math):
    import sdf_playground_amd as sp

    text = mau.scene_text(fast_math)
    assert (mau.TOKEN in text) == fast_math
    ok, log = sp.check_scene_source(text)
    assert ok, log


@pytest.fixture(scope="module")
def host_scene():
    """the accuracy scene through the host build of the query kernels, as the probes' CPU tier builds theirs"""
    import ctypes
    import os

    import cppbuild
    import query_util as qu

    gen = os.path.join(cppbuild.BUILD, "math_accuracy.scene.inc")
    assert cppbuild.scene_include(gen, mau.scene_text(False)) == []
    deps = [gen, os.path.join(cppbuild.HERE, "cpp", "host_common.h")] + cppbuild.csrc_headers()
    L = ctypes.CDLL(qu.build_lib("query_host_math_accuracy", "query_host.cpp", ["-I" + cppbuild.CSRC, '-DSDFR_HLSL_SCENE_FILE="%s"' % gen, "-DSDFR_SCENE_HAS_PREPARE=1"], deps))
    L.qh_points.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

    def values(case, x, y):
        U = qu.host_frame(qu.po.default_frame("fast_sphere", 8, 8, stime=float(mau.CASE_NAMES.index(case))))
        p = np.ascontiguousarray(np.stack([x, y, np.zeros_like(x)], 1), np.float32)
        d = np.empty(len(p), np.float32)
        assert L.qh_points(b"probe", ctypes.byref(U), len(p), p.ctypes.data, d.ctypes.data, None) == 0
        return d

    return values


@pytest.mark.parametrize("fast_math", MODES, ids=["ieee", "fast"])
def test_accuracy_scene_on_the_host_passes_what_the_device_must_pass(host_scene, table, fast_math):
    """the points are at most 32 768 per function and lie inside the swept ranges; the scene's expressions are the functions they are
    named after; and the negative control -- sin1 without the third Cody-Waite term -- is caught at large arguments of the domain"""
    for case in mau.CASE_NAMES:
        x, y = mau.device_points(case, table, fast_math)
        assert 1000 < len(x) <= mau.MAX_POINTS and x.dtype == np.float32 and y.dtype == np.float32, case
        v = host_scene(case, x, y)
        if case == "control_sin":
            assert mau.control_caught(table, v, x) > 0.99
            assert mau.same(v, mau.evaluate("sin1", x))[np.abs(x) < 0.75].all()  # (the same function where nothing is reduced)
        else:
            failures = mau.check_case(case, table, v, x, y)
            assert not failures, "\n".join(failures)

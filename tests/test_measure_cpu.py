"""CPU tier of sdfr_measure: the stage functions of sdf_playground_amd/csrc/sdfr_measure.h and the properties of sdfr_measure_plan.h, built for
the host (tests/cpp/measure_host.cpp), against the header's definition restated in numpy (tests/measure_util.py), every bit of every
column and of the reduced record equal, on span_util's slab ladder and a sphere; the reduction against the pairwise definition itself;
the invariants; the accuracy of the definition on an analytic sphere; the plan (the stand-alone program tests/cpp/measure_plan_host.cpp,
also under the address and undefined-behaviour sanitizers); the struct layouts; the command line's argument faults."""
import ctypes
import math
import re
import struct
import subprocess

import numpy as np
import pytest

import cppbuild
import measure_util as mu
import span_util as su

F, D = np.float32, np.float64
NAN, INF = float("nan"), float("inf")

# span_util's slab ladder along x (tests/test_span_cpu.py): dyadic centres and half-widths; NaN where 5 <= x <= 5.5
C = [-2.0, -0.75, 0.5, 1.25, 2.5, 3.75, 5.75]
R = [0.25, 0.125, 0.25, 0.0625, 0.5, 0.125, 0.25]
NAN_LO, NAN_HI = 5.0, 5.5
FIELD = su.slab_field(C, R, NAN_LO, NAN_HI)

# (what, grid, params): columns along +-x whose starts walk across the ladder
LADDER_CASES = [
    ("across the whole ladder, 19 x 5", mu.grid((-3.0, 0, 0), (0.5, 0, 0.01), (0.03125, 0.1, 0), (1, 0, 0), 19, 5), su.params(0.0625, 12.0)),
    ("starts inside, ends inside", mu.grid((-2.125, 0, 0), (0.3125, 0, 0), (0.01, 0.1, 0), (1, 0.1, 0), 23, 9), su.params(0.0625, 2.5)),
    ("out of steps", mu.grid((-3.0, 0, 0), (0.37, 0, 0), (0.05, 0.1, 0), (1, 0, 0), 9, 17), su.params(0.03125, 12.0, max_steps=7)),
    ("backwards, half speed, an iso", mu.grid((6.5, 0, 0), (-0.4, 0, 0), (0.07, 1, 0), (-0.5, 0, 0.2), 24, 3), su.params(0.1, 20.0, iso=0.05)),
    ("one column", mu.grid((0.125, 0, 0), (1, 0, 0), (0, 1, 0), (1, 0, 0), 1, 1), su.params(0.0625, 0.375)),
    ("a ragged tile, 7 x 5", mu.grid((-3.0, 0, 0), (1.25, 0, 0), (0.1, 1, 0), (1, 0, 0), 7, 5), su.params(0.0625, 12.0)),
    ("81 tiles, 72 x 65", mu.grid((-3.0, 0, 0), (0.125, 0, 0), (0.001, 1, 0), (1, 0, 0), 72, 65), su.params(0.0625, 3.0)),
    ("an empty region", mu.grid((-2.9, -5, 0), (0.01, 0, 0), (0, 0, 1), (0, 1, 0), 12, 9), su.params(0.0625, 10.0)),
    ("no direction: every column invalid", mu.grid((-3.0, 0, 0), (0.5, 0, 0), (0, 1, 0), (0, -0.0, 0), 9, 3), su.params(0.0625, 12.0)),
    ("a NaN direction: every column invalid", mu.grid((-3.0, 0, 0), (0.5, 0, 0), (0, 1, 0), (1, NAN, 0), 5, 5), su.params(0.0625, 12.0)),
    ("origins that overflow: columns past the second invalid", mu.grid((-3.0, 0, 0), (3e38, 0, 0), (0, 1, 0), (1, 0, 0), 5, 2), su.params(0.0625, 12.0)),
    ("through the NaN slab", mu.grid((4.5, 0, 0), (0.0625, 0, 0), (0, 1, 0), (1, 0, 0), 20, 2), su.params(0.0625, 1.75)),
]


@pytest.fixture(scope="module")
def ladder():
    """the restatement, once per case"""
    return [(what, g, p) + mu.measure(FIELD, g, p) for what, g, p in LADDER_CASES]


def test_host_text_equals_the_definition(ladder):
    seen = dict(hit=0, open=0, out_of_steps=0, invalid=0, spans=0, starts=0, ends=0)
    for what, g, p, want, want_col in ladder:
        got, col, extras = mu.host_measure_slabs(g, p, C, R, NAN_LO, NAN_HI)
        mu.assert_same_columns(what, col, want_col)
        S = want["summaries"]
        assert (extras[:, 0] == S["crossings"]).all(), what
        mu.assert_same_result(what, got, want)
        for k, name in (("hit", "columns_hit"), ("open", "columns_open"), ("out_of_steps", "columns_out_of_steps"), ("invalid", "columns_invalid"), ("spans", "spans")):
            seen[k] += want[name]
        seen["starts"] += int(((S["flags"] & su.STARTS_INSIDE) != 0).sum())
        seen["ends"] += int(((S["flags"] & su.ENDS_INSIDE) != 0).sum())
    assert seen["hit"] > 1000 and seen["out_of_steps"] > 100 and seen["invalid"] == 27 + 25 + 6 and seen["starts"] > 20 and seen["ends"] > 50, seen
    by = {what: want for what, _g, _p, want, _c in ladder}
    empty = by["an empty region"]
    assert (empty["columns_hit"], empty["hit_lo"], empty["hit_hi"], empty["spans"]) == (0, (12, 9), (-1, -1), 0) and empty["steps"] > 0
    assert np.isposinf(empty["t_lo"]) and np.isneginf(empty["t_hi"]) and not mu.bits64(empty["moments"]).any()  # ten times +0.0
    none = by["no direction: every column invalid"]
    assert none["columns_invalid"] == 27 and none["steps"] == 0 and not mu.bits64(none["moments"]).any()
    some = by["origins that overflow: columns past the second invalid"]
    assert some["columns_invalid"] == 6 and some["columns_hit"] == 2 and some["hit_hi"] == (0, 1)
    assert by["81 tiles, 72 x 65"]["passes"] == 2 and by["a ragged tile, 7 x 5"]["passes"] == 0
    assert by["through the NaN slab"]["columns_hit"] == 40


def test_designed_columns():
    """columns whose numbers can be worked out by hand (the rays of test_span_cpu.test_designed_rays)"""
    # starts inside the slab (0.25, 0.75) at 0.625 and leaves it at t = 0.125: m0 = 1/8, m1 = (1/2)(1/64), m2 = (1/512)/3
    got, col, _e = mu.host_measure_slabs(mu.grid((0.625, 0, 0), (1, 0, 0), (0, 1, 0), (1, 0, 0), 1, 1), su.params(0.0625, 0.5), C, R, NAN_LO, NAN_HI)
    c = col[0, 0]
    assert (c["m0"], c["m1"], c["m2"], c["spans"], c["flags"], c["valid"]) == (0.125, 0.5 * 0.015625, 0.001953125 / 3.0, 1, su.STARTS_INSIDE, 1)
    assert list(got.moments) == [c["m0"], 0, 0, c["m1"], 0, 0, c["m2"], 0, 0, 0] and (got.columns_hit, got.columns_open, got.t_lo, got.t_hi) == (1, 1, 0, 0.125)
    # the same column as (i, j) = (2, 1) of a grid whose other columns start far in front of the ladder: u = 2, v = 1
    g = mu.grid((0.625 - 2 * 4.0 - 16.0, -1.0, 0), (4.0, 0, 0), (16.0, 1.0, 0), (1, 0, 0), 3, 2)
    want, want_col = mu.measure(FIELD, g, su.params(0.0625, 0.5))
    got, col, _e = mu.host_measure_slabs(g, su.params(0.0625, 0.5), C, R, NAN_LO, NAN_HI)
    mu.assert_same_result("a column at (2, 1)", got, want)
    assert want["columns_hit"] == 1 and want["hit_lo"] == want["hit_hi"] == (2, 1)
    m0, m1, m2 = 0.125, 0.5 * 0.015625, 0.001953125 / 3.0
    assert list(got.moments) == [m0, 2 * m0, m0, m1, 4 * m0, m0, m2, 2 * m0, m1, 2 * m1]


# ---- the reduction: the pairwise definition itself is the reference ----------------------------------------------------------------
def pairwise_definition(values):
    """`values` (Python floats): group in runs of 64 by index, pad the last with +0.0, replace each run by its tree sum -- level by level
    x[m] = x[2m] + x[2m + 1] --, until one value remains; a single value is its own result"""
    values = list(values)
    while len(values) > 1:
        runs = []
        for r in range(0, len(values), 64):
            x = values[r:r + 64] + [0.0] * (64 - len(values[r:r + 64]))
            while len(x) > 1:
                x = [x[2 * m] + x[2 * m + 1] for m in range(len(x) // 2)]
            runs.append(x[0])
        values = runs
    return values[0]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096, 4097])
def test_reduction_is_the_pairwise_tree(n):
    rng = np.random.default_rng(1000 + n)
    rec = rng.standard_normal((n, 10)) * np.exp(rng.uniform(-20, 20, (n, 10)))  # mixed signs, forty orders of magnitude: the order matters
    rec[n // 2, :] = -0.0
    rec[:, 9] = -0.0  # a component of nothing but -0.0: padded with +0.0 the sum is +0.0, a single record keeps its -0.0
    want = np.array([pairwise_definition([float(x) for x in rec[:, c]]) for c in range(10)], D)
    got, passes = mu.host_reduce_records(rec)
    again, passes_numpy = mu.reduce_records(rec)
    assert (mu.bits64(got) == mu.bits64(want)).all() and (mu.bits64(again) == mu.bits64(want)).all(), n
    assert passes == passes_numpy == {1: 0, 63: 1, 64: 1, 65: 2, 4096: 2, 4097: 3}[n]
    assert math.copysign(1.0, want[9]) == (-1.0 if n in (1, 64, 4096) else 1.0)  # whole runs of -0.0 stay -0.0; a padded run does not
    if n > 64:
        assert (mu.bits64(want) != mu.bits64(np.sum(rec, 0))).any()  # (not np.sum's order)


def test_order_keys_keep_the_order():
    L = mu.host_lib()
    values = np.array([-INF, -3e38, -1.5, -1e-45, -0.0, 0.0, 1e-45, 0.5, 1.0, 3e38, INF], F)
    keys = [L.msh_order_key(float(v)) for v in values]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert [F(L.msh_order_value(k)).view(np.uint32) for k in keys] == [v.view(np.uint32) for v in values]


# ---- the properties ---------------------------------------------------------------------------------------------------------------
def _same_properties(got, want, what):
    for name in ("volume", "mass"):
        assert struct.pack("d", got[name]) == struct.pack("d", want[name]), (what, name, got[name], want[name])
    for name in ("centroid", "inertia"):
        assert struct.pack("%dd" % len(want[name]), *got[name]) == struct.pack("%dd" % len(want[name]), *want[name]), (what, name, got[name], want[name])


def test_properties_equal_their_restatement(ladder):
    tilted = mu.grid((0.3, -1.1, 2.7), (0.11, 0.02, -0.03), (0.01, 0.13, 0.04), (-0.2, 0.1, 0.7), 9, 17)
    for what, g, _p, want, _c in ladder:
        for grid_, density in ((g, 1.0), (tilted, 2.7e3)):
            _same_properties(mu.host_properties(grid_, want, density), mu.properties(grid_, want, density), what)
    zero = dict(moments=np.zeros(10))
    assert mu.host_properties(tilted, zero, 3.0) == mu.properties(tilted, zero, 3.0) == dict(volume=0.0, mass=0.0, centroid=(0.0,) * 3, inertia=(0.0,) * 6)
    # a unit cube as one column: volume 1, centroid its middle, inertia 1/6 about every axis
    cube = dict(moments=np.array([1.0, 0, 0, 0.5, 0, 0, 1 / 3.0, 0, 0, 0]))
    one = mu.properties(mu.grid((0.5, 0.5, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 1, 1), cube, 1.0)
    assert one["volume"] == 1.0 and one["centroid"] == (0.5, 0.5, 0.5)
    assert np.allclose(one["inertia"], (1 / 6.0, 1 / 6.0, 1 / 6.0, 0, 0, 0), atol=1e-15)
    # through the library's C ABI, which needs no GPU
    import sdf_playground_amd as sp

    res = sp.MeasureResult()
    res.moments[:] = [float(x) for x in cube["moments"]]
    props = sp.measureProperties(sp.MeasureGrid((ctypes.c_float * 3)(0.5, 0.5, 0), (ctypes.c_float * 3)(1, 0, 0), (ctypes.c_float * 3)(0, 1, 0), (ctypes.c_float * 3)(0, 0, 1), 1, 1), res, 1.0)
    _same_properties(props, one, "the C ABI")
    L = sp.load_library()
    assert L.sdfr_measure_properties(None, ctypes.byref(res), 1.0, ctypes.byref(sp.SolidProperties())) == -1
    with pytest.raises(sp.SdfrError):
        sp.measureProperties(sp.MeasureGrid(), res, NAN)


# ---- invariants -------------------------------------------------------------------------------------------------------------------
def test_invariants(ladder):
    for what, g, _p, want, col in ladder:
        flat = col.reshape(-1)
        # moments[0] is the tree sum of the columns' m0, laid out in tiles
        nu, nv = g["nu"], g["nv"]
        tu, tv = -(-nu // 8), -(-nv // 8)
        lanes = np.zeros((tv * 8, tu * 8), D)
        lanes[:nv, :nu] = col["m0"]
        tiles = mu.tree64(lanes.reshape(tv, 8, tu, 8).transpose(0, 2, 1, 3).reshape(tv * tu, 64))
        assert mu.bits64(pairwise_definition([float(x) for x in tiles])) == mu.bits64(want["moments"][0]), what
        S = want["summaries"]
        assert want["steps"] == int(flat["steps"].astype(np.int64).sum()) == int(S["steps"].astype(np.int64).sum()), what
        assert want["spans"] == int(flat["spans"].astype(np.int64).sum()) and want["crossings"] == int(S["crossings"].astype(np.int64).sum()), what
        assert want["columns_hit"] == int((flat["spans"] > 0).sum()) and want["columns_invalid"] == int((flat["valid"] != 1).sum()), what
        assert want["crossings"] == 2 * want["spans"] - int(((S["flags"] & 1) != 0).sum()) - int(((S["flags"] & 2) != 0).sum()), what
        # m0 is the fp64 sum of what sdfr_query_ray_spans sums in fp32
        assert np.allclose(flat["m0"], S["inside_length"], rtol=1e-5, atol=1e-6), what
        assert (flat["m0"] >= 0).all() and (flat["m1"] >= 0).all() and (flat["m2"] >= 0).all()


def test_a_grid_moved_by_whole_columns():
    """On dyadic data every sum is exact, whatever its order, so the algebra holds to the bit: the same columns seen from a grid whose
    origin lies a columns back along u (the extra columns see nothing) have i + a in place of i.  Faces, starts and min_step are dyadic,
    so every crossing is: a sample lands on a face, or u = d / min_step with min_step a power of two.  (m2 has a division by 3 and is
    not dyadic: moments[6] is left out.)"""
    p = su.params(0.0625, 0.25)
    for swap in (False, True):
        def make(x0, n):
            du, dv = (0.5, 0, 0), (0, 1.0, 0)
            return mu.grid((x0, 0, 0), dv if swap else du, du if swap else dv, (1, 0, 0), 3 if swap else n, n if swap else 3)
        a = 2
        near, far = make(-2.5, 13), make(-2.5 - a * 0.5, 13 + a)
        m, col = mu.measure(FIELD, near, p)
        M, COL = mu.measure(FIELD, far, p)
        got, _c, _e = mu.host_measure_slabs(far, p, C, R, NAN_LO, NAN_HI)
        mu.assert_same_result("moved", got, M)
        assert m["columns_hit"] == M["columns_hit"] > 6 and m["spans"] == M["spans"]
        extra = COL[:a, :] if swap else COL[:, :a]
        assert (extra["spans"] == 0).all()  # the columns added in front see nothing
        m, M = m["moments"], M["moments"]
        first, second, cross, along = ((2, 5, 7, 8) if swap else (1, 4, 7, 9))  # sum i m0, sum i^2 m0, sum i j m0, sum i m1
        other = 1 if swap else 2
        assert M[0] == m[0] and M[3] == m[3] and M[other] == m[other]
        assert M[first] == m[first] + a * m[0]
        assert M[second] == m[second] + 2 * a * m[first] + a * a * m[0]
        assert M[cross] == m[cross] + a * m[other]
        assert M[along] == m[along] + a * m[3]


# ---- accuracy of the definition on an analytic sphere -----------------------------------------------------------------------------
# The restatement against the closed forms 4/3 pi rho^3, the centre and 2/5 m rho^2, the sphere fully inside the box, min_step = cell / 2,
# sixteen seeded sub-cell offsets of the centre per resolution.  The worst values the restatement gave (measure_util.RECORDED_WORST), as
# relative errors of the volume and of I_zz and the centroid's distance in cells; asserted: twice that, since sixteen offsets sample the
# worst case thinly.
RECORDED_WORST = mu.RECORDED_WORST


def sphere_errors(ratio, seed=2024, offsets=16):
    cell = 1.0 / 16
    rho = ratio * cell
    rng = np.random.default_rng(seed + ratio)
    worst = [0.0, 0.0, 0.0]
    half = math.ceil(ratio) + 2  # cells from the box's middle to its faces: two cells of margin around the sphere
    for _ in range(offsets):
        centre = rng.uniform(-0.5, 0.5, 3) * cell
        g, depth = mu.box_grid([-half * cell] * 3, [half * cell] * 3, cell, "z")
        res, _col = mu.measure(mu.sphere_field(centre, rho), g, su.params(cell / 2, depth))
        assert res["columns_open"] == 0 and res["columns_out_of_steps"] == 0 and res["columns_invalid"] == 0
        props = mu.properties(g, res, 1.0)
        c32 = np.asarray(centre, F).astype(D)  # the field's centre is fp32
        volume = 4.0 / 3.0 * math.pi * float(F(rho)) ** 3
        worst[0] = max(worst[0], abs(props["volume"] - volume) / volume)
        worst[1] = max(worst[1], abs(props["inertia"][2] - 0.4 * volume * float(F(rho)) ** 2) / (0.4 * volume * float(F(rho)) ** 2))
        worst[2] = max(worst[2], float(np.linalg.norm(np.array(props["centroid"]) - c32)) / cell)
    return worst


@pytest.mark.parametrize("ratio", [8, 16, 32])
def test_sphere_accuracy(ratio):
    worst = sphere_errors(ratio)
    print("rho / cell = %d: worst relative error of the volume %.3e, of I_zz %.3e, centroid off by %.4f cells" % ((ratio,) + tuple(worst)))
    for got, recorded in zip(worst, RECORDED_WORST[ratio]):
        assert got <= 2 * recorded, (ratio, worst, RECORDED_WORST[ratio])


def test_host_text_on_a_sphere():
    cell = 1.0 / 16
    g, depth = mu.box_grid([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], cell, "z")
    centre, rho, p = (0.013, -0.021, 0.007), 0.8, su.params(cell / 2, depth)
    want, want_col = mu.measure(mu.sphere_field(centre, rho), g, p)
    got, col, _e = mu.host_measure_sphere(g, p, centre, rho)
    mu.assert_same_columns("sphere", col, want_col)
    mu.assert_same_result("sphere", got, want)
    assert want["passes"] == 1 and want["columns_hit"] > 500 and want["spans"] == want["columns_hit"]
    # ... and a tilted grid: du, dv, dw not along the axes, |dw| != 1
    tilted = mu.grid((-1.8, -1.7, -1.3), (0.09, 0.02, -0.01), (-0.015, 0.1, 0.02), (0.21, 0.26, 1.3), 31, 21)
    p = su.params(0.03, 2.0)
    want, want_col = mu.measure(mu.sphere_field(centre, rho), tilted, p)
    got, col, _e = mu.host_measure_sphere(tilted, p, centre, rho)
    mu.assert_same_columns("tilted", col, want_col)
    mu.assert_same_result("tilted", got, want)
    props = mu.properties(tilted, want, 1.0)
    volume = 4.0 / 3.0 * math.pi * 0.8 ** 3
    assert want["columns_open"] == 0 and abs(props["volume"] - volume) / volume < 0.02 and np.linalg.norm(np.array(props["centroid"]) - centre) < 0.02
    _same_properties(mu.host_properties(tilted, want, 1.0), props, "tilted")


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
INVALID = -1  # SDFR_ERR_INVALID_ARGUMENT
NULL_POINTER, BAD_ON_HOST, BAD_GRID, BAD_PARAMS = "null pointer", "on_host must be 0 or 1", "bad measure grid", "bad span parameters"


def _exe(name, flags):
    return cppbuild.plan_program("measure_plan_host", name, flags)


@pytest.fixture(scope="module")
def exe():
    return _exe("measure_plan_host", [])


def request(grid=True, origin=(0.5, -1, 2), du=(0.1, 0, 0), dv=(0, 0.1, 0), dw=(0, 0, 1), nu=9, nv=17, params=True, t_max=0.0, min_step=0.01, iso=0.0,
            max_steps=256, max_spans=0, out=True, columns=False, on_host=1, range_=80.0):
    return dict(grid=grid, origin=origin, du=du, dv=dv, dw=dw, nu=nu, nv=nv, params=params, t_max=t_max, min_step=min_step, iso=iso, max_steps=max_steps,
                max_spans=max_spans, out=out, columns=columns, on_host=on_host, range_=range_)


def line_of(r):
    f = lambda v: repr(float(v))  # noqa: E731
    return " ".join([str(int(r["grid"]))] + [f(x) for k in ("origin", "du", "dv", "dw") for x in r[k]] + [str(r["nu"]), str(r["nv"]), str(int(r["params"])),
                    f(r["t_max"]), f(r["min_step"]), f(r["iso"]), str(r["max_steps"]), str(r["max_spans"]), str(int(r["out"])), str(int(r["columns"])),
                    str(r["on_host"]), f(r["range_"])])


def f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def f32_bits(v):
    return struct.unpack("I", struct.pack("f", v))[0]


def rules(r):
    """the issue's rules, in the order their errors win -> (status, text, plan or None)"""
    if not r["grid"] or not r["params"] or not r["out"]:
        return INVALID, NULL_POINTER, None
    if r["on_host"] not in (0, 1):
        return INVALID, BAD_ON_HOST, None
    vectors = [[f32(x) for x in r[k]] for k in ("origin", "du", "dv", "dw")]
    if not (all(math.isfinite(x) for v in vectors for x in v) and all(any(x != 0 for x in v) for v in vectors[1:])
            and 1 <= r["nu"] <= 8192 and 1 <= r["nv"] <= 8192 and r["nu"] * r["nv"] <= 1 << 24):
        return INVALID, BAD_GRID, None
    t_max, min_step, iso = f32(r["t_max"]), f32(r["min_step"]), f32(r["iso"])
    if not (math.isfinite(t_max) and t_max >= 0 and math.isfinite(min_step) and min_step > 0 and math.isfinite(iso)
            and 1 <= r["max_steps"] <= 1 << 20 and r["max_spans"] == 0):
        return INVALID, BAD_PARAMS, None
    tiles = -(-r["nu"] // 8) * -(-r["nv"] // 8)
    passes, n = [], tiles
    while n > 1:
        passes.append(n)
        n = -(-n // 64)
    return 0, "", dict(t_max=r["range_"] if t_max == 0 else r["t_max"], blocks=tiles, passes=passes, result_in=len(passes) % 2,
                       work=(tiles * 80, -(-tiles // 64) * 80, 128 * (2 + 13 * 16)), column_bytes=r["nu"] * r["nv"] * 40 if r["columns"] else 0)


def expected_line(r):
    status, text, plan = rules(r)
    out = "%d;%s" % (status, text)
    if plan:
        out += ";%d %d %08x %08x %08x %d %d;%d;%d" % (r["nu"], r["nv"], f32_bits(plan["t_max"]), f32_bits(r["min_step"]), f32_bits(r["iso"]), r["max_steps"],
                                                      int(r["columns"]), plan["blocks"], len(plan["passes"]))
        out += "".join(" %d" % n for n in plan["passes"])
        out += ";%d;%d %d %d;%d" % ((plan["result_in"],) + plan["work"] + (plan["column_bytes"],))
    return out


def run(exe, reqs):
    text = "".join(line_of(r) + "\n" for r in reqs)
    lines = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(reqs)
    return lines


BAD_GRIDS = [dict(origin=(NAN, 0, 0)), dict(origin=(0, INF, 0)), dict(du=(0, 0, 0)), dict(du=(0, -0.0, 0)), dict(du=(NAN, 1, 0)), dict(dv=(0, 0, 0)), dict(dv=(0, 0, -INF)),
             dict(dw=(0, 0, 0)), dict(dw=(0, NAN, 1)), dict(nu=0), dict(nv=0), dict(nu=-4), dict(nu=8193), dict(nv=8193), dict(nu=8192, nv=2049), dict(nu=4097, nv=4096)]
BAD_PARAMETERS = [dict(t_max=NAN), dict(t_max=INF), dict(t_max=-0.5), dict(min_step=0.0), dict(min_step=-1.0), dict(min_step=NAN), dict(min_step=INF),
                  dict(iso=NAN), dict(iso=-INF), dict(max_steps=0), dict(max_steps=(1 << 20) + 1), dict(max_steps=-3), dict(max_spans=-1), dict(max_spans=1),
                  dict(max_spans=4), dict(max_spans=65)]


def fault_cases():
    cases = [("bad grid %r" % (b,), request(**b), BAD_GRID) for b in BAD_GRIDS]
    cases += [("bad parameters %r" % (b,), request(columns=c, **b), BAD_PARAMS) for b in BAD_PARAMETERS for c in (False, True)]
    cases += [("null grid", request(grid=False), NULL_POINTER), ("null params", request(params=False), NULL_POINTER), ("null out", request(out=False), NULL_POINTER),
              ("on_host 2", request(on_host=2), BAD_ON_HOST), ("on_host -1", request(on_host=-1), BAD_ON_HOST)]
    # two faults at once, one request per adjacent pair of checks: the earlier text wins
    cases += [("null out + on_host 2", request(out=False, on_host=2), NULL_POINTER), ("null grid + bad parameters", request(grid=False, min_step=0.0), NULL_POINTER),
              ("on_host 2 + bad grid", request(on_host=2, nu=0), BAD_ON_HOST), ("bad grid + bad parameters", request(dw=(0, 0, 0), max_spans=3), BAD_GRID),
              ("on_host 2 + bad parameters", request(on_host=-7, max_steps=0), BAD_ON_HOST)]
    return cases


def good_cases():
    sizes = [(1, 1), (7, 5), (8, 8), (9, 17), (72, 65), (520, 512), (8192, 2048), (2048, 8192), (4097, 4095), (1, 8192), (4096, 4096)]
    cases = [("%d x %d" % s, request(nu=s[0], nv=s[1], columns=c, on_host=h)) for s in sizes for c, h in ((False, 1), (True, 1), (True, 0), (False, 0))]
    cases += [("t_max given", request(t_max=2.5)), ("the limits", request(max_steps=1 << 20, iso=-3.5, min_step=1e-30)), ("tilted", request(du=(0.1, 0.2, -0.3), dv=(-1e-3, 5, 0), dw=(3, 3, 3)))]
    return cases


def test_argument_faults(exe):
    cases = fault_cases()
    got = run(exe, [r for _what, r, _text in cases])
    for (what, r, text), line in zip(cases, got):
        assert line == "%d;%s" % (INVALID, text), what
        assert line == expected_line(r), what
    assert {text for _w, _r, text in cases} == {NULL_POINTER, BAD_ON_HOST, BAD_GRID, BAD_PARAMS}


def test_good_requests(exe):
    cases = good_cases()
    got = run(exe, [r for _what, r in cases])
    by_name = {}
    for (what, r), line in zip(cases, got):
        assert line.startswith("0;;"), (what, line)
        assert line == expected_line(r), what
        by_name.setdefault(what, line)
    # blocks; passes and the records each reads; where the result ends up; the workspace; the bytes of columns
    assert by_name["1 x 1"].split(";")[3:] == ["1", "0", "0", "80 80 26880", "0"]
    assert by_name["7 x 5"].split(";")[3:5] == ["1", "0"] and by_name["8 x 8"].split(";")[3:5] == ["1", "0"]
    assert by_name["9 x 17"].split(";")[3:] == ["6", "1 6", "1", "480 80 26880", "0"]
    assert by_name["72 x 65"].split(";")[3:] == ["81", "2 81 2", "0", "6480 160 26880", "0"]
    assert by_name["520 x 512"].split(";")[3:6] == ["4160", "3 4160 65 2", "1"]
    assert by_name["8192 x 2048"].split(";")[3:6] == ["262144", "3 262144 4096 64", "1"]
    assert by_name["4097 x 4095"].split(";")[3:6] == ["262656", "4 262656 4104 65 2", "0"]  # past 2^18 tiles: a fourth pass
    assert by_name["t_max given"].split(";")[2].split()[2] == "%08x" % f32_bits(2.5) and by_name["1 x 1"].split(";")[2].split()[2] == "%08x" % f32_bits(80.0)
    assert got[1].split(";")[-1] == "40" and got[2].split(";")[-1] == "40" and got[3].split(";")[-1] == "0"


def test_under_sanitizers(exe):
    """the same program built with the address and undefined-behaviour sanitizers, over every request above: the same answers"""
    reqs = [r for _w, r, _t in fault_cases()] + [r for _w, r in good_cases()]
    checked = _exe("measure_plan_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert run(checked, reqs) == run(exe, reqs)


# ---- layouts and the command line -------------------------------------------------------------------------------------------------
def test_struct_layouts():
    import sdf_playground_amd as sp

    L = mu.host_lib()
    assert [L.msh_sizes(k) for k in range(9)] == [56, 40, 160, 88, 96, 26880, 80, 136, 152]
    for S in (sp.MeasureGrid, mu.HostGrid):
        assert ctypes.sizeof(S) == 56 and [(n, getattr(S, n).offset) for n, _t in S._fields_] == [("origin", 0), ("du", 12), ("dv", 24), ("dw", 36), ("nu", 48), ("nv", 52)]
    for S in (sp.MeasureResult, mu.HostResult):
        assert ctypes.sizeof(S) == 160
        assert [(n, getattr(S, n).offset) for n, _t in S._fields_] == [("moments", 0), ("columns_hit", 80), ("columns_open", 88), ("columns_out_of_steps", 96),
                                                                      ("columns_invalid", 104), ("steps", 112), ("spans", 120), ("crossings", 128), ("hit_lo", 136),
                                                                      ("hit_hi", 144), ("t_lo", 152), ("t_hi", 156)]
    for S in (sp.SolidProperties, mu.HostProperties):
        assert ctypes.sizeof(S) == 88 and [(n, getattr(S, n).offset) for n, _t in S._fields_] == [("volume", 0), ("mass", 8), ("centroid", 16), ("inertia", 40)]
    for dt in (sp.MEASURE_COLUMN_DTYPE, mu.COLUMN_DTYPE):
        assert dt.itemsize == 40
        assert [(n, dt.fields[n][1], dt.fields[n][0].str) for n in dt.names] == [("m0", 0, "<f8"), ("m1", 8, "<f8"), ("m2", 16, "<f8"), ("spans", 24, "<u4"), ("steps", 28, "<u4"),
                                                                                 ("flags", 32, "<u4"), ("valid", 36, "<i4")]
    for symbol in ("sdfr_measure", "sdfr_measure_properties"):
        assert symbol in sp.EXPORTED_SYMBOLS
    header = open(cppbuild.ROOT + "/include/sdfr.h").read()

    def fields(name):
        body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return re.findall(r"\b(u?int32_t|int64_t|float|double)\s+([a-z_0-9, \[\]]+);", body)

    assert fields("sdfr_measure_grid") == [("float", "origin[3]"), ("float", "du[3], dv[3]"), ("float", "dw[3]"), ("int32_t", "nu, nv")]
    assert fields("sdfr_measure_result") == [("double", "moments[10]"), ("int64_t", "columns_hit, columns_open, columns_out_of_steps, columns_invalid"),
                                             ("int64_t", "steps, spans, crossings"), ("int32_t", "hit_lo[2], hit_hi[2]"), ("float", "t_lo, t_hi")]
    assert fields("sdfr_measure_column") == [("double", "m0, m1, m2"), ("uint32_t", "spans, steps, flags"), ("int32_t", "valid")]
    assert fields("sdfr_solid_properties") == [("double", "volume, mass"), ("double", "centroid[3]"), ("double", "inertia[6]")]


def test_measure_grid_of_a_box():
    import sdf_playground_amd as sp

    for axis in "xyz":
        g, depth = sp.measureGrid((-1.0, 0.0, 2.0), (1.0, 0.5, 2.75), 0.125, axis)
        want, want_depth = mu.box_grid((-1.0, 0.0, 2.0), (1.0, 0.5, 2.75), 0.125, axis)
        assert depth == want_depth and (g.nu, g.nv) == (want["nu"], want["nv"])
        for name in ("origin", "du", "dv", "dw"):
            assert list(getattr(g, name)) == list(want[name]), (axis, name)
    g, depth = sp.measureGrid((-1.0, 0.0, 2.0), (1.0, 0.5, 2.75), 0.125, "z")
    assert (g.nu, g.nv, depth) == (16, 4, 0.75) and list(g.origin) == [-0.9375, 0.0625, 2.0] and list(g.dw) == [0, 0, 1]
    g, depth = sp.measureGrid((-1.0, 0.0, 2.0), (1.0, 0.5, 2.75), 0.125, "x")
    assert (g.nu, g.nv, depth) == (4, 6, 2.0) and list(g.du) == [0, 0.125, 0] and list(g.dv) == [0, 0, 0.125] and list(g.dw) == [1, 0, 0]
    for bad in (dict(cell=0.0), dict(cell=-1.0), dict(box_hi=(1.0, 0.0, 2.75)), dict(axis="w"), dict(cell=1e-5)):
        args = dict(box_lo=(-1.0, 0.0, 2.0), box_hi=(1.0, 0.5, 2.75), cell=0.125, axis="z")
        args.update(bad)
        with pytest.raises(ValueError):
            sp.measureGrid(**args)


def test_cli_measure_arguments(capsys):
    from sdf_playground_amd import cli

    def refused(args, text):
        with pytest.raises(SystemExit) as e:
            cli.main(args)
        assert e.value.code == 2 and text in capsys.readouterr().err, args

    scene = ["--scene", "fast_sphere"]
    box = ["--measure-box", "-1", "-1", "-1", "1", "1", "1"]
    refused(scene + ["--measure"], "--measure needs --measure-box and --measure-cell")
    refused(scene + ["--measure"] + box, "--measure needs --measure-box and --measure-cell")
    refused(scene + ["--measure", "--measure-cell", "0.1"], "--measure needs --measure-box and --measure-cell")
    refused(scene + box, "need --measure")
    refused(scene + ["--measure-cell", "0.1"], "need --measure")
    refused(scene + ["--measure-step", "0.1"], "need --measure")
    refused(scene + ["--measure-density", "2"], "need --measure")
    refused(scene + ["--measure"] + box + ["--measure-cell", "0"], "cell > 0")
    refused(scene + ["--measure"] + box + ["--measure-cell", "1e-5"], "at most 8192 per axis")
    refused(scene + ["--measure", "--measure-box", "1", "-1", "-1", "1", "1", "1", "--measure-cell", "0.1"], "lo < hi")
    refused(scene + ["--measure"] + box + ["--measure-cell", "0.1", "--measure-axis", "w"], "invalid choice")
    refused(scene + ["--measure"] + box + ["--measure-cell", "0.1", "--measure-step", "0"], "--measure-step must be finite and > 0")
    refused(scene + ["--measure"] + box + ["--measure-cell", "0.1", "--measure-step", "nan"], "--measure-step must be finite and > 0")
    refused(scene + ["--measure"] + box + ["--measure-cell", "0.1", "--measure-density", "-1"], "--measure-density must be finite and > 0")
    refused(scene + ["--measure"] + box + ["--measure-cell", "0.1", "--measure-density", "inf"], "--measure-density must be finite and > 0")
    # the report: the properties, the counts, and a warning only when there is something to warn of
    import sdf_playground_amd as sp

    grid, _depth = sp.measureGrid((-1, -1, -1), (1, 1, 1), 0.5)
    res = sp.MeasureResult()
    res.columns_hit, res.steps = 4, 99
    props = dict(volume=1.5, mass=3.0, centroid=(0.0, 0.1, 0.2), inertia=(1.0, 2.0, 3.0, 0.0, 0.0, 0.0), result=res, grid=grid)
    report = cli.measure_report("s", props, 0.5, "z", 0.25, 2.0)
    assert report["volume"] == 1.5 and report["centroid"] == [0.0, 0.1, 0.2] and report["columns"] == [4, 4] and report["columns_hit"] == 4 and "warning" not in report
    res.columns_open, res.columns_out_of_steps = 3, 2
    report = cli.measure_report("s", props, 0.5, "z", 0.25, 2.0)
    assert "3 columns" in report["warning"] and "2 columns ran out of steps" in report["warning"]

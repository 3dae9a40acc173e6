"""CPU tier of the span queries (sdfr_query_ray_spans, sdfr_pick_spans, sdfr_mesh_spans): the stage function of
sdf_playground_amd/csrc/sdfr_span.h, built for the host (tests/cpp/span_host.cpp), against the header's definition restated in numpy
(tests/span_util.py), every word equal, on a ladder of slabs; the invariants of every result; the chord bound the GPU tier relies on,
checked on a sphere; the plan (sdfr_span_plan.h, built as the stand-alone program tests/cpp/span_plan_host.cpp, also under the address
and undefined-behaviour sanitizers); the struct layouts; the command line's argument faults."""
import ctypes
import math
import re
import struct
import subprocess

import numpy as np
import pytest

import cppbuild
import query_util as qu
import span_util as su

F = np.float32
NAN, INF = float("nan"), float("inf")

# the slab ladder along x: dyadic centres and half-widths, so that distances, steps and quotients are often exact and samples land
# exactly on faces; NaN where 5 <= x <= 5.5, right in front of the last slab (5.5, 6)
C = [-2.0, -0.75, 0.5, 1.25, 2.5, 3.75, 5.75]
R = [0.25, 0.125, 0.25, 0.0625, 0.5, 0.125, 0.25]
NAN_LO, NAN_HI = 5.0, 5.5
FIELD = su.slab_field(C, R, NAN_LO, NAN_HI)


def ladder_rays(seed, n):
    """rays across the ladder: origins with x in [-3, 6.5] (some inside slabs, some in the NaN slab), directions mostly along +-x with
    |dx| in 0.25 .. 2 (t is in units of |dir|), some exactly (+-1, 0, 0); then the items without an answer"""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-3.0, 6.5, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)], 1)
    d = np.stack([rng.choice([-1.0, 1.0], n) * np.exp(rng.uniform(np.log(0.25), np.log(2.0), n)), rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)], 1)
    d[: n // 4] = np.stack([np.sign(d[: n // 4, 0]), np.zeros(n // 4), np.zeros(n // 4)], 1)
    o[: n // 8, 0] = np.round(o[: n // 8, 0] * 16) / 16  # dyadic starts: exact steps
    special_o = np.array([[NAN, 0, 0], [0, INF, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, -INF], [1, 1, 1]], np.float64)
    special_d = np.array([[1, 0, 0], [1, 0, 0], [0, 0, 0], [-0.0, 0.0, -0.0], [NAN, 1, 0], [1, 0, 0], [0, INF, 0]], np.float64)
    return np.concatenate([o, special_o]).astype(F), np.concatenate([d, special_d]).astype(F), len(special_o)


PARAMS = [su.params(0.0625, 12.0, max_steps=4096, max_spans=3), su.params(0.0625, 12.0, max_steps=4096, max_spans=1),
          su.params(0.0625, 12.0, max_steps=4096, max_spans=0), su.params(0.03125, 12.0, max_steps=7, max_spans=3),
          su.params(0.1, 2.5, iso=0.05, max_steps=4096, max_spans=4), su.params(0.0625, 0.3, iso=-0.03125, max_steps=64, max_spans=2),
          su.params(0.25, 0.0, max_steps=1, max_spans=1)]


def _compare(what, got, want):
    for name in su.SUMMARY_DTYPE.names:
        qu.assert_same("%s %s" % (what, name), np.ascontiguousarray(got[0][name]).view(np.uint32), np.ascontiguousarray(want[0][name]).view(np.uint32))
    assert got[1].shape == want[1].shape, what
    if got[1].size:
        qu.assert_same("%s spans" % (what,), got[1].reshape(-1, 2), want[1].reshape(-1, 2))


def test_host_text_equals_the_definition():
    o, d, n_special = ladder_rays(17, 400)
    seen = dict(starts=0, ends=0, out_of_steps=0, finished=0, nan_samples=0)
    over = {}
    for p in PARAMS:
        want = su.march_spans(FIELD, o, d, p)
        got = su.host_march_slabs(o, d, p, C, R, NAN_LO, NAN_HI)
        _compare(p, got, want)
        su.check_invariants(got[0], got[1], p)
        su.check_invariants(want[0], want[1], p)
        S = want[0]
        assert (S["valid"][-n_special:] == 0).all() and (S["valid"][:-n_special] == 1).all()
        seen["starts"] += int(((S["flags"] & su.STARTS_INSIDE) != 0).sum())
        seen["ends"] += int(((S["flags"] & su.ENDS_INSIDE) != 0).sum())
        seen["out_of_steps"] += int(((S["flags"] & su.OUT_OF_STEPS) != 0).sum())
        seen["finished"] += int(((S["valid"] == 1) & ((S["flags"] & su.OUT_OF_STEPS) == 0)).sum())
        over[p["max_spans"], p["max_steps"]] = int((S["spans"] > p["max_spans"]).sum())
    assert seen["starts"] > 50 and seen["ends"] > 50 and seen["out_of_steps"] > 100 and seen["finished"] > 1000, seen
    # rays that cross more slabs than are stored, at every capacity
    assert over[0, 4096] > 100 and over[1, 4096] > 100 and over[3, 4096] > 20, over
    # max_steps = 7: most rays run out of steps
    S7 = su.march_spans(FIELD, o, d, PARAMS[3])[0]
    assert ((S7["flags"] & su.OUT_OF_STEPS) != 0).sum() > 200 and (S7["steps"][(S7["flags"] & su.OUT_OF_STEPS) != 0] == 7).all()


def _one(origin, direction, p):
    o, d = np.array([origin], F), np.array([direction], F)
    want = su.march_spans(FIELD, o, d, p)
    got = su.host_march_slabs(o, d, p, C, R, NAN_LO, NAN_HI)
    _compare((origin, direction, p), got, want)
    su.check_invariants(got[0], got[1], p)
    return got[0][0], got[1][0]


def test_designed_rays():
    # lands exactly on t_max: D(-3) = |-3 + 2| - 0.25 = 0.75 = t_max, so t' == t_max and the second sample is the last
    S, spans = _one((-3.0, 0, 0), (1, 0, 0), su.params(0.125, 0.75))
    assert FIELD(np.array([[-3.0, 0, 0]], F))[0] == F(0.75)
    assert (S["steps"], S["t_end"], S["flags"], S["spans"], S["crossings"]) == (2, F(0.75), 0, 0, 0)
    # ... and a ray whose max_steps-th sample is the one at t_max is not out of steps
    S, spans = _one((-3.0, 0, 0), (1, 0, 0), su.params(0.125, 0.75, max_steps=2))
    assert (S["steps"], S["flags"]) == (2, 0)
    S, spans = _one((-3.0, 0, 0), (1, 0, 0), su.params(0.125, 0.75, max_steps=1))
    assert (S["steps"], S["flags"], S["t_end"]) == (1, su.OUT_OF_STEPS, 0)
    # starts inside the slab (0.25, 0.75), leaves it: one span from 0, closed by an exact crossing (s = -0.0625 then 0.0 at the face:
    # 0 is outside, u = 1)
    S, spans = _one((0.625, 0, 0), (1, 0, 0), su.params(0.0625, 0.5, max_spans=2))
    assert S["flags"] == su.STARTS_INSIDE and S["spans"] == 1 and S["crossings"] == 1
    assert list(spans[0]) == [0, F(0.125)] and list(spans[1]) == [0, 0] and S["inside_length"] == F(0.125)
    # ends inside at t_max: from 0.125 towards +x, t_max = 0.375 ends at x = 0.5, the middle of the slab
    S, spans = _one((0.125, 0, 0), (1, 0, 0), su.params(0.0625, 0.375, max_spans=2))
    assert S["flags"] == su.ENDS_INSIDE and S["spans"] == 1 and S["crossings"] == 1 and spans[0, 1] == S["t_end"] == F(0.375)
    assert abs(float(spans[0, 0]) - 0.125) <= 0.0625
    # the 0.5 rule: through the NaN slab [5, 5.5] into the slab (5.5, 6).  From 4.5 the first step is D = 0.625 to x = 5.125 (NaN: steps
    # of min_step), the sample at 5.5 is still NaN, the one at 5.5625 is inside: u = NaN / NaN -> 0.5, t_in = (5.5 + 0.03125) - 4.5
    S, spans = _one((4.5, 0, 0), (1, 0, 0), su.params(0.0625, 1.25, max_spans=2))
    assert S["spans"] == 1 and spans[0, 0] == F(1.03125) and (S["flags"] & su.ENDS_INSIDE)
    # ... and out of a slab into NaN: from inside (3.625, 3.875) backwards is plain; from 5.75 towards -x the sample after the face is NaN
    S, spans = _one((5.75, 0, 0), (-1, 0, 0), su.params(0.0625, 1.0, max_spans=2))
    assert S["flags"] & su.STARTS_INSIDE and S["spans"] == 1 and spans[0, 0] == 0
    # (s = -0.25 at the start, so the first step is 0.25 long and lands on x = 5.5: NaN -> outside, u = NaN -> 0.5, the middle of THAT step)
    assert spans[0, 1] == F(0.125) and S["inside_length"] == F(0.125)
    # more slabs than slots: from -3 to 6.5 there are 7 slabs, 3 are stored, all are counted and summed
    p = su.params(0.03125, 9.5, max_spans=3)
    S, spans = _one((-3.0, 0, 0), (1, 0, 0), p)
    assert S["spans"] == 7 and S["crossings"] == 14 and S["flags"] == 0
    want_length = 2 * sum(R)
    assert abs(float(S["inside_length"]) - want_length) <= 7 * 0.03125  # the NaN face is cut at a bracket's middle
    assert np.allclose(spans[:, 0], [0.75, 2.125, 3.25], atol=1e-6) and np.allclose(spans[:, 1], [1.25, 2.375, 3.75], atol=1e-6)
    # t is in units of |dir|: half the direction, twice the t (a direction longer than 1 would step further in space than the distance allows)
    S2, spans2 = _one((-3.0, 0, 0), (0.5, 0, 0), su.params(0.03125, 19.0, max_spans=3))
    assert S2["spans"] == 7 and np.allclose(spans2, spans * F(2), atol=1e-5)


def test_chord_bound_on_a_sphere():
    """What the GPU tier relies on for the probe sphere: rays of unit direction with impact parameter b <= rho / 2 give one span whose
    ends lie within min_step^2 / (16 rho) + 1e-5 of the chord's.  (Linear interpolation over a bracket of h = min_step: the error of
    the root is at most h^2 |s''| / (8 |s'|), with |s''| <= b^2 / r^3 = 1 / (4 rho) at r = rho and |s'| >= cos 30 deg: h^2 / (27.7 rho).)
    The worst case seen here is 0.57 of the bound (min_step 0.2, rho 1)."""
    rng = np.random.default_rng(5)
    centre, worst = np.array([0.1, -0.2, 0.3]), 0.0
    for rho, min_step in ((1.0, 0.05), (1.0, 0.2), (0.37, 0.03), (2.5, 0.3)):
        n = 400
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        e = np.cross(d, rng.normal(size=(n, 3)))
        e /= np.linalg.norm(e, axis=1, keepdims=True)
        b = rng.uniform(0, 0.5 * rho, n)
        back = rng.uniform(1.5 * rho, 3.0 * rho, n)
        o = (centre + b[:, None] * e - back[:, None] * d).astype(F)
        d = d.astype(F)
        p = su.params(min_step, 6.0 * rho, max_spans=2)
        S, spans = su.host_march_sphere(o, d, p, centre, rho)
        su.check_invariants(S, spans, p)
        assert (S["spans"] == 1).all() and (S["flags"] == 0).all() and (S["crossings"] == 2).all()
        # the analytic chord of the rays as given (fp32 origins and directions, read as doubles)
        o64, d64 = o.astype(np.float64), d.astype(np.float64)
        oc = o64 - centre
        dd, od = (d64 * d64).sum(1), (oc * d64).sum(1)
        disc = od * od - dd * ((oc * oc).sum(1) - rho * rho)
        t0, t1 = (-od - np.sqrt(disc)) / dd, (-od + np.sqrt(disc)) / dd
        bound = min_step * min_step / (16 * rho) + 1e-5
        err = max(np.abs(spans[:, 0, 0] - t0).max(), np.abs(spans[:, 0, 1] - t1).max())
        assert err <= bound, (rho, min_step, err, bound)
        worst = max(worst, (err - 1e-5) / (bound - 1e-5))
        assert np.allclose(S["inside_length"], t1 - t0, atol=2 * bound)
    assert worst < 0.75, worst
    print("worst chord-end error over the bound: %.3f" % worst)


# ---- the plan -------------------------------------------------------------------------------------------------------------------
INVALID = -1  # SDFR_ERR_INVALID_ARGUMENT
RAYS, PICK, FRAME, MESH = 1, 2, 3, 4  # QUERY_*
NULL_POINTER, BAD_ON_HOST, BAD_PARAMS, BAD_COUNT = "null pointer", "on_host must be 0 or 1", "bad span parameters", "bad item count"
BAD_FRAME, BAD_REACH, NULL_SPANS, BAD_FRAME_N = "bad frame size", "reach must be finite and > 0", "null spans with max_spans > 0", "without a pixel list n must be width * height"


def _exe(name, flags):
    return cppbuild.plan_program("span_plan_host", name, flags)


@pytest.fixture(scope="module")
def exe():
    return _exe("span_plan_host", [])


def request(kind=RAYS, n=100, in0=True, in1=True, width=19, height=11, reach=0.5, params=True, t_max=0.0, min_step=0.01, iso=0.0, max_steps=256, max_spans=3,
            summaries=True, spans=True, on_host=0, range_=80.0):
    if kind == PICK and in1:
        in1 = False
    return dict(kind=kind, n=n, in0=in0, in1=in1, width=width, height=height, reach=reach, params=params, t_max=t_max, min_step=min_step, iso=iso,
                max_steps=max_steps, max_spans=max_spans, summaries=summaries, spans=spans, on_host=on_host, range_=range_)


def line_of(r):
    f = lambda v: repr(float(v))  # noqa: E731
    return " ".join([str(r["kind"]), str(r["n"]), str(int(r["in0"])), str(int(r["in1"])), str(r["width"]), str(r["height"]), f(r["reach"]), str(int(r["params"])),
                     f(r["t_max"]), f(r["min_step"]), f(r["iso"]), str(r["max_steps"]), str(r["max_spans"]), str(int(r["summaries"])), str(int(r["spans"])),
                     str(r["on_host"]), f(r["range_"])])


def f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def f32_bits(v):
    return struct.unpack("I", struct.pack("f", v))[0]


def rules(r):
    """the issue's rules, in the order their errors win -> (status, text, plan or None; plan "nothing": n = 0)"""
    pick = r["kind"] == PICK
    frame = pick and not r["in0"]
    if not r["params"] or not r["summaries"] or (not pick and (not r["in0"] or not r["in1"])):
        return INVALID, NULL_POINTER, None
    if r["on_host"] not in (0, 1):
        return INVALID, BAD_ON_HOST, None
    t_max, min_step, iso = f32(r["t_max"]), f32(r["min_step"]), f32(r["iso"])
    if not (math.isfinite(t_max) and t_max >= 0 and math.isfinite(min_step) and min_step > 0 and math.isfinite(iso)
            and 1 <= r["max_steps"] <= 1 << 20 and 0 <= r["max_spans"] <= 64):
        return INVALID, BAD_PARAMS, None
    if r["n"] < 0 or r["n"] * max(r["max_spans"], 1) > 1 << 30:
        return INVALID, BAD_COUNT, None
    if pick and not (r["width"] >= 1 and r["height"] >= 1 and r["width"] * r["height"] <= 1 << 30):
        return INVALID, BAD_FRAME, None
    if r["kind"] == MESH and not (math.isfinite(f32(r["reach"])) and f32(r["reach"]) > 0):
        return INVALID, BAD_REACH, None
    if r["max_spans"] > 0 and not r["spans"]:
        return INVALID, NULL_SPANS, None
    if r["n"] == 0:
        return 0, "", "nothing"
    if frame and r["n"] != r["width"] * r["height"]:
        return INVALID, BAD_FRAME_N, None
    n = r["n"]
    kind = FRAME if frame else r["kind"]
    blocks = -(-r["width"] // 8) * -(-r["height"] // 8) if frame else -(-n // 64)
    return 0, "", dict(kind=kind, there=(int(not pick), int(not pick), int(pick and not frame), 1, int(r["max_spans"] > 0)),
                       reach=r["reach"] if r["kind"] == MESH else 0.0, t_max=r["range_"] if t_max == 0 else r["t_max"],
                       bytes=(0 if frame else n * (8 if pick else 12), 0 if pick else n * 12, n * 32, n * r["max_spans"] * 8),
                       frame=(r["width"], r["height"]) if pick else (1, 1), blocks=blocks)


def expected_line(r):
    status, text, plan = rules(r)
    out = "%d;%s" % (status, text)
    if plan == "nothing":
        return out + ";1"
    if plan:
        out += ";0;%d %d %d %d %d %d %d" % ((plan["kind"], r["n"]) + plan["there"])
        out += " %08x %08x %08x %08x %d %d" % (f32_bits(plan["reach"]), f32_bits(plan["t_max"]), f32_bits(r["min_step"]), f32_bits(r["iso"]), r["max_steps"], r["max_spans"])
        out += ";%d %d %d %d;%d %d;%d" % (plan["bytes"] + plan["frame"] + (plan["blocks"],))
    return out


def run(exe, reqs):
    text = "".join(line_of(r) + "\n" for r in reqs)
    lines = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(reqs)
    return lines


BAD_PARAMETERS = [dict(t_max=NAN), dict(t_max=INF), dict(t_max=-0.5), dict(min_step=0.0), dict(min_step=-1.0), dict(min_step=NAN), dict(min_step=INF),
                  dict(iso=NAN), dict(iso=-INF), dict(max_steps=0), dict(max_steps=(1 << 20) + 1), dict(max_steps=-3), dict(max_spans=-1), dict(max_spans=65)]


def fault_cases():
    """(what, request, the text that wins)"""
    cases = [("bad parameters %r" % (b,), request(kind=k, **b), BAD_PARAMS) for b in BAD_PARAMETERS for k in (RAYS, PICK, MESH)]
    cases += [("null params", request(params=False), NULL_POINTER), ("null summaries", request(summaries=False), NULL_POINTER),
              ("null origins", request(in0=False), NULL_POINTER), ("null dirs", request(in1=False), NULL_POINTER),
              ("null normals", request(kind=MESH, in1=False), NULL_POINTER), ("null summaries, n = 0", request(n=0, summaries=False), NULL_POINTER),
              ("on_host 2", request(on_host=2), BAD_ON_HOST), ("on_host -1", request(kind=PICK, on_host=-1), BAD_ON_HOST),
              ("n -1", request(n=-1), BAD_COUNT), ("n 2^30 + 1", request(n=(1 << 30) + 1, max_spans=0), BAD_COUNT),
              ("n * max_spans past 2^30", request(n=(1 << 24) + 1, max_spans=64), BAD_COUNT), ("n 2^62", request(n=1 << 62, max_spans=64), BAD_COUNT),
              ("frame 0 x 11", request(kind=PICK, width=0), BAD_FRAME), ("frame 19 x -1", request(kind=PICK, height=-1), BAD_FRAME),
              ("frame too large", request(kind=PICK, width=1 << 16, height=(1 << 14) + 1), BAD_FRAME),
              ("reach 0", request(kind=MESH, reach=0.0), BAD_REACH), ("reach nan", request(kind=MESH, reach=NAN), BAD_REACH),
              ("reach inf", request(kind=MESH, reach=INF), BAD_REACH), ("reach -1", request(kind=MESH, reach=-1.0), BAD_REACH),
              ("null spans", request(spans=False), NULL_SPANS), ("null spans, n = 0", request(n=0, spans=False), NULL_SPANS),
              ("whole frame, n off", request(kind=PICK, in0=False, n=208), BAD_FRAME_N)]
    # two faults at once, one request per adjacent pair of checks: the earlier text wins
    cases += [("null params + on_host 2", request(params=False, on_host=2), NULL_POINTER),
              ("on_host 2 + bad parameters", request(on_host=2, min_step=0.0), BAD_ON_HOST),
              ("bad parameters + bad count", request(max_spans=65, n=-1), BAD_PARAMS),
              ("bad count + bad frame", request(kind=PICK, n=-1, width=0), BAD_COUNT),
              ("bad count + bad reach", request(kind=MESH, n=-1, reach=0.0), BAD_COUNT),
              ("bad frame + null spans", request(kind=PICK, width=0, spans=False), BAD_FRAME),
              ("bad reach + null spans", request(kind=MESH, reach=-1.0, spans=False), BAD_REACH),
              ("null spans + whole frame n off", request(kind=PICK, in0=False, n=5, spans=False), NULL_SPANS)]
    return cases


def good_cases():
    cases = [("n = %d" % n, request(kind=k, n=n, on_host=h)) for n in (1, 63, 64, 65, 130) for k in (RAYS, PICK, MESH) for h in (0, 1)]
    cases += [("a 19 x 11 frame", request(kind=PICK, in0=False, n=209)), ("a 19 x 11 frame, no spans", request(kind=PICK, in0=False, n=209, max_spans=0, spans=False)),
              ("an 8 x 8 frame", request(kind=PICK, in0=False, n=64, width=8, height=8)), ("a 1920 x 1080 frame", request(kind=PICK, in0=False, n=1920 * 1080, width=1920, height=1080)),
              ("n = 0", request(n=0)), ("n = 0, whole frame", request(kind=PICK, in0=False, n=0)), ("t_max given", request(t_max=2.5)),
              ("max_spans 0 with spans", request(max_spans=0)), ("max_spans 0, null spans", request(max_spans=0, spans=False)),
              ("2^30 items", request(n=1 << 30, max_spans=0, spans=False)), ("2^30 spans", request(n=1 << 24, max_spans=64)),
              ("the limits", request(max_steps=1 << 20, max_spans=64, iso=-3.5, min_step=1e-30)), ("rays ignore reach and frame", request(reach=NAN, width=0))]
    return cases


def test_argument_faults(exe):
    cases = fault_cases()
    got = run(exe, [r for _what, r, _text in cases])
    for (what, r, text), line in zip(cases, got):
        assert line == "%d;%s" % (INVALID, text), what
        assert line == expected_line(r), what
    assert {text for _w, _r, text in cases} == {NULL_POINTER, BAD_ON_HOST, BAD_PARAMS, BAD_COUNT, BAD_FRAME, BAD_REACH, NULL_SPANS, BAD_FRAME_N}


def test_good_requests(exe):
    cases = good_cases()
    got = run(exe, [r for _what, r in cases])
    by_name = {}
    for (what, r), line in zip(cases, got):
        assert line.startswith("0;;"), (what, line)
        assert line == expected_line(r), what
        by_name.setdefault(what, line)
    # blocks for n = 1, 63, 64, 65 and a 19 x 11 frame
    assert [by_name["n = %d" % n].split(";")[-1] for n in (1, 63, 64, 65, 130)] == ["1", "1", "1", "2", "3"]
    assert by_name["a 19 x 11 frame"].split(";")[-3:] == ["0 0 6688 5016", "19 11", "6"]
    assert by_name["a 19 x 11 frame"].split(";")[3].split()[:7] == ["3", "209", "0", "0", "0", "1", "1"]
    assert by_name["a 1920 x 1080 frame"].split(";")[-1] == str(240 * 135)
    assert by_name["n = 0"] == "0;;1"
    # t_max 0 is limits.range
    assert by_name["n = 1"].split(";")[3].split()[8] == "%08x" % f32_bits(80.0) and by_name["t_max given"].split(";")[3].split()[8] == "%08x" % f32_bits(2.5)
    assert by_name["max_spans 0 with spans"].split(";")[3].split()[6] == "0"  # the kernel gets no span array it will not use


def test_under_sanitizers(exe):
    """the same program built with the address and undefined-behaviour sanitizers, over every request above: the same answers"""
    reqs = [r for _w, r, _t in fault_cases()] + [r for _w, r in good_cases()]
    checked = _exe("span_plan_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert run(checked, reqs) == run(exe, reqs)


# ---- layouts and the command line -----------------------------------------------------------------------------------------------
def test_struct_layouts():
    import sdf_playground_amd as sp

    for S in (sp.SpanParams, su.HostParams):
        assert ctypes.sizeof(S) == 20
        assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _t in S._fields_] == [("t_max", 0, 4), ("min_step", 4, 4), ("iso", 8, 4), ("max_steps", 12, 4),
                                                                                          ("max_spans", 16, 4)]
    assert su.host_lib().sph_params_size() == 20 and su.host_lib().sph_summary_words() == 8
    for dt in (sp.SPAN_SUMMARY_DTYPE, su.SUMMARY_DTYPE):
        assert dt.itemsize == 32
        assert [(n, dt.fields[n][1], dt.fields[n][0].str) for n in dt.names] == [("crossings", 0, "<u4"), ("spans", 4, "<u4"), ("steps", 8, "<u4"), ("valid", 12, "<i4"),
                                                                                 ("inside_length", 16, "<f4"), ("t_end", 20, "<f4"), ("flags", 24, "<u4"), ("reserved", 28, "<u4")]
    assert (sp.SPAN_STARTS_INSIDE, sp.SPAN_ENDS_INSIDE, sp.SPAN_OUT_OF_STEPS) == (1, 2, 4) == (su.STARTS_INSIDE, su.ENDS_INSIDE, su.OUT_OF_STEPS)
    for symbol in ("sdfr_query_ray_spans", "sdfr_pick_spans", "sdfr_mesh_spans"):
        assert symbol in sp.EXPORTED_SYMBOLS
    # the header declares the same fields in the same order
    header = open(cppbuild.ROOT + "/include/sdfr.h").read()

    def fields(name):
        body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return re.findall(r"\b(u?int32_t|float)\s+([a-z_, ]+);", body)

    assert fields("sdfr_span_params") == [("float", "t_max"), ("float", "min_step"), ("float", "iso"), ("int32_t", "max_steps"), ("int32_t", "max_spans")]
    assert fields("sdfr_span") == [("float", "t_in, t_out")]
    assert fields("sdfr_span_summary") == [("uint32_t", "crossings"), ("uint32_t", "spans"), ("uint32_t", "steps"), ("int32_t", "valid"), ("float", "inside_length"),
                                           ("float", "t_end"), ("uint32_t", "flags"), ("uint32_t", "reserved")]
    assert re.search(r"#define SDFR_SPAN_STARTS_INSIDE 1u\s*#define SDFR_SPAN_ENDS_INSIDE 2u\s*#define SDFR_SPAN_OUT_OF_STEPS 4u", header)


def test_thickness_rule_and_colours():
    from sdf_playground_amd import obj

    S = np.zeros(6, su.SUMMARY_DTYPE)
    spans = np.zeros((6, 1, 2), F)
    S["valid"] = [1, 1, 1, 1, 0, -1]
    S["spans"] = [1, 1, 0, 2, 0, 0]
    S["flags"] = [0, su.ENDS_INSIDE, 0, su.ENDS_INSIDE, 0, 0]  # a wall that ends; one the march's end closes; none; two, the second one open
    spans[:, 0] = [(0.5, 0.75), (0.5, 2.0), (0, 0), (0.25, 0.5), (0, 0), (0, 0)]
    t = su.thickness(S, spans)
    assert list(t) == [0.25, INF, INF, 0.25, INF, INF]
    grey = obj.thickness_colors(t, 0.5)
    assert grey.shape == (6, 3) and grey.dtype == F and list(grey[:, 0]) == [0.5, 1, 1, 0.5, 1, 1] and (grey[:, 0] == grey[:, 2]).all()


def test_cli_span_arguments(capsys):
    from sdf_playground_amd import cli

    image = cli.xray_image(np.array([0.0, 1.0, INF, NAN, -1.0, 0.5], F), 3, 2, 2.0)
    assert image.shape == (2, 3, 4) and image.dtype == np.uint8 and (image[..., 3] == 255).all() and (image[..., 0] == image[..., 2]).all()
    assert list(image[..., 0].ravel()) == [0, round(255 * (1 - math.exp(-2.0))), 255, 255, 0, round(255 * (1 - math.exp(-1.0)))]

    def refused(args, text):
        with pytest.raises(SystemExit) as e:
            cli.main(args)
        assert e.value.code == 2 and text in capsys.readouterr().err, args

    scene = ["--scene", "labyrinth"]
    mesh = ["--mesh", "m.obj", "--mesh-box", "-6", "0", "-3", "0", "2", "3", "--mesh-cell", "0.05"]
    refused(scene + ["--xray", "x.png"], "--xray needs --xray-step")
    refused(scene + ["--xray-step", "0.01"], "need --xray")
    refused(scene + ["--xray-density", "2"], "need --xray")
    refused(scene + ["--xray", "x.png", "--xray-step", "0"], "--xray-step must be finite and > 0")
    refused(scene + ["--xray", "x.png", "--xray-step", "-0.1"], "--xray-step must be finite and > 0")
    refused(scene + ["--xray", "x.png", "--xray-step", "nan"], "--xray-step must be finite and > 0")
    refused(scene + ["--xray", "x.png", "--xray-step", "0.01", "--xray-density", "0"], "--xray-density must be finite and > 0")
    refused(scene + ["--xray", "x.png", "--xray-step", "0.01", "--xray-density", "inf"], "--xray-density must be finite and > 0")
    refused(scene + ["--mesh-thickness", "0.5"], "--mesh-thickness needs --mesh")
    refused(scene + mesh + ["--mesh-thickness", "0"], "--mesh-thickness must be finite and > 0")
    refused(scene + mesh + ["--mesh-thickness", "inf"], "--mesh-thickness must be finite and > 0")
    refused(scene + mesh + ["--mesh-thickness", "0.5", "--mesh-colors"], "excludes")
    refused(scene + mesh + ["--mesh-thickness", "0.5", "--mesh-ao", "0.4"], "excludes")
    refused(scene + mesh + ["--mesh-thickness", "0.5", "--mesh-lit"], "excludes")

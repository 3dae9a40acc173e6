"""CPU tier of the probe scenes (tests/probe_scenes.py): every generated text compiles for gfx950 in both math modes; the same table run
through a host build of the query kernels (tests/cpp/query_host.cpp over the probe text) equals the oracle's kat_batch bit for bit; the
inputs are usable (few NaN results, few inputs outside the fast forms' domains); and every SDF_HD function of sdfr_math.h, sdfr_noise.h
and sdfr_lib.h has a probe or a stated reason to have none.  The GPU tier is tests/test_gpu_probe.py."""
import ctypes
import os

import numpy as np
import pytest

import cppbuild
import probe_scenes as ps
import query_util as qu

MODES = [False, True]


@pytest.fixture(scope="module")
def census_oracle(oracle):
    oracle.build(census=True, ref=False)
    return oracle


# ---- the texts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast_math", MODES, ids=["ieee", "fast"])
@pytest.mark.parametrize("group", ps.GROUPS)
def test_probe_text_compiles_for_gfx950(group, fast_math):
    import sdf_playground_amd as sp

    text = ps.scene_text(group, fast_math)
    assert (ps.TOKEN in text) == fast_math
    ok, log = sp.check_scene_source(text)
    assert ok, log


def test_no_probe_indexes_memory_by_an_argument():
    """the expressions and helpers are calls, literals and a[k] with a literal k; nothing subscripts by a value"""
    import re

    for group in ps.GROUPS:
        for m in re.finditer(r"\[([^\]]*)\]", ps.scene_text(group, True)):
            assert re.fullmatch(r"\d+|%d" % ps.MAX_INPUTS, m.group(1).strip()), (group, m.group(0))


# ---- the host build against the oracle --------------------------------------------------------------------------------------------
_host = {}


def host_lib(group):
    if group not in _host:
        gen = os.path.join(cppbuild.BUILD, "probe_%s.scene.inc" % group)
        assert cppbuild.scene_include(gen, ps.scene_text(group, False)) == ps.VAR_NAMES
        deps = [gen, os.path.join(cppbuild.HERE, "cpp", "host_common.h")] + cppbuild.csrc_headers()
        L = ctypes.CDLL(qu.build_lib("query_host_probe_%s" % group, "query_host.cpp",
                                     ["-I" + cppbuild.CSRC, '-DSDFR_HLSL_SCENE_FILE="%s"' % gen, "-DSDFR_SCENE_HAS_PREPARE=1"], deps))
        vp = ctypes.c_void_p
        L.qh_points.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, vp, vp, vp]
        _host[group] = L
    return _host[group]


def host_values(group, probe):
    """the probe's N_POINTS values from the host build of query_point over the probe scene, call by call as the GPU test queries them"""
    L = host_lib(group)
    U = qu.host_frame(qu.po.default_frame("fast_sphere", 8, 8, stime=float(probe.case)))
    pts = ps.points(probe)
    out = np.empty(ps.N_POINTS, np.float32)
    for rows, variables in ps.calls(probe):
        for k in range(8):
            U.scene_var[k] = 0.0
        for name, v in variables.items():
            U.scene_var[ps.VAR_NAMES.index(name)] = v
        p = np.ascontiguousarray(pts[rows])
        d = np.empty(len(p), np.float32)
        assert L.qh_points(b"probe", ctypes.byref(U), len(p), p.ctypes.data, d.ctypes.data, None) == 0
        out[rows] = d
    return out


@pytest.mark.parametrize("group", ps.GROUPS)
def test_host_build_of_the_probes_equals_the_oracle(oracle, group):
    """sdfr_math.h / sdfr_noise.h / sdfr_lib.h compiled for the CPU, function by function, on the probes' inputs: bit for bit the oracle
    (NaN by class).  What the GPU tier then adds is the device build alone."""
    failed = []
    for probe in ps.probes(group):
        got, want = host_values(group, probe), ps.expected(oracle, probe)
        keep = np.ones(ps.N_POINTS, bool)
        if not ps.same(got, want).all():
            failed.append(ps.mismatch_report(probe, got, want, keep))
    assert not failed, "\n".join(failed)


# ---- the inputs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ps.GROUPS)
def test_inputs_give_numbers_and_stay_inside_the_fast_domains(census_oracle, group, capsys):
    """From the oracle alone: at most a quarter of a probe's expected values are NaN, and the fast-math run keeps at least 80 % of
    its inputs (an input is dropped only where the census flags its evaluation)."""
    lines, bad = [], []
    for probe in ps.probes(group):
        want = ps.expected(census_oracle, probe)
        nan = float(np.isnan(want).mean())
        keep = ps.kept(census_oracle, probe, True)
        dropped = ps.N_POINTS - int(keep.sum())
        flags = ps.expected(census_oracle, probe, census=True)[1] if probe.fast else np.zeros(ps.N_POINTS, np.uint8)
        lines.append("%-28s NaN %5.1f %%  dropped %4d (%4.1f %%: sqrt %d, div_c %d, rcp %d, far %d)" % (
            probe.name, 100 * nan, dropped, 100.0 * dropped / ps.N_POINTS, *(int(((flags >> b) & 1).sum()) for b in range(4))))
        if nan > 0.25 or keep.mean() < 0.8:
            bad.append(lines[-1])
        if probe.fast:  # the census build computes what the plain build computes
            assert ps.same(ps.expected(census_oracle, probe, census=True)[0], want).all(), probe.name
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)


def _bit_set(values, positive):
    v = np.ascontiguousarray(values, np.float32)
    v = v[~np.isnan(v)]
    return set((np.abs(v) if positive else v).view(np.uint32).tolist())


def test_every_argument_carries_its_edges():
    """EVERY device input of every probe, the ones that travel as the point and the ones that travel as variables: each value of
    probe_scenes.required_edges is there at least once (a `pos` argument up to its sign; an index of a constant has no edges).  For the
    general kinds that means, on a variable too: NaN, both infinities, both zeros, denormals, FLT_MAX, 2^24, 2^31 and an integer beyond
    2^24.  The edges of different arguments are crossed, and a probe of more than three inputs holds its variables constant within a call."""
    core = ps.required_edges("any", True)
    for must in (np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 3.4028234663852886e38, 16777216.0, -2147483648.0, 16777218.0):
        m = np.float32(must)
        assert any((np.isnan(m) and np.isnan(e)) or np.array(e).view(np.uint32) == np.array(m).view(np.uint32) for e in core), must
    for probe in ps.probes():
        x = ps.oracle_inputs(probe)
        assert x.shape == (ps.N_POINTS, len(probe.kinds)) and x.dtype == np.float32
        d = ps.device_inputs(probe)
        for j, c in enumerate(probe.dev_cols):
            kind = probe.kinds[c]
            if kind == "const":
                assert set(d[:, j].tolist()) == set(float(k) for k in range(len(probe.consts))), probe.name  # every constant
                continue
            need = ps.required_edges(kind, per_call=j >= 3)
            have = _bit_set(x[:, c], kind == "pos")
            for e in need:
                if np.isnan(e):
                    assert np.isnan(x[:, c]).any(), (probe.name, j, "NaN")
                else:
                    assert int(np.abs(e).view(np.uint32) if kind == "pos" else np.array(e, np.float32).view(np.uint32)) in have, (probe.name, j, float(e))
        # crossed: some tuple holds special values (not finite, zero or denormal) in two arguments at once, a point argument and a variable
        # among them where the probe has both
        special = ~np.isfinite(x[:, probe.dev_cols]) | (np.abs(x[:, probe.dev_cols]) < np.float32(1.17549435e-38))
        general = [j for j, c in enumerate(probe.dev_cols) if probe.kinds[c] in ps._ANY_FAMILY]
        if len(general) >= 2:
            assert (special[:, general].sum(axis=1) >= 2).any(), probe.name
        if [j for j in general if j < 3] and [j for j in general if j >= 3]:
            assert (special[:, [j for j in general if j < 3]].any(axis=1) & special[:, [j for j in general if j >= 3]].any(axis=1)).any(), probe.name
        for rows, variables in ps.calls(probe):
            assert len(variables) == max(0, probe.arity - 3)
            for j in range(3, probe.arity):
                assert (d[rows, j].view(np.uint32) == d[rows, j].view(np.uint32)[0]).all()


# ---- coverage ----------------------------------------------------------------------------------------------------------------------
def test_every_library_function_has_a_probe_or_a_reason():
    functions, covered = ps.header_functions(), ps.covered_functions()
    assert len(functions) > 100
    missing = sorted(functions - covered - set(ps.EXCLUDED))
    assert not missing, "SDF_HD functions without a probe and without a reason: %s" % missing
    stale = sorted((covered | set(ps.EXCLUDED)) - functions)
    assert not stale, "named in tests/probe_scenes.py but not in the headers: %s" % stale
    for name, reason in ps.EXCLUDED.items():
        assert name not in covered, name
        assert any(reason.startswith(r) for r in ps.REASONS), (name, reason)
        if reason.startswith(ps.INTERNAL):  # says of what
            assert len(reason) > len(ps.INTERNAL), (name, reason)
    # each probe's kat function exists and writes the output the probe reads
    from oracle import pyoracle as po

    for probe in ps.probes(controls=True):
        assert po.kat_batch(probe.kat, np.zeros((1, len(probe.kinds)), np.float32)).shape[1] > probe.out, probe.name


# ---- the oracle side --------------------------------------------------------------------------------------------------------------
def test_new_kat_entries_have_their_analytic_values(oracle):
    f32 = np.float32

    def kat(fn, *a):
        return oracle.kat_batch(fn, np.array([a], f32))[0]

    assert kat("fma", 2, 3, 4)[0] == 10 and kat("sqrt", 9)[0] == 3 and kat("rcp", 4)[0] == 0.25 and kat("rsqrt", 4)[0] == 0.5
    assert kat("saturate", -1)[0] == 0 and kat("clamp", 5, 0, 2)[0] == 2 and kat("lerp", 1, 3, 0.5)[0] == 2 and kat("abs", -0.0)[0] == 0 and not np.signbit(kat("abs", -0.0)[0])
    assert kat("floor", -1.5)[0] == -2 and kat("trunc", -1.5)[0] == -1
    assert kat("ftoi", -2.7)[0] == -2 and kat("ftoi", np.nan)[0] == 0 and kat("ftoi", 3e9)[0] == f32(2147483647) and kat("ftoi", -np.inf)[0] == -2147483648.0
    assert abs(float(kat("atan", 1)[0]) - np.pi / 4) < 1e-7
    assert kat("dot2", 1, 2, 3, 4)[0] == 11 and kat("dot3", 1, 2, 3, 4, 5, 6)[0] == 32 and kat("dot4", 1, 2, 3, 4, 5, 6, 7, 8)[0] == 70
    assert kat("length2", 3, 4)[0] == 5 and kat("length3", 3, 4, 12)[0] == 13 and tuple(kat("normalize2", 0, 2)) == (0, 1)
    assert tuple(kat("lerp2", 0, 0, 2, 4, 0.5)) == (1, 2) and tuple(kat("lerp3", 0, 0, 0, 2, 4, 6, 0.5)) == (1, 2, 3) and tuple(kat("mad", 1, 2, 3, 2, 1, 1, 1)) == (3, 5, 7)
    assert kat("div_const", 6, 3)[0] == 2 and kat("fmod_const", 7, 3)[0] == f32(f32(7) / f32(3) - 2) * f32(3) and kat("fmod_const", 7, 3)[0] == kat("fmod", 7, 3)[0]
    assert kat("sdLimit1", 0.25, 2, 1)[0] == 0.125 and kat("sdLimit3", 0, 0, 0, 1, 2, -4, 1, 1, 1)[0] == 0.125
    assert kat("opRepInfConst", 1.5, 2)[0] == kat("opRepInf", 1.5, 2)[0] == -0.5
    assert kat("opShell", 0.5, 1, 2)[0] == 0.5 and kat("opChamfer", 1, 1, 0)[0] == f32(2) * f32(0.70710678118654752)
    assert kat("opChamferMerge", 3, 4, 100)[0] < 0 and kat("opPipeMerge", -1, -2, 0.1, 4)[0] <= -2
    assert tuple(kat("opAB2UV", 1, 1)) == (f32(2) * f32(0.70710678118654752), 0)
    assert kat("staircase", 2.5, 0.25, 1)[0] == 0.75  # min(0.25, 0.5) + 2 * 0.25
    assert kat("smax1", 5, 1, 0.5)[0] == 1 and kat("smax1", -5, 1, 0.5)[0] == 5  # far from the blend: max(b, -a)
    assert tuple(kat("HUEtoRGB", 0)) == (1, 0, 0) and tuple(kat("HUEtoRGB", 0.5)) == (0, 1, 1) and abs(float(kat("RGBtoBrightness", 1, 1, 1)[0]) - 1) < 1e-6
    h = int(oracle.kat_u32("hash", 12345).view(np.uint32)[0])
    bits = np.array([12345], np.uint32).view(f32)
    assert int(oracle.kat_batch("hash_hi", bits.reshape(1, 1))[0, 0]) == h >> 8 and int(oracle.kat_batch("hash_lo", bits.reshape(1, 1))[0, 0]) == h & 0xFF
    assert tuple(kat("tile_color_at", 0.25, 0, 0.75, 0, -1, 0)) == tuple(oracle.kat("tile_color", 0.25, 0.75))  # straight down: the floor under the point
    v = kat("voronoi", 0.3, 0.6, 0.0)  # no jitter: the sites are the cell centres
    assert tuple(v[:2]) == (0, 0) and abs(float(v[2]) - float(np.hypot(0.2, 0.1))) < 1e-6 and abs(float(v[3]) - 0.3) < 1e-6
    assert tuple(kat("braid", 3.5, 4.5, 0.1, 4, 2, 7, 8))[:2] == (3, 4) and tuple(kat("truchet_band", 3.5, 4.5, 0.5, 0.01, 7, 8))[:2] == (3, 4)
    assert kat("coordinate_material", 0.5, 0.5, 0.5, 0, 0, 1, 0.1)[0] == 0 and kat("coordinate_material", 0.0, 0.5, 0.5, 0, 0, 1, 0.1)[0] == 1
    # the scene helpers that have no line in the reference's shaders: stated in the oracle from their meaning
    assert tuple(kat("sort3_desc", 1, 3, 2)) == (3, 2, 1) and tuple(kat("sort3_desc", 2, 2, 5)) == (5, 2, 2) and kat("any3", 0, -0.0, 0)[0] == 0 and kat("any3", 0, 1e-45, 0)[0] == 1
    assert tuple(kat("set_rgb", 1, 2, 3, 4, 9)) == (9, 9, 9, 4)
    assert kat("ray_passes_ball", 0, 0, -5, 0, 0, 1, 0, 0, 0, 1)[0] == 0 and kat("ray_passes_ball", 0, 0, 5, 0, 0, 1, 0, 0, 0, 1)[0] == 1  # towards it; it lies behind
    assert kat("ray_passes_ball", 2, 0, -5, 0, 0, 3, 0, 0, 0, 1)[0] == 1 and kat("ray_passes_ball", 0.5, 0, -5, 0, 0, 3, 0, 0, 0, 1)[0] == 0  # passes at 2; at 0.5
    assert kat("ray_passes_ball", 0, 0, 0.5, 0, 0, 1, 0, 0, 0, 1)[0] == 0  # starts inside
    leaves = lambda *a: kat("ray_leaves_floor_and_ball", *a)[0]  # p, dir, top, c, radius
    assert leaves(0, 5, 0, 0, 0.1, 1, 4, 0, 1, 9, 1) == 1 and leaves(0, 5, 0, 0, -0.1, 1, 4, 0, 1, 9, 1) == 0  # above the top and rising; descending
    assert leaves(0, 1, 0, 0, 0, 1, 4, 0, 1, 9, 1) == 0 and leaves(0, 1, 0, 0, 0, -1, 4, 0, 1, 9, 1) == 1  # level: at the ball; away from it
    assert leaves(0, 0, 0, 0, 1, 0, 4, 9, 9, 9, 1) == 0 and leaves(0, -1, 0, 0, 1, 0, 4, 9, 9, 9, 1) == 0  # on and under the floor: never
    with pytest.raises(KeyError):
        oracle.kat_batch("no_such_function", np.zeros((1, 1), f32))


def test_census_flags_name_the_inputs_outside_the_fast_domains(census_oracle):
    """per input: bit 0 sqrt1's domain (+0 and [2^-96, FLT_MAX]), bit 1 div_c's (0 and 2^-100 .. 2^110), bit 2 rcp1's (0, inf and
    2^-100 .. 2^100), bit 3 an overflowed argument; an evaluation inside the domains raises none"""
    def flags(fn, rows):
        return census_oracle.kat_batch(fn, np.array(rows, np.float32), census=True)[1].tolist()

    assert flags("sqrt", [[0.0], [4.0], [2.0 ** -96], [3.4e38], [-0.0], [-1.0], [1e-40], [2.0 ** -97], [np.inf], [np.nan]]) == [0, 0, 0, 0, 1, 1, 1, 1, 8, 8]
    assert flags("rcp", [[0.0], [-0.0], [np.inf], [-np.inf], [2.0 ** -100], [-(2.0 ** 100)], [np.nan], [2.0 ** -101], [2.0 ** 101], [1e-45]]) == [0, 0, 0, 0, 0, 0, 0, 4, 4, 4]
    assert flags("div_const", [[0.0, 3.0], [2.0 ** -100, 3.0], [2.0 ** 110, 3.0], [2.0 ** -101, 3.0], [2.0 ** 111, 3.0], [np.nan, 3.0]]) == [0, 0, 0, 2, 8, 8]
    assert flags("rsqrt", [[4.0], [0.0], [-4.0]]) == [0, 0, 1]  # (the root of a sum in sqrt1's domain is in rcp1's)
    assert flags("atan2", [[1.0, 1.0], [3.0, 1.0], [2.0 ** 60, 2.0 ** -60], [1.0, 0.0], [2.0 ** 127, 2.0 ** -127]]) == [0, 0, 4, 0, 0]  # t = |y| / |x| beyond 2^100; inf is exact
    cone = flags("sdRoundCone", [[0, 0, 0, 0, 0, 0, 0, 1, 0, 0.2, 0.1], [0, 0, 0, 0, 0, 0, 0, 2.0 ** -51, 0, 0.2, 0.1]])
    assert cone[0] == 0 and cone[1] & 4  # l2 = 2^-102: the reciprocal of the squared length (and, with it, a root of something as small)
    assert flags("length3", [[3.0, 4.0, 12.0], [1e-20, 0.0, 0.0]]) == [0, 1]  # the sum of squares is 1e-40

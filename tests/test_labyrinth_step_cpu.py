"""CPU tier: the labyrinth's march step after its exact rewrites (SceneLabyrinth::rep20 / fold / floor_dist, sdfr_scenes.h) gives the very
bits of the formulas it replaced -- x - 20 * floor(x / 20) - 10 with product and difference apart, compare-and-swap of the two absolute
values, the floor's height as a multiplication, an addition and a multiply-add -- which tests/cpp/labyrinth_step_host.cpp holds written out.  Every
input the comments beside the code exclude has a case here that asserts what the comment says happens there.  Then the whole
pipeline, the host build of the product's headers (tests/hostsim), against the oracle from the cameras of
tests/labyrinth_step_cameras.py, those at y = -0, on and under the floor among them."""
import ctypes
import os

import numpy as np
import pytest

import cppbuild
import labyrinth_step_cameras as lsc

SRC = os.path.join(cppbuild.HERE, "cpp", "labyrinth_step_host.cpp")
F32 = np.float32
EDGE = F32(67108848.0)  # the largest |p| rep20's comment claims: |p + 10| < 20 * 3355443


@pytest.fixture(scope="module")
def step_lib():
    return ctypes.CDLL(cppbuild.csrc_lib("step", SRC))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _fold(lib, p):
    p = np.ascontiguousarray(p, F32)
    now, before = np.empty_like(p), np.empty_like(p)
    lib.step_fold(ctypes.c_int64(len(p)), _ptr(p), _ptr(now), _ptr(before))
    return now, before


def _rep(lib, x):
    x = np.ascontiguousarray(x, F32)
    now, before = np.empty_like(x), np.empty_like(x)
    lib.step_rep(ctypes.c_int64(len(x)), _ptr(x), _ptr(now), _ptr(before))
    return now, before


def _floor(lib, p, d, fast):
    p, d = np.ascontiguousarray(p, F32), np.ascontiguousarray(d, F32)
    now, before, shared = (np.empty(len(p), F32) for _ in range(3))
    lib.step_floor(ctypes.c_int64(len(p)), _ptr(p), _ptr(d), int(fast), _ptr(now), _ptr(before), _ptr(shared))
    assert np.array_equal(before.view(np.uint32), shared.view(np.uint32)) or np.array_equal(before, shared, equal_nan=True)  # the written-out dot is ground_dist's
    return now, before


def _same_bits(a, b):
    bad = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(len(a), -1).any(axis=1))
    return bad


def _dirs(rng, n):
    d = rng.normal(size=(n, 3)).astype(F32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(F32)
    d[::7, 1] = 0.0  # level rays: the fast plane divides by 1e-20
    d[3::7, 1] = np.abs(d[3::7, 1])
    return d


def _nudged(values):
    """every value and its two neighbours on either side (about zero: the two smallest denormals of either sign)"""
    v = np.asarray(values, F32)
    out = [v]
    for towards in (F32(np.inf), F32(-np.inf)):
        w = v
        for _ in range(2):
            w = np.nextafter(w, towards)
            out.append(w)
    return np.concatenate(out)


@pytest.mark.parametrize("seed", [1, 2])
def test_fold_and_floor_match_on_a_million_points(step_lib, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-300.0, 300.0, size=(1_000_000, 3)).astype(F32)
    now, before = _fold(step_lib, p)
    bad = _same_bits(now, before)
    assert len(bad) == 0, (len(bad), p[bad[0]], now[bad[0]], before[bad[0]])
    d = _dirs(rng, len(p))
    for fast in (True, False):
        now, before = _floor(step_lib, p, d, fast)
        bad = _same_bits(now, before)
        assert len(bad) == 0, (fast, len(bad), p[bad[0]], now[bad[0]], before[bad[0]])


def test_fold_matches_on_and_beside_every_multiple_of_ten(step_lib):
    """coordinates on, and 1 and 2 floats off, every multiple of 10 up to 2^20 (the cell borders, centres and mirror planes), both signs,
    each paired with another such coordinate, with itself (the diagonal wz = wx) and with its mirror image"""
    k = np.arange(0, (1 << 20) // 10 + 1, dtype=np.float64) * 10.0
    x = _nudged(np.concatenate([k, -k]).astype(F32))
    rng = np.random.default_rng(3)
    for z in (rng.permutation(x), x, -x, x + F32(20.0), np.zeros_like(x)):
        for a, b in ((x, z), (z, x)):
            p = np.stack([a, rng.uniform(-3, 6, len(x)).astype(F32), b.astype(F32)], axis=1)
            now, before = _fold(step_lib, p)
            bad = _same_bits(now, before)
            assert len(bad) == 0, (len(bad), p[bad[0]], now[bad[0]], before[bad[0]])
    # the folded cell is what walls() is written for: 0 <= wz <= wx <= 10
    assert (now[:, 2] >= 0).all() and (now[:, 2] <= now[:, 0]).all() and (now[:, 0] <= 10).all()


def _zeros_and_denormals():
    tiny = [0.0, 1e-45, 3e-42, 1.1754942e-38, 1.17549435e-38]  # +0, the smallest and a middling denormal, the largest one, the smallest normal
    v = np.array(tiny + [-t for t in tiny], F32)
    assert np.signbit(v[5]) and v[5] == 0
    return v


def test_fold_matches_for_zeros_and_denormals_of_every_sign(step_lib):
    v = np.concatenate([_zeros_and_denormals(), np.array([10.0, -10.0, 20.0, -20.0, 3.0, -7.5], F32)])
    p = np.array([(x, y, z) for x in v for y in v for z in v], F32)
    now, before = _fold(step_lib, p)
    assert len(_same_bits(now, before)) == 0


def test_floor_matches_for_zeros_and_denormals_of_every_sign(step_lib):
    """floor_dist's comment: the two fused multiply-adds are the dot for every input -- and the shorter forms it names are not: p.y + 0 parts
    from the dot exactly for p.y = -0 with p.x and p.z both negative (or -0), p.y alone exactly for p.y = -0 with one of them not"""
    v = np.concatenate([_zeros_and_denormals(), np.array([1.0, -1.0, 250.0, -250.0], F32)])
    p = np.array([(x, y, z) for x in v for y in v for z in v], F32)
    rng = np.random.default_rng(4)
    for fast in (True, False):
        for d in (_dirs(rng, len(p)), np.tile(np.array([[0.6, -0.8, 0.0]], F32), (len(p), 1)), np.tile(np.array([[0.6, 0.0, 0.8]], F32), (len(p), 1))):
            now, before = _floor(step_lib, p, d, fast)
            assert len(_same_bits(now, before)) == 0, fast
    minus0 = (p[:, 1] == 0) & np.signbit(p[:, 1])
    both_negative = np.signbit(p[:, 0]) & np.signbit(p[:, 2])
    assert (minus0 & both_negative).sum() == len(v) * len(v) // 4 and (minus0 & ~both_negative).sum() == 3 * len(v) * len(v) // 4
    _now, dot = _floor(step_lib, p, np.zeros_like(p), False)
    assert np.array_equal((p[:, 1] + F32(0.0)).view(np.uint32) != dot.view(np.uint32), minus0 & both_negative)
    assert np.array_equal(np.ascontiguousarray(p[:, 1]).view(np.uint32) != dot.view(np.uint32), minus0 & ~both_negative)


def test_a_zero_of_either_sign_is_the_same_distance_up_to_its_sign(step_lib):
    """floor_dist's comment, "a rendered pixel cannot tell": at y = -0, whatever the other two coordinates, the scene's distance is <= +0 (the ray
    ends there as a hit) and differs from the distance at y = +0 by the zero's sign at most"""
    rng = np.random.default_rng(5)
    n = 200_000
    xz = rng.uniform(-40.0, 40.0, size=(n, 2)).astype(F32)
    d = _dirs(rng, n)
    out = {}
    for name, y in (("minus", F32(-0.0)), ("plus", F32(0.0))):
        p = np.stack([xz[:, 0], np.full(n, y, F32), xz[:, 1]], axis=1)
        res = np.empty(n, F32)
        step_lib.step_dist(ctypes.c_int64(n), _ptr(np.ascontiguousarray(p)), _ptr(d), 1, _ptr(res))
        out[name] = res
    assert (out["minus"] <= 0).all() and (out["plus"] <= 0).all()
    assert np.array_equal(out["minus"], out["plus"])  # values: -0 == +0
    differ = out["minus"].view(np.uint32) != out["plus"].view(np.uint32)
    assert (out["minus"][differ] == 0).all() and differ.any() and (out["minus"] < 0).any()  # inside a wall the distance is the wall's, the same bits


def test_rep20_up_to_the_edge_of_its_domain(step_lib):
    """rep20's comment claims the fused form for |p| <= 67108848 (20 * floor is a float there): asserted on the inside, up to and
    including the edge; beyond it the claim ends, and the forms do part within the next few thousand floats"""
    rng = np.random.default_rng(6)
    inside = np.concatenate([
        (EDGE.view(np.int32) - np.arange(0, 200_000, dtype=np.int32)).view(F32),  # the last 200000 floats up to the edge
        rng.uniform(1 << 20, float(EDGE), 500_000).astype(F32),
        (F32(2.0) ** np.arange(20, 26, dtype=np.float32)).astype(F32), _nudged(F32(2.0) ** np.arange(20, 26, dtype=np.float32)),
    ])
    inside = inside[np.abs(inside) <= EDGE]
    assert inside.max() == EDGE
    for x in (inside, -inside):
        now, before = _rep(step_lib, x)
        bad = _same_bits(now, before)
        assert len(bad) == 0, (len(bad), x[bad[0]], now[bad[0]], before[bad[0]])
    # the first float beyond the edge and the ones after it: no claim, only a record that the edge is not far from where the forms part
    beyond = (EDGE.view(np.int32) + np.arange(1, 200_000, dtype=np.int32)).view(F32)
    now, before = _rep(step_lib, beyond)
    assert len(_same_bits(now, before)) > 0
    now, before = _rep(step_lib, -beyond)
    assert len(_same_bits(now, before)) > 0


def test_non_finite_coordinates_are_outside_the_domain(step_lib):
    """the comment beside fold: a non-finite p.x or p.z is a NaN of the repetition in both forms, which the swap kept in its place and
    max1 / min1 drop; no march reaches such a point (rep20's comment).  The floor's dot is NaN there, and so is floor_dist."""
    inf, nan = F32(np.inf), F32(np.nan)
    for bad_x in (inf, -inf, nan):
        now, before = _rep(step_lib, np.array([bad_x], F32))
        assert np.isnan(now[0]) and np.isnan(before[0])
        p = np.array([(bad_x, 1.5, 3.0), (3.0, 1.5, bad_x)], F32)
        now, before = _fold(step_lib, p)
        assert np.isnan(before[0, 0]) and before[0, 2] == 3.0 and np.isnan(before[1, 2]) and before[1, 0] == 3.0  # |rep(3)| = 3
        assert (now[:, 0] == 3.0).all() and (now[:, 2] == 3.0).all() and (now[:, 1] == 1.5).all()
        d = np.tile(np.array([[0.6, -0.8, 0.0]], F32), (2, 1))
        for fast in (True, False):
            now, before = _floor(step_lib, p, d, fast)
            assert np.isnan(before).all() and np.isnan(now).all()
    # a non-finite height is the same in both
    p = np.array([(1.0, inf, 2.0), (1.0, -inf, 2.0), (1.0, nan, 2.0)], F32)
    now, before = _floor(step_lib, p, np.tile(np.array([[0.6, -0.8, 0.0]], F32), (3, 1)), False)
    assert np.array_equal(now, before, equal_nan=True)


# ---- the pipeline -------------------------------------------------------------------------------------------------------
CAMERAS = lsc.cameras()


@pytest.fixture(scope="module")
def oracle_frames(oracle):
    """{camera name: (frame, oracle image, oracle per-pixel counters)}: rendered once, shared, left unchanged"""
    out = {}
    for cam in CAMERAS:
        f, _basis = lsc.oracle_frame(oracle, cam)
        ref, rst, _ = oracle.render("labyrinth", f, stats=True)
        ref.setflags(write=False)
        rst.setflags(write=False)
        out[cam[0]] = (f, ref, rst)
    return out


@pytest.mark.parametrize("name", [c[0] for c in CAMERAS])
def test_every_camera_sees_hits_and_misses(oracle_frames, name):
    """the oracle alone.  From above the floor: pixels whose rays all leave and pixels with hits, so that neither tier's comparison passes by
    seeing nothing.  From on or under the floor every primary ray ends at its first sample, as a hit of the floor (the fast plane is <= 0
    there): that is what those cameras are for, and their pixels still differ by the shading and the shadow rays."""
    _f, ref, rst = oracle_frames[name]
    if name.startswith(("sweep", "far")):
        no_hit = int((rst[..., 2] == 0).sum())
        assert lsc.W * lsc.H // 10 < no_hit < lsc.W * lsc.H * 9 // 10, (name, no_hit)
        assert len(np.unique(ref.reshape(-1, 4), axis=0)) > 500, name
    else:
        assert (rst[..., 2] >= 1).all() and int(rst[..., 1].max()) < 40, name
        if name != "below_floor":  # (from under the floor the hit is shaded black: nothing to tell pixels apart)
            assert len(np.unique(ref.reshape(-1, 4), axis=0)) > 500, name
        if name.startswith("minus0"):
            assert int(rst[..., 0].min()) == 2  # a shadow ray leaves every hit


@pytest.mark.parametrize("name", [c[0] for c in CAMERAS])
@pytest.mark.parametrize("shortcuts", [0, 1])
def test_host_pipeline_matches_the_oracle(oracle_frames, name, shortcuts):
    import hostsim

    f, ref, rst = oracle_frames[name]
    hf = hostsim.frame_from_oracle(f)
    hf.step_shortcuts = shortcuts
    img, st = hostsim.render("labyrinth", hf)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), (name, int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum()))
    assert np.array_equal(st[..., 0], rst[..., 0]) and np.array_equal(st[..., 2], rst[..., 2]), name
    if shortcuts:
        assert (st[..., 1] <= rst[..., 1]).all(), name
    else:
        assert np.array_equal(st[..., 1], rst[..., 1]), name


def test_host_pipeline_matches_the_oracle_with_reflective_marble(oracle):
    import hostsim

    f, _basis = lsc.oracle_frame(oracle, CAMERAS[1], extension_marble_reflection=0.25)
    ref, rst, _ = oracle.render("labyrinth", f, stats=True)
    f0, _ = lsc.oracle_frame(oracle, CAMERAS[1])
    assert int(rst[..., 0].sum()) > int(oracle.render("labyrinth", f0, stats=True)[1][..., 0].sum())  # the marble does reflect: more rays
    hf = hostsim.frame_from_oracle(f)
    hf.step_shortcuts = 0
    img, st = hostsim.render("labyrinth", hf)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)) and np.array_equal(st, rst)

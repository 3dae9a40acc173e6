"""CPU tier: the march's step for a ray's first three samples (march_advance_unrelaxed, sdfr_pixel.h), which the labyrinth's pixel kernel runs
as straight-line code in front of its march loop (PeelUnrelaxedSamples; render_pixel), against the general step it stands for there, march_pre +
march_advance: every field of the state and the status, bit for bit.  Random states and the edges -- a distance below dist_eps, negative, zero
of either sign, infinite, NaN, a sample beyond the range, an iteration limit of 1 to 4 -- then whole rays: three specialised passes, the
factor, the general passes, against the general schedule; and the same with the factor one sample early, which has to show."""
import ctypes
import os

import numpy as np
import pytest

import cppbuild

SRC = os.path.join(cppbuild.HERE, "cpp", "march_peel_host.cpp")
F32, U32, I32 = np.float32, np.uint32, np.int32
DIST_EPS = 1e-4
CONTINUE, HIT, MISS = 0, 1, 2
FIELDS = ["start.x", "start.y", "start.z", "dir.x", "dir.y", "dir.z", "t", "last_d", "last_safe", "factor", "d", "iter"]
# what an evaluation can return: ordinary steps, a hit by a hair on either side of dist_eps, inside a body, zeros, infinities, NaNs of both signs
EDGE_D = np.array([0.5, 3.0, 1e-4, np.nextafter(F32(1e-4), F32(0)), np.nextafter(F32(1e-4), F32(1)), 1e-5, 0.0, -0.0, -0.25, -1e-30, 1e-40, np.inf, -np.inf,
                   np.nan, -np.nan, 3e38], F32)


@pytest.fixture(scope="module")
def peel_lib():
    return ctypes.CDLL(cppbuild.csrc_lib("march_peel", SRC))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _one_nan(words):
    """every NaN of the float fields as the one quiet NaN: where two NaNs meet in a sum (a ray whose distance was NaN twice) the result's sign and
    payload are those of the operand the host's add instruction happens to name first, which no source text decides; NaN or not is compared"""
    out = words.copy()
    f = out[:, :11]
    f[np.isnan(f.view(F32))] = 0x7FC00000
    return out


def _same(general, special, gst, sst, what):
    general, special = _one_nan(general), _one_nan(special)
    bad = np.nonzero((general != special).any(axis=1) | (gst != sst))[0]
    assert bad.size == 0, (what, int(bad.size), int(bad[0]), [(FIELDS[k], hex(general[bad[0], k]), hex(special[bad[0], k])) for k in range(12) if general[bad[0], k] != special[bad[0], k]],
                           int(gst[bad[0]]), int(sst[bad[0]]))


def _states(rng, n):
    """n march states as the first three passes can meet them (factor 1, iter 0 .. 2), the rest anything: [n, 12] words"""
    f = np.empty((n, 11), F32)
    f[:, 0:6] = rng.uniform(-30, 30, (n, 6))
    f[:, 6] = rng.uniform(0, 60, n) * (rng.random(n) < 0.9)  # t; a tenth at the ray's start
    f[:, 7] = rng.uniform(-1, 5, n)
    f[:, 8] = rng.uniform(0, 60, n)
    f[:, 9] = 1.0
    f[:, 10] = rng.uniform(-1, 5, n)
    w = np.empty((n, 12), U32)
    w[:, :11] = f.view(U32)
    w[:, 11] = rng.integers(0, 3, n)
    return w


def test_one_pass_is_march_pre_and_march_advance(peel_lib):
    rng = np.random.default_rng(19)
    n = 40000
    state = _states(rng, n)
    d = rng.uniform(-0.5, 4, n).astype(F32)
    edge = rng.random(n) < 0.5
    d[edge] = rng.choice(EDGE_D, int(edge.sum()))
    t = state[:, 6].view(F32)
    # the range: far, short of the sample, and the sample's own distance (t > range is false there) with its neighbours
    dist_max = np.where(rng.random(n) < 0.5, F32(100.0), rng.uniform(-1, 60, n).astype(F32)).astype(F32)
    near = rng.random(n) < 0.2
    dist_max[near] = np.nextafter(t[near], rng.choice(np.array([-1, 0, 100], F32), int(near.sum())).astype(F32))
    # the limit: 1 .. 4 and the usual ones, above the state's count as march_advance requires
    iter_count = np.maximum(rng.choice(np.array([1, 2, 3, 4, 5, 100, 256], U32), n), state[:, 11] + 1).astype(U32)
    gen, spe = np.empty_like(state), np.empty_like(state)
    gst, sst = np.empty(n, I32), np.empty(n, I32)
    peel_lib.peel_one(ctypes.c_int64(n), _ptr(state), _ptr(d), _ptr(dist_max), _ptr(iter_count), ctypes.c_float(DIST_EPS), _ptr(gen), _ptr(gst), _ptr(spe), _ptr(sst))
    _same(gen, spe, gst, sst, "one pass")
    # the cases did not all go one way: every status, stops by range and by distance, rays ended by each limit, NaN samples that march on
    assert set(np.unique(gst)) == {CONTINUE, HIT, MISS}
    out_of_range = t > dist_max
    assert (out_of_range & (gst == MISS)).sum() > 1000 and (~out_of_range & (d < F32(DIST_EPS)) & (gst == HIT)).sum() > 1000
    for limit in (1, 2, 3):
        ended = (iter_count == limit) & (state[:, 11] == limit - 1) & ~out_of_range & ~(d < F32(DIST_EPS))
        assert ended.sum() > 50 and (gst[ended] == MISS).all() and (gen[ended, 11] == limit).all()
    assert (np.isnan(d) & (gst == CONTINUE)).sum() > 100
    assert (gen[:, 9].view(F32) == 1.0).all()  # the factor stays: march_pre changes it at the fourth sample


def _rays(rng, n, samples):
    start_dir = rng.uniform(-30, 30, (n, 6)).astype(F32)
    d = rng.uniform(1.0, 1.9, (n, samples)).astype(F32)  # (no distance below half the one before: relaxed steps over-step only where made to, below)
    edge = rng.random((n, samples)) < 0.15
    d[edge] = rng.choice(EDGE_D, int(edge.sum()))
    if samples >= 4:
        # a hit at the fourth sample, the first relaxed one, is a hit only if it is no over-step: more than half the third distance, which was no hit
        graze = rng.random(n) < 0.05
        d[graze, :4] = np.array([0.6, 0.3, 1.5 * DIST_EPS, 0.9 * DIST_EPS], F32)
    # relaxed steps that over-step: a distance much smaller than the one before (last_d + d < 1.5 last_d), from the fifth sample on
    small = rng.random((n, samples)) < 0.15
    small[:, :4] = False
    d[small] = (np.roll(d, 1, axis=1)[small] * rng.uniform(0.05, 0.45, int(small.sum()))).astype(F32)
    dist_max = np.where(rng.random(n) < 0.6, F32(100.0), rng.uniform(-1, 8, n).astype(F32)).astype(F32)
    iter_count = rng.choice(np.array([1, 2, 3, 4, 5, 100, 256], U32), n, p=[0.06, 0.06, 0.06, 0.06, 0.06, 0.35, 0.35]).astype(U32)
    return start_dir, np.ascontiguousarray(d), dist_max, iter_count


def _run_rays(lib, rays, samples, peeled):
    start_dir, d, dist_max, iter_count = rays
    n = len(dist_max)
    gen, spe = np.empty((n, 12), U32), np.empty((n, 12), U32)
    gst, sst, passes = np.empty(n, I32), np.empty(n, I32), np.empty(n, I32)
    lib.peel_ray(ctypes.c_int64(n), samples, peeled, _ptr(start_dir), _ptr(d), _ptr(dist_max), _ptr(iter_count), ctypes.c_float(DIST_EPS),
                 _ptr(gen), _ptr(gst), _ptr(spe), _ptr(sst), _ptr(passes))
    return gen, spe, gst, sst, passes


@pytest.mark.parametrize("samples", [1, 2, 3, 4, 9])
def test_peeled_rays_are_the_general_march(peel_lib, samples):
    """`samples` evaluations of a ray from its start.  After three, the specialised passes and the factor against three general passes and
    march_pre; after nine, the relaxed passes behind them as well, rewinds among them"""
    rays = _rays(np.random.default_rng(100 + samples), 20000, samples)
    gen, spe, gst, sst, passes = _run_rays(peel_lib, rays, samples, 3)
    _same(gen, spe, gst, sst, "%d samples" % samples)
    going = gst == CONTINUE
    if samples >= 3:
        assert (gen[going, 9].view(F32) > 1.0).sum() > 300  # relaxed rays
    else:
        assert (gen[:, 9].view(F32) == 1.0).all()
    for k in range(1, min(samples, 4) + 1):  # rays that ended at each sample, by hit and by miss
        assert ((passes == k) & (gst == HIT)).sum() > 20 and ((passes == k) & (gst == MISS)).sum() > 20, k
    if samples == 9:
        assert (going & (gen[:, 9].view(F32) == 1.0) & (gen[:, 11] > 4)).sum() > 100  # rays that rewound after the fourth sample and march on


def test_the_factor_one_sample_early_shows(peel_lib):
    """the negative control: two specialised passes, then the factor -- the third sample is stepped over with 1.5 times its distance, or taken
    back.  (Read after that sample: the rays' later distances are given, not measured where the march stands.)"""
    rays = _rays(np.random.default_rng(7), 20000, 3)
    gen, spe, gst, sst, _passes = _run_rays(peel_lib, rays, 3, 2)
    differ = (gen != spe).any(axis=1) | (gst != sst)
    assert (gst == CONTINUE).sum() > 5000 and (differ[gst == CONTINUE]).mean() > 0.9
    with pytest.raises(AssertionError):
        _same(gen, spe, gst, sst, "factor early")

"""The labyrinth frames of the tests of the peeled march (PeelUnrelaxedSamples, sdfr_scene_traits.h: a ray's first three samples as straight-line code
in front of the march loop): tests/test_march_peel_pipeline_cpu.py on the host build, tests/test_gpu_march_peel.py on the kernels.  Each case is
an eye of tests/labyrinth_shed_cameras.py or one of its own, with limits of its own, and is rendered with every iteration limit of ITER_COUNTS:
1, 2 and 3 end every ray inside the peeled passes, 4 in the first pass of the loop behind them.

What the cases have to contain is checked on the oracle alone (classify; the tests assert it): primary rays that end at their first, second,
third and fourth sample, each by a hit, by the range and by the iteration limit, and rays that rewind after the fourth."""
import functools

import numpy as np

import labyrinth_shed_cameras as cams

W, H = 96, 54
ITER_COUNTS = [1, 2, 3, 4, 5, 100, 256]
LIMITS = dict(bounce_count=16, ray_count=8, light_count=8, range=100.0, max_cost_default=7, extension_lights=0, extension_marble_reflection=0.0,
              dist_eps=0.0001, grad_eps=0.0001, reflect_eps=0.001, refract_eps=0.001, shadow_eps=0.0003)
_SHED = {c[0]: c for c in cams.cameras()}
PRIMARY = dict(bounce_count=1)  # primary rays alone: a pixel's counters are its one ray's


def _eye(name, eye, view):
    return (name, "dir", eye, view, 0.3)


# 4.2e-4 in front of wall 1's face z = 2, looking along it: the distance shrinks by the same factor from sample to sample, and the rays reach
# dist_eps at their second, third, fourth ... sample depending on their slant
_NEAR_WALL = _eye("near_wall", (3.5, 2.0, 2.0 - 4.2e-4), (0.8, 0.05, 0.45))
# name -> (camera, limits that differ from LIMITS)
CASES = {
    "sweep0": (_SHED["sweep0"], {}),
    "sweep5": (_SHED["sweep5"], {}),
    "sweep11": (_SHED["sweep11"], {}),
    "sweep5_short_range": (_SHED["sweep5"], dict(range=3.0)),                       # shadow rays and primary rays that run out of range
    "inside_wall": (_SHED["inside_wall1"], {}),                                     # the first sample is a hit
    "above_looking_up": (_eye("above_looking_up", (3.0, 6.0, 5.5), (0.3, 0.8, 0.4)), {}),  # above the wall tops (y = 4.01), rising: escapes before any evaluation
    "on_floor": (_eye("on_floor", (1.0, 0.0, 1.0), (0.6, -0.3, 0.7)), {}),
    "below_floor": (_SHED["below_floor"], {}),
    "near_wall": (_NEAR_WALL, {}),
    "primary_near_wall": (_NEAR_WALL, dict(PRIMARY, range=9.24e-4)),                # hits at samples 2, 3, 4; the range at 3 and 4; rewinds
    "primary_inside_wall": (_SHED["inside_wall1"], PRIMARY),                        # hits at sample 1
    "primary_range_half": (_SHED["sweep5"], dict(PRIMARY, range=0.5)),              # the first step is longer: out of range at sample 2
    "primary_range_negative": (_SHED["sweep5"], dict(PRIMARY, range=-1.0)),         # out of range where the ray starts: sample 1
}


def limits_of(case, iter_count):
    out = dict(LIMITS, iter_count=iter_count)
    out.update(CASES[case][1])
    return out


def oracle_frame(case, iter_count):
    """-> (the oracle's frame, its camera basis)"""
    from oracle import pyoracle as po

    return cams.oracle_frame(po, CASES[case][0], W, H, **limits_of(case, iter_count))


@functools.lru_cache(maxsize=None)
def reference(case, iter_count):
    """the oracle's render: (basis, image, per-pixel rays / evaluations / hits, totals), made once and read-only"""
    from oracle import pyoracle as po

    f, basis = oracle_frame(case, iter_count)
    img, st, tot = po.render("labyrinth", f, stats=True)
    for a in (img, st, tot):
        a.setflags(write=False)
    return basis, img, st, tot


def _rewinds_after_the_fourth(case):
    """pixels whose primary ray rewinds at its fifth to twelfth sample, from the oracle's own march (tests/cpp/query_oracle.h: march_ray through
    the pixel, which leaves the distance it reached): the three counters do not show a rewind, the distance does -- between the iteration
    limits K - 1 and K it goes back only if the K-th sample was taken back, the ray ended by neither limit's run"""
    import query_util as qu

    ys, xs = np.mgrid[0:H, 0:W]
    px = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)
    rewound, before = np.zeros(len(px), bool), None
    for k in range(4, 13):
        h = qu.oracle_pick("labyrinth", oracle_frame(case, k)[0], px)
        now = (h[:, 0].view(np.float32).copy(), h[:, 8] == k, h[:, 10] == 0)  # distance, ended by the limit, no hit
        if before is not None:
            rewound |= now[1] & now[2] & before[1] & before[2] & (now[0] < before[0])
        before = now
    return int(rewound.sum())


def classify():
    """{("hit" | "range" | "limit", sample 1 .. 4): pixels, "rewinds": pixels} over the cases of primary rays alone, from the oracle: a ray that
    ends at sample n with the limit 256 ended by a hit or, a miss, by the range; with the limit n, a miss after n evaluations that marches on
    under the limit 256 ended by the limit"""
    out = {(how, n): 0 for how in ("hit", "range", "limit") for n in (1, 2, 3, 4)}
    out["rewinds"] = 0
    for case, (_cam, own) in CASES.items():
        if own.get("bounce_count") != 1:
            continue
        full = reference(case, 256)[2]
        assert (full[..., 0] == 1).all()
        for n in (1, 2, 3, 4):
            out["hit", n] += int(((full[..., 1] == n) & (full[..., 2] == 1)).sum())
            out["range", n] += int(((full[..., 1] == n) & (full[..., 2] == 0)).sum())
            cut = reference(case, n)[2]
            out["limit", n] += int(((cut[..., 1] == n) & (cut[..., 2] == 0) & (full[..., 1] > n)).sum())
        out["rewinds"] += _rewinds_after_the_fourth(case)
    return out

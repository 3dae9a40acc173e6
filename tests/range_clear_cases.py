"""The labyrinth frames of the tests of SceneLabyrinth::ray_bounds (RayBounds, sdfr_scene_traits.h: a descending ray that is still above the wall
tops, y = 4.01, where its range ends is a miss before its first evaluation): tests/test_range_clear_pipeline_cpu.py on the host build,
tests/test_gpu_range_clear.py on the kernels.  96 x 54 pixels, a field of view of 60 degrees: a row is about 0.02 in dir.y.

The band of a frame is its primary rays with dir.y < 0 and eye.y + range * dir.y > 4.01.  Pixel directions are formed here as the frame's
basis gives them, in double precision; a pixel within MARGIN of either edge of the band counts neither as in it nor as below it, so that no
assertion hangs on the last bit of a direction."""
import functools

import numpy as np

import march_peel_cases as mp

W, H = mp.W, mp.H
ITER_COUNTS = [1, 3, 100, 256]
TOP = 4.01
MARGIN = 1e-4

# name -> (camera, limits that differ from march_peel_cases.LIMITS, wide: the band is many rows)
CASES = {
    # eye at 6 with a range of 10: the band is dir.y in (-0.199, 0), about ten rows
    "short_range": (mp._eye("short_range", (3.0, 6.0, 5.5), (0.6, -0.1, 0.7)), dict(range=10.0), True),
    # eye at 30 with the default range: dir.y in (-0.2599, 0)
    "high_eye": (mp._eye("high_eye", (3.0, 30.0, 5.5), (0.6, -0.15, 0.7)), {}, True),
    # the benchmark's geometry: eye at 5, range 100: the band is dir.y in (-0.0099, 0), half a row of this frame.  Looking along
    # dir.y = -0.005 the rows next to the middle of the frame pass it on either side (dir.y = +0.0057 and -0.0157): no pixel in the band, the
    # nearest misses to it.  Looking along +0.0057 the first row under the middle has dir.y = -0.005: one row in the band.
    "bench_geometry": (mp._eye("bench_geometry", (1.5, 5.0, 0.5), (0.65, -0.005, 0.76)), {}, False),
    "bench_geometry_row": (mp._eye("bench_geometry_row", (1.5, 5.0, 0.5), (0.65, 0.0057, 0.76)), {}, False),
    # between the walls: no ray of the frame is in the band (its shadow rays towards the sun rise anyway)
    "between_walls": (mp._eye("between_walls", (1.0, 2.0, 1.0), (0.6, -0.1, 0.7)), {}, False),
}


def limits_of(case, iter_count):
    out = dict(mp.LIMITS, iter_count=iter_count)
    out.update(CASES[case][1])
    return out


def oracle_frame(case, iter_count):
    """-> (the oracle's frame, its camera basis)"""
    from oracle import pyoracle as po

    return mp.cams.oracle_frame(po, CASES[case][0], W, H, **limits_of(case, iter_count))


@functools.lru_cache(maxsize=None)
def reference(case, iter_count):
    """the oracle's render: (basis, image, per-pixel rays / evaluations / hits, totals), made once and read-only"""
    from oracle import pyoracle as po

    f, basis = oracle_frame(case, iter_count)
    img, st, tot = po.render("labyrinth", f, stats=True)
    for a in (img, st, tot):
        a.setflags(write=False)
    return basis, img, st, tot


def pixel_dir_y(basis, width, height, xs, ys):
    """dir.y of the primary rays through pixels (xs, ys): normalize(front + sx right + sy top), sx = (x + 0.5) / W * 2 - 1, sy = 1 - (y + 0.5) / H * 2"""
    front, right, top = (np.asarray(basis[i], np.float64) for i in (1, 2, 3))
    sx = (np.asarray(xs, np.float64) + 0.5) / width * 2.0 - 1.0
    sy = 1.0 - (np.asarray(ys, np.float64) + 0.5) / height * 2.0
    d = front[None, :] + sx[..., None] * right[None, :] + sy[..., None] * top[None, :]
    return d[..., 1] / np.sqrt((d * d).sum(axis=-1))


def band_masks(basis, width, height, xs, ys, reach):
    """-> (in the band for certain, descending and below the band for certain, possibly in the band, just below the band: no more than
    three times as steep as its lower edge) for pixels (xs, ys); reach = the range"""
    eye_y = float(basis[0][1])
    dy = pixel_dir_y(basis, width, height, xs, ys)
    end = eye_y + reach * dy
    inside = (dy < -1e-7) & (end > TOP + MARGIN)
    below = (dy < 0.0) & (end < TOP - MARGIN)
    maybe = (dy < 1e-7) & (end > TOP - MARGIN)
    just_below = below & (end > eye_y - 3.0 * (eye_y - TOP))
    return inside, below, maybe, just_below


@functools.lru_cache(maxsize=None)
def masks(case):
    basis = reference(case, 256)[0]
    ys, xs = np.mgrid[0:H, 0:W]
    out = band_masks(basis, W, H, xs, ys, limits_of(case, 256)["range"])
    for a in out:
        a.setflags(write=False)
    return out

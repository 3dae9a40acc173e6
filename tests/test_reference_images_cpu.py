"""The oracle against the reference's OWN rendered frames (missing item 1).

The reference holds screenshots of this very path: Images/*.png, 1200 x 800, taken from its window
(README.md:30-104; window size, fovy 60 deg, aspect 1.5, roll 0: Engine/Application.cpp:39-40, 214-224).  Camera and time
are not recorded, but they are seven numbers: tools/fit_reference_images.py found them by least squares on the oracle's
frame pushed through the oracle's HDR::process (fp16 target, bloom, tone map, unorm8), and tests/golden/reference_images.json
keeps them with the statistics of |oracle - screenshot|.  This test re-renders at the committed parameters and asserts the
statistics on a fixed sample of each screenshot, every 16th row (tests/golden/reference/screenshots/: RGB and edge flag, made
by tools/make_reference_fixtures.py; `sample_stats` beside the full-frame `stats`).

What this pins that nothing else does: oracle/driver.h (ray generation, march, normal, shading, shadow / reflection /
refraction rays, queue order), sdf_lib.h (primitives, operators, checker filter, sky), noise.h (the sky and the marble are
simplex turbulence: a wrong permutation or gradient is a different cloud), postprocess.h (bloom, tone map) -- against pixels
the reference's HLSL produced on its author's GPU.  Sixteen screenshots; the worst of them has 92 % of ALL pixels within 3 / 255
(what is left there: the sky mirrored in cube tops, flame shapes, edge pixels shifted by a fraction of a pixel)."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

with open(os.path.join(HERE, "golden", "reference_images.json")) as _f:
    FITS = json.load(_f)["images"]
SAMPLES = os.path.join(HERE, "golden", "reference", "screenshots")


def _params(e):
    return list(e["eye"]) + [e["yaw"], e["pitch"], e["stime"]]


@pytest.mark.parametrize("name", sorted(FITS))
def test_oracle_reproduces_the_reference_s_screenshot(oracle, name):
    import fit_reference_images as fr

    e = FITS[name]
    assert fr.TARGETS[name][0] == e["file"] and fr.TARGETS[name][1] == e["scene"] and fr.TARGETS[name][3] == e.get("variables", {})
    assert fr.ROWS_FROM.get(name, 0) == e.get("rows_from", 0)  # (spiral.png: from the horizon down, its sky is an older one)
    # the sample stands for the whole screenshot: its statistics (committed) are those of the full frame (committed by the fit).
    # Both numbers are stored, so this runs no code: it attests that the fixture was representative when it was made
    # (tools/make_reference_fixtures.py); what the oracle computes today is checked below.
    full, want = e["stats"], e["sample_stats"]
    assert abs(full["mean_abs_err"] - want["mean_abs_err"]) < 0.02 and abs(full["within_3"] - want["within_3"]) < 0.003, (full, want)
    stats, _d = fr.compare_sample(name, _params(e), SAMPLES, variables=e.get("variables", {}))
    # the committed statistics are reproduced (same oracle, same screenshot) ...
    assert abs(stats["mean_abs_err"] - want["mean_abs_err"]) < 0.02 and abs(stats["within_3"] - want["within_3"]) < 0.003, (stats, want)
    # ... and they say "agrees": all pixels, edges included.  (lense1.png carries its own limits: four bounces of reflection and refraction
    # between two lattices of mirrors turn the last bit of the reference's GPU arithmetic into salt-and-pepper on 6 % of its pixels.)
    lim = dict(mean_abs_err=0.6, within_3=0.92, within_8=0.985, flat_within_8=0.99)
    lim.update(e.get("limits", {}))
    assert stats["mean_abs_err"] < lim["mean_abs_err"], stats
    assert stats["within_3"] > lim["within_3"] and stats["within_8"] > lim["within_8"], stats
    assert stats["flat_within_8"] > lim["flat_within_8"], stats
    assert stats["rays"] == full["rays"]


def test_the_statistic_tells_a_wrong_scene_from_the_right_one(oracle):
    """Images/multi-lights.png was taken with an older version of sdf_scene_light_shadows.hlsl: with today's file at the same
    camera the five lights stand in the same places but wear the colours in reverse order, and the comparison says so loudly;
    with the lights' phases stepped the other way (oracle scene light_shadows_backwards) it agrees."""
    import fit_reference_images as fr

    e = FITS["multi-lights"]
    p = _params(e)
    p[5] = 7.85  # today's file puts the lights where the screenshot has them at this time (fitted the same way)
    stats, _d = fr.compare_sample("multi-lights-todays-file", p, SAMPLES)
    assert stats["mean_abs_err"] > 10.0 and stats["within_3"] < 0.3, stats


def test_a_camera_a_hundredth_off_is_noticed(oracle):
    import fit_reference_images as fr

    e = FITS["sphere"]
    p = _params(e)
    good, _d = fr.compare_sample("sphere", p, SAMPLES)
    p[0] += 0.01
    off, _d = fr.compare_sample("sphere", p, SAMPLES)
    assert good["within_3"] > 0.999 and off["within_3"] < 0.99 and off["mean_abs_err"] > 5 * good["mean_abs_err"]


@pytest.mark.parametrize("name", sorted(n for n in FITS if FITS[n].get("variables")))
def test_moved_sliders_sit_on_their_grid(oracle, name):
    """Some screenshots were taken with sliders of the variable panel moved (neon: the glow's colour; coordinate material: the cutting
    box and the line threshold).  The values least squares finds are recorded rounded; here: they lie on the sliders' grids (the
    `step=` of the scene file's VAR_ tags -- the reference's VariableManager moves a slider in whole steps) within their ranges, and
    with the scene file's defaults the comparison fails loudly."""
    import fit_reference_images as fr

    e = FITS[name]
    table = {row[0]: row for row in oracle.var_table(e["scene"])}
    for k, v in e["variables"].items():
        step = table[k][4]
        assert abs(v / step - round(v / step)) < 1e-3 and table[k][1] <= v <= table[k][2], (k, v)
    defaults, _d = fr.compare_sample(name, _params(e), SAMPLES, variables={})
    assert defaults["mean_abs_err"] > 3.0 and defaults["within_3"] < 0.9, defaults

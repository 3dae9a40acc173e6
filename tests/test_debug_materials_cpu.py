"""CPU tier, SURVEY.md 8(f)-4: the driver's debug material views MATERIAL_ITER / PLAIN / NORMAL1 /
NORMAL2 (pshader_sdf.hlsl:430-455; iter_count_to_color, sdf_materials.hlsl:143-186).  No scene of
the reference emits them, so a test scene does (oracle/test_scenes.h; the library's diagnostic scene
"debug_materials", csrc/sdfr_scene_debug.h): the oracle against a numpy statement of the colour
rules at chosen pixels, and the host build of the product's pipeline stages against the oracle."""
import numpy as np
import pytest

from frame_cases import MATERIALS_CAMS as CAMS, materials_frame as _frame


def _heat(it, max_it):
    """iter_count_to_color (sdf_materials.hlsl:156-186) in fp32; lerp(a, b, t) = fma(t, b - a, a)"""
    rel = np.float32(it) / np.float32(max_it)
    stops = [(np.float32(0.1), (0, 0, 0), (0, 0, 1), np.float32(0.0), np.float32(0.1)), (np.float32(0.5), (0, 0, 1), (0, 1, 0), np.float32(0.1), np.float32(0.4)),
             (np.float32(0.9), (0, 1, 0), (1, 1, 0), np.float32(0.5), np.float32(0.4)), (np.float32(np.inf), (1, 1, 0), (1, 0, 0), np.float32(0.9), np.float32(0.1))]
    for lim, a, b, off, span in stops:
        if rel < lim:
            t = (rel - off) / span
            return np.array([np.float32(np.float64(t) * (b[i] - a[i]) + a[i]) for i in range(3)], np.float32)


@pytest.mark.parametrize("iter_count", [100, 37])
def test_oracle_colours_follow_the_reference_rules(oracle, iter_count):
    f = _frame(oracle, CAMS[0], iter_count)
    img, st, _ = oracle.render("debug_materials", f, stats=True)
    # primary-ray-only pixels (one ray, it hit): the ball is unlit, coloured by the march iterations
    # of THAT ray relative to ITER_COUNT - 1, and switches tone mapping off (alpha 0)
    only = (st[..., 0] == 1) & (st[..., 2] == 1)
    assert only.sum() > 200
    ys, xs = np.nonzero(only)
    seen = set()
    for y, x in zip(ys, xs):
        evals = int(st[y, x, 1])
        # a hit after k evaluations has iter = k - 1 (+ rewinds, which the evaluation count includes)
        want = _heat(evals - 1, iter_count - 1)
        px = img[y, x]
        if px[3] == 0.0 and np.array_equal(px[:3], want):
            seen.add(evals)
    assert len(seen) >= 5, seen  # several different iteration colours, bit-equal to the rule
    # the four views are all on screen: heat colours (blue / green ramps, alpha 0), the plain block's
    # colour mixed with its reflections (alpha 1), normal colours (alpha 0, max channel exactly 1 for NORMAL1)
    a0 = img[img[..., 3] == 0.0][:, :3]
    assert len(a0) > 500
    assert ((a0.max(axis=1) == 1.0) & (a0.min(axis=1) >= np.float32(0.01) / 1.0 - 1e-3)).sum() > 50  # NORMAL1: normalised to max 1, floor 0.01
    plain = (np.abs(img[..., 0] - 0.2) < 0.2) & (np.abs(img[..., 2] - 0.9) < 0.35) & (img[..., 3] == 1.0) & (st[..., 0] >= 2)
    assert plain.sum() > 50  # PLAIN: unlit diffuse + a reflection ray


@pytest.mark.parametrize("cam", range(len(CAMS)))
@pytest.mark.parametrize("iter_count,extra", [(100, {}), (37, {}), (250, dict(max_cost_default=9)), (64, dict(debug_ny=1.0, debug_y=0.3))])
def test_pipeline_stages_host_build_vs_oracle(oracle, cam, iter_count, extra):
    import hostsim

    f = _frame(oracle, CAMS[cam], iter_count, **extra)
    ref, rst, _ = oracle.render("debug_materials", f, stats=True)
    img, st = hostsim.render("debug_materials", hostsim.frame_from_oracle(f))
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), (cam, iter_count, extra)
    assert np.array_equal(st, rst)


def test_debug_scene_is_not_in_the_reference_scene_list(oracle):
    import sdf_playground_amd as sp

    assert "debug_materials" not in oracle.scene_names() and len(oracle.scene_names()) == 22
    assert "debug_materials" not in sp.scene_names() and len(sp.scene_names()) == 22

"""CPU tier: the oracle and the host build of the product's pipeline stages against the
committed golden fixtures, and against each other."""
import math

import numpy as np
import pytest

import golden_util as gu


@pytest.mark.parametrize("path", gu.golden_files(), ids=lambda p: p.split("/")[-1][:-4])
def test_oracle_reproduces_golden(oracle, path):
    g = np.load(path)
    f = gu.oracle_frame(oracle, g)
    img, st, tot = oracle.render(gu.scene_of(path), f, stats=True)
    assert np.array_equal(img.view(np.uint32), g["rgba"].view(np.uint32))
    assert np.array_equal(st, g["stats"].astype(np.uint32))
    assert np.array_equal(tot, g["totals"])
    # alpha is the tone-mapping flag (pshader_sdf.hlsl:636-638)
    assert set(np.unique(img[..., 3])) <= {0.0, 1.0}


@pytest.mark.parametrize("path", gu.golden_files(), ids=lambda p: p.split("/")[-1][:-4])
def test_pipeline_stages_host_build_reproduce_golden(oracle, path):
    """The product's per-pixel stages (sdf_playground_amd/csrc/*.h) compiled for the CPU by
    tests/hostsim -- a test-only build -- must agree bit for bit with the fixtures."""
    import hostsim

    g = np.load(path)
    f = hostsim.frame_from_oracle(gu.oracle_frame(oracle, g))
    img, st = hostsim.render(gu.scene_of(path), f)
    assert np.array_equal(img.view(np.uint32), g["rgba"].view(np.uint32))
    assert np.array_equal(st, g["stats"].astype(np.uint32))


def test_camera_of_golden_inputs(oracle):
    # the fixtures' camera basis is what the camera restatement gives for the recorded eye/target
    fovy = np.float32(60.0) * np.float32(3.14159265358979) / np.float32(180.0)
    for path in gu.golden_files():
        g = np.load(path)
        fn = oracle.camera_direction if bool(g["target_is_direction"]) else oracle.camera_lookat
        b = fn(g["eye"], g["target"], fovy, np.float32(1.0))
        assert np.array_equal(b.view(np.uint32), g["basis"].view(np.uint32))


def test_detmath_product_vs_oracle_bitwise(oracle):
    """Two independent statements of the deterministic elementary functions (oracle/detmath.h
    and sdf_playground_amd/csrc/sdfr_math.h) must agree on every sampled input."""
    import hostsim

    L = hostsim.lib()
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.uniform(-3000, 3000, 20000), rng.uniform(-1e-3, 1e-3, 2000), [0.0, -0.0, 1e30, -1e30, np.inf, np.nan]]).astype(np.float32)
    ys = rng.uniform(-10, 10, len(xs)).astype(np.float32)
    for idx, name in [(0, "sin"), (1, "cos"), (3, "exp2"), (4, "log2")]:
        for x in xs[:6000]:
            a = np.float32(L.hostsim_math(idx, float(x), 0.0))
            b = oracle.kat(name, x)[0]
            assert a.view(np.uint32) == b.view(np.uint32) or (np.isnan(a) and np.isnan(b)), (name, x)
    for x, y in zip(xs[:6000], ys[:6000]):
        for idx, name in [(2, "atan2"), (5, "pow"), (6, "fmod"), (7, "min"), (8, "max")]:
            a = np.float32(L.hostsim_math(idx, float(x), float(y)))
            b = oracle.kat(name, x, y)[0]
            assert a.view(np.uint32) == b.view(np.uint32) or (np.isnan(a) and np.isnan(b)), (name, x, y)


def test_extension_limits_and_debug_views_host_vs_oracle(oracle):
    """Run-time limits (extensions of the reference's #defines) and the driver's debug
    variables: host build of the pipeline stages vs oracle, bit for bit."""
    import hostsim

    cases = [
        ("fast_sphere", dict(iter_count=64, max_cost_default=2), {}),
        ("cube_sea", dict(iter_count=128, max_cost_default=6), {}),
        ("labyrinth", dict(iter_count=256), {}),
        ("labyrinth", dict(iter_count=256, extension_marble_reflection=0.25), {}),  # BASELINE configs[2] as worded: reflective marble
        ("light_shadows", dict(ray_count=4, bounce_count=6), {}),
        ("lense", dict(max_cost_default=9), dict(scene_var=(1.5, -0.5, 9.0, 0.8))),
        ("labyrinth", {}, dict(debug_ny=1.0, debug_y=1.5, debug_scale=0.5)),
        ("fractal", {}, dict(show_objects=0.0, debug_nx=0.3, debug_ny=1.0, debug_y=0.2)),
        ("gems", dict(light_count=0, bounce_count=0), {}),
    ]
    for scene, limits, variables in cases:
        g = np.load([p for p in gu.golden_files() if gu.scene_of(p) == scene][0])
        f = gu.oracle_frame(oracle, g)
        f.width, f.height = 48, 32
        for k, v in limits.items():
            setattr(f, k, v)
        for k, v in variables.items():
            if k == "scene_var":
                for i, x in enumerate(v):
                    f.scene_var[i] = x
            else:
                setattr(f, k, v)
        ref, rst, _ = oracle.render(scene, f, stats=True)
        img, st = hostsim.render(scene, hostsim.frame_from_oracle(f))
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), (scene, limits, variables)
        assert np.array_equal(st, rst)


def test_fast_math_domain_is_respected_on_all_scenes(oracle):
    """The kernels' fast exact sqrt / constant division are valid on a stated domain
    (sdfr_math.h).  The counting build of the oracle records every sqrt argument and every
    constant-division numerator outside it: none on any scene."""
    oracle.build(census=True, ref=False)
    for path in gu.golden_files():
        g = np.load(path)
        f = gu.oracle_frame(oracle, g)
        f.width, f.height = 40, 40
        oracle.census(gu.scene_of(path), f)
        assert oracle.census.last_domain_violations == (0, 0), path
        # overflowed ("far field") arguments need a ray that escaped by ~1e18 units in one step, i.e.
        # a step in which the fast floor/bounding plane (height / 1e-20) was the only object: the
        # transparency continuation rays of basic_clouds and the rays above tree's canopy plane.
        # There IEEE yields +inf and the fast sequences NaN; both are absorbed by the min() /
        # comparison that follows -- and the GPU parity tests cover both scenes.
        if gu.scene_of(path) not in ("basic_clouds", "tree"):
            assert oracle.census.last_far_field == 0, path


def test_sin_and_cos_arguments_stay_inside_the_stated_domain_on_all_scenes(oracle):
    """sin1 and cos1 are within 3e-7 of the truth, and within [-1, 1], for |x| <= 2^16 (tests/golden/math_accuracy.json; far beyond, the
    reduction no longer reduces).  The counting build of the oracle records the arguments the scenes hand to sin and cos: on every
    golden fixture, at the sixteen cameras and times fitted to the reference's screenshots and on every frame bench.py sweeps -- each
    at a small size -- all are finite and inside the domain, and the largest per scene is the one the table records."""
    import math_accuracy_util as mau

    measured = mau.census(oracle)
    recorded = mau.load()["census"]
    assert sorted(measured) == ["bench", "golden", "reference_cameras"]
    assert len(measured["golden"]) == len({gu.scene_of(p) for p in gu.golden_files()}) and sum(1 for c in mau.census_frames(oracle) if c[0] == "reference_cameras") == 16
    for group, scenes in measured.items():
        for scene, m in scenes.items():
            if scene not in mau.NONFINITE_SINCOS_ALLOWED:
                assert m["sincos_nonfinite"] == 0, (group, scene)
            assert m["sincos_max"] <= mau.SINCOS_DOMAIN, (group, scene, m["sincos_max"])
            assert m == recorded[group][scene], (group, scene)


@pytest.mark.parametrize("scene", ["lense", "gems", "light_shadows"])
def test_extension_lights_host_stages_match_oracle(oracle, scene):
    """The "8 lights" extension (SURVEY.md 8d cfg 5): 7 orbiting point lights in slots 1..7."""
    import hostsim

    f = oracle.default_frame(scene, 96, 64, stime=0.8)
    f.extension_lights = 7
    ref, rst, tot = oracle.render(scene, f, stats=True)
    base, _, tot0 = oracle.render(scene, oracle.default_frame(scene, 96, 64, stime=0.8), stats=True)
    assert int(tot[1]) > int(tot0[1]) and not np.array_equal(ref, base)   # more shadow rays, another picture
    img, st = hostsim.render(scene, hostsim.frame_from_oracle(f))
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(st, rst)


def _frames256():
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames256.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("case", _frames256()["frames"], ids=lambda c: "%s-t%g%s" % (c["scene"], c["stime"], "-cfg1" if c["limits"] else ""))
def test_oracle_reproduces_256x256_digests(oracle, case):
    """256x256 start-up-camera frames of the configuration scenes, pinned by digest."""
    import hashlib

    f = oracle.default_frame(case["scene"], 256, 256, stime=case["stime"])
    for k, v in case["limits"].items():
        setattr(f, k, v)
    img, st, tot = oracle.render(case["scene"], f, stats=True)
    assert [int(x) for x in tot] == case["totals"]
    assert hashlib.sha256(img.tobytes()).hexdigest() == case["rgba_sha256"]
    assert hashlib.sha256(st.tobytes()).hexdigest() == case["stats_sha256"]

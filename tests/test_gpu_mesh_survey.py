"""GPU tier of sdfr_mesh_survey and sdfr_mesh_fit through libsdfr.so: every integer equal to the definitions of include/sdfr.h restated in
numpy (mesh_survey_util.survey / fit), fed with the oracle's distances for the built-in scenes and with the library's own
queryDistance for the run-time probe scene; the counts against sdfr_mesh_extract's counting call; the fitted grid's mesh against the
search grid's, bit for bit; no side effects on rendering; the argument errors through the raw C ABI."""
import ctypes

import numpy as np
import pytest

import gpu_util as gu
import mesh_survey_util as su
import mesh_util as mu
import query_util as qu
from gpu_util import renderer  # noqa: F401

pytestmark = pytest.mark.gpu

W, H = 64, 48
# the five scenes and origins of tests/test_gpu_mesh.py's CASES, on its grid: ragged against 256-thread blocks and 64-lane waves alike
DIMS, CELL = (37, 29, 21), 0.1
CASES = {"fast_sphere": (0.0, (-1.85, -0.3, -1.05)), "labyrinth": (1.25, (-5.35, -0.3, -2.55)), "gyroid": (0.5, (-1.85, -0.3, -1.05)),
         "sierpinski": (0.5, (-1.85, -0.3, -1.05)), "noise_lod": (0.5, (-1.85, -0.3, -1.05))}
BANDS = (0.0, 0.05, 0.175)

_probe_loaded = [False]  # is the probe scene the renderer's scene (it is compiled once per load)


def _setup(r, scene, of):
    """the handle's state = the oracle frame `of`"""
    _probe_loaded[0] = False
    gu.setup(r, scene, of)


def _probe(r, **values):
    """the probe scene with its variables set; -> distance(origin, cell, dims) by the library's own point query"""
    su.load_probe(r, "survey_probe", su.PROBE_DEFAULTS, loaded=_probe_loaded[0], **values)
    _probe_loaded[0] = True
    return lambda origin, cell, dims: r.queryDistance(mu.lattice_points(origin, cell, dims))


def _assert_same(what, got, want):
    assert set(got) == set(want), what
    for key in want:
        assert got[key] == want[key], (what, key, got[key], want[key])


def _counting_call(r, origin, cell, dims, iso=0.0):
    import sdf_playground_amd as sp

    grid = sp.MeshGrid((ctypes.c_float * 3)(*origin), cell, dims[0], dims[1], dims[2], iso)
    counts = sp.MeshCounts()
    assert sp.load_library().sdfr_mesh_extract(r._h, ctypes.byref(grid), 0, 0, None, None, None, ctypes.byref(counts), 1) == 0
    return int(counts.vertices), int(counts.triangles)


# ---- the survey ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", sorted(CASES))
def test_survey_equals_the_definition(renderer, scene):
    stime, origin = CASES[scene]
    of = qu.frame(scene, stime, W, H)
    D, _ = qu.oracle_points(scene, of, mu.lattice_points(origin, CELL, DIMS), normals=False)
    _setup(renderer, scene, of)
    for band in BANDS:
        want = su.survey(D, DIMS, 0.0, band)
        assert want["active_cells"] > 500
        if band > 0:
            assert want["near_cells"] > want["active_cells"]
        # no two axes have the same bounds: a swap of axes would show
        assert len(set(zip(want["near_lo"], want["near_hi"]))) == 3 and len(set(zip(want["active_lo"], want["active_hi"]))) == 3
        _assert_same((scene, band), renderer.surveyMesh(origin, CELL, DIMS, band=band), want)
    assert _counting_call(renderer, origin, CELL, DIMS) == (want["active_cells"], 2 * want["quads"])


def test_many_blocks(renderer):
    """labyrinth at 48^3 cells: 460 blocks add into the same words, and the counts pass 2^16"""
    scene, origin, cell, dims = "labyrinth", (-5.5, -0.25, -3.5), 0.125, (48, 48, 48)
    of = qu.frame(scene, 1.25, W, H)
    D, _ = qu.oracle_points(scene, of, mu.lattice_points(origin, cell, dims), normals=False)
    _setup(renderer, scene, of)
    assert (49 ** 3 + 255) // 256 == 460
    for band in (0.0, 2.0):
        want = su.survey(D, dims, 0.0, band)
        assert want["active_cells"] > 5000 and (band == 0 or 1 << 16 < want["near_cells"] < 48 ** 3)
        _assert_same(band, renderer.surveyMesh(origin, cell, dims, band=band), want)
    assert _counting_call(renderer, origin, cell, dims) == (want["active_cells"], 2 * want["quads"])


def test_placement_by_variables(renderer):
    cases = []
    # a 70 x 3 x 2 grid, 852 lattice points: three blocks and 84 points of a fourth; a sphere of 0.05 about the last lattice point makes
    # it the only inside point and the last cell, on three faces, the only active one
    cases.append(("last cell", dict(cx=8.76, cy=0.385, cz=0.26, radius=0.05), (0.0, 0.0, 0.0), 0.125, (70, 3, 2), 0.1,
                  dict(active_cells=1, quads=0, inside_points=1, active_lo=(69, 2, 1), active_hi=(69, 2, 1), face_active=(0, 1, 0, 1, 0, 1))))
    # one cell straddling the surface: bounds 0, all six faces
    cases.append(("1x1x1", dict(cx=0.01, cy=0.02, cz=0.03, radius=0.5), (0.0, 0.0, 0.0), 1.0, (1, 1, 1), 0.0,
                  dict(active_cells=1, quads=0, near_cells=1, inside_points=1, active_lo=(0, 0, 0), active_hi=(0, 0, 0), face_active=(1,) * 6)))
    # a slab of one cell through the sphere's flank
    cases.append(("nx=1", dict(cx=0.03, cy=0.05, cz=0.07, radius=1.0), (0.35, -1.4, -1.05), 0.1, (1, 29, 21), 0.15, None))
    # a box in empty space
    cases.append(("empty", dict(cx=0.03, cy=0.05, cz=0.07, radius=1.0), (-1.0, 3.0, -1.0), 0.1, (9, 7, 5), 0.15,
                  dict(active_cells=0, quads=0, near_cells=0, inside_points=0, active_lo=(9, 7, 5), active_hi=(-1, -1, -1), near_lo=(9, 7, 5), near_hi=(-1, -1, -1),
                       face_active=(0,) * 6)))
    for what, variables, origin, cell, dims, band, pinned in cases:
        distance = _probe(renderer, **variables)
        want = su.survey(distance(origin, cell, dims), dims, 0.0, band)
        for key, value in (pinned or {}).items():
            assert want[key] == value, (what, key, want[key])
        if what == "nx=1":
            assert want["active_cells"] > 20 and want["quads"] > 0 and want["face_active"][0] == want["face_active"][1] == want["active_cells"]
        _assert_same(what, renderer.surveyMesh(origin, cell, dims, band=band), want)
        assert _counting_call(renderer, origin, cell, dims) == (want["active_cells"], 2 * want["quads"]), what


def test_band_edge_and_nan(renderer):
    # the plane y = 0.25 over layers of 0.125: |s| == 0.25 exactly at y = 0 and y = 0.5.  Those layers are near, so cell rows 0 .. 4 are;
    # with the band one float smaller, rows 0 .. 3 are
    origin, cell, dims = (0.0, 0.0, 0.0), 0.125, (5, 8, 3)
    distance = _probe(renderer, kind=1.0, height=0.25)
    D = distance(origin, cell, dims)
    assert np.array_equal(D.reshape(4, 9, 6)[0, :, 0], (np.arange(9, dtype=np.float32) * np.float32(0.125) - np.float32(0.25)))
    for band, top in ((0.25, 4), (float(np.nextafter(np.float32(0.25), np.float32(0))), 3)):
        want = su.survey(D, dims, 0.0, band)
        assert want["near_lo"][1] == 0 and want["near_hi"][1] == top and want["active_lo"][1] == want["active_hi"][1] == 1
        assert want["near_cells"] == (top + 1) * 15 and want["inside_points"] == 2 * 24
        _assert_same(band, renderer.surveyMesh(origin, cell, dims, band=band), want)
    # NaN where x > 0.3: those corners are neither inside nor near
    D = _probe(renderer, kind=2.0, height=0.25, split=0.3)(origin, cell, dims)
    assert np.isnan(D).sum() == 3 * 9 * 4
    want = su.survey(D, dims, 0.0, 0.25)
    assert want["inside_points"] == 2 * 3 * 4 and want["near_hi"] == (2, 4, 2) and want["active_hi"][0] == 2
    _assert_same("NaN", renderer.surveyMesh(origin, cell, dims, band=0.25), want)


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------
def _same_mesh(a, b, what):
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), what


def _check_fits(r, what, distance, origin):
    full = r.extractMesh(origin, su.FIT_CELL, su.FIT_DIMS)
    assert len(full[0]) > 500
    seen = {}
    for levels in range(4):
        want = su.fit(distance, origin, su.FIT_CELL, su.FIT_DIMS, 0.0, levels, 1)
        got = r.fitMesh(origin, su.FIT_CELL, su.FIT_DIMS, levels=levels, margin=1)
        _assert_same((what, levels), got, want)
        assert got["state"] == su.FOUND and got["surveys"] == levels + 1 and got["dims"] != su.FIT_DIMS
        if (got["origin"], got["dims"]) not in seen:
            seen[got["origin"], got["dims"]] = r.extractMesh(got["origin"], su.FIT_CELL, got["dims"])
        _same_mesh(seen[got["origin"], got["dims"]], full, (what, levels))
    assert r.fitMesh(origin, su.FIT_CELL, su.FIT_DIMS)["surveys"] == 1  # levels=None: 64 cells per axis need no coarse level
    return got


@pytest.mark.parametrize("scene", sorted(su.FIT_SCENES))
def test_fit_equals_the_definition(renderer, scene):
    stime, origin = su.FIT_SCENES[scene]
    of = qu.frame(scene, stime, W, H)
    _setup(renderer, scene, of)
    got = _check_fits(renderer, scene, su.oracle_distance(scene, of), origin)
    if scene == "labyrinth":
        _same_mesh(renderer.extractMesh(got["origin"], su.FIT_CELL, got["dims"], sharp=True), renderer.extractMesh(origin, su.FIT_CELL, su.FIT_DIMS, sharp=True), "sharp")


def test_fit_of_the_probe_scene(renderer):
    origin = (-2.0, -1.5, -1.75)
    _check_fits(renderer, "sphere", _probe(renderer, cx=0.28, cy=0.05, cz=0.07, radius=0.8), origin)
    # the sphere far away: nothing near at the coarsest level
    distance = _probe(renderer, cx=50.0, radius=0.8)
    want = su.fit(distance, origin, su.FIT_CELL, su.FIT_DIMS, 0.0, 3, 1)
    assert (want["state"], want["level"], want["surveys"]) == (su.EMPTY, 3, 1)
    _assert_same("empty", renderer.fitMesh(origin, su.FIT_CELL, su.FIT_DIMS, levels=3), want)
    # too large before any survey: 4096 x 8 x 8 at levels = 1
    got = renderer.fitMesh((0.0, 0.0, 0.0), 0.125, (4096, 8, 8), levels=1)
    assert got == dict(state=su.TOO_LARGE, level=1, surveys=0, lo=(0, 0, 0), hi=(4096, 8, 8), origin=None, dims=None, survey=None)
    # ... and after two: a floor keeps the window 4096 cells long
    distance = _probe(renderer, kind=1.0, height=0.25)
    want = su.fit(distance, (0.0, 0.0, 0.0), 0.125, (4096, 8, 8), 0.0, 3, 1)
    assert (want["state"], want["level"], want["surveys"]) == (su.TOO_LARGE, 1, 2)
    _assert_same("too large", renderer.fitMesh((0.0, 0.0, 0.0), 0.125, (4096, 8, 8), levels=3), want)
    # large indices: 2^20 x 4 x 4 cells, the sphere near the far end
    distance = _probe(renderer, cx=(1 << 20) * 0.0625 - 2.0, cy=0.125, cz=0.125, radius=0.2)
    want = su.fit(distance, (0.0, 0.0, 0.0), 0.0625, (1 << 20, 4, 4), 0.0, 10, 1)
    assert want["state"] == su.FOUND and want["surveys"] == 11 and want["lo"][0] > (1 << 20) - 64 and want["survey"]["active_cells"] > 8
    _assert_same("far", renderer.fitMesh((0.0, 0.0, 0.0), 0.0625, (1 << 20, 4, 4), levels=10), want)
    assert renderer.fitMesh((0.0, 0.0, 0.0), 0.0625, (1 << 20, 4, 4)) == renderer.fitMesh((0.0, 0.0, 0.0), 0.0625, (1 << 20, 4, 4), levels=10)


# ---- the protocol ----------------------------------------------------------------------------------------------------------------------
def test_survey_and_fit_leave_rendering_alone(renderer):
    import torch

    scene = "labyrinth"
    stime, origin = su.FIT_SCENES[scene]
    of = qu.frame(scene, stime, W, H)
    _setup(renderer, scene, of)
    distance = su.oracle_distance(scene, of)
    survey_ref = su.survey(distance(origin, su.FIT_CELL, su.FIT_DIMS), su.FIT_DIMS, 0.0, 0.1)
    fit_ref = su.fit(distance, origin, su.FIT_CELL, su.FIT_DIMS, 0.0, 2, 1)
    with gu.rendering_untouched(renderer, W, H) as (img0, s0):
        _assert_same("survey", renderer.surveyMesh(origin, su.FIT_CELL, su.FIT_DIMS, band=0.1), survey_ref)
        _assert_same("fit", renderer.fitMesh(origin, su.FIT_CELL, su.FIT_DIMS, levels=2), fit_ref)
    # two frames in flight: both calls run on the lane of the frame submitted last, between extractions that leave device work behind
    renderer.setFramesInFlight(2)
    try:
        imgs = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        for k in range(4):
            renderer.render(None, W, H, out=imgs[k % 2])
            dpos, _dn, _di = renderer.extractMesh(origin, su.FIT_CELL, su.FIT_DIMS, device=True)
            _assert_same("survey", renderer.surveyMesh(origin, su.FIT_CELL, su.FIT_DIMS, band=0.1), survey_ref)
            _assert_same("fit", renderer.fitMesh(origin, su.FIT_CELL, su.FIT_DIMS, levels=2), fit_ref)
            renderer.sync()
            assert len(dpos) == survey_ref["active_cells"]
            assert np.array_equal(imgs[k % 2].cpu().numpy().view(np.uint32), img0.view(np.uint32))
            assert gu.stats(renderer) == s0
    finally:
        renderer.setFramesInFlight(1)


def test_arguments(renderer):
    import sdf_playground_amd as sp

    L = sp.load_library()
    _setup(renderer, "fast_sphere", qu.frame("fast_sphere", 0.0, W, H))
    h = renderer._h
    o, dims = (-0.5, -0.3, -0.5), (8, 8, 8)
    NO_SCENE = -4

    def grid(origin=o, cell=0.1, dims=dims, iso=0.0):
        return sp.MeshGrid((ctypes.c_float * 3)(*origin), cell, dims[0], dims[1], dims[2], iso)

    def survey(handle, g, band, out=True):
        s = sp.MeshSurvey(active_cells=-7, quads=-7)
        rc = L.sdfr_mesh_survey(handle, ctypes.byref(g) if g is not None else None, band, ctypes.byref(s) if out else None)
        assert rc == 0 or (s.active_cells, s.quads) == (-7, -7)  # nothing is written on error
        return rc, L.sdfr_last_error(handle).decode() if handle and rc else ""

    def fit(handle, g, levels, margin, out=True):
        f = sp.MeshFit(state=-7, surveys=-7)
        rc = L.sdfr_mesh_fit(handle, ctypes.byref(g) if g is not None else None, levels, margin, ctypes.byref(f) if out else None)
        assert rc == 0 or (f.state, f.surveys) == (-7, -7)
        return rc, L.sdfr_last_error(handle).decode() if handle and rc else ""

    assert survey(h, grid(), 0.0) == (0, "") and fit(h, grid(), 1, 1) == (0, "")
    bad = [grid(cell=0.0), grid(cell=float("nan")), grid(origin=(float("inf"), 0.0, 0.0)), grid(iso=float("nan")), grid(dims=(0, 8, 8))]
    for g in bad + [grid(dims=(8, 8, 1025)), grid(dims=(1024, 1024, 1024))]:
        assert survey(h, g, 0.0) == (su.INVALID, su.BAD_GRID)
    for g in bad + [grid(dims=(8, 8, (1 << 20) + 1))]:
        assert fit(h, g, 1, 1) == (su.INVALID, su.BAD_SEARCH)
    for band in (-0.5, float("nan"), float("inf")):
        assert survey(h, grid(), band) == (su.INVALID, su.BAD_BAND)
    for levels in (-1, 11):
        assert fit(h, grid(), levels, 1) == (su.INVALID, su.BAD_LEVELS)
    assert fit(h, grid(cell=3e38), 1, 1) == (su.INVALID, su.BAD_LEVELS)
    for margin in (-1, 9):
        assert fit(h, grid(), 1, margin) == (su.INVALID, su.BAD_MARGIN)
    assert survey(h, None, 0.0) == (su.INVALID, su.NULL_POINTER) and survey(h, grid(), 0.0, out=False) == (su.INVALID, su.NULL_POINTER)
    assert fit(h, None, 1, 1) == (su.INVALID, su.NULL_POINTER) and fit(h, grid(), 1, 1, out=False) == (su.INVALID, su.NULL_POINTER)
    # two faults at once: the text of the one checked first
    assert survey(h, None, -1.0) == (su.INVALID, su.NULL_POINTER) and survey(h, bad[0], -1.0) == (su.INVALID, su.BAD_GRID)
    assert fit(h, bad[0], 11, 9) == (su.INVALID, su.BAD_SEARCH) and fit(h, grid(), 11, 9) == (su.INVALID, su.BAD_LEVELS)
    assert survey(None, grid(), 0.0)[0] == su.INVALID and fit(None, grid(), 1, 1)[0] == su.INVALID
    fresh = sp.SDFRenderer(0)
    try:
        assert survey(fresh._h, grid(), 0.0)[0] == NO_SCENE and fit(fresh._h, grid(), 1, 1)[0] == NO_SCENE
        assert survey(fresh._h, bad[0], 0.0)[0] == su.INVALID and fit(fresh._h, grid(), 1, 9)[0] == su.INVALID  # the arguments come first
    finally:
        fresh.close()
    # a survey records no stage timings: those stay the last extraction's
    ms = (ctypes.c_double * 4)()
    renderer.extractMesh(o, 0.1, dims)
    renderer.setProfiling(True)
    try:
        renderer.surveyMesh(o, 0.1, dims)
        assert L.sdfr_mesh_get_timings(h, ctypes.byref(ms)) == su.INVALID
    finally:
        renderer.setProfiling(False)

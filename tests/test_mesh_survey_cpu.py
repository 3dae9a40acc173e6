"""CPU tier of sdfr_mesh_survey and sdfr_mesh_fit: the definitions of include/sdfr.h restated in numpy (mesh_survey_util.survey / fit)
against the library's own text run sequentially (tests/cpp/mesh_survey_host.cpp over sdf_playground_amd/csrc/sdfr_mesh_survey.h and
sdfr_mesh_plan.h), every integer equal; the fit over exact distances and over one that breaks the contract; the scenes the GPU fit
test may use; the argument faults and their precedence; the struct layouts; the CLI's --mesh-fit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mesh_survey_util as su
import mesh_util as mu
import query_util as qu

F = np.float32
NAN, INF = float("nan"), float("inf")
# ragged shapes: single cells, slabs on every axis, more points than a block of 256, a row longer than a wave of 64
SHAPES = ((1, 1, 1), (1, 5, 3), (7, 1, 2), (5, 4, 1), (2, 2, 2), (13, 9, 11), (70, 3, 2), (37, 5, 3))


def _assert_same_survey(what, got, want):
    assert set(got) == set(want) == set(su.SURVEY_KEYS), what
    for key in su.SURVEY_KEYS:
        assert got[key] == want[key], (what, key, got[key], want[key])


def _random_lattices(dims, rng):
    """(what, D, iso, band): special values on a dyadic ladder, so that |s| == band happens exactly; and a smooth field with them sown in"""
    points = (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1)
    iso, band = 0.125, 0.25
    ladder = np.array([-0.5, -0.25, -0.0, 0.0, 0.25, 0.5, 0.75, NAN, INF, -INF], np.float32)
    D = (ladder[rng.integers(0, len(ladder), points)] + F(iso)).astype(np.float32)
    yield "ladder", D, iso, band
    yield "ladder, band 0", D, iso, 0.0
    p = mu.lattice_points((0.0, 0.0, 0.0), 0.25, dims).astype(np.float64)
    smooth = (np.linalg.norm(p - np.array(dims) * 0.125, axis=1) - 0.3 * max(dims) * 0.25).astype(np.float32)
    sown = smooth.copy()
    where = rng.integers(0, points, max(1, points // 7))
    sown[where] = ladder[rng.integers(0, len(ladder), len(where))]
    yield "smooth", smooth, 0.0, 0.3
    yield "smooth with special values", sown, 0.0, 0.25
    yield "noise", rng.normal(0.0, 0.3, points).astype(np.float32), 0.05, 0.1


def test_survey_equals_the_host_text():
    rng = np.random.default_rng(20)
    exact_edge = nan_corner = 0
    for dims in SHAPES:
        for what, D, iso, band in _random_lattices(dims, rng):
            want = su.survey(D, dims, iso, band)
            rc, err, got = su.host_survey(D, (0.0, 0.0, 0.0), 0.25, dims, iso, band)
            assert (rc, err) == (0, ""), (dims, what)
            _assert_same_survey((dims, what), got, want)
            # the counts are the extraction's: vertices and triangles of the definition of sdfr_mesh_extract
            pos, idx = mu.surface_nets(D, (0.0, 0.0, 0.0), 0.25, dims, iso)
            assert (want["active_cells"], 2 * want["quads"]) == (len(pos), len(idx)), (dims, what)
            assert want["near_cells"] >= want["active_cells"]
            with np.errstate(invalid="ignore"):
                s = D - F(iso)
                exact_edge += int((np.abs(s) == F(band)).sum()) if band > 0 else 0
            nan_corner += int(np.isnan(s).sum())
    assert exact_edge > 100 and nan_corner > 100
    # |s| == band is near, the next float above is not; NaN is neither near nor inside; -0 is not inside
    for value, near, inside in ((0.25, 1, 0), (-0.25, 1, 8), (float(np.nextafter(F(0.25), F(1))), 0, 0), (NAN, 0, 0), (-0.0, 1, 0), (-INF, 0, 8)):
        got = su.host_survey(np.full(8, value, np.float32), (0.0, 0.0, 0.0), 1.0, (1, 1, 1), 0.0, 0.25)[2]
        assert (got["near_cells"], got["inside_points"], got["active_cells"]) == (near, inside, 0), value
        _assert_same_survey(value, got, su.survey(np.full(8, value, np.float32), (1, 1, 1), 0.0, 0.25))
    # one active cell: bounds 0, all six faces
    one = su.host_survey(np.array([-1, 1, 1, 1, 1, 1, 1, 1], np.float32), (0.0, 0.0, 0.0), 1.0, (1, 1, 1), 0.0, 0.0)[2]
    assert one["active_cells"] == 1 and one["active_lo"] == one["active_hi"] == (0, 0, 0) and one["face_active"] == (1,) * 6 and one["quads"] == 0
    # nothing: lo = n, hi = -1
    none = su.host_survey(np.ones(6 * 4 * 3, np.float32), (0.0, 0.0, 0.0), 1.0, (5, 3, 2), 0.0, 0.5)[2]
    assert none["near_lo"] == none["active_lo"] == (5, 3, 2) and none["near_hi"] == none["active_hi"] == (-1, -1, -1) and not any(none["face_active"])


def test_under_sanitizers():
    """the stand-alone program (its own main) under the address and undefined-behaviour sanitizers: one survey, one fit, and the numbers
    the definitions give for the same sphere"""
    lines = subprocess.run([su.sanitizer_program()], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == 3

    def sphere(origin, cell, dims):
        x, y, z = (mu.lattice_points(origin, cell, dims)[:, a] - F(c) for a, c in enumerate((3.3, 1.1, 0.7)))
        return np.sqrt((x * x + y * y) + z * z) - F(0.8)

    def numbers(s):
        return [s["active_cells"], s["quads"], s["near_cells"], s["inside_points"], *s["active_lo"], *s["active_hi"], *s["near_lo"], *s["near_hi"], *s["face_active"]]

    g = ((2.5, 0.0, -0.25), 0.125, (13, 9, 11))
    want = su.survey(sphere(*g), g[2], 0.0, 0.25)
    assert [int(x) for x in lines[0].split()] == numbers(want) and want["active_cells"] > 50 and any(want["face_active"])
    f = su.fit(sphere, (-4.0, -2.0, -3.0), 0.0625, (200, 96, 80), 0.0, 3, 1)
    assert [int(x) for x in lines[1].split()] == [f["state"], f["level"], f["surveys"], *f["lo"], *f["hi"], *f["dims"]]
    assert [int(x) for x in lines[2].split()] == numbers(f["survey"]) and f["state"] == su.FOUND and max(f["dims"]) < 40


# ---- the fit over exact distances --------------------------------------------------------------------------------------------------
def _placements(count, seed):
    """(shape, distance, origin, cell, dims): dyadic origins and cells, the shape's centre inside the search grid"""
    rng = np.random.default_rng(seed)
    for k in range(count):
        shape = ("sphere", "torus", "box")[k % 3]
        cell = (0.0625, 0.125, 0.03125)[int(rng.integers(0, 3))]
        dims = tuple(int(v) for v in rng.integers(17, 34, 3))
        origin = tuple(float(v) * 0.25 for v in rng.integers(-8, 9, 3))
        size = float(rng.uniform(2.5, 7.0)) * cell
        centre = tuple(origin[a] + float(rng.uniform(0.2, 0.8)) * dims[a] * cell for a in range(3))
        yield shape, su.shape_distance(shape, centre, size), origin, cell, dims


def test_fit_over_exact_distances():
    """200 placements of a sphere, a torus and a box, levels 0..3 in turn, margins 1 and 2: the host text and the restatement agree, the
    state is FOUND, the window holds every active cell and the margin, and the fitted grid's mesh is the search grid's bit for bit"""
    clipped = shrunk = 0
    for k, (shape, distance, origin, cell, dims) in enumerate(_placements(200, 7)):
        levels, margin = k % 4, 1 + (k // 4) % 2
        what = (k, shape, origin, cell, dims, levels, margin)
        want = su.fit(distance, origin, cell, dims, 0.0, levels, margin)
        rc, err, got = su.host_fit(distance, origin, cell, dims, 0.0, levels, margin)
        assert (rc, err) == (0, "") and got == want, what
        assert want["state"] == su.FOUND and want["level"] == 0 and want["surveys"] == levels + 1, what
        D = distance(origin, cell, dims)
        full = su.survey(D, dims, 0.0, 0.0)
        assert full["active_cells"] > 0 and su.contains_active(want, full, dims, margin), what
        assert want["dims"] == tuple(h - l for l, h in zip(want["lo"], want["hi"])), what
        assert want["survey"]["active_cells"] == full["active_cells"] and want["survey"]["quads"] == full["quads"], what
        pos, idx = mu.surface_nets(D, origin, cell, dims, 0.0)
        fpos, fidx = mu.surface_nets(distance(want["origin"], cell, want["dims"]), want["origin"], cell, want["dims"], 0.0)
        assert np.array_equal(fpos.view(np.uint32), pos.view(np.uint32)) and np.array_equal(fidx, idx), what
        clipped += any(full["face_active"])
        shrunk += want["dims"] != dims
    assert clipped > 10 and shrunk > 150  # surfaces that leave the search grid are among them, and most fits are smaller than their search


def test_a_distance_that_overestimates_loses_cells():
    """the negative control: 4 * distance breaks the contract.  Small spheres fall between the points of a coarse level: with levels >= 2
    some placement loses cells, with levels = 0 none does, and the exact distance loses none at any level"""
    rng = np.random.default_rng(11)
    cell, dims, origin = 0.0625, (32, 32, 32), (-1.0, -1.0, -1.0)
    lost = {levels: 0 for levels in range(4)}
    for k in range(24):
        # a sphere of 1.5 cells about the centre of a cell of level 2 or 3 (4 or 8 search cells): every corner of that cell is then
        # further than 1.75 / 4 coarse cells from the surface, while the exact distance has them well within 1.75
        coarse = cell * (4 << (k % 2))
        centre = tuple(origin[a] + (int(rng.integers(1, 2 / coarse - 1)) + 0.5) * coarse + float(rng.uniform(-0.004, 0.004)) for a in range(3))
        exact = su.shape_distance("sphere", centre, 1.5 * cell)
        over = su.scaled(exact, 4.0)
        full = su.survey(exact(origin, cell, dims), dims, 0.0, 0.0)
        assert full["active_cells"] > 0
        assert su.survey(over(origin, cell, dims), dims, 0.0, 0.0) == full  # (scaling keeps the signs: the same cells are active)
        for levels in range(4):
            assert su.contains_active(su.fit(exact, origin, cell, dims, 0.0, levels, 1), full, dims, 1), (centre, levels)
            got = su.fit(over, origin, cell, dims, 0.0, levels, 1)
            assert su.host_fit(over, origin, cell, dims, 0.0, levels, 1)[2] == got
            lost[levels] += not su.contains_active(got, full, dims, 1)
    assert lost[0] == 0 and lost[2] > 0 and lost[3] > 0, lost


@pytest.mark.parametrize("scene", sorted(su.FIT_SCENES))
def test_gpu_fit_scenes_keep_the_contract(scene):
    """the precondition of tests/test_gpu_mesh_survey.py's fit cases: over the oracle's distances of the scene, every level count gives
    FOUND and a mesh equal to the search grid's"""
    stime, origin = su.FIT_SCENES[scene]
    distance = su.oracle_distance(scene, qu.frame(scene, stime))
    pos, idx = mu.surface_nets(distance(origin, su.FIT_CELL, su.FIT_DIMS), origin, su.FIT_CELL, su.FIT_DIMS, 0.0)
    assert len(pos) > 500
    for levels in range(4):
        f = su.fit(distance, origin, su.FIT_CELL, su.FIT_DIMS, 0.0, levels, 1)
        assert f["state"] == su.FOUND and f["survey"]["active_cells"] == len(pos), (scene, levels, f)
        fpos, fidx = mu.surface_nets(distance(f["origin"], su.FIT_CELL, f["dims"]), f["origin"], su.FIT_CELL, f["dims"], 0.0)
        assert np.array_equal(fpos.view(np.uint32), pos.view(np.uint32)) and np.array_equal(fidx, idx), (scene, levels)


# ---- the plans -----------------------------------------------------------------------------------------------------------------------
O, DIMS = (-0.5, -0.3, -0.5), (8, 8, 8)
# the eleven bad grids of tests/test_mesh_plan_cpu.py
BAD_GRIDS = [dict(cell=0.0), dict(cell=-0.1), dict(cell=INF), dict(cell=NAN), dict(origin=(NAN, 0.0, 0.0)), dict(origin=(0.0, INF, 0.0)), dict(iso=NAN),
             dict(dims=(0, 8, 8)), dict(dims=(8, -1, 8)), dict(dims=(8, 8, 1025)), dict(dims=(1024, 1024, 1024))]


def _flat(dims):
    return lambda origin, cell, n: np.full((n[0] + 1) * (n[1] + 1) * (n[2] + 1), 1e9, np.float32)  # further than any level's band


def test_survey_argument_faults():
    def check(text, origin=O, cell=0.1, dims=DIMS, iso=0.0, band=0.0, **null):
        assert su.survey_fault(origin, cell, dims, iso, band, **null) == text
        rc, err, got = su.host_survey(np.ones((dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1) if text is None else 8, np.float32), origin, cell, dims, iso, band, **null)
        assert (rc, err, got is None) == ((0, "", False) if text is None else (su.INVALID, text, True)), (text, origin, cell, dims, iso, band, null)

    check(None)
    check(None, band=0.5)
    check(None, dims=(1, 1, 1), band=1e30)
    for g in BAD_GRIDS:
        check(su.BAD_GRID, **g)
    for band in (-0.001, NAN, INF, -INF):
        check(su.BAD_BAND, band=band)
    check(su.NULL_POINTER, grid=False)
    check(su.NULL_POINTER, out=False)
    # two faults at once: the earlier text wins
    check(su.NULL_POINTER, grid=False, band=-1.0)
    check(su.NULL_POINTER, out=False, cell=0.0)
    check(su.BAD_GRID, cell=0.0, band=-1.0)


def test_fit_argument_faults():
    def check(text, origin=O, cell=0.1, dims=DIMS, iso=0.0, levels=1, margin=1, **null):
        assert su.fit_fault(origin, cell, dims, iso, levels, margin, **null) == text
        rc, err, got = su.host_fit(_flat(dims), origin, cell, dims, iso, levels, margin, **null)
        assert (rc, err, got is None) == ((0, "", False) if text is None else (su.INVALID, text, True)), (text, origin, cell, dims, iso, levels, margin, null)

    check(None)
    check(None, levels=0, margin=0)
    check(None, levels=10, margin=8)
    for g in BAD_GRIDS[:9]:
        check(su.BAD_SEARCH, **g)
    check(su.BAD_SEARCH, dims=(8, 8, (1 << 20) + 1))
    for levels in (-1, 11):
        check(su.BAD_LEVELS, levels=levels)
    check(su.BAD_LEVELS, cell=3e38, levels=1)  # cell * 2 is no longer finite
    check(None, cell=1e38, levels=1)
    for margin in (-1, 9):
        check(su.BAD_MARGIN, margin=margin)
    check(su.NULL_POINTER, grid=False)
    check(su.NULL_POINTER, out=False)
    # two faults at once, one pair per adjacent checks: the earlier text wins
    check(su.NULL_POINTER, grid=False, levels=11)
    check(su.NULL_POINTER, out=False, cell=0.0)
    check(su.BAD_SEARCH, cell=0.0, levels=11)
    check(su.BAD_LEVELS, levels=11, margin=9)
    check(su.BAD_SEARCH, dims=(0, 8, 8), margin=9)


def test_fit_too_large_and_empty():
    # search grids past an extraction's limits are fine as long as the coarsest level is extractable
    for dims, levels, state, level, surveys in (((4096, 8, 8), 1, su.TOO_LARGE, 1, 0), ((4096, 8, 8), 2, su.EMPTY, 2, 1), ((1 << 20, 4, 4), 9, su.TOO_LARGE, 9, 0),
                                                ((1 << 20, 4, 4), 10, su.EMPTY, 10, 1), ((1025, 1, 1), 0, su.TOO_LARGE, 0, 0), ((1024, 1, 1), 0, su.EMPTY, 0, 1)):
        want = su.fit(_flat(dims), O, 0.1, dims, 0.0, levels, 1)  # (nothing near at any level)
        assert (want["state"], want["level"], want["surveys"]) == (state, level, surveys), dims
        assert want["lo"] == (0, 0, 0) and want["hi"] == dims and want["origin"] is None and want["dims"] is None
        assert (want["survey"] is None) == (surveys == 0)
        assert su.host_fit(_flat(dims), O, 0.1, dims, 0.0, levels, 1) == (0, "", want), dims
    # 2^31 lattice points at the coarsest level: the count of points, not only the cells per axis, is checked
    big = su.fit(lambda *a: pytest.fail("surveyed"), O, 0.1, (2048, 2048, 2048), 0.0, 1, 1)
    assert (big["state"], big["level"], big["surveys"]) == (su.TOO_LARGE, 1, 0)
    # TOO_LARGE after two surveys: a floor under 4096 x 8 x 8 cells keeps the window as long as the search at every level
    floor = lambda origin, cell, n: (mu.lattice_points(origin, cell, n)[:, 1] - F(0.25)).astype(np.float32)  # noqa: E731
    late = su.fit(floor, (0.0, 0.0, 0.0), 0.125, (4096, 8, 8), 0.0, 3, 1)
    assert (late["state"], late["level"], late["surveys"]) == (su.TOO_LARGE, 1, 2) and late["lo"][0] == 0 and late["hi"][0] == 4096 and late["survey"] is not None
    assert su.host_fit(floor, (0.0, 0.0, 0.0), 0.125, (4096, 8, 8), 0.0, 3, 1) == (0, "", late)
    # a small sphere near the far end of 2^20 cells
    far = su.shape_distance("sphere", ((1 << 20) * 0.0625 - 2.0, 0.125, 0.125), 0.2)
    f = su.fit(far, (0.0, 0.0, 0.0), 0.0625, (1 << 20, 4, 4), 0.0, 10, 1)
    assert f["state"] == su.FOUND and f["surveys"] == 11 and f["lo"][0] > (1 << 20) - 64 and f["survey"]["active_cells"] > 8
    assert su.host_fit(far, (0.0, 0.0, 0.0), 0.0625, (1 << 20, 4, 4), 0.0, 10, 1) == (0, "", f)
    assert [su.default_levels(d) for d in ((64, 48, 56), (65, 1, 1), (1, 1, 1), (1 << 20, 4, 4), (4096, 8, 8))] == [0, 1, 0, 10, 6]


# ---- the ABI and the Python layer ----------------------------------------------------------------------------------------------------
def test_structs_match_the_header(tmp_path):
    import sdf_playground_amd as sp

    survey_fields = ("active_cells", "quads", "near_cells", "inside_points", "active_lo", "active_hi", "near_lo", "near_hi", "face_active")
    fit_fields = ("state", "level", "surveys", "lo", "hi", "grid", "last")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdfr.h"\nint main(void) {\nprintf("%zu", sizeof(sdfr_mesh_survey_result));\n'
                   + "".join('printf(" %%zu", offsetof(sdfr_mesh_survey_result, %s));\n' % f for f in survey_fields)
                   + 'printf(" %zu", sizeof(sdfr_mesh_fit_result));\n'
                   + "".join('printf(" %%zu", offsetof(sdfr_mesh_fit_result, %s));\n' % f for f in fit_fields)
                   + 'printf(" %d %d %d\\n", SDFR_FIT_EMPTY, SDFR_FIT_FOUND, SDFR_FIT_TOO_LARGE);\nreturn 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I" + os.path.join(qu.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = ([ctypes.sizeof(sp.MeshSurvey)] + [getattr(sp.MeshSurvey, f).offset for f in survey_fields]
            + [ctypes.sizeof(sp.MeshFit)] + [getattr(sp.MeshFit, f).offset for f in fit_fields] + [sp.FIT_EMPTY, sp.FIT_FOUND, sp.FIT_TOO_LARGE])
    assert got == want == [128, 0, 8, 16, 24, 32, 44, 56, 68, 80, 200, 0, 4, 8, 12, 24, 36, 72, 0, 1, 2]
    assert "sdfr_mesh_survey" in sp.EXPORTED_SYMBOLS and "sdfr_mesh_fit" in sp.EXPORTED_SYMBOLS
    assert (su.EMPTY, su.FOUND, su.TOO_LARGE) == (sp.FIT_EMPTY, sp.FIT_FOUND, sp.FIT_TOO_LARGE)
    assert hasattr(sp.SDFRenderer, "surveyMesh") and hasattr(sp.SDFRenderer, "fitMesh")
    for dims in ((64, 48, 56), (65, 1, 1), (129, 128, 7), (1 << 20, 4, 4), (4097, 3, 3), (1, 1, 1)):
        assert sp.default_fit_levels(dims) == su.default_levels(dims), dims
    header = open(os.path.join(qu.ROOT, "include", "sdfr.hpp")).read()
    assert "bool surveyMesh(" in header and "bool fitMesh(" in header


def test_cli_mesh_fit_without_a_gpu(capsys):
    from sdf_playground_amd import cli

    a = cli.make_parser().parse_args(["--scene", "tree", "--mesh", "t.obj", "--mesh-fit", "--mesh-box", "-8", "-8", "-8", "8", "8", "8", "--mesh-cell", "0.02"])
    assert a.mesh_fit and a.mesh_fit_levels is None and a.mesh_fit_margin == 1
    a = cli.make_parser().parse_args(["--scene", "tree", "--mesh", "t.obj", "--mesh-fit", "--mesh-fit-levels", "4", "--mesh-fit-margin", "2"])
    assert (a.mesh_fit_levels, a.mesh_fit_margin) == (4, 2)
    assert not cli.make_parser().parse_args(["--scene", "tree"]).mesh_fit
    # a search box may have up to 2^20 cells per axis; without --mesh-fit the limit is the extraction's, with the message it has always had
    assert cli.mesh_grid_from_box((-8, -8, -8, 8, 8, 8), 0.01, 1 << 20) == ((-8, -8, -8), (1600, 1600, 1600))
    with pytest.raises(ValueError, match="at most 1024 per axis"):
        cli.mesh_grid_from_box((-8, -8, -8, 8, 8, 8), 0.01)
    with pytest.raises(ValueError, match="at most 1048576 per axis"):
        cli.mesh_grid_from_box((0, 0, 0, 1, 1, 1), 1e-7, 1 << 20)

    def refused(args, text):
        with pytest.raises(SystemExit) as e:
            cli.main(args)
        assert e.value.code == 2 and text in capsys.readouterr().err, args

    box = ["--mesh-box", "-8", "-8", "-8", "8", "8", "8", "--mesh-cell", "0.01"]
    refused(["--scene", "tree", "--mesh-fit"] + box, "--mesh-fit needs --mesh")
    refused(["--scene", "tree", "--mesh", "t.obj", "--mesh-fit"], "--mesh needs --mesh-box and --mesh-cell")
    refused(["--scene", "tree", "--mesh", "t.obj"], "--mesh needs --mesh-box and --mesh-cell")
    refused(["--scene", "tree", "--mesh", "t.obj"] + box, "at most 1024 per axis")
    refused(["--scene", "tree", "--mesh", "t.obj", "--mesh-fit-levels", "2"] + box, "--mesh-fit-levels needs --mesh-fit")
    refused(["--scene", "tree", "--mesh", "t.obj", "--mesh-fit", "--mesh-fit-levels", "11"] + box, "--mesh-fit-levels must be 0..10")
    refused(["--scene", "tree", "--mesh", "t.obj", "--mesh-fit", "--mesh-fit-margin", "9"] + box, "--mesh-fit-margin 0..8")
    refused(["--scene", "tree", "--mesh", "t.obj", "--mesh-fit", "--mesh-box", "0", "0", "0", "1", "1", "1", "--mesh-cell", "1e-7"], "at most 1048576 per axis")
    # what the fit's three outcomes print
    survey = dict(face_active=(0, 0, 3, 0, 0, 0))
    found = dict(state=su.FOUND, level=0, surveys=4, lo=(8, 0, 16), hi=(40, 24, 48), origin=(-1.5, 0.0, -1.0), dims=(32, 24, 32), survey=survey)
    text = cli.fit_message(found, (1600, 1600, 1600), 0.0625)
    assert text.startswith("fitted box -1.5 0 -1 0.5 1.5 1: 32x24x32 of 1600x1600x1600 cells, 4 surveys") and "on 1 faces" in text
    empty = dict(state=su.EMPTY, level=3, surveys=1, lo=(0, 0, 0), hi=(1600, 1600, 1600), origin=None, dims=None, survey=survey)
    assert "no surface inside --mesh-box" in cli.fit_message(empty, (1600, 1600, 1600), 0.0625) and "level 3" in cli.fit_message(empty, (1600,) * 3, 0.0625)
    large = dict(state=su.TOO_LARGE, level=1, surveys=2, lo=(0, 2, 0), hi=(4096, 6, 8), origin=None, dims=None, survey=survey)
    assert "4096x4x8 cells at level 1" in cli.fit_message(large, (4096, 8, 8), 0.125)

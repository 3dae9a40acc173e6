"""CPU tier of sdfr_mesh_extract_sharp: the stage functions of sdf_playground_amd/csrc/sdfr_mesh_sharp.h, built for the CPU with the
scene behind a callback (tests/cpp/mesh_sharp_host.cpp), against the header's definition restated in numpy
(mesh_sharp_util.sharp_nets) bit for bit; what the scheme is for -- vertices on the surface, corners met, flat faces -- on analytic
shapes, where plain surface nets must fail the same bounds; the clamp; the guards; the sanitizers; the ABI.

The geometry bounds are about ten times what a numpy prototype of the scheme measured; the values this stand-in
gives are written next to each bound."""
import os

import numpy as np
import pytest

import mesh_sharp_util as su
import mesh_util as mu
import query_kernels_util as ku
import query_util as qu

ORIGIN, CELL, DIMS = su.GRID
ROOT = qu.ROOT


_cases = {}


def _analytic_case(name):
    """(D at the lattice, the restatement's positions and info, the stand-in's positions and indices, surface nets' positions and indices)"""
    if name not in _cases:
        f = su.analytic(name)
        D = f(mu.lattice_points(ORIGIN, CELL, DIMS), False)[0]
        ref, info = su.sharp_nets(D, ORIGIN, CELL, DIMS, 0.0, f)
        pos, idx = su.host_extract(D, ORIGIN, CELL, DIMS, 0.0, f)
        _cases[name] = (D, ref, info, pos, idx) + mu.surface_nets(D, ORIGIN, CELL, DIMS, 0.0)
    return _cases[name]


@pytest.mark.parametrize("name", sorted(su.ANALYTIC))
def test_stand_in_equals_the_restatement_on_analytic_scenes(name):
    _D, ref, _info, pos, idx, nets_pos, nets_idx = _analytic_case(name)
    assert len(ref) > 100 and len(idx) > 100
    qu.assert_same(name + " positions", pos, ref)
    assert np.array_equal(idx, nets_idx) and pos.shape == nets_pos.shape
    assert not np.array_equal(pos.view(np.uint32), nets_pos.view(np.uint32))


@pytest.mark.parametrize("scene,origin", [("labyrinth", (-5.35, -0.3, -2.55)), ("cube", (-0.7, 0.0, -0.6))])
def test_stand_in_equals_the_restatement_on_the_oracle(scene, origin):
    of = qu.frame(scene, 1.25)

    def f(points, normals):
        return qu.oracle_points(scene, of, points, normals=normals)

    D = f(mu.lattice_points(origin, CELL, DIMS), False)[0]
    ref, _info = su.sharp_nets(D, origin, CELL, DIMS, 0.0, f)
    pos, idx = su.host_extract(D, origin, CELL, DIMS, 0.0, f)
    nets_pos, nets_idx = mu.surface_nets(D, origin, CELL, DIMS, 0.0)
    assert len(ref) > 100
    qu.assert_same(scene + " positions", pos, ref)
    assert np.array_equal(idx, nets_idx) and pos.shape == nets_pos.shape


def test_iso_moves_the_surface():
    f = su.analytic("box")
    D = f(mu.lattice_points(ORIGIN, CELL, DIMS), False)[0]
    ref, _info = su.sharp_nets(D, ORIGIN, CELL, DIMS, 0.04, f)
    pos, idx = su.host_extract(D, ORIGIN, CELL, DIMS, 0.04, f)
    qu.assert_same("positions", pos, ref)
    assert np.array_equal(idx, mu.surface_nets(D, ORIGIN, CELL, DIMS, 0.04)[1])
    # every vertex is nearer the offset surface than one cell (its edges are rounded, not creases: planes there only approximate it)
    assert np.abs(f(pos, False)[0] - 0.04).max() < CELL and np.abs(f(ref, False)[0]).min() > 0.02


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
def _box_measures(pos, idx):
    """(max |D| at the vertices, the largest distance from a corner to its nearest vertex, min cos of the solid triangles' normals to the
    scene's), in cells"""
    f = su.analytic("box")
    at_vertices = np.abs(f(pos, False)[0]).max() / CELL
    corner = max(np.linalg.norm(pos.astype(np.float64) - c[None], axis=1).min() for c in su.box_corners()) / CELL
    fn, area, fc = su.triangles(pos, idx)
    solid = area > 1e-3 * CELL * CELL
    cos = (fn[solid] * f(fc[solid].astype(np.float32), True)[1].astype(np.float64)).sum(1).min()
    return at_vertices, corner, cos


def test_the_box_keeps_its_edges_and_corners():
    _D, _ref, _info, pos, idx, nets_pos, nets_idx = _analytic_case("box")
    at_vertices, corner, cos = _box_measures(pos, idx)
    print("sharp box: |D| %.4g cell, corners %.4g cell, min cos %.6f" % (at_vertices, corner, cos))
    assert at_vertices <= 0.05  # measured 0.0043
    assert corner <= 0.05       # measured 0.0096
    assert cos >= 0.99          # measured 0.999975
    # plain surface nets on the same grid fails all three
    n_vertices, n_corner, n_cos = _box_measures(nets_pos, nets_idx)
    print("nets box: |D| %.4g cell, corners %.4g cell, min cos %.6f" % (n_vertices, n_corner, n_cos))
    assert n_vertices > 0.05 and n_corner > 0.05 and n_cos < 0.99


def _surface_measures(name, pos, idx):
    """(max |D| at the vertices, max |D| at the triangles' centroids, triangles facing inward), in cells"""
    f = su.analytic(name)
    fn, area, fc = su.triangles(pos, idx)
    solid = area > 0
    d, nn = f(fc.astype(np.float32), True)
    inward = int(((fn[solid] * nn[solid].astype(np.float64)).sum(1) <= 0).sum())
    return np.abs(f(pos, False)[0]).max() / CELL, np.abs(d).max() / CELL, inward


def test_the_rotated_box():
    _D, _ref, _info, pos, idx, _np, _ni = _analytic_case("rotated_box")
    at_vertices, at_centroids, inward = _surface_measures("rotated_box", pos, idx)
    print("sharp rotated box: |D| %.4g cell at vertices, %.4g cell at centroids, %d inward" % (at_vertices, at_centroids, inward))
    assert at_vertices <= 0.05   # measured 0.0032
    assert at_centroids <= 0.05  # measured 0.0046
    assert inward == 0


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_smooth_shapes_are_not_worse_than_surface_nets(name):
    _D, _ref, _info, pos, idx, nets_pos, nets_idx = _analytic_case(name)
    _v, at_centroids, inward = _surface_measures(name, pos, idx)
    _nv, nets_centroids, _ni = _surface_measures(name, nets_pos, nets_idx)
    print("%s: centroid |D| sharp %.4g cell, nets %.4g cell" % (name, at_centroids, nets_centroids))
    assert inward == 0 and at_centroids <= nets_centroids


# ---- the clamp -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(su.ANALYTIC))
def test_every_vertex_stays_within_half_a_cell_of_its_cell(name):
    _D, _ref, info, pos, _idx, _np, _ni = _analytic_case(name)
    assert su.in_clamp(pos, info)
    h = np.float32(0.5) * np.float32(CELL)
    axes = mu.lattice_axes(ORIGIN, CELL, DIMS)
    for a in range(3):  # the bounds, from the words of the header
        assert np.array_equal(info["lo"][:, a], axes[a][info["cells"][:, a]] - h) and np.array_equal(info["hi"][:, a], axes[a][info["cells"][:, a] + 1] + h)


def test_the_cliff_needs_the_clamp():
    # two nearly parallel planes that do not meet where the surface changes from one to the other: the cells that see both solve for
    # the planes' far intersection, and the clamp stops them
    _D, _ref, info, pos, _idx, _np, _ni = _analytic_case("cliff")
    on_bound = (pos == info["lo"]) | (pos == info["hi"])
    assert on_bound.any()
    # no other analytic scene needs it
    for name in ("box", "rotated_box", "sphere", "torus"):
        _D, _ref, info, pos, _idx, _np, _ni = _analytic_case(name)
        assert not ((pos == info["lo"]) | (pos == info["hi"])).any(), name


# ---- the guards ----------------------------------------------------------------------------------------------------------------------
def _key(points):
    """a number 0 .. 7 per point, from its bits"""
    b = np.ascontiguousarray(points, np.float32).view(np.uint32).astype(np.uint64)
    return ((b[:, 0] * 2654435761 + b[:, 1] * 40503 + b[:, 2] * 2246822519) >> np.uint64(7)) % 8


def _hostile(mode):
    """the box, with the answers spoiled at the points a key selects: NaN, infinite and huge distances at the bisection's midpoints,
    NaN, infinite and zero normals at the crossings.  (s_lo == s_hi itself cannot be reached: the bracket keeps s_lo < 0 on one side and
    s_hi >= 0 or NaN on the other; infinities of both signs make s_lo / (s_lo - s_hi) NaN, huge values make the difference overflow.)"""
    base = su.analytic("box")

    def f(points, normals):
        d, nn = base(points, normals)
        key = _key(points)
        if not normals:
            if mode in ("distances", "all"):
                with np.errstate(all="ignore"):
                    d = np.where(key == 0, np.float32(np.nan), d)
                    d = np.where(key == 1, np.sign(d) * np.float32(np.inf), d)
                    d = np.where(key == 2, np.sign(d) * np.float32(3e38), d)
                    d = np.where(key == 3, -d, d)
            return d.astype(np.float32), None
        if mode in ("normals", "all"):
            nn = np.where((key == 4)[:, None], np.float32(np.nan), nn)
            nn = np.where((key == 5)[:, None], np.float32(0.0), nn)
            nn[:, 1] = np.where(key == 6, np.float32(np.inf), nn[:, 1])
            d = np.where(key == 7, np.float32(np.nan), d)
        if mode == "no_planes":
            nn = np.zeros_like(nn)
        return d.astype(np.float32), nn.astype(np.float32)

    return f


@pytest.mark.parametrize("mode", ["distances", "normals", "all", "no_planes"])
def test_guards(mode):
    f = _hostile(mode)
    D = su.analytic("box")(mu.lattice_points(ORIGIN, CELL, DIMS), False)[0]
    ref, info = su.sharp_nets(D, ORIGIN, CELL, DIMS, 0.0, f)
    pos, idx = su.host_extract(D, ORIGIN, CELL, DIMS, 0.0, f)
    assert np.isfinite(pos).all() and len(pos) > 100
    qu.assert_same(mode + " positions", pos, ref)
    assert su.in_clamp(pos, info) and np.array_equal(idx, mu.surface_nets(D, ORIGIN, CELL, DIMS, 0.0)[1])
    if mode == "no_planes":
        assert (info["planes"] == 0).all()
        qu.assert_same("the mass points", pos, info["m"])
    elif mode != "distances":
        assert (info["planes"] < info["crossings"]).any()  # crossings that contribute no plane


# ---- the sanitizers ------------------------------------------------------------------------------------------------------------------
def test_the_program_under_sanitizers_gives_the_same_meshes():
    plain, checked = su.run_program(False), su.run_program(True)
    for name in su.ANALYTIC:
        _D, ref, _info, _pos, idx, _np, _ni = _analytic_case(name)
        for what, got in (("plain", plain[name]), ("sanitized", checked[name])):
            qu.assert_same("%s %s positions" % (name, what), got[0], ref)
            assert np.array_equal(got[1], idx), (name, what)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_and_exported():
    import sdf_playground_amd as sp

    assert "sdfr_mesh_extract_sharp" in sp.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, "include", "sdfr.h")).read()
    assert "int sdfr_mesh_extract_sharp(sdfr_renderer *r, const sdfr_mesh_grid *grid" in header
    lib = sp.load_library()
    assert lib.sdfr_mesh_extract_sharp.argtypes == lib.sdfr_mesh_extract.argtypes
    # a NULL handle is refused before anything is looked at, as by sdfr_mesh_extract
    assert lib.sdfr_mesh_extract_sharp(None, None, 0, 0, None, None, None, None, 1) == -1


def test_a_run_time_scene_compiles_with_the_sharp_kernel():
    import sdf_playground_amd as sp

    csrc = os.path.join(ROOT, "sdf_playground_amd", "csrc")
    # the kind's row, and its two kernels in the query unit of a run-time scene (tests/cpp/query_kernels_host.cpp)
    rep = ku.report()
    row, = [r for r in rep.rows if r.name == "MESH_SHARP"]
    assert (row.stem, row.body, row.args) == ("mesh_sharp", "mesh_sharp_kernel", "MeshSharpArgs")
    for symbol, dbg in (("sdfr_jit_mesh_sharp", "false"), ("sdfr_jit_mesh_sharp_debug", "true")):
        assert 'void %s(SceneKernelArgs<MeshSharpArgs> a) { mesh_sharp_kernel<Scene, %s>(a); }' % (symbol, dbg) in "\n".join(rep.query)
    assert "mesh_sharp_kernel" in open(os.path.join(csrc, "sdfr_query_kernel.h")).read()
    ok, log = sp.check_scene_source(os.path.join(qu.SCENES_DIR, "pendulum.scene.h"))
    assert ok, log

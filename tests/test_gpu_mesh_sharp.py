"""GPU tier of sdfr_mesh_extract_sharp through libsdfr.so: positions bit for bit against the definition of include/sdfr.h restated in
numpy (mesh_sharp_util.sharp_nets) and fed with the oracle's distances and normals; indices and counts equal to sdfr_mesh_extract's;
normals equal to the point query's at the vertices; host and device memory; iso and a dyadic cell; the smallest grids and the vertex
counts around the kernel's groups of four; the capacity rule; a box's corners and faces through the library; the clamp; no side effects on
rendering; composition with the per-vertex queries and the atlas; the CLI."""
import ctypes

import numpy as np
import pytest

import gpu_util as gu
import mesh_sharp_util as su
import mesh_util as mu
import query_util as qu
from gpu_util import renderer  # noqa: F401

pytestmark = pytest.mark.gpu

W, H = 64, 48
DIMS = (37, 29, 21)  # as test_gpu_mesh.py: no multiple of the lattice kernel's bricks, of 256 or of 4
CELL = 0.1
# scene: (time, origin, variables)
CASES = {"fast_sphere": (0.0, (-1.85, -0.3, -1.05), None), "labyrinth": (1.25, (-5.35, -0.3, -2.55), None), "gyroid": (0.5, (-1.85, -0.3, -1.05), None),
         "sierpinski": (0.5, (-1.85, -0.3, -1.05), None), "noise_lod": (0.5, (-1.85, -0.3, -1.05), None),
         # one box of half size 0.8 about (0.03, 1.55, 0.07), off the lattice, in a grid clear of the floor
         "cube": (0.5, (-1.82, 0.31, -0.98), {"size": 0.8, "xpos": 0.03, "ypos": 0.55, "zpos": 0.07})}
CUBE_CENTRE, CUBE_HALF = np.array([0.03, 1.55, 0.07]), 0.8

_refs = {}


def _reference(scene, stime, origin, cell, dims, iso=0.0, variables=None):
    """(the oracle frame, positions, info, surface nets' positions and indices): the definition fed with the oracle (once per case)"""
    key = (scene, stime, origin, cell, dims, iso)
    if key not in _refs:
        of = qu.frame(scene, stime, W, H, variables)

        def f(points, normals):
            return qu.oracle_points(scene, of, points, normals=normals)

        D = f(mu.lattice_points(origin, cell, dims), False)[0]
        pos, info = su.sharp_nets(D, origin, cell, dims, iso, f)
        _refs[key] = (of, pos, info) + mu.surface_nets(D, origin, cell, dims, iso)
    return _refs[key]


def _check_mesh(r, what, ref, origin, cell, dims, iso=0.0, device=True):
    _of, pos_ref, info, _nets_pos, _nets_idx = ref
    n_pos, _n_nrm, n_idx = r.extractMesh(origin, cell, dims, iso=iso)
    pos, nrm, idx = r.extractMesh(origin, cell, dims, iso=iso, sharp=True)
    assert pos.shape == pos_ref.shape == n_pos.shape and idx.shape == n_idx.shape, (what, pos.shape, pos_ref.shape, idx.shape)
    qu.assert_same(what + " positions (host)", pos, pos_ref)
    assert np.array_equal(idx, n_idx), what
    assert su.in_clamp(pos, info), what
    if len(pos):
        _, n_ref = r.queryDistance(pos, normals=True)
        qu.assert_same(what + " normals (host)", nrm, n_ref)
    if device:
        import torch

        dpos, dnrm, didx = r.extractMesh(origin, cell, dims, iso=iso, device=True, sharp=True)
        r.sync()
        torch.cuda.synchronize()
        qu.assert_same(what + " positions (device)", dpos.cpu().numpy(), pos_ref)
        assert np.array_equal(didx.cpu().numpy().view(np.uint32), n_idx), what
        if len(pos):
            qu.assert_same(what + " normals (device)", dnrm.cpu().numpy(), n_ref)
        p2, none, i2 = r.extractMesh(origin, cell, dims, iso=iso, normals=False, sharp=True)
        assert none is None and np.array_equal(p2.view(np.uint32), pos.view(np.uint32)) and np.array_equal(i2, idx)
    return pos, nrm, idx


@pytest.mark.parametrize("scene", sorted(CASES))
def test_sharp_mesh_equals_the_definition(renderer, scene):
    stime, origin, variables = CASES[scene]
    ref = _reference(scene, stime, origin, CELL, DIMS, variables=variables)
    gu.setup(renderer, scene, ref[0], variables)
    try:
        assert len(ref[1]) > 500 and len(ref[4]) > 500
        pos, _nrm, _idx = _check_mesh(renderer, scene, ref, origin, CELL, DIMS)
        assert not np.array_equal(pos.view(np.uint32), ref[3].view(np.uint32))  # (not surface nets' vertices)
    finally:
        if variables:
            renderer.resetVariables()


def test_iso_and_a_dyadic_cell(renderer):
    scene, origin, cell, dims, iso = "sierpinski", (-1.5, 0.0, -1.5), 0.0625, (48, 40, 44), 0.05
    ref = _reference(scene, 0.5, origin, cell, dims, iso)
    gu.setup(renderer, scene, ref[0])
    assert len(ref[1]) > 500
    _check_mesh(renderer, scene, ref, origin, cell, dims, iso, device=False)


def test_smallest_grids(renderer):
    scene = "fast_sphere"
    stime = CASES[scene][0]
    # a 1 x 1 x 1 grid straddling the floor: one vertex, no triangle
    one = ((0.31, -0.04, 0.27), 0.1, (1, 1, 1))
    ref = _reference(scene, stime, *one)
    gu.setup(renderer, scene, ref[0])
    assert len(ref[1]) == 1 and len(ref[4]) == 0
    _check_mesh(renderer, scene + " 1x1x1", ref, *one)
    # nx = 1: a slab through the sphere's flank, quads only along x edges
    slab = ((0.35, -0.3, -1.05), CELL, (1, 29, 21))
    ref = _reference(scene, stime, *slab)
    assert len(ref[1]) > 20 and len(ref[4]) > 0
    _check_mesh(renderer, scene + " nx=1", ref, *slab)
    # a box in empty space
    pos, nrm, idx = renderer.extractMesh((-1.0, 3.0, -1.0), 0.1, (9, 7, 5), sharp=True)
    assert pos.shape == (0, 3) and nrm.shape == (0, 3) and idx.shape == (0, 3)


@pytest.mark.parametrize("vertices", [1, 3, 4, 5, 7, 8, 12, 13])
def test_vertex_counts_around_the_groups_of_four(renderer, vertices):
    # a row of cells straddling the floor, away from the sphere: one vertex per cell, 4 vertices (16 lanes each) per wave of the kernel
    scene = "fast_sphere"
    grid = ((2.31, -0.04, 2.27), 0.1, (vertices, 1, 1))
    ref = _reference(scene, CASES[scene][0], *grid)
    assert len(ref[1]) == vertices
    gu.setup(renderer, scene, ref[0])
    _check_mesh(renderer, "%d vertices" % vertices, ref, *grid)


def test_capacity(renderer):
    import sdf_playground_amd as sp
    import torch

    L = sp.load_library()
    scene = "fast_sphere"
    stime, origin, _v = CASES[scene]
    ref = _reference(scene, stime, origin, CELL, DIMS)
    gu.setup(renderer, scene, ref[0])
    pos_ref, idx_ref = ref[1], ref[4]
    V, T = len(pos_ref), len(idx_ref)
    g = sp.MeshGrid((ctypes.c_float * 3)(*origin), CELL, DIMS[0], DIMS[1], DIMS[2], 0.0)

    def raw(vcap, tcap, pos, nrm, idx):
        counts = sp.MeshCounts(-1, -1)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
        rc = L.sdfr_mesh_extract_sharp(renderer._h, ctypes.byref(g), vcap, tcap, p(pos), p(nrm), p(idx), ctypes.byref(counts), 1)
        return rc, int(counts.vertices), int(counts.triangles)

    assert raw(0, 0, None, None, None) == (0, V, T)  # the counting call
    for vcap, tcap in ((V - 1, T), (V, T - 1)):
        pos, nrm, idx = np.full((V, 3), 7.5, np.float32), np.full((V, 3), 7.5, np.float32), np.full((T, 3), 0xABCDEF01, np.uint32)
        assert raw(vcap, tcap, pos, nrm, idx) == (0, V, T)
        assert (pos == 7.5).all() and (nrm == 7.5).all() and (idx == 0xABCDEF01).all()
        dpos = torch.full((V, 3), 7.5, dtype=torch.float32, device="cuda")
        didx = torch.full((T, 3), 0x2BCDEF01, dtype=torch.int32, device="cuda")
        counts = sp.MeshCounts()
        assert L.sdfr_mesh_extract_sharp(renderer._h, ctypes.byref(g), vcap, tcap, ctypes.c_void_p(dpos.data_ptr()), None, ctypes.c_void_p(didx.data_ptr()),
                                         ctypes.byref(counts), 0) == 0
        renderer.sync()
        assert (counts.vertices, counts.triangles) == (V, T) and bool((dpos == 7.5).all()) and bool((didx == 0x2BCDEF01).all())
    # exact capacities succeed, and fill nothing past the counts
    pos, nrm, idx = np.full((V + 1, 3), 7.5, np.float32), np.full((V + 1, 3), 7.5, np.float32), np.full((T + 1, 3), 0xABCDEF01, np.uint32)
    assert raw(V, T, pos, nrm, idx) == (0, V, T)
    qu.assert_same("positions", pos[:V], pos_ref)
    assert np.array_equal(idx[:T], idx_ref) and (pos[V] == 7.5).all() and (nrm[V] == 7.5).all() and (idx[T] == 0xABCDEF01).all()
    assert not (nrm[:V] == 7.5).any()
    # the argument errors are sdfr_mesh_extract's
    assert raw(-1, 0, None, None, None)[0] == -1 and L.sdfr_last_error(renderer._h).decode() == "negative capacity"


def _cube_measures(r, pos, cells):
    """(max |D| at the vertices off the grid's boundary cells, the largest distance from a corner of the box to its nearest vertex), in cells"""
    inner = np.ones(len(pos), bool)
    for a in range(3):
        inner &= (cells[:, a] >= 1) & (cells[:, a] <= DIMS[a] - 2)
    assert inner.any()
    at_vertices = np.abs(r.queryDistance(pos[inner])).max() / CELL
    corners = CUBE_CENTRE[None] + CUBE_HALF * np.array([[(c & 1) * 2 - 1, ((c >> 1) & 1) * 2 - 1, (c >> 2) * 2 - 1] for c in range(8)], np.float64)
    return at_vertices, max(np.linalg.norm(pos.astype(np.float64) - c[None], axis=1).min() for c in corners) / CELL


def test_the_cube_keeps_its_edges_and_corners(renderer):
    scene = "cube"
    stime, origin, variables = CASES[scene]
    ref = _reference(scene, stime, origin, CELL, DIMS, variables=variables)
    gu.setup(renderer, scene, ref[0], variables)
    try:
        pos, _nrm, _idx = renderer.extractMesh(origin, CELL, DIMS, sharp=True)
        nets, _nn, _ni = renderer.extractMesh(origin, CELL, DIMS)
        at_vertices, corner = _cube_measures(renderer, pos, ref[2]["cells"])
        n_vertices, n_corner = _cube_measures(renderer, nets, ref[2]["cells"])
    finally:
        renderer.resetVariables()
    print("cube: |D| sharp %.4g cell, nets %.4g cell; corners sharp %.4g cell, nets %.4g cell" % (at_vertices, n_vertices, corner, n_corner))
    assert at_vertices <= 0.05 and corner <= 0.05
    assert n_vertices > 0.05 and n_corner > 0.05


def test_sharp_mesh_leaves_rendering_alone(renderer):
    import torch

    scene = "labyrinth"
    stime, origin, _v = CASES[scene]
    ref = _reference(scene, stime, origin, CELL, DIMS)
    gu.setup(renderer, scene, ref[0])
    pos_ref = ref[1]
    with gu.rendering_untouched(renderer, 64, 48) as (img0, s0):
        _p, _n, idx_ref = _check_mesh(renderer, scene, ref, origin, CELL, DIMS)
    # two frames in flight: the extraction runs on the lane of the frame submitted last; device arrays are read after sdfr_sync
    renderer.setFramesInFlight(2)
    try:
        imgs = [torch.empty((48, 64, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        for k in range(4):
            renderer.render(None, 64, 48, out=imgs[k % 2])
            pos, _nrm, idx = renderer.extractMesh(origin, CELL, DIMS, sharp=True)
            dpos, _dn, didx = renderer.extractMesh(origin, CELL, DIMS, device=True, sharp=True)
            renderer.sync()
            qu.assert_same("positions", pos, pos_ref)
            qu.assert_same("positions (device)", dpos.cpu().numpy(), pos_ref)
            assert np.array_equal(idx, idx_ref) and np.array_equal(didx.cpu().numpy().view(np.uint32), idx_ref)
            assert np.array_equal(imgs[k % 2].cpu().numpy().view(np.uint32), img0.view(np.uint32))
            assert gu.stats(renderer) == s0
    finally:
        renderer.setFramesInFlight(1)
    # the stage timings keep their four slots, the sharp vertices in "emit"
    renderer.setProfiling(True)
    try:
        renderer.extractMesh(origin, CELL, DIMS, sharp=True)
        t = renderer.getMeshTimings()
        assert len(t) == 4 and all(v > 0 for v in t.values()), t
    finally:
        renderer.setProfiling(False)


def test_composition(renderer):
    scene = "labyrinth"
    stime, origin, _v = CASES[scene]
    ref = _reference(scene, stime, origin, CELL, DIMS)
    gu.setup(renderer, scene, ref[0])
    options = dict(surfaces=True, occlusion=True, lighting=True, atlas=dict(tile=4))
    sharp = renderer.extractMesh(origin, CELL, DIMS, sharp=True, **options)
    nets = renderer.extractMesh(origin, CELL, DIMS, **options)
    assert len(sharp) == len(nets) == 7
    qu.assert_same("positions", sharp[0], ref[1])
    assert np.array_equal(sharp[2], nets[2])
    for a, b in zip(sharp[:6], nets[:6]):
        assert a.shape == b.shape and a.dtype == b.dtype
    assert sorted(sharp[6]) == sorted(nets[6])
    for key, a in sharp[6].items():
        if hasattr(a, "shape"):
            assert a.shape == nets[6][key].shape and a.dtype == nets[6][key].dtype, key
    # every texel of a tile whose quad is well formed has an answer
    at = sharp[6]["atlas"]
    valid = sharp[6]["valid"]
    T = at.tile
    tiles = valid[:at.rows * T, :at.tiles_per_row * T].reshape(at.rows, T, at.tiles_per_row, T).transpose(0, 2, 1, 3).reshape(-1, T * T)[:at.quads]
    well_formed = (tiles != -1).any(1)
    assert well_formed.any() and not (tiles[well_formed] == -1).any()
    # the vertices sit on the surface: at least as many see it along their normal as of surface nets' vertices
    share, nets_share = float((sharp[3]["valid"] == 1).mean()), float((nets[3]["valid"] == 1).mean())
    print("meshSurfaces valid: sharp %.4f, nets %.4f" % (share, nets_share))
    assert share >= nets_share


def test_cli_writes_a_sharp_obj(tmp_path):
    from sdf_playground_amd import cli

    common = ["--scene", "cube", "--mesh-box", "-1.45", "0.25", "-1.45", "1.45", "2.55", "1.45", "--mesh-cell", "0.1"]
    nets, sharp = tmp_path / "nets.obj", tmp_path / "sharp.obj"
    assert cli.main(common + ["--mesh", str(nets)]) == 0
    assert cli.main(common + ["--mesh", str(sharp), "--mesh-sharp"]) == 0
    lines = {k: p.read_text().splitlines() for k, p in (("nets", nets), ("sharp", sharp))}
    pick = lambda k, tag: [s for s in lines[k] if s.startswith(tag + " ")]  # noqa: E731
    assert len(pick("sharp", "f")) > 50 and pick("sharp", "f") == pick("nets", "f")
    assert len(pick("sharp", "v")) == len(pick("nets", "v")) and pick("sharp", "v") != pick("nets", "v")

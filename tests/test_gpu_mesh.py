"""GPU tier of sdfr_mesh_extract through libsdfr.so: counts, positions and indices bit for bit against the definition of
include/sdfr.h restated in numpy (mesh_util.surface_nets) and fed with the oracle's distances at the lattice points; normals equal to
the point query's at the vertices; host and device memory; the prefix sums at depth; degenerate grids; the capacity rule; closed,
outward-oriented surfaces of two analytic scenes; no side effects on rendering; argument checks."""
import ctypes

import numpy as np
import pytest

import gpu_util as gu
import mesh_util as mu
import query_util as qu
from gpu_util import DEFAULT_LIMITS
from gpu_util import renderer  # noqa: F401

pytestmark = pytest.mark.gpu

W, H = 64, 48
# 37 x 29 x 21 cells: no multiple of the lattice kernel's 4 x 4 x 4 bricks nor of the 256-element blocks of the other kernels
DIMS = (37, 29, 21)
CELL = 0.1
# scene: (time, origin); the gyroid's surface leaves the box (an open mesh), the labyrinth's box lies over a wall's corner
CASES = {"fast_sphere": (0.0, (-1.85, -0.3, -1.05)), "labyrinth": (1.25, (-5.35, -0.3, -2.55)), "gyroid": (0.5, (-1.85, -0.3, -1.05)),
         "sierpinski": (0.5, (-1.85, -0.3, -1.05)), "noise_lod": (0.5, (-1.85, -0.3, -1.05))}
assert "noise_lod" in qu.HLSL  # the run-time scene: its lattice kernel comes from the lazily compiled query module

_refs = {}


def _reference(scene, stime, origin, cell, dims, iso=0.0):
    """the definition fed with the oracle's distances (computed once per case)"""
    key = (scene, stime, origin, cell, dims, iso)
    if key not in _refs:
        of = qu.frame(scene, stime, W, H)
        D, _ = qu.oracle_points(scene, of, mu.lattice_points(origin, cell, dims), normals=False)
        _refs[key] = (of,) + mu.surface_nets(D, origin, cell, dims, iso)
    return _refs[key]


def _check_mesh(r, what, pos_ref, idx_ref, origin, cell, dims, iso=0.0, device=True):
    pos, nrm, idx = r.extractMesh(origin, cell, dims, iso=iso)
    assert pos.shape == pos_ref.shape and idx.shape == idx_ref.shape, (what, pos.shape, pos_ref.shape, idx.shape, idx_ref.shape)
    qu.assert_same(what + " positions (host)", pos, pos_ref)
    assert np.array_equal(idx, idx_ref), what
    if len(pos):
        _, n_ref = r.queryDistance(pos, normals=True)
        qu.assert_same(what + " normals (host)", nrm, n_ref)
    if device:
        import torch

        dpos, dnrm, didx = r.extractMesh(origin, cell, dims, iso=iso, device=True)
        r.sync()
        torch.cuda.synchronize()
        qu.assert_same(what + " positions (device)", dpos.cpu().numpy(), pos_ref)
        assert np.array_equal(didx.cpu().numpy().view(np.uint32), idx_ref), what
        if len(pos):
            qu.assert_same(what + " normals (device)", dnrm.cpu().numpy(), n_ref)
        p2, none, i2 = r.extractMesh(origin, cell, dims, iso=iso, normals=False)
        assert none is None and np.array_equal(p2.view(np.uint32), pos.view(np.uint32)) and np.array_equal(i2, idx)
    return pos, nrm, idx


@pytest.mark.parametrize("scene", sorted(CASES))
def test_mesh_equals_the_definition(renderer, scene):
    stime, origin = CASES[scene]
    of, pos_ref, idx_ref = _reference(scene, stime, origin, CELL, DIMS)
    gu.setup(renderer, scene, of)
    assert len(pos_ref) > 500 and len(idx_ref) > 500
    _check_mesh(renderer, scene, pos_ref, idx_ref, origin, CELL, DIMS)


def test_the_gyroid_mesh_is_open(renderer):
    _of, pos_ref, idx_ref = _reference("gyroid", *CASES["gyroid"], CELL, DIMS)
    e = mu.directed_edges(idx_ref)
    und = np.minimum(e[:, 0], e[:, 1]) * len(pos_ref) + np.maximum(e[:, 0], e[:, 1])
    assert (np.unique(und, return_counts=True)[1] == 1).any()


def test_iso_and_a_dyadic_cell(renderer):
    scene, origin, cell, dims, iso = "sierpinski", (-1.5, 0.0, -1.5), 0.0625, (48, 40, 44), 0.05
    of, pos_ref, idx_ref = _reference(scene, 0.5, origin, cell, dims, iso)
    gu.setup(renderer, scene, of)
    assert len(pos_ref) > 500
    _check_mesh(renderer, scene, pos_ref, idx_ref, origin, cell, dims, iso, device=False)


def test_scan_at_depth(renderer):
    # The prefix sums work on blocks of 256 elements (SDFR_MESH_BLOCK, sdfr_mesh.h) and recurse on the block totals.  48^3 cells =
    # 110592 (+1) flags: 433 blocks, whose totals take 2 blocks, whose totals take the final single block -- so both levels that
    # can have more than one block do, for the cells and for the 49^3 = 117649 (+1) lattice points alike (460 -> 2 -> 1).
    scene, origin, cell, dims = "labyrinth", (-5.5, -0.25, -3.5), 0.125, (48, 48, 48)
    assert (dims[0] * dims[1] * dims[2] + 1 + 255) // 256 > 256
    of, pos_ref, idx_ref = _reference(scene, 1.25, origin, cell, dims)
    gu.setup(renderer, scene, of)
    assert len(pos_ref) > 5000
    _check_mesh(renderer, scene, pos_ref, idx_ref, origin, cell, dims)


def test_degenerate_grids(renderer):
    scene = "fast_sphere"
    stime, origin = CASES[scene]
    # nx = 1: vertices, and quads only along x edges (for y and z edges P's x coordinate would have to be >= 1 and <= 0)
    dims = (1, 29, 21)
    o = (0.35, -0.3, -1.05)  # a slab through the sphere's flank, where x edges cross its surface
    of, pos_ref, idx_ref = _reference(scene, stime, o, CELL, dims)
    gu.setup(renderer, scene, of)
    assert len(pos_ref) > 20 and len(idx_ref) > 0
    pos, _nrm, idx = _check_mesh(renderer, scene + " nx=1", pos_ref, idx_ref, o, CELL, dims)
    # a 1 x 1 x 1 grid straddling the floor: one vertex, no triangle
    one = ((0.31, -0.04, 0.27), 0.1, (1, 1, 1))
    _of, p1, i1 = _reference(scene, stime, *one)
    assert len(p1) == 1 and len(i1) == 0
    _check_mesh(renderer, scene + " 1x1x1", p1, i1, *one)
    # a box in empty space
    pos, nrm, idx = renderer.extractMesh((-1.0, 3.0, -1.0), 0.1, (9, 7, 5))
    assert pos.shape == (0, 3) and nrm.shape == (0, 3) and idx.shape == (0, 3)
    dpos, _dn, didx = renderer.extractMesh((-1.0, 3.0, -1.0), 0.1, (9, 7, 5), device=True)
    assert tuple(dpos.shape) == (0, 3) and tuple(didx.shape) == (0, 3)


def _raw(L, h, grid, vcap, tcap, pos, nrm, idx, on_host=1):
    import sdf_playground_amd as sp

    counts = sp.MeshCounts(-1, -1)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
    rc = L.sdfr_mesh_extract(h, ctypes.byref(grid) if grid is not None else None, vcap, tcap, p(pos), p(nrm), p(idx), ctypes.byref(counts), on_host)
    return rc, int(counts.vertices), int(counts.triangles)


def _grid(origin, cell, dims, iso=0.0):
    import sdf_playground_amd as sp

    return sp.MeshGrid((ctypes.c_float * 3)(*origin), cell, dims[0], dims[1], dims[2], iso)


def test_capacity(renderer):
    import sdf_playground_amd as sp
    import torch

    L = sp.load_library()
    scene = "fast_sphere"
    stime, origin = CASES[scene]
    of, pos_ref, idx_ref = _reference(scene, stime, origin, CELL, DIMS)
    gu.setup(renderer, scene, of)
    V, T = len(pos_ref), len(idx_ref)
    g = _grid(origin, CELL, DIMS)
    assert _raw(L, renderer._h, g, 0, 0, None, None, None) == (0, V, T)  # the counting call
    for vcap, tcap in ((V - 1, T), (V, T - 1)):
        pos, nrm, idx = np.full((V, 3), 7.5, np.float32), np.full((V, 3), 7.5, np.float32), np.full((T, 3), 0xABCDEF01, np.uint32)
        assert _raw(L, renderer._h, g, vcap, tcap, pos, nrm, idx) == (0, V, T)
        assert (pos == 7.5).all() and (nrm == 7.5).all() and (idx == 0xABCDEF01).all()
        dpos = torch.full((V, 3), 7.5, dtype=torch.float32, device="cuda")
        didx = torch.full((T, 3), 0x2BCDEF01, dtype=torch.int32, device="cuda")
        counts = sp.MeshCounts()
        assert L.sdfr_mesh_extract(renderer._h, ctypes.byref(g), vcap, tcap, ctypes.c_void_p(dpos.data_ptr()), None, ctypes.c_void_p(didx.data_ptr()),
                                   ctypes.byref(counts), 0) == 0
        renderer.sync()
        assert (counts.vertices, counts.triangles) == (V, T) and bool((dpos == 7.5).all()) and bool((didx == 0x2BCDEF01).all())
    # exact capacities succeed, and fill nothing past the counts
    pos, nrm, idx = np.full((V + 1, 3), 7.5, np.float32), np.full((V + 1, 3), 7.5, np.float32), np.full((T + 1, 3), 0xABCDEF01, np.uint32)
    assert _raw(L, renderer._h, g, V, T, pos, nrm, idx) == (0, V, T)
    qu.assert_same("positions", pos[:V], pos_ref)
    assert np.array_equal(idx[:T], idx_ref) and (pos[V] == 7.5).all() and (nrm[V] == 7.5).all() and (idx[T] == 0xABCDEF01).all()
    assert not (nrm[:V] == 7.5).any()


SPHERE = """struct Scene
{
	static SDF_HD void prepare(FrameU &) {}
	struct RayInv {};
	static SDF_HD RayInv ray_setup(const FrameU &, vec3, const RayFlags &) { return RayInv(); }
	static SDF_HD float dist(const FrameU &, const RayInv &, vec3 p, vec3, bool) { return sd_sphere(p - V3(0.03f, 0.05f, 0.07f), 1.f); }
	static SDF_HD void material(const FrameU &, const SurfacePoint &, Material &) {}
	static SDF_HD bool light(const FrameU &, int i, Light &L) { return sun_light(i, L); }
	static SDF_HD float ambient() { return 0.1f; }
	static SDF_HD vec3 background(const FrameU &U, vec3 dir, uint32_t) { return sky_color(dir, U.sky_s, U.sky_c); }
};
"""
TORUS = SPHERE.replace("return sd_sphere(p - V3(0.03f, 0.05f, 0.07f), 1.f);",
                       "const vec3 q = p - V3(0.03f, 0.05f, 0.07f); return length(V2(length(V2(q.x, q.z)) - 1.f, q.y)) - 0.4f;")


@pytest.mark.parametrize("name", sorted(mu.TOPOLOGY))
def test_topology(renderer, name):
    origin, cell, dims, _euler = mu.TOPOLOGY[name]
    renderer.initShaderSource("mesh_" + name, SPHERE if name == "sphere" else TORUS)
    renderer.setLimits(**DEFAULT_LIMITS)
    pos, nrm, idx = renderer.extractMesh(origin, cell, dims)
    assert len(pos) > 500
    # the scene is the analytic distance (to rounding), and the mesh the definition's on the library's own lattice distances
    D = renderer.queryDistance(mu.lattice_points(origin, cell, dims))
    assert np.abs(D - mu.analytic_distance(name, mu.lattice_points(origin, cell, dims))).max() < 1e-5
    pos_ref, idx_ref = mu.surface_nets(D, origin, cell, dims, 0.0)
    qu.assert_same(name + " positions", pos, pos_ref)
    assert np.array_equal(idx, idx_ref)
    mu.check_surface(name, pos, idx, cell, renderer.queryDistance(pos), lambda p: renderer.queryDistance(p.astype(np.float32), normals=True)[1])
    assert ((nrm.astype(np.float64) * mu.analytic_normal(name, pos)).sum(1) > 0.99).all()


def test_mesh_leaves_rendering_alone(renderer):
    import torch

    scene = "labyrinth"
    stime, origin = CASES[scene]
    of, pos_ref, idx_ref = _reference(scene, stime, origin, CELL, DIMS)
    gu.setup(renderer, scene, of)
    with gu.rendering_untouched(renderer, 64, 48) as (img0, s0):
        _check_mesh(renderer, scene, pos_ref, idx_ref, origin, CELL, DIMS)
    # two frames in flight: the extraction runs on the lane of the frame submitted last; device arrays are read after sdfr_sync
    renderer.setFramesInFlight(2)
    try:
        imgs = [torch.empty((48, 64, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        for k in range(4):
            renderer.render(None, 64, 48, out=imgs[k % 2])
            pos, _nrm, idx = renderer.extractMesh(origin, CELL, DIMS)
            dpos, _dn, didx = renderer.extractMesh(origin, CELL, DIMS, device=True)
            renderer.sync()
            qu.assert_same("positions", pos, pos_ref)
            qu.assert_same("positions (device)", dpos.cpu().numpy(), pos_ref)
            assert np.array_equal(idx, idx_ref) and np.array_equal(didx.cpu().numpy().view(np.uint32), idx_ref)
            assert np.array_equal(imgs[k % 2].cpu().numpy().view(np.uint32), img0.view(np.uint32))
            assert gu.stats(renderer) == s0
    finally:
        renderer.setFramesInFlight(1)


def test_arguments(renderer):
    import sdf_playground_amd as sp

    L = sp.load_library()
    gu.setup(renderer, "fast_sphere", qu.frame("fast_sphere", 0.0, W, H))
    h = renderer._h
    o, dims = (-0.5, -0.3, -0.5), (8, 8, 8)
    buf, ibuf = np.zeros((4096, 3), np.float32), np.zeros((8192, 3), np.uint32)
    INVALID, NO_SCENE = -1, -4

    def refused(text, *args, **kwargs):
        """SDFR_ERR_INVALID_ARGUMENT, with the text tests/test_mesh_plan_cpu.py names for the fault"""
        return _raw(L, h, *args, **kwargs)[0] == INVALID and L.sdfr_last_error(h).decode() == text

    assert _raw(L, h, _grid(o, 0.1, dims), 4096, 8192, buf, None, ibuf)[0] == 0  # (normals may be NULL)
    bad_grids = [_grid(o, 0.0, dims), _grid(o, -0.1, dims), _grid(o, float("inf"), dims), _grid(o, float("nan"), dims),
                 _grid((float("nan"), 0.0, 0.0), 0.1, dims), _grid((0.0, float("inf"), 0.0), 0.1, dims), _grid(o, 0.1, dims, float("nan")),
                 _grid(o, 0.1, (0, 8, 8)), _grid(o, 0.1, (8, -1, 8)), _grid(o, 0.1, (8, 8, 1025)), _grid(o, 0.1, (1024, 1024, 1024))]
    for g in bad_grids:
        assert refused("bad mesh grid", g, 0, 0, None, None, None)
    assert refused("on_host must be 0 or 1", _grid(o, 0.1, (1023, 1023, 1023)), 0, 0, None, None, None, on_host=2)  # (the largest grid is a good one)
    g = _grid(o, 0.1, dims)
    assert refused("null pointer", None, 0, 0, None, None, None)
    assert L.sdfr_mesh_extract(h, ctypes.byref(g), 0, 0, None, None, None, None, 1) == INVALID  # counts is required
    assert L.sdfr_last_error(h).decode() == "null pointer"
    assert refused("null array with a capacity", g, 1, 0, None, None, None)
    assert refused("null array with a capacity", g, 0, 1, None, None, None)
    assert refused("null array with a capacity", g, 4096, 1, buf, None, None)
    assert refused("negative capacity", g, -1, 0, None, None, None)
    assert refused("negative capacity", g, 0, -1, None, None, None)
    for bad in (-1, 2):
        assert refused("on_host must be 0 or 1", g, 0, 0, None, None, None, on_host=bad)
    # two faults at once: the text of the one checked first
    assert refused("null pointer", None, 0, 0, None, None, None, on_host=2)
    assert refused("on_host must be 0 or 1", bad_grids[0], 0, 0, None, None, None, on_host=2)
    assert refused("bad mesh grid", bad_grids[7], -1, 0, None, None, None)
    assert refused("negative capacity", g, -1, 1, None, None, None)
    assert _raw(L, None, g, 0, 0, None, None, None)[0] == INVALID
    fresh = sp.SDFRenderer(0)
    try:
        assert _raw(L, fresh._h, g, 0, 0, None, None, None)[0] == NO_SCENE
    finally:
        fresh.close()
    # stage timings exist only for an extraction made with profiling on
    ms = (ctypes.c_double * 4)()
    renderer.extractMesh(o, 0.1, dims)
    assert L.sdfr_mesh_get_timings(h, ctypes.byref(ms)) == INVALID
    renderer.setProfiling(True)
    try:
        renderer.extractMesh(o, 0.1, dims)
        t = renderer.getMeshTimings()
        assert all(v > 0 for v in t.values()), t
    finally:
        renderer.setProfiling(False)


def test_cli_writes_an_obj(tmp_path):
    from sdf_playground_amd import cli

    out = tmp_path / "sphere.obj"
    assert cli.main(["--scene", "fast_sphere", "--mesh", str(out), "--mesh-box", "-1", "0.2", "-1", "1", "1.8", "1", "--mesh-cell", "0.1"]) == 0
    lines = out.read_text().splitlines()
    nv, nn, nf = (sum(1 for s in lines if s.startswith(tag + " ")) for tag in ("v", "vn", "f"))
    assert nv > 50 and nn == nv and nf > 50
    assert max(int(c.split("//")[0]) for s in lines if s.startswith("f ") for c in s.split()[1:]) == nv

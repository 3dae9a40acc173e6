"""GPU tier of sdfr_components_label and sdfr_components_label_lattice through libsdfr.so: every label, record and count equal to the
definition of include/sdfr.h restated in numpy (components_util.label), fed with the oracle's distances for the scenes of the issue's
table and with the synthetic lattices of the CPU tier; host and device memory; small and ragged grids; determinism; the capacity rule;
odd alignments; the argument errors through the raw C ABI; no scene; no side effects on rendering; a hollow sphere whose answer is known
without any oracle; the CLI."""
import ctypes
import json

import numpy as np
import pytest

import components_util as cu
import gpu_util as gu
import mesh_util as mu
import query_util as qu
from gpu_util import renderer  # noqa: F401

pytestmark = pytest.mark.gpu


def _both_sides(r, what, want, call):
    """call(device) on the host and on the device against the definition's"""
    cu.assert_same(what + " (host)", call(False), want)
    counts, records, labels = call(True)
    cu.assert_same(what + " (device)", (counts,) + gu.to_host((records, labels)), want)


# ---- the loaded scene -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(cu.TABLE))
def test_scene_equals_the_definition(renderer, key):
    (scene, _stime, origin, cell, dims, iso, variables), pinned, _largest = cu.TABLE[key]
    of, _D, want = cu.oracle_case(key)
    for name, value in pinned.items():
        assert want[0][name] == value, (key, name)  # (the CPU tier holds the whole table; a trivial partition cannot pass here either)
    gu.setup(renderer, scene, of, variables)
    try:
        _both_sides(renderer, key, want, lambda device: renderer.labelComponents(origin, cell, dims, iso=iso, labels=True, device=device))
        counts, records, none = renderer.labelComponents(origin, cell, dims, iso=iso)
        assert none is None
        cu.assert_same(key + " without labels", (counts, records, None), want)
        assert counts["inside_points"] == renderer.surveyMesh(origin, cell, dims, iso=iso)["inside_points"]
    finally:
        if variables:
            renderer.resetVariables()


@pytest.mark.parametrize("dims", [(1, 1, 1), (7, 5, 3), (8, 8, 8), (9, 17, 5)])
def test_small_and_ragged_grids(renderer, dims):
    scene, origin, cell = "fast_sphere", (-0.43, 0.55, -0.37), 0.1  # across the sphere's flank
    of = qu.frame(scene, 0.0, cu.W, cu.H)
    D = qu.oracle_points(scene, of, mu.lattice_points(origin, cell, dims), normals=False)[0]
    want = cu.label(D, dims)
    gu.setup(renderer, scene, of)
    _both_sides(renderer, str(dims), want, lambda device: renderer.labelComponents(origin, cell, dims, labels=True, device=device))


# ---- the caller's lattice -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dims", cu.synthetic_cases(((8, 8, 8), (33, 9, 5))))
def test_lattice_equals_the_definition(renderer, name, dims):
    D, iso = cu.synthetic(name, dims)
    want = cu.label(D, dims, iso)
    _both_sides(renderer, name, want, lambda device: renderer.labelLattice(D, iso=iso, labels=True, device=device))
    got = renderer.labelLattice(gu.to_device(D), iso=iso, labels=True)  # a device tensor in
    cu.assert_same(name + " (tensor)", (got[0],) + gu.to_host(got[1:]), want)


def test_many_bricks_race_on_one_component(renderer):
    dims = (64, 64, 64)  # 729 bricks
    D, iso = cu.synthetic("serpentine", dims)
    want = cu.label(D, dims, iso)
    assert want[0]["solids"] == 1 and want[0]["largest_solid_points"] > 60000
    first = renderer.labelLattice(gu.to_device(D), labels=True)
    cu.assert_same("serpentine 64", (first[0],) + gu.to_host(first[1:]), want)
    # the same call twice gives the same bits
    again = renderer.labelLattice(gu.to_device(D), labels=True)
    assert again[0] == first[0]
    for a, b in zip(gu.to_host(first[1:]), gu.to_host(again[1:])):
        assert np.array_equal(a, b)


def test_more_components_than_the_workspace_first_has_room_for():
    import sdf_playground_amd as sp

    dims = (47, 47, 31)  # 73728 points, each its own component: more than the 65536 records the workspace is first cut for
    D, iso = cu.synthetic("checkerboard", dims)
    want = cu.label(D, dims, iso)
    assert want[0]["components"] == 48 * 48 * 32 > 1 << 16
    fresh = sp.SDFRenderer(0)  # (its workspace has to grow in the middle of the call)
    try:
        _both_sides(fresh, "checkerboard", want, lambda device: fresh.labelLattice(D, labels=True, device=device))
    finally:
        fresh.close()


def test_determinism_of_a_scene(renderer):
    key = "gyroid"
    (scene, _t, origin, cell, dims, iso, _v), _p, _l = cu.TABLE[key]
    gu.setup(renderer, scene, cu.oracle_case(key)[0])
    a = renderer.labelComponents(origin, cell, dims, iso=iso, labels=True)
    b = renderer.labelComponents(origin, cell, dims, iso=iso, labels=True)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


# ---- the protocol ----------------------------------------------------------------------------------------------------------------------
def _raw(r, grid, capacity, records, labels, on_host=1, lattice=None, counts=True, handle=True):
    """-> (status, error text, the counts or None).  records / labels / lattice: numpy arrays, device tensors or None"""
    import sdf_playground_amd as sp

    L, h = gu.raw(r)
    h = h if handle else None
    c = sp.ComponentCounts(components=-7, solids=-7)
    p = lambda a: None if a is None else (ctypes.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else a.ctypes.data_as(ctypes.c_void_p))  # noqa: E731
    g = ctypes.byref(grid) if grid is not None else None
    out = ctypes.byref(c) if counts else None
    if lattice is None:
        rc = L.sdfr_components_label(h, g, capacity, p(records), p(labels), out, on_host)
    else:
        rc = L.sdfr_components_label_lattice(h, g, p(lattice) if lattice is not False else None, capacity, p(records), p(labels), out, on_host)
    if rc != 0:
        assert (c.components, c.solids) == (-7, -7)  # nothing is written on error
    return rc, (L.sdfr_last_error(h).decode() if h and rc else ""), (c.as_dict() if rc == 0 else None)


def _grid(dims, iso=0.0, origin=(0.0, 0.0, 0.0), cell=1.0):
    import sdf_playground_amd as sp

    return sp.MeshGrid((ctypes.c_float * 3)(*origin), cell, dims[0], dims[1], dims[2], iso)


def test_fill_rule_and_alignment(renderer):
    import torch

    dims = (33, 9, 5)
    D, iso = cu.synthetic("noise", dims)
    want = cu.label(D, dims, iso)
    C, N = want[0]["components"], D.size
    assert C > 8
    g = _grid(dims, iso)
    PATTERN = 0xA5
    assert _raw(renderer, g, 0, None, None, lattice=D) == (0, "", want[0])  # the counting call
    # one below the count: the records stay untouched, the counts are right, the labels are written all the same
    records, labels = np.full(C * 40, PATTERN, np.uint8), np.full(N, 0xABCDEF01, np.uint32)
    assert _raw(renderer, g, C - 1, records, labels, lattice=D) == (0, "", want[0])
    assert (records == PATTERN).all() and np.array_equal(labels.reshape(D.shape), want[2])
    d_records, d_labels = torch.full((C * 10,), 0x25252525, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
    assert _raw(renderer, g, C - 1, d_records, d_labels, on_host=0, lattice=gu.to_device(D)) == (0, "", want[0])
    assert bool((d_records == 0x25252525).all()) and np.array_equal(gu.to_host(d_labels).view(np.uint32).reshape(D.shape), want[2])
    # the exact capacity and one more fill C records and nothing past them; records 8 bytes off 16-byte alignment, labels 4 bytes off
    for capacity in (C, C + 1):
        store_r, store_l = np.full((C + 1) * 40 + 32, PATTERN, np.uint8), np.full(N + 8, 0xABCDEF01, np.uint32)
        at_r = (-store_r.ctypes.data) % 16 + 8
        at_l = ((-store_l.ctypes.data) % 16) // 4 + 1
        records, labels = store_r[at_r:at_r + (C + 1) * 40], store_l[at_l:at_l + N]
        assert records.ctypes.data % 16 == 8 and labels.ctypes.data % 16 == 4
        assert _raw(renderer, g, capacity, records, labels, lattice=D) == (0, "", want[0])
        cu.assert_same("host", (want[0], records[:C * 40].view(cu.RECORD_DTYPE), labels.reshape(D.shape)), want)
        assert (records[C * 40:] == PATTERN).all() and (store_l[:at_l] == 0xABCDEF01).all() and (store_l[at_l + N:] == 0xABCDEF01).all()
        d_store_r = torch.full(((C + 1) * 10 + 8,), 0x25252525, dtype=torch.int32, device="cuda")
        d_store_l = torch.full((N + 8,), 0x25252525, dtype=torch.int32, device="cuda")
        o_r = ((-d_store_r.data_ptr()) % 16) // 4 + 2
        o_l = ((-d_store_l.data_ptr()) % 16) // 4 + 1
        d_records, d_labels = d_store_r[o_r:o_r + (C + 1) * 10], d_store_l[o_l:o_l + N]
        assert d_records.data_ptr() % 16 == 8 and d_labels.data_ptr() % 16 == 4
        assert _raw(renderer, g, capacity, d_records, d_labels, on_host=0, lattice=gu.to_device(D)) == (0, "", want[0])
        cu.assert_same("device", (want[0], gu.to_host(d_records[:C * 10]), gu.to_host(d_labels).reshape(D.shape)), want)
        assert bool((d_store_r[o_r + C * 10:] == 0x25252525).all()) and bool((d_store_l[o_l + N:] == 0x25252525).all()) and bool((d_store_l[:o_l] == 0x25252525).all())


def test_arguments(renderer):
    import sdf_playground_amd as sp

    gu.setup(renderer, "fast_sphere", qu.frame("fast_sphere", 0.0, cu.W, cu.H))
    dims = (8, 8, 8)
    D = np.ones(9 ** 3, np.float32)
    records = np.zeros(4, cu.RECORD_DTYPE)
    bad = [_grid(dims, cell=0.0), _grid(dims, cell=float("nan")), _grid(dims, origin=(float("inf"), 0.0, 0.0)), _grid(dims, iso=float("nan")), _grid((0, 8, 8)),
           _grid((8, 8, 1025)), _grid((1024, 1024, 1024))]
    for lattice in (None, D):  # both entries
        assert _raw(renderer, _grid(dims), 0, None, None, lattice=lattice)[0] == 0
        for g in bad:
            assert _raw(renderer, g, 0, None, None, lattice=lattice)[:2] == (cu.INVALID, cu.BAD_GRID)
        assert _raw(renderer, None, 0, None, None, lattice=lattice)[:2] == (cu.INVALID, cu.NULL_POINTER)
        assert _raw(renderer, _grid(dims), 0, None, None, lattice=lattice, counts=False)[:2] == (cu.INVALID, cu.NULL_POINTER)
        assert _raw(renderer, _grid(dims), 0, None, None, on_host=2, lattice=lattice)[:2] == (cu.INVALID, cu.BAD_FLAG)
        assert _raw(renderer, _grid(dims), -1, None, None, lattice=lattice)[:2] == (cu.INVALID, cu.NEGATIVE)
        assert _raw(renderer, _grid(dims), 4, None, None, lattice=lattice)[:2] == (cu.INVALID, cu.NULL_ARRAY)
        # two faults at once: the text of the one checked first
        assert _raw(renderer, None, -1, None, None, on_host=2, lattice=lattice)[:2] == (cu.INVALID, cu.NULL_POINTER)
        assert _raw(renderer, bad[0], -1, None, None, on_host=2, lattice=lattice)[:2] == (cu.INVALID, cu.BAD_FLAG)
        assert _raw(renderer, bad[0], -1, None, None, lattice=lattice)[:2] == (cu.INVALID, cu.BAD_GRID)
        assert _raw(renderer, _grid(dims), -1, None, None, lattice=lattice)[:2] == (cu.INVALID, cu.NEGATIVE)
        assert _raw(renderer, _grid(dims), 0, None, None, lattice=lattice, handle=False)[0] == cu.INVALID
    assert _raw(renderer, _grid(dims), 0, None, None, lattice=False)[:2] == (cu.INVALID, cu.NULL_POINTER)
    fresh = sp.SDFRenderer(0)
    try:
        assert _raw(fresh, _grid(dims), 0, None, None)[0] == cu.NO_SCENE
        assert _raw(fresh, bad[0], 0, None, None)[0] == cu.INVALID and _raw(fresh, _grid(dims), 4, None, None)[0] == cu.INVALID  # the arguments come first
        # the caller's lattice needs no scene
        want = cu.label(*(cu.synthetic("comb", dims)[0], dims))
        assert _raw(fresh, _grid(dims), 4, records, None, lattice=cu.synthetic("comb", dims)[0])[2] == want[0]
        cu.assert_same("no scene", fresh.labelLattice(cu.synthetic("comb", dims)[0], labels=True), want)
    finally:
        fresh.close()


def test_labelling_leaves_rendering_alone(renderer):
    import torch

    key = "labyrinth"
    (scene, _t, origin, cell, dims, iso, _v), _p, _l = cu.TABLE[key]
    of, D, want = cu.oracle_case(key)
    gu.setup(renderer, scene, of)
    L, h = gu.raw(renderer)
    ms0, ms1 = (ctypes.c_double * 4)(), (ctypes.c_double * 4)()
    renderer.setProfiling(True)
    try:
        renderer.extractMesh(origin, cell, dims)
        assert L.sdfr_mesh_get_timings(h, ctypes.byref(ms0)) == 0
        with gu.rendering_untouched(renderer, cu.W, cu.H) as (img0, s0):
            cu.assert_same("scene", renderer.labelComponents(origin, cell, dims, labels=True), want)
            cu.assert_same("lattice", renderer.labelLattice(D, labels=True), want)
            assert L.sdfr_mesh_get_timings(h, ctypes.byref(ms1)) == 0 and list(ms0) == list(ms1)
    finally:
        renderer.setProfiling(False)
    # two frames in flight: the call runs on the lane of the frame submitted last, between extractions that leave device work behind
    renderer.setFramesInFlight(2)
    try:
        imgs = [torch.empty((cu.H, cu.W, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        for k in range(4):
            renderer.render(None, cu.W, cu.H, out=imgs[k % 2])
            dpos, _dn, _di = renderer.extractMesh(origin, cell, dims, device=True)
            cu.assert_same("scene", renderer.labelComponents(origin, cell, dims, labels=True), want)
            got = renderer.labelComponents(origin, cell, dims, labels=True, device=True)
            renderer.sync()
            cu.assert_same("scene (device)", (got[0],) + gu.to_host(got[1:]), want)
            assert len(dpos) > 500
            assert np.array_equal(imgs[k % 2].cpu().numpy().view(np.uint32), img0.view(np.uint32))
            assert gu.stats(renderer) == s0
    finally:
        renderer.setFramesInFlight(1)


# ---- an answer known without the oracle -----------------------------------------------------------------------------------------------
# A hollow sphere (outer radius 0.85, inner 0.55, centre off the lattice) beside a separate sphere of radius 0.3, nothing else.  `channel`
# is the width of a square channel through the shell along +y; 0: none.
HOLLOW = """struct Scene
{
	static SDF_HD void prepare(FrameU &) {}
	struct RayInv {};
	static SDF_HD RayInv ray_setup(const FrameU &, vec3, const RayFlags &) { return RayInv(); }
	static SDF_HD float dist(const FrameU &U, const RayInv &, vec3 p, vec3, bool)
	{
		const float channel = VAR_channel(min = 0, max = 1, start = 0);
		const vec3 q = p - V3(0.013f, 0.021f, 0.017f);
		float shell = fmaxf(sd_sphere(q, 0.85f), -sd_sphere(q, 0.55f));
		if (channel > 0.f) shell = fmaxf(shell, -fmaxf(fmaxf(fabsf(q.x), fabsf(q.z)) - 0.5f * channel, -q.y));
		return fminf(shell, sd_sphere(p - V3(1.613f, 0.021f, 0.017f), 0.3f));
	}
	static SDF_HD void material(const FrameU &, const SurfacePoint &, Material &) {}
	static SDF_HD bool light(const FrameU &, int i, Light &L) { return sun_light(i, L); }
	static SDF_HD float ambient() { return 0.1f; }
	static SDF_HD vec3 background(const FrameU &U, vec3 dir, uint32_t) { return sky_color(dir, U.sky_s, U.sky_c); }
};
"""


def test_a_hollow_sphere_and_a_ball(renderer):
    origin, cell, dims = (-1.0, -1.0, -1.0), 0.05, (61, 40, 40)  # clear of both
    renderer.initShaderSource("hollow_sphere", HOLLOW)
    renderer.setLimits(**gu.DEFAULT_LIMITS)
    assert renderer.setValue("channel", 0.0)
    counts, records, labels = renderer.labelComponents(origin, cell, dims, labels=True)
    assert {k: counts[k] for k in ("solids", "closed_solids", "voids", "closed_voids")} == dict(solids=2, closed_solids=2, voids=2, closed_voids=1)
    # it is the library's own distances that were labelled
    D = renderer.queryDistance(mu.lattice_points(origin, cell, dims))
    cu.assert_same("hollow", (counts, records, labels), cu.label(D, dims))
    cavity = records[(records["flags"] & (cu.INSIDE | cu.FACES)) == 0]
    assert len(cavity) == 1 and 0.9 < cavity["points"][0] * cell ** 3 / (4.0 / 3.0 * np.pi * 0.55 ** 3) < 1.1
    # a channel 3 cells wide through the shell opens the cavity
    assert renderer.setValue("channel", 3 * cell)
    counts, _records, _none = renderer.labelComponents(origin, cell, dims)
    assert {k: counts[k] for k in ("solids", "closed_solids", "voids", "closed_voids")} == dict(solids=2, closed_solids=2, voids=1, closed_voids=0)


def test_cli_prints_the_counts(capsys):
    from sdf_playground_amd import cli

    key = "fast_sphere"
    (scene, _t, origin, cell, dims, _iso, _v), pinned, _l = cu.TABLE[key]
    hi = [origin[a] + cell * dims[a] for a in range(3)]
    capsys.readouterr()
    assert cli.main(["--scene", scene, "--time", "0", "--components", "--components-box"] + ["%.9g" % v for v in tuple(origin) + tuple(hi)] + ["--components-cell", str(cell)]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["counts"]["solids"] >= 1 and out["counts"]["components"] == len(out["components"]) and "warning" in out
    assert sum(c["points"] for c in out["components"]) == (out["dims"][0] + 1) * (out["dims"][1] + 1) * (out["dims"][2] + 1)

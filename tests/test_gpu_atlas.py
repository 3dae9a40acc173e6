"""GPU tier of the texture atlas (sdfr_atlas_texels, sdfr_atlas_bake) through libsdfr.so: bit for bit against the oracle's definition
(tests/cpp/atlas_oracle.cpp with the surface and lighting oracles applied to its texels) on the two test meshes at tiles of 4, 8 and
16 texels, host and device memory, every layer mask, step shortcuts on against off; the bake against meshSurfaces / meshLighting of
atlasTexels' own output; the hand-made mesh with its malformed, out-of-range, degenerate and NaN parts; a run-time scene and a scene
change on one handle; no side effects on rendering; argument errors; and extractMesh(atlas=...) end to end."""
import ctypes

import numpy as np
import pytest

import atlas_util as au
import gpu_util as gu
import lighting_util as lu
import query_util as qu
import surface_util as su
from gpu_util import DEFAULT_LIMITS
from gpu_util import renderer  # noqa: F401

pytestmark = pytest.mark.gpu

W, H = au.W, au.H
CASES = [(4, 64), (8, 64), (16, 128)]


def _setup(r, scene, of):
    """the handle's state = the oracle frame `of`, with the four limits the tests move taken from it"""
    gu.setup(r, scene, of, limits=lu.frame_limits(of))


def _bake_to_host(baked):
    """a bake's dictionary with its device tensors as numpy"""
    return dict(zip(baked, gu.to_host(tuple(baked.values()))))


def _assert_texels(what, got, want):
    _atlas, P, N, valid = got
    assert np.array_equal(np.asarray(valid), want[2]), what + ": valid"
    qu.assert_same(what + ": positions", np.asarray(P).reshape(-1, 3), want[0].reshape(-1, 3))
    qu.assert_same(what + ": normals", np.asarray(N).reshape(-1, 3), want[1].reshape(-1, 3))


@pytest.mark.parametrize("tile,width", CASES)
@pytest.mark.parametrize("scene", sorted(au.MESHES))
def test_texels_and_bake_equal_oracle(renderer, scene, tile, width):
    import torch

    of, pos, nrm, idx, cell = au.mesh(scene)
    _setup(renderer, scene, of)
    want_texels = au.oracle_texels(pos, nrm, idx, tile, width)
    _assert_texels("%s T=%d texels (host)" % (scene, tile), renderer.atlasTexels(pos, nrm, idx, tile, width), want_texels)
    dp, dn, di = gu.to_device(pos), gu.to_device(nrm), gu.to_device(idx)
    got = renderer.atlasTexels(dp, dn, di, tile, width)
    torch.cuda.synchronize()
    _assert_texels("%s T=%d texels (device)" % (scene, tile), (got[0],) + tuple(t.cpu().numpy() for t in got[1:]), want_texels)

    want, reach = au.reference(scene, tile, width, "2cell")
    au.assert_condition(want)
    every = ("albedo", "normal", "lit")
    au.assert_bake("%s T=%d bake (host)" % (scene, tile), renderer.bakeAtlas(pos, nrm, idx, tile, width, reach, every), want)
    au.assert_bake("%s T=%d bake (device)" % (scene, tile), _bake_to_host(renderer.bakeAtlas(dp, dn, di, tile, width, reach, every)), want)
    # every layer mask, alone and in pairs: the planes asked for, and only those
    for layers in (("albedo",), ("normal",), ("lit",), ("albedo", "lit"), ("normal", "lit"), ("albedo", "normal")):
        got = _bake_to_host(renderer.bakeAtlas(dp, dn, di, tile, width, reach, layers))
        assert sorted(got) == sorted(layers + ("atlas", "valid"))
        au.assert_bake("%s T=%d layers %s" % (scene, tile, "+".join(layers)), got, want, sum(b for b, k in au.LAYER_NAMES.items() if k in layers))
    # step shortcuts: only misses end early, and a miss is zeros either way
    renderer.setStepShortcuts(True)
    au.assert_bake("%s T=%d bake, shortcuts" % (scene, tile), _bake_to_host(renderer.bakeAtlas(dp, dn, di, tile, width, reach, every)), want)
    renderer.setStepShortcuts(False)
    # another reach
    want2, reach2 = au.reference(scene, tile, width, 0.2)
    au.assert_condition(want2)
    au.assert_bake("%s T=%d bake, reach 0.2" % (scene, tile), renderer.bakeAtlas(pos, nrm, idx, tile, width, reach2, every), want2)


def test_extension_lights(renderer):
    scene = "fast_sphere"
    _of, pos, nrm, idx, _cell = au.mesh(scene)
    _setup(renderer, scene, au.frame_with(scene, 7))
    want, reach = au.reference(scene, 4, 64, 0.2, 7)
    au.assert_bake("extension lights", renderer.bakeAtlas(pos, nrm, idx, 4, 64, reach, ("albedo", "normal", "lit")), want)
    renderer.setLimits(**DEFAULT_LIMITS)


@pytest.mark.parametrize("scene", sorted(au.MESHES))
def test_bake_is_the_mesh_queries_of_its_texels(renderer, scene):
    """the composition the header promises: sdfr_atlas_bake = sdfr_mesh_surfaces / sdfr_mesh_lighting of sdfr_atlas_texels' output"""
    import torch

    of, pos, nrm, idx, cell = au.mesh(scene)
    _setup(renderer, scene, of)
    tile, width, reach = 8, 64, 2 * cell
    dp, dn, di = gu.to_device(pos), gu.to_device(nrm), gu.to_device(idx)
    _atlas, P, N, state = renderer.atlasTexels(dp, dn, di, tile, width)
    baked = _bake_to_host(renderer.bakeAtlas(dp, dn, di, tile, width, reach, ("albedo", "normal", "lit")))
    srf = renderer.meshSurfaces(P.reshape(-1, 3), N.reshape(-1, 3), reach)
    lit = renderer.meshLighting(P.reshape(-1, 3), N.reshape(-1, 3), reach)
    torch.cuda.synchronize()
    srf, lit, state = su.surfaces_array(srf.cpu().numpy()), lu.lighting_array(lit.cpu().numpy()), state.cpu().numpy().reshape(-1)
    live = state == 1
    assert live.sum() == (len(idx) // 2) * tile * tile
    valid = baked["valid"].reshape(-1)
    assert np.array_equal(valid[live], srf[live, 3].view(np.int32)) and np.array_equal(valid[~live], state[~live])
    hit = live & (srf[:, 3] == 1)
    assert hit.mean() > 0.3
    planes = {k: baked[k].view(np.uint32).reshape(-1, 4) for k in ("albedo", "normal", "lit")}
    lit_material = (srf[:, 1] & 2) != 0
    qu.assert_same("albedo", planes["albedo"][hit][:, :3], np.where(lit_material[:, None], srf[:, 4:7], srf[:, 16:19])[hit])
    qu.assert_same("alpha", planes["albedo"][hit][:, 3], srf[hit, 7])
    qu.assert_same("normal", planes["normal"][hit][:, :3], srf[hit, 28:31])
    qu.assert_same("lit", planes["lit"][hit][:, :3], lit[hit, 12:15])
    assert (planes["lit"][hit][:, 3] == au.ONE).all() and not planes["normal"][:, 3].any()
    for k in planes:
        assert not planes[k][~hit].any()


@pytest.mark.parametrize("tile,width", [(4, 8), (8, 16), (16, 16)])
def test_handmade_mesh(renderer, tile, width):
    scene = "fast_sphere"
    of = au.frame_with(scene)
    _setup(renderer, scene, of)
    pos, nrm, idx = au.handmade()
    want_texels = au.oracle_texels(pos, nrm, idx, tile, width)
    assert sorted(np.unique(want_texels[2]).tolist()) == [-1, 0, 1]
    _assert_texels("hand-made texels", renderer.atlasTexels(pos, nrm, idx, tile, width), want_texels)
    want = au.oracle_bake(scene, of, pos, nrm, idx, tile, width, 0.26)
    for device in (False, True):
        got = _bake_to_host(renderer.bakeAtlas(pos, nrm, idx, tile, width, 0.26, ("albedo", "normal", "lit"), device=device))
        au.assert_bake("hand-made bake", got, want)
        for k in ("albedo", "normal", "lit"):
            assert not got[k][got["valid"] != 1].any()
    assert (want["valid"] == 1).any()
    # no quads: the 8-row image is filled with -1 and zeros
    got = renderer.bakeAtlas(pos, nrm, idx[:0], tile, width, 0.26, ("albedo", "normal", "lit"))
    assert got["valid"].shape == (8, width) and (got["valid"] == -1).all() and not any(got[k].any() for k in ("albedo", "normal", "lit"))
    empty = renderer.atlasTexels(pos, nrm, idx[:0], tile, width)
    assert (empty[3] == -1).all() and not empty[1].any() and not empty[2].any()


def _raw_bake(L, h, atlas, v, pos, nrm, idx, reach, layers, planes, valid, on_host=1):
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
    return L.sdfr_atlas_bake(h, ctypes.byref(atlas) if atlas is not None else None, v, p(pos), p(nrm), p(idx), reach, layers, p(planes[0]), p(planes[1]), p(planes[2]),
                             p(valid), on_host)


def test_out_of_range_indices_read_no_vertex(renderer):
    """an index that is no vertex makes its tile invalid before any vertex is loaded: vertex arrays of one vertex, indices up to 2^32 - 1"""
    scene = "fast_sphere"
    _setup(renderer, scene, au.frame_with(scene))
    pos, nrm, idx = au.handmade()
    wild = idx.copy()
    wild[0, 1] = 0xffffffff
    wild[2:4] = [[1, 2, 3], [1, 3, 0x7fffffff]]
    got = renderer.bakeAtlas(gu.to_device(pos[:1]), gu.to_device(nrm[:1]), gu.to_device(wild), 8, 16, 0.26, ("albedo", "lit"))
    assert (_bake_to_host(got)["valid"] == -1).all()
    got = renderer.atlasTexels(pos[:1], nrm[:1], wild, 4, 8)
    assert (got[3] == -1).all()


def test_run_time_scene_and_scene_change():
    # built-in scene -> run-time scene (its lazily compiled query module has the bake kernel) -> the same built-in scene
    import sdf_playground_amd as sp

    _of, pos, nrm, idx, cell = au.mesh("fast_sphere")
    idx = idx[:2 * 150]
    r = sp.SDFRenderer(0)
    try:
        rounds = []
        for scene in ("fast_sphere", qu.HLSL[0], "fast_sphere"):
            of = qu.frame(scene, 0.5, W, H)
            _setup(r, scene, of)
            want = au.oracle_bake(scene, of, pos, nrm, idx, 4, 64, 0.3)
            got = r.bakeAtlas(pos, nrm, idx, 4, 64, 0.3, ("albedo", "normal", "lit"))
            au.assert_bake(scene, got, want)
            rounds.append(got)
        au.assert_bake("first and third round", rounds[0], {k: (a.view(np.uint32) if k in au.LAYER_NAMES.values() else a) for k, a in rounds[2].items()})
        assert (rounds[0]["valid"] == 1).mean() > 0.5
    finally:
        r.close()


def test_atlas_leaves_rendering_alone(renderer):
    scene = "labyrinth"
    of = qu.frame(scene, 0.4, 96, 64)
    _setup(renderer, scene, of)
    _of, pos, nrm, idx, _cell = au.mesh("fast_sphere")
    with gu.rendering_untouched(renderer, 96, 64):
        renderer.atlasTexels(pos, nrm, idx[:200], 8, 64)
        renderer.bakeAtlas(pos, nrm, idx[:200], 8, 64, 0.3, ("albedo", "normal", "lit"))
        _bake_to_host(renderer.bakeAtlas(gu.to_device(pos), gu.to_device(nrm), gu.to_device(idx[:200]), 4, 64, 0.3, ("lit",)))
        renderer.extractMesh((-5.35, -0.3, -2.55), 0.25, (5, 4, 3), atlas=dict(tile=4, layers=("albedo", "lit")))


def test_arguments(renderer):
    import sdf_playground_amd as sp

    scene = "fast_sphere"
    _setup(renderer, scene, au.frame_with(scene))
    L, h = sp.load_library(), renderer._h
    pos, nrm, idx = au.handmade()
    atlas = sp.atlasLayout(len(idx), 8, 16)
    n = atlas.width * atlas.height
    planes = [np.full((n, 4), 7, np.float32) for _ in range(3)]
    valid = np.full(n, 7, np.int32)
    tp, tn = np.full((n, 3), 7, np.float32), np.full((n, 3), 7, np.float32)
    INVALID, NO_SCENE = -1, -4
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None  # noqa: E731
    none = [None, None, None]
    # the layout
    out = sp.Atlas()
    for bad in ((7, 8, 16), (8, 5, 16), (8, 8, 12), (8, 16, 24), (-2, 8, 16), (8, 8, 16392), (2 * ((1 << 30) // 64) + 4096, 8, 16384)):
        assert L.sdfr_atlas_layout(*bad, ctypes.byref(out)) == INVALID
    assert L.sdfr_atlas_layout(8, 8, 16, None) == INVALID
    assert L.sdfr_atlas_uvs(None, p(tp)) == INVALID and L.sdfr_atlas_uvs(ctypes.byref(atlas), None) == INVALID
    # an atlas the layout did not make
    wrong = sp.Atlas.from_buffer_copy(atlas)
    wrong.height += 8
    assert _raw_bake(L, h, wrong, len(pos), pos, nrm, idx, 0.26, 7, planes, valid) == INVALID
    assert _raw_bake(L, h, None, len(pos), pos, nrm, idx, 0.26, 7, planes, valid) == INVALID
    assert L.sdfr_atlas_uvs(ctypes.byref(wrong), p(tp)) == INVALID
    # reach, layers, pointers, vertex count, on_host, the handle
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert _raw_bake(L, h, atlas, len(pos), pos, nrm, idx, bad, 7, planes, valid) == INVALID
    for bad in (0, 8, 0xffffffff):
        assert _raw_bake(L, h, atlas, len(pos), pos, nrm, idx, 0.26, bad, planes, valid) == INVALID
    for layers, missing in ((1, 0), (2, 1), (4, 2), (7, 1)):
        assert _raw_bake(L, h, atlas, len(pos), pos, nrm, idx, 0.26, layers, [a if k != missing else None for k, a in enumerate(planes)], valid) == INVALID
    assert _raw_bake(L, h, atlas, len(pos), pos, nrm, idx, 0.26, 7, planes, None) == INVALID
    assert _raw_bake(L, h, atlas, len(pos), None, nrm, idx, 0.26, 7, planes, valid) == INVALID
    assert _raw_bake(L, h, atlas, len(pos), pos, None, idx, 0.26, 7, planes, valid) == INVALID
    assert _raw_bake(L, h, atlas, len(pos), pos, nrm, None, 0.26, 7, planes, valid) == INVALID
    assert _raw_bake(L, h, atlas, -1, pos, nrm, idx, 0.26, 7, planes, valid) == INVALID
    assert _raw_bake(L, h, atlas, 2 ** 31, pos, nrm, idx, 0.26, 7, planes, valid) == INVALID
    for bad in (2, -1):
        assert _raw_bake(L, h, atlas, len(pos), pos, nrm, idx, 0.26, 7, planes, valid, bad) == INVALID
    assert _raw_bake(L, None, atlas, len(pos), pos, nrm, idx, 0.26, 7, planes, valid) == INVALID
    A = ctypes.byref(atlas)
    assert L.sdfr_atlas_texels(h, A, len(pos), p(pos), p(nrm), p(idx), None, p(tn), p(valid), 1) == INVALID
    assert L.sdfr_atlas_texels(h, A, len(pos), p(pos), p(nrm), p(idx), p(tp), None, p(valid), 1) == INVALID
    assert L.sdfr_atlas_texels(h, A, len(pos), p(pos), p(nrm), p(idx), p(tp), p(tn), None, 1) == INVALID
    assert L.sdfr_atlas_texels(h, A, len(pos), p(pos), p(nrm), p(idx), p(tp), p(tn), p(valid), 3) == INVALID
    assert L.sdfr_atlas_texels(None, A, len(pos), p(pos), p(nrm), p(idx), p(tp), p(tn), p(valid), 1) == INVALID
    fresh = sp.SDFRenderer(0)
    try:
        assert _raw_bake(L, fresh._h, atlas, len(pos), pos, nrm, idx, 0.26, 7, planes, valid) == NO_SCENE
        assert all((a == 7).all() for a in planes + [valid, tp, tn])
        # the texels, and a bake without triangles, need no scene
        assert L.sdfr_atlas_texels(fresh._h, A, len(pos), p(pos), p(nrm), p(idx), p(tp), p(tn), p(valid), 1) == 0
        assert np.array_equal(valid.reshape(atlas.height, atlas.width), au.oracle_texels(pos, nrm, idx, 8, 16)[2])
        empty = sp.atlasLayout(0, 8, 16)
        valid[:] = 7
        assert _raw_bake(L, fresh._h, empty, 0, None, None, None, 0.26, 1, [planes[0], None, None], valid) == 0
        assert (valid[:8 * 16] == -1).all() and (valid[8 * 16:] == 7).all() and not planes[0][:8 * 16].any() and (planes[0][8 * 16:] == 7).all()
    finally:
        fresh.close()
    # albedo only does not need the lit pointer, and touches no other plane
    planes[0][:] = 7
    assert _raw_bake(L, h, atlas, len(pos), pos, nrm, idx, 0.26, 1, [planes[0], None, None], valid) == 0
    assert (planes[1] == 7).all() and (planes[2] == 7).all() and set(np.unique(valid)) <= {-1, 0, 1}
    # a plane that is not aligned to 16 bytes is written by word stores
    import torch

    base = torch.full((n * 4 + 1,), 7.0, device="cuda")
    dv = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    dp, dn, di = gu.to_device(pos), gu.to_device(nrm), gu.to_device(idx)
    dev = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert L.sdfr_atlas_bake(h, A, len(pos), dev(dp), dev(dn), dev(di), 0.26, 4, None, None, dev(base[1:]), dev(dv), 0) == 0
    torch.cuda.synchronize()
    want = au.oracle_bake(scene, au.frame_with(scene), pos, nrm, idx, 8, 16, 0.26)
    assert float(base[0]) == 7.0
    au.assert_bake("unaligned lit plane", {"lit": base[1:].cpu().numpy(), "valid": dv.cpu().numpy().reshape(atlas.height, atlas.width)}, want, au.LIT)


def test_extract_mesh_with_atlas(renderer, tmp_path):
    import sdf_playground_amd as sp
    from sdf_playground_amd import obj

    scene = "fast_sphere"
    stime, origin, cell, dims = au.MESHES[scene]
    of = au.frame_with(scene)
    _setup(renderer, scene, of)
    pos, nrm, idx, baked = renderer.extractMesh(origin, cell, dims, atlas=dict(tile=8, width=64, layers=("albedo", "lit"), occlusion=True))
    assert len(idx) // 2 == 822 and sorted(baked) == ["albedo", "atlas", "lit", "openness", "uvs", "valid"]
    atlas, uvs, valid = baked["atlas"], baked["uvs"], baked["valid"]
    assert (atlas.tile, atlas.width, atlas.height, atlas.quads) == (8, 64, 824, 822) and uvs.shape == (len(idx), 3, 2)
    # the bake of the extracted mesh is the oracle's bake of it
    want = au.oracle_bake(scene, of, pos, nrm, idx, 8, 64, 2 * cell)
    au.assert_bake("extractMesh atlas", baked, want, au.ALBEDO | au.LIT)
    # every triangle's UV corners lie on the centres of its quad's corner texels
    x = uvs[..., 0].astype(np.float64) * atlas.width - 0.5
    y = uvs[..., 1].astype(np.float64) * atlas.height - 0.5
    assert np.abs(x - np.rint(x)).max() < 1e-3 and np.abs(y - np.rint(y)).max() < 1e-3
    q = np.arange(len(idx)) // 2
    x0, y0 = (q % atlas.tiles_per_row) * 8, (q // atlas.tiles_per_row) * 8
    ax, ay = np.rint(x).astype(int) - x0[:, None], np.rint(y).astype(int) - y0[:, None]
    assert np.isin(ax, (0, 7)).all() and np.isin(ay, (0, 7)).all()
    # ... and the texel there is the vertex (up to the roundings of the interpolation: three operations, see test_atlas_cpu.py)
    _a, P, _N, state = renderer.atlasTexels(pos, nrm, idx, 8, 64)
    bound = 3 * 0.5 * np.finfo(np.float32).eps * 2 * np.abs(pos).max()
    assert np.abs(P[np.rint(y).astype(int), np.rint(x).astype(int)].astype(np.float64) - pos[idx.astype(np.int64)]).max() <= bound
    tiles = state != -1
    img = obj.atlas_rgba8(baked["albedo"], valid)
    assert (img[..., 3][tiles] == 255).mean() >= 0.99 and (img[..., 3][~tiles] == 0).all() and (valid[tiles] == 1).mean() >= 0.99
    o = baked["openness"]
    assert o.shape == valid.shape and ((o >= 0) & (o <= 1)).all() and o[tiles].mean() > 0.5 and not o[~tiles].any()
    assert sp.atlasDefaultWidth(822, 8) == 232


@pytest.mark.parametrize("layer,more", [("albedo", []), ("lit", ["--mesh-colors", "--atlas-tile", "4", "--atlas-width", "128"]), ("normal", ["--mesh-lit", "--atlas-tile", "16"])])
def test_cli_writes_obj_mtl_and_png(tmp_path, layer, more, capsys):
    import struct

    import sdf_playground_amd as sp
    from sdf_playground_amd import cli

    stime, origin, cell, dims = au.MESHES["fast_sphere"]
    box = [str(v) for v in origin] + [str(o + cell * d) for o, d in zip(origin, dims)]
    mesh, png = tmp_path / "sphere.obj", tmp_path / "tex" / "sphere_atlas.png"
    png.parent.mkdir()
    assert cli.main(["--scene", "fast_sphere", "--time", str(stime), "--mesh", str(mesh), "--mesh-box"] + box + ["--mesh-cell", str(cell), "--mesh-atlas", str(png),
                     "--atlas-layer", layer] + more) == 0
    assert "atlas %s:" % layer in capsys.readouterr().out
    text = mesh.read_text().splitlines()
    faces = [line for line in text if line.startswith("f ")]
    vts = [line for line in text if line.startswith("vt ")]
    quads = len(faces) // 2
    assert quads > 500 and len(vts) == 3 * len(faces) and "mtllib sphere.mtl" in text and "usemtl atlas" in text
    corners = np.array([[[int(x) for x in c.split("/")] for c in line.split()[1:]] for line in faces])
    assert np.array_equal(corners[:, :, 0], corners[:, :, 2]) and np.array_equal(corners[:, :, 1].reshape(-1), np.arange(1, 3 * len(faces) + 1))
    assert (tmp_path / "sphere.mtl").read_text().splitlines()[-1] == "map_Kd tex/sphere_atlas.png"
    tile = int(more[more.index("--atlas-tile") + 1]) if "--atlas-tile" in more else 8
    atlas = sp.atlasLayout(2 * quads, tile, 128 if "--atlas-width" in more else None)
    data = png.read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", data[16:24]) == (atlas.width, atlas.height)
    uv = np.array([[float(x) for x in line.split()[1:]] for line in vts])
    qu.assert_same("the OBJ's texture coordinates", np.stack([uv[:, 0], 1.0 - uv[:, 1]], 1).astype(np.float32), sp.atlasUVs(atlas).reshape(-1, 2))

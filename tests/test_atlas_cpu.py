"""CPU tier of the texture atlas (sdfr_atlas_layout, sdfr_atlas_uvs, sdfr_atlas_texels, sdfr_atlas_bake): the library's host plan
(sdf_playground_amd/csrc/sdfr_atlas_plan.h) and its texel map and bake (sdfr_atlas.h) built for the CPU (tests/cpp/atlas_host.cpp)
against the oracle's definition (tests/cpp/atlas_oracle.cpp, written from include/sdfr.h, with the surface and lighting oracles applied
to its texels), bit for bit; and the OBJ / MTL / RGBA8 side in Python."""
import io
import os
import subprocess

import numpy as np
import pytest

import atlas_util as au
import query_util as qu

TILES = (4, 8, 16, 32)


# ---- layout and argument checks -----------------------------------------------------------------------------------------------------
def test_layout_equals_oracle():
    seen_ok = seen_bad = 0
    for tile in (3, 4, 5, 8, 12, 16, 32, 64, 0, -8):
        for width in (0, -8, 4, 8, 12, 16, 20, 24, 32, 36, 40, 48, 64, 96, 100, 128, 16384, 16392):
            for triangles in (-2, 0, 1, 2, 3, 4, 6, 14, 15, 16, 18, 30, 32, 34, 1644, 2166, 2167):
                want, got = au.oracle_layout(triangles, tile, width), au.host_layout(triangles, tile, width)
                assert got == want, (triangles, tile, width, got, want)
                seen_ok += want is not None
                seen_bad += want is None
    assert seen_ok > 300 and seen_bad > 300
    # every allowed tile; quads that end mid-row; no quads; the height rounding from rows * T = 4 to 8
    for tile in TILES:
        assert au.host_layout(2 * 5, tile, 64)["tile"] == tile
    assert au.host_layout(2 * 822, 4, 64) == dict(triangles=1644, quads=822, tile=4, width=64, height=208, tiles_per_row=16, rows=52)
    assert au.host_layout(2 * 822, 8, 64)["height"] == 824 and 822 % 8 != 0
    assert au.host_layout(0, 8, 64) == dict(triangles=0, quads=0, tile=8, width=64, height=8, tiles_per_row=8, rows=0)
    assert au.host_layout(2 * 3, 4, 64)["height"] == 8 and au.host_layout(2 * 3, 4, 64)["rows"] == 1
    assert au.host_layout(2 * 17, 4, 64)["height"] == 8 and au.host_layout(2 * 33, 4, 64)["height"] == 16
    # odd triangle counts, a width that is no multiple of 8 or of the tile
    assert au.host_layout(7, 8, 64) is None and au.host_layout(8, 8, 60) is None and au.host_layout(8, 16, 24) is None and au.host_layout(8, 32, 16400) is None
    # W * H past what the renderer takes as a frame: 2^30 texels
    big = 2 * ((1 << 30) // 64)
    assert au.host_layout(big, 8, 16384) == au.oracle_layout(big, 8, 16384) != None  # noqa: E711
    assert au.host_layout(big + 2 * 2048, 8, 16384) is None and au.oracle_layout(big + 2 * 2048, 8, 16384) is None


def _plan(triangles=12, tile=8, width=16, damage=0, have_atlas=1, vertex_count=12, bake=1, reach=0.2, layers=7, have=0x7f, on_host=1):
    bytes_ = np.zeros(7, np.uint64)
    blocks, needs = np.zeros(1, np.uint32), np.zeros(1, np.int32)
    err = np.zeros(64, np.uint8)
    rc = au.host_lib().ah_plan(triangles, tile, width, damage, have_atlas, vertex_count, bake, reach, layers, have, on_host, qu._p(bytes_), qu._p(blocks), qu._p(needs),
                               err.ctypes.data_as(__import__("ctypes").c_char_p))
    return rc, bytes(err).split(b"\0")[0].decode(), bytes_.tolist(), int(blocks[0]), int(needs[0])


def test_plan_checks_arguments_in_order():
    rc, err, nbytes, blocks, needs = _plan()
    # 6 quads at T = 8, W = 16: 2 tiles per row, 3 rows, H = 24: positions, normals, indices, three planes, valid
    assert (rc, err) == (0, "") and nbytes == [144, 144, 144, 16 * 24 * 16, 16 * 24 * 16, 16 * 24 * 16, 16 * 24 * 4] and blocks == 2 * 3 and needs == 1
    assert _plan(bake=0)[2:] == ([144, 144, 144, 16 * 24 * 12, 16 * 24 * 12, 16 * 24 * 4, 0], 6, 0)
    assert _plan(layers=1)[2] == [144, 144, 144, 16 * 24 * 16, 0, 0, 16 * 24 * 4]
    assert _plan(layers=1, have=0x4f)[0] == 0  # albedo only needs neither the normal nor the lit pointer
    assert _plan(layers=4, have=0x67)[0] == 0
    # no triangles: an image of 8 rows, nothing read, no scene needed
    assert _plan(triangles=0, have=0x78) == (0, "", [0, 0, 0, 16 * 8 * 16] * 1 + [16 * 8 * 16, 16 * 8 * 16, 16 * 8 * 4], 2, 0)
    # the order in which the errors win
    assert _plan(have_atlas=0, vertex_count=-1, on_host=2, reach=0.0)[:2] == (-1, "bad atlas")
    assert _plan(damage=8, vertex_count=-1)[:2] == (-1, "bad atlas")
    assert _plan(tile=5, vertex_count=-1)[:2] == (-1, "bad atlas")
    assert _plan(vertex_count=-1, on_host=2)[:2] == (-1, "bad vertex count")
    assert _plan(vertex_count=1 << 31)[:2] == (-1, "bad vertex count")
    assert _plan(on_host=2, reach=0.0)[:2] == (-1, "on_host must be 0 or 1")
    for reach in (0.0, -1.0, float("inf"), float("nan")):
        assert _plan(reach=reach, layers=0)[:2] == (-1, "reach must be finite and > 0")
    assert _plan(reach=float("nan"), bake=0)[0] == 0  # the texels take no reach
    assert _plan(layers=0, have=0)[:2] == (-1, "bad layers") and _plan(layers=8)[:2] == (-1, "bad layers")
    for missing in (0, 1, 2, 6):
        assert _plan(have=0x7f & ~(1 << missing))[:2] == (-1, "null pointer")
    for bit, plane in ((1, 3), (2, 4), (4, 5)):
        assert _plan(layers=bit, have=0x7f & ~(1 << plane))[:2] == (-1, "null pointer")
    assert _plan(bake=0, have=0x7f & ~(1 << 3))[:2] == (-1, "null pointer") and _plan(bake=0, have=0x7f & ~(1 << 4))[:2] == (-1, "null pointer")
    assert _plan(bake=0, have=0x5f)[0] == 0


# ---- UVs ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,width,quads", [(4, 64, 822), (8, 64, 822), (16, 128, 1083), (32, 96, 7), (8, 8, 3)])
def test_uvs_equal_oracle_and_sit_on_corner_texels(tile, width, quads):
    want, got = au.oracle_uvs(2 * quads, tile, width), au.host_uvs(2 * quads, tile, width)
    qu.assert_same("uvs", got.reshape(-1, 2), want.reshape(-1, 2))
    lay = au.host_layout(2 * quads, tile, width)
    # corner k of quad q is texel (x0 + cx, y0 + cy): u * W - 0.5 and v * H - 0.5 are those integers
    x = got[..., 0].astype(np.float64) * lay["width"] - 0.5
    y = got[..., 1].astype(np.float64) * lay["height"] - 0.5
    q = np.arange(2 * quads) // 2
    x0, y0 = (q % lay["tiles_per_row"]) * tile, (q // lay["tiles_per_row"]) * tile
    cx = np.where(np.arange(2 * quads)[:, None] % 2 == 0, [[0, 1, 1]], [[0, 1, 0]]) * (tile - 1)
    cy = np.where(np.arange(2 * quads)[:, None] % 2 == 0, [[0, 0, 1]], [[0, 1, 1]]) * (tile - 1)
    assert np.abs(x - (x0[:, None] + cx)).max() < 1e-3 and np.abs(y - (y0[:, None] + cy)).max() < 1e-3


# ---- the texel map ------------------------------------------------------------------------------------------------------------------
def _assert_texels(what, got, want):
    assert np.array_equal(got[2], want[2]), what + ": valid"
    qu.assert_same(what + ": positions", got[0].reshape(-1, 3), want[0].reshape(-1, 3))
    qu.assert_same(what + ": normals", got[1].reshape(-1, 3), want[1].reshape(-1, 3))


@pytest.mark.parametrize("tile", [4, 8, 16, 32])
@pytest.mark.parametrize("scene", sorted(au.MESHES))
def test_texels_equal_oracle(scene, tile):
    _of, pos, nrm, idx, _cell = au.mesh(scene)
    assert (len(pos), len(idx) // 2) == {"fast_sphere": (872, 822), "debug_materials": (1145, 1083)}[scene]
    # the mesh is quads: triangles 2q and 2q + 1 share q0 and q2
    assert np.array_equal(idx[1::2, 0], idx[0::2, 0]) and np.array_equal(idx[1::2, 1], idx[0::2, 2])
    width = 64 if tile <= 8 else 128
    want = au.oracle_texels(pos, nrm, idx, tile, width)
    _assert_texels("%s T=%d" % (scene, tile), au.host_texels(pos, nrm, idx, tile, width), want)
    P, N, valid = want
    lay = au.host_layout(len(idx), tile, width)
    assert (len(idx) // 2) % lay["tiles_per_row"] != 0  # a ragged last row of tiles
    tiles = valid != -1
    assert tiles.sum() == (len(idx) // 2) * tile * tile and (valid[tiles] == 1).all()
    assert not P[~tiles].any() and not N[~tiles].any()
    assert np.abs(np.linalg.norm(N[tiles].astype(np.float64), axis=1) - 1).max() < 1e-6
    # the corner texels are the vertices: q0 exactly (A0 + 0 + 0), the others up to the roundings of A0 + 1 * (A1 - A0) and of a sum
    # -- three operations of half an ulp each on numbers no larger than twice the largest coordinate
    bound = 3 * 0.5 * np.finfo(np.float32).eps * 2 * np.abs(pos).max()
    q = np.arange(len(idx) // 2)
    x0, y0 = (q % lay["tiles_per_row"]) * tile, (q // lay["tiles_per_row"]) * tile
    for k, (cx, cy) in enumerate(((0, 0), (tile - 1, 0), (tile - 1, tile - 1), (0, tile - 1))):
        vertex = idx[2 * q + (k == 3), (0, 1, 2, 2)[k]]
        if k == 0:
            qu.assert_same("corner 0", np.ascontiguousarray(P[y0 + cy, x0 + cx]), pos[vertex])
        assert np.abs(P[y0 + cy, x0 + cx].astype(np.float64) - pos[vertex]).max() <= bound, k


def test_diagonal_takes_the_first_formula():
    """on u == v the two formulas may round differently: the definition says u >= v takes triangle 2q's, and the library does"""
    _of, pos, nrm, idx, _cell = au.mesh("debug_materials")
    tile, width = 8, 64
    P, _N, valid = au.host_texels(pos, nrm, idx, tile, width)
    lay = au.host_layout(len(idx), tile, width)
    differ = 0
    f32 = np.float32
    for q in range(len(idx) // 2):
        A0, A1, A2, A3 = (pos[i].astype(f32) for i in (idx[2 * q][0], idx[2 * q][1], idx[2 * q][2], idx[2 * q + 1][2]))
        x0, y0 = (q % lay["tiles_per_row"]) * tile, (q // lay["tiles_per_row"]) * tile
        for a in range(tile):
            u = f32(a) / f32(tile - 1)
            first = (A0 + u * (A1 - A0)).astype(f32) + (u * (A2 - A1)).astype(f32)
            second = (A0 + u * (A3 - A0)).astype(f32) + (u * (A2 - A3)).astype(f32)
            got = P[y0 + a, x0 + a]
            assert valid[y0 + a, x0 + a] == 1 and np.array_equal(got.view(np.uint32), first.astype(f32).view(np.uint32)), (q, a)
            differ += not np.array_equal(first.view(np.uint32), second.astype(f32).view(np.uint32))
    assert differ > 0  # the pin distinguishes the two


@pytest.mark.parametrize("tile,width", [(4, 8), (8, 16), (16, 16)])
def test_handmade_mesh(tile, width):
    pos, nrm, idx = au.handmade()
    want = au.oracle_texels(pos, nrm, idx, tile, width)
    _assert_texels("hand-made T=%d" % tile, au.host_texels(pos, nrm, idx, tile, width), want)
    P, N, valid = want
    lay = au.host_layout(6, tile, width)
    tpr = lay["tiles_per_row"]
    y, x = np.mgrid[0:lay["height"], 0:lay["width"]]
    q = (y // tile) * tpr + x // tile
    a, b = x % tile, y % tile
    assert (valid[q >= 1] == -1).all()  # the malformed pair, the index that is no vertex, the tiles of no quad
    assert (valid[(q == 0) & (a > b)] == 1).all() and (valid[(q == 0) & (a <= b)] == 0).all()  # M = 0 on the diagonal, NaN below it
    assert not P[valid != 1].any() and not N[valid != 1].any()
    # fewer vertices than the indices name: every tile is invalid, and no vertex is read (the arrays are shorter than the indices say)
    none = au.host_texels(pos[:1], nrm[:1], idx, tile, width, vertex_count=1)
    _assert_texels("one vertex", none, au.oracle_texels(pos[:1], nrm[:1], idx, tile, width, vertex_count=1))
    assert (none[2] == -1).all()
    # no quads at all
    empty = au.host_texels(pos, nrm, idx[:0], tile, width)
    assert empty[2].shape == (8, width) and (empty[2] == -1).all() and not empty[0].any()


# ---- the whole bake -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,extension_lights", [("fast_sphere", 0), ("fast_sphere", 7), ("debug_materials", 0)])
def test_bake_equals_oracle(scene, extension_lights):
    _of, pos, nrm, idx, cell = au.mesh(scene)
    of = au.frame_with(scene, extension_lights)
    for reach_key, shortcuts in (("2cell", False), (0.2, True)):
        want, reach = au.reference(scene, 4, 64, reach_key, extension_lights)
        au.assert_condition(want)
        got = au.host_bake(scene, qu.host_frame(of, shortcuts), pos, nrm, idx, 4, 64, reach)
        au.assert_bake("%s, reach %g%s" % (scene, reach, ", shortcuts" if shortcuts else ""), got, want)
        assert (want["lit"][..., 3][want["valid"] == 1] == au.ONE).all() and not want["lit"][want["valid"] != 1].any()
    if scene == "debug_materials":
        # unlit materials: their albedo plane is the surface's unlit colour, which the lit plane repeats
        unlit = (want["valid"] == 1) & (want["albedo"][..., :3] == want["lit"][..., :3]).all(-1)
        assert unlit.sum() > 100
    if extension_lights:
        plain = au.reference(scene, 4, 64, 0.2, 0)[0]
        assert (want["lit"] != plain["lit"]).any() and np.array_equal(want["albedo"], plain["albedo"])
    # one layer at a time: the other planes are not touched, the values are the same
    for layers in (au.ALBEDO, au.NORMAL, au.LIT, au.ALBEDO | au.LIT):
        got = au.host_bake(scene, qu.host_frame(of), pos, nrm, idx, 4, 64, reach, layers)
        au.assert_bake("%s, layers %d" % (scene, layers), got, want, layers)
        assert all((got[k] is None) == (not layers & bit) for bit, k in au.LAYER_NAMES.items())


def test_bake_of_the_handmade_mesh():
    pos, nrm, idx = au.handmade()
    of = au.frame_with("fast_sphere")
    want = au.oracle_bake("fast_sphere", of, pos, nrm, idx, 4, 8, 0.26)
    got = au.host_bake("fast_sphere", qu.host_frame(of), pos, nrm, idx, 4, 8, 0.26)
    au.assert_bake("hand-made", got, want)
    assert sorted(np.unique(want["valid"]).tolist()) == [-1, 0, 1]
    for k in ("albedo", "normal", "lit"):
        assert not got[k][got["valid"] != 1].any()


# ---- OBJ, MTL, RGBA8 ----------------------------------------------------------------------------------------------------------------
def _parse_obj(text):
    v, vn, vt, f = [], [], [], []
    for line in text.splitlines():
        p = line.split()
        if not p or p[0].startswith("#"):
            continue
        if p[0] in ("v", "vn", "vt"):
            {"v": v, "vn": vn, "vt": vt}[p[0]].append([float(x) for x in p[1:]])
        elif p[0] == "f":
            f.append([[int(x) if x else 0 for x in c.split("/")] for c in p[1:]])
    return v, vn, vt, f


def test_write_obj_without_uvs_is_unchanged_and_with_uvs_reads_back():
    from sdf_playground_amd import obj

    pos = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0.25]], np.float32)
    nrm = np.array([[0, 0, 1]] * 4, np.float32)
    idx = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    out = io.StringIO()
    obj.write_obj(out, pos, nrm, idx, comment="two\nlines", uvs=None)
    assert out.getvalue() == ("# two\n# lines\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0.25\nvn 0 0 1\nvn 0 0 1\nvn 0 0 1\nvn 0 0 1\n"
                              "f 1//1 2//2 3//3\nf 1//1 3//3 4//4\n")
    out = io.StringIO()
    obj.write_obj(out, pos, None, idx, colors=np.array([[1, 0.5, 0]] * 4, np.float32))
    assert out.getvalue() == "v 0 0 0 1 0.5 0\nv 1 0 0 1 0.5 0\nv 1 1 0 1 0.5 0\nv 0 1 0.25 1 0.5 0\nf 1 2 3\nf 1 3 4\n"

    uvs = au.host_uvs(2, 8, 24)
    for normals in (nrm, None):
        out = io.StringIO()
        obj.write_obj(out, pos, normals, idx, uvs=uvs, material="atlas", mtllib="m.mtl")
        text = out.getvalue()
        assert text.startswith("mtllib m.mtl\n") and "\nusemtl atlas\nf " in text
        v, vn, vt, f = _parse_obj(text)
        assert np.array_equal(np.array(v, np.float32), pos) and len(vn) == (4 if normals is not None else 0)
        faces = np.array(f)
        assert np.array_equal(faces[:, :, 0] - 1, idx) and np.array_equal(faces[:, :, 1] - 1, np.arange(6).reshape(2, 3))
        if normals is not None:
            assert np.array_equal(faces[:, :, 2] - 1, idx)
        back = np.array(vt, np.float64)
        back[:, 1] = 1.0 - back[:, 1]  # OBJ's origin is bottom-left
        qu.assert_same("uvs read back", back.astype(np.float32), uvs.reshape(-1, 2))
    with pytest.raises(ValueError):
        obj.write_obj(io.StringIO(), pos, nrm, idx, uvs=uvs[:1])


def test_write_mtl_and_rgba8(tmp_path):
    from sdf_playground_amd import cli, obj

    path = tmp_path / "m.mtl"
    obj.write_mtl(str(path), "atlas.png")
    text = path.read_text()
    assert text.startswith("newmtl atlas\n") and "map_Kd atlas.png\n" in text
    plane = np.zeros((2, 3, 4), np.float32)
    plane[0, 0] = (0.25, 1.5, -0.5, 1.0)
    plane[0, 1] = (np.nan, 1.0, 0.5, 0.25)
    plane[0, 2] = (1.0, 1.0, 1.0, 1.0)
    valid = np.array([[1, 1, 0], [-1, -1, 1]], np.int32)
    img = obj.atlas_rgba8(plane, valid)
    assert img.dtype == np.uint8 and img.shape == (2, 3, 4)
    grey = [int(np.floor(c * 255 + 0.5)) for c in obj.MISSING_COLOR] + [255]
    assert img.tolist() == [[[64, 255, 0, 255], [0, 255, 128, 255], grey], [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 255]]]
    a = cli.make_parser().parse_args(["--scene", "gems", "--mesh", "m.obj", "--mesh-atlas", "a.png", "--atlas-tile", "16", "--atlas-width", "256", "--atlas-layer", "lit"])
    assert (a.mesh_atlas, a.atlas_tile, a.atlas_width, a.atlas_layer) == ("a.png", 16, 256, "lit")
    d = cli.make_parser().parse_args(["--scene", "gems", "--mesh", "m.obj", "--mesh-atlas", "a.png"])
    assert (d.atlas_tile, d.atlas_width, d.atlas_layer) == (8, None, "albedo")


def test_default_width_and_layout_in_python():
    import sdf_playground_amd as sp

    for tile in TILES:
        for quads in (0, 1, 2, 63, 64, 65, 822, 1083, 100000):
            w = sp.atlasDefaultWidth(quads, tile)
            side = int(np.ceil(np.sqrt(quads)))
            assert w % 8 == 0 and w % tile == 0 and w >= max(tile * side, 8) and w - max(8, tile) < max(tile * side, 8)
            assert au.host_layout(2 * quads, tile, w) is not None


def test_atlas_struct_matches_header(tmp_path):
    import sdf_playground_amd as sp

    fields = ("triangles", "quads", "tile", "width", "height", "tiles_per_row", "rows", "reserved")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdfr.h"\nint main(void) {\nprintf("%zu", sizeof(sdfr_atlas));\n'
                   + "".join('printf(" %%zu", offsetof(sdfr_atlas, %s));\n' % f for f in fields)
                   + 'printf(" %u %u %u\\n", SDFR_ATLAS_ALBEDO, SDFR_ATLAS_NORMAL, SDFR_ATLAS_LIT);\nreturn 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I" + os.path.join(qu.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    import ctypes

    want = [ctypes.sizeof(sp.Atlas)] + [getattr(sp.Atlas, f).offset for f in fields] + [sp.ATLAS_LAYERS[k] for k in ("albedo", "normal", "lit")]
    assert got == want == [40, 0, 8, 16, 20, 24, 28, 32, 36, 1, 2, 4]
    assert (au.ALBEDO, au.NORMAL, au.LIT) == (1, 2, 4)

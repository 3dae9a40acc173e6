"""CPU tier of the lighting queries (sdfr_query_ray_lighting, sdfr_pick_lighting, sdfr_mesh_lighting): the library's lighting
functions (sdf_playground_amd/csrc/sdfr_lighting.h) built for the CPU (tests/cpp/lighting_host.cpp) against the oracle's definition
of the records (tests/cpp/lighting_oracle.h), bit for bit -- a NaN compares as "is a NaN" --, for every scene compiled ahead of
time and the run-time scenes with an oracle twin, with step shortcuts off and on; the definition itself against the oracle's driver,
pixel for pixel, where sdfr_lighting.lit is defined to be the pixel; the records' own promises; and the layouts against the Python
mirrors."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import lighting_util as lu
import mesh_util as mu
import query_util as qu
import surface_util as su
from lighting_util import MESHES, PIXEL_FRAMES, pixel_classes, pixel_frame

N_RAYS = 2000
W, H = 64, 48
FW, FH = 61, 45  # a whole frame with ragged 8 x 8 tiles on both edges


def _same(what, got, want, shortcuts):
    """with step shortcuts a miss may end early (a smaller t, distance and iteration count in its hit record): every hit's record and
    every lighting record and sample is the same"""
    if shortcuts:
        hit = want[0][:, 10] == 1
        assert np.array_equal(got[0][:, 10], want[0][:, 10])
        qu.assert_same(what + ": hits that hit", got[0][hit], want[0][hit])
        got, want = (None,) + got[1:], (None,) + want[1:]
    lu.assert_same(what, got, want)


def _compare(scene, of, seed, n_rays=N_RAYS, frame=True):
    """host against oracle, shortcuts off and on; -> the oracle's (rays, picks)"""
    o, dirs = qu.ray_samples(of, seed + 7, n_rays)
    ref = lu.oracle_rays(scene, of, o, dirs)
    px = qu.pick_grid(W, H)
    pick_ref = lu.oracle_pick(scene, of, px)
    short_ref = lu.oracle_rays(scene, of, o[:500], dirs[:500], 3.0)
    if frame:
        of.width, of.height = FW, FH
        fpx = su.frame_pixels(FW, FH)
        frame_ref = lu.oracle_pick(scene, of, fpx)
        of.width, of.height = W, H
    for shortcuts in (False, True):
        U = qu.host_frame(of, shortcuts)
        tag = "%s%s" % (scene, ", shortcuts" if shortcuts else "")
        _same(tag + " rays", lu.host_rays(scene, U, o, dirs), ref, shortcuts)
        _same(tag + " rays, max_distance 3", lu.host_rays(scene, U, o[:500], dirs[:500], 3.0), short_ref, shortcuts)
        _same(tag + " pick", lu.host_pick(scene, U, W, H, px), pick_ref, shortcuts)
        if frame:
            _same(tag + " frame", lu.host_pick(scene, U, FW, FH, fpx), frame_ref, shortcuts)
    # the same lighting whether the samples are asked for or not
    U = qu.host_frame(of)
    lu.assert_same("%s rays without samples" % scene, lu.host_rays(scene, U, o[:300], dirs[:300], lights=False), (ref[0][:300], ref[1][:300], None))
    # the hit records are the ray query's
    qu.assert_same("%s rays: hits against the ray query's" % scene, ref[0], qu.oracle_rays(scene, of, o, dirs))
    qu.assert_same("%s pick: hits against the pick's" % scene, pick_ref[0], qu.oracle_pick(scene, of, px))
    assert (pick_ref[1][W * H:, 0] == 0xffffffff).all() and not pick_ref[1][W * H:, 1:].any()  # pick_grid's pixels outside the frame
    lu.well_formed(*ref, of.light_count)
    lu.well_formed(*pick_ref, of.light_count)
    return ref, pick_ref


@pytest.mark.parametrize("stime", qu.TIMES)
@pytest.mark.parametrize("scene", qu.BUILTIN + qu.HLSL)
def test_lighting_equals_oracle(scene, stime):
    of = qu.frame(scene, stime, W, H)
    (h, g, s), (ph, pg, ps) = _compare(scene, of, seed=zlib.crc32(("%s %g" % (scene, stime)).encode()) & 0xffff)
    # an unlit hit is the surface query's colour and looks at no light
    srf = su.oracle_pick(scene, of, qu.pick_grid(W, H))[1]
    unlit = (srf[:, 3] == 1) & ((srf[:, 1] & 2) == 0)
    qu.assert_same("%s: own of unlit hits" % scene, pg[unlit][:, 4:7], srf[unlit][:, 16:19])
    assert not pg[unlit][:, [1, 2, 3, 7, 8, 9, 10, 11]].any() and not ps[unlit].any()
    # the samples reach lit surfaces: the comparison is not one of misses alone
    assert (g[:, 1] != 0).any() or (pg[:, 1] != 0).any() or scene in ("basic_clouds", "debug_materials", "normal_test")


@pytest.mark.parametrize("scene", sorted(qu.MOVED_VARS))
def test_lighting_with_moved_variables(scene):
    _compare(scene, qu.frame(scene, 0.5, W, H, qu.MOVED_VARS[scene]), seed=11, frame=False)


@pytest.mark.parametrize("scene", ["labyrinth", "dialect_tour"])
def test_debug_plane_and_hidden_objects(scene):
    _compare(scene, qu.frame(scene, 0.75, W, H, {"debug_nx": 0.3, "debug_ny": 1.0, "debug_y": 0.4}), seed=21, frame=False)
    _compare(scene, qu.frame(scene, 0.75, W, H, {"show_objects": 0.0, "debug_ny": 1.0}), seed=22, frame=False)


@pytest.mark.parametrize("scene", ["labyrinth", "gems", "light_shadows", "noise_lod"])
@pytest.mark.parametrize("light_count", [0, 1, 8])
def test_light_count(scene, light_count):
    of = qu.frame(scene, 0.5, W, H)
    of.light_count = light_count
    _rays, (ph, pg, ps) = _compare(scene, of, seed=31, n_rays=600, frame=False)
    hit = pg[:, 0] == 1
    assert hit.any() and not (pg[:, 1] >> np.uint32(light_count)).any()
    if light_count == 0:
        assert not pg[:, [1, 2, 3, 8, 9, 10, 11]].any()


@pytest.mark.parametrize("scene", ["gems", "labyrinth", "basic_transparency"])
def test_extension_lights(scene):
    of = qu.frame(scene, 0.5, W, H)
    of.extension_lights = 7
    _rays, (ph, pg, ps) = _compare(scene, of, seed=41, n_rays=600, frame=False)
    lit = (pg[:, 0] == 1) & (pg[:, 7] != 0)
    assert lit.any() and ((pg[lit, 1] & 0xfe) == 0xfe).all()  # slots 1 .. 7 are the extension's
    assert (ps[lit][:, 1:, 1] == 0).all()  # ... point lights


def test_no_chain_starts_at_max_cost_2():
    of = qu.frame("light_shadows", 0.5, W, H)
    of.max_cost_default = 2
    _rays, (ph, pg, ps) = _compare("light_shadows", of, seed=51, n_rays=600, frame=False)
    assert (pg[:, 1] != 0).any() and not pg[:, [2, 3, 8, 9, 10, 11]].any()
    state = ps[:, :, 0]
    assert (state[state != 0] == lu.NO_CHAIN).all() and ps[state == lu.NO_CHAIN][:, 12:15].any()


def test_marble_reflection_extension():
    of = qu.frame("labyrinth", 0.25, W, H)
    plain = lu.oracle_pick("labyrinth", of, qu.pick_grid(W, H))
    of.extension_marble_reflection = 0.25
    _rays, pick = _compare("labyrinth", of, seed=61, n_rays=600, frame=False)
    # a reflection colour spawns a ray of its own: the lighting of the hit is what it was
    lu.assert_same("lighting with and without the marble extension", pick, plain)


@pytest.mark.parametrize("scene", sorted(MESHES))
def test_mesh_vertices(scene):
    stime, origin, cell, dims = MESHES[scene]
    of = qu.frame(scene, stime, W, H)
    D = qu.oracle_points(scene, of, mu.lattice_points(origin, cell, dims), normals=False)[0]
    pos, _idx = mu.host_extract(D, origin, cell, dims, 0.0)
    assert len(pos) > 500
    _d, nrm = qu.oracle_points(scene, of, pos)
    for reach, shortcuts in ((2 * cell, False), (0.2, True)):
        ref = lu.oracle_mesh(scene, of, pos, nrm, reach)
        _same("%s mesh, reach %g" % (scene, reach), lu.host_mesh(scene, qu.host_frame(of, shortcuts), pos, nrm, reach), ref, shortcuts)
        lu.well_formed(*ref, of.light_count)
    assert (ref[1][:, 0] == 1).mean() > 0.5


# ---- the pin against the driver itself: where `lit` is defined to be the pixel, it is orc::ps_main's rgb, bit for bit -----------------
# (the frames and their classes of pixels: lighting_util.PIXEL_FRAMES, shared with the GPU tier)
@pytest.mark.parametrize("key", sorted(PIXEL_FRAMES))
def test_lit_is_the_driver_s_pixel(key):
    scene, of = pixel_frame(key)
    px = su.frame_pixels(W, H)
    _h, g, s = lu.oracle_pick(scene, of, px)
    srf = su.oracle_pick(scene, of, px)[1]
    img = qu.po.render(scene, of)[0].reshape(-1, 4)
    ok, single, lit_hits = pixel_classes(scene, of, g, srf)
    assert lit_hits.sum() > 200 and ok.sum() >= 0.5 * lit_hits.sum(), (int(ok.sum()), int(lit_hits.sum()))
    qu.assert_same("%s: lit against the driver's pixels" % key, lu.f32(g[:, 12:15])[ok], np.ascontiguousarray(img[ok, :3]))
    qu.assert_same("%s: lit against the driver's pixels, single chains" % key, lu.f32(g[:, 12:15])[single], np.ascontiguousarray(img[single, :3]))
    traced, visible, segments = g[:, 2], g[:, 3], g[:, 11].astype(np.int64)
    if key == "basic_transparency":
        # chains of two and more segments exist, some escape tinted, and the driver's pixel confirms what they delivered
        long_chain = s[:, :, 2] >= 2
        assert long_chain.any() and (s[long_chain][:, 0] == lu.ESCAPED).any() and (s[long_chain][:, 0] == lu.BLOCKED).any()
        assert (single & (segments >= 2) & (visible != 0)).any()
    else:
        assert (ok & (visible != traced)).any() and (ok & (visible != 0)).any()  # shadowed and lit pixels among them
        assert (ok & (lu.popcount(g[:, 1]) >= 2)).any()  # several used lights


# ---- layouts ------------------------------------------------------------------------------------------------------------------------
def test_lighting_dtypes_match_header(tmp_path):
    import sdf_playground_amd as sp

    fields = ("valid", "used_mask", "traced_mask", "visible_mask", "own", "ambient_factor", "direct", "segments", "lit", "reserved")
    sfields = ("state", "flags", "segments", "reserved0", "dir", "distance", "color", "light_dot", "influenced", "specular_factor", "delivered", "reserved1")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdfr.h"\nint main(void) {\nprintf("%zu", sizeof(sdfr_lighting));\n'
                   + "".join('printf(" %%zu", offsetof(sdfr_lighting, %s));\n' % f for f in fields)
                   + 'printf(" %zu", sizeof(sdfr_light_sample));\n'
                   + "".join('printf(" %%zu", offsetof(sdfr_light_sample, %s));\n' % f for f in sfields)
                   + 'printf(" %u %d %d %d %d\\n", SDFR_LIGHT_DIRECTIONAL, SDFR_LIGHT_UNUSED, SDFR_LIGHT_NO_CHAIN, SDFR_LIGHT_BLOCKED, SDFR_LIGHT_ESCAPED);\nreturn 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I" + os.path.join(qu.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    dt, st = sp.LIGHTING_DTYPE, sp.LIGHT_SAMPLE_DTYPE
    want = ([dt.itemsize] + [dt.fields[k][1] for k in fields] + [st.itemsize] + [st.fields[k][1] for k in sfields]
            + [sp.LIGHT_DIRECTIONAL, sp.LIGHT_UNUSED, sp.LIGHT_NO_CHAIN, sp.LIGHT_BLOCKED, sp.LIGHT_ESCAPED])
    assert got == want == [64, 0, 4, 8, 12, 16, 28, 32, 44, 48, 60, 80, 0, 4, 8, 12, 16, 28, 32, 44, 48, 60, 64, 76, 1, 0, 1, 2, 3]
    assert lu.LIGHTING_WORDS * 4 == dt.itemsize and lu.SAMPLE_WORDS * 4 == st.itemsize


def test_obj_colours_and_gbuffer_arrays():
    import sdf_playground_amd as sp
    from sdf_playground_amd import cli, obj

    g = np.zeros(4, sp.LIGHTING_DTYPE)
    g["valid"] = [1, 1, 0, -1]
    g["lit"][0] = (0.25, 1.5, -0.5)
    g["lit"][1] = (0.125, np.nan, 0.75)
    g["own"][0] = (0.0625, 0.5, 0.0)
    g["visible_mask"] = [3, 0, 0, 0]
    rgb, missing = obj.lighting_colors(g)
    assert missing == 2 and rgb.dtype == np.float32
    assert rgb.tolist() == [[0.25, 1.0, 0.0], [0.125, 0.0, 0.75], list(obj.MISSING_COLOR), list(obj.MISSING_COLOR)]
    a = cli.gbuffer_lighting_arrays(g, 2, 2)
    assert sorted(a) == ["direct", "lit", "own", "traced_mask", "used_mask", "visible_mask"]
    assert a["lit"].shape == (2, 2, 3) and a["own"][0, 0].tolist() == [0.0625, 0.5, 0.0] and a["visible_mask"].tolist() == [[3, 0], [0, 0]]
    args = cli.make_parser().parse_args(["--scene", "gems", "--mesh", "m.obj", "--mesh-lit", "--gbuffer", "g.npz", "--gbuffer-lighting"])
    assert args.mesh_lit and args.gbuffer_lighting

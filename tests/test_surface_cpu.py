"""CPU tier of the surface queries (sdfr_query_ray_surfaces, sdfr_pick_surfaces, sdfr_mesh_surfaces): the library's surface
functions (sdf_playground_amd/csrc/sdfr_surface.h) built for the CPU (tests/cpp/surface_host.cpp) against the oracle's definition
of the record (tests/cpp/surface_oracle.h), bit for bit -- a NaN compares as "is a NaN" --, for every scene compiled ahead of time
and the run-time scenes with an oracle twin; and sdfr_surface's layout against the Python mirror SURFACE_DTYPE."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import query_util as qu
import surface_util as su

N_RAYS = 2000
W, H = 64, 48
FW, FH = 61, 45  # a whole frame with ragged 8 x 8 tiles on both edges


def _compare(scene, of, seed, shortcuts=False):
    U = qu.host_frame(of, shortcuts)
    o, dirs = qu.ray_samples(of, seed + 7, N_RAYS)
    ref = su.oracle_rays(scene, of, o, dirs)
    su.assert_same("%s rays" % scene, su.host_rays(scene, U, o, dirs), ref)
    # the hit records are the ray query's
    qu.assert_same("%s rays: hits against the ray query's" % scene, ref[0], qu.oracle_rays(scene, of, o, dirs))
    su.assert_same("%s rays, max_distance 3" % scene, su.host_rays(scene, U, o[:500], dirs[:500], 3.0), su.oracle_rays(scene, of, o[:500], dirs[:500], 3.0))
    px = qu.pick_grid(W, H)
    pick_ref = su.oracle_pick(scene, of, px)
    su.assert_same("%s pick" % scene, su.host_pick(scene, U, W, H, px), pick_ref)
    assert (pick_ref[1][W * H:, 3] == 0xffffffff).all()  # pick_grid's pixels outside the frame
    # a whole frame of another size
    of.width, of.height = FW, FH
    fpx = su.frame_pixels(FW, FH)
    su.assert_same("%s frame" % scene, su.host_pick(scene, U, FW, FH, fpx), su.oracle_pick(scene, of, fpx))
    of.width, of.height = W, H
    return ref, pick_ref


def _well_formed(hits, surfaces):
    """what the record promises whatever the scene: valid = hit, the hit's material id, zeros on a miss, zero padding"""
    assert np.array_equal(surfaces[:, 3], hits[:, 10])
    assert np.array_equal(surfaces[:, 0], hits[:, 9])
    miss = hits[:, 10] != 1
    others = [k for k in range(32) if k != 3]
    assert not surfaces[miss][:, others].any()
    assert not surfaces[:, [19, 23, 27, 31]].any()
    assert (surfaces[:, 1] <= 3).all()


@pytest.mark.parametrize("stime", qu.TIMES)
@pytest.mark.parametrize("scene", qu.BUILTIN + qu.HLSL)
def test_surfaces_equal_oracle(scene, stime):
    of = qu.frame(scene, stime, W, H)
    (h, s), (ph, ps) = _compare(scene, of, seed=zlib.crc32(("%s %g" % (scene, stime)).encode()) & 0xffff)
    _well_formed(h, s)
    _well_formed(ph, ps)
    # the samples reach surfaces: the comparison is not one of misses alone
    assert (s[:, 3] == 1).sum() > 0 or scene in ("basic_clouds",)


@pytest.mark.parametrize("scene", sorted(qu.MOVED_VARS))
def test_surfaces_with_moved_variables(scene):
    of = qu.frame(scene, 0.5, W, H, qu.MOVED_VARS[scene])
    _compare(scene, of, seed=11)


@pytest.mark.parametrize("scene", ["labyrinth", "lense", "normal_test", "dialect_tour"])
def test_debug_plane_and_hidden_objects(scene):
    of = qu.frame(scene, 0.75, W, H, {"debug_nx": 0.3, "debug_ny": 1.0, "debug_y": 0.4})
    _rays, (ph, ps) = _compare(scene, of, seed=21)
    # the plane is in the picture: its material is unlit and its colour is there
    plane = ps[:, 0] == 5  # MATERIAL_DISTANCE_PLANE (sdf_materials.hlsl)
    assert plane.any() and (ps[plane, 1] & 2 == 0).all() and ps[plane][:, 16:19].any()
    of = qu.frame(scene, 0.75, W, H, {"show_objects": 0.0, "debug_ny": 1.0})
    _compare(scene, of, seed=22)


def test_marble_reflection_extension():
    of = qu.frame("labyrinth", 0.25, W, H)
    of.extension_marble_reflection = 0.25
    _rays, (ph, ps) = _compare("labyrinth", of, seed=31)
    quarter = np.float32(0.25).view(np.uint32)
    marble = (ps[:, 3] == 1) & ((ps[:, 0] == 21) | (ps[:, 0] == 22))  # MATERIAL_MARBLE_DARK, MATERIAL_MARBLE_LIGHT
    assert marble.any() and (ps[marble][:, 20:23] == quarter).all()
    assert not ps[~marble][:, 20:23].any()


@pytest.mark.parametrize("scene", ["fast_sphere", "debug_materials", "labyrinth", "noise_lod"])
def test_mesh_vertices(scene):
    # vertex-like points: the oracle's ray hits moved a fraction of a cell off the surface, with the point query's normals there
    of = qu.frame(scene, 0.5, W, H)
    U = qu.host_frame(of)
    o, dirs = qu.ray_samples(of, 41, N_RAYS)
    hits = qu.oracle_rays(scene, of, o, dirs)
    pos = hits[:, 2:5].view(np.float32)[(hits[:, 10] == 1)]
    pos = pos[np.isfinite(pos).all(1)]
    assert len(pos) > 100
    cell = 0.125
    rng = np.random.default_rng(42)
    pts = (pos + rng.uniform(-0.4, 0.4, pos.shape) * cell).astype(np.float32)
    _d, nrm = qu.oracle_points(scene, of, pts)
    for reach in (2 * cell, 0.3):
        ref = su.oracle_mesh(scene, of, pts, nrm, reach)
        su.assert_same("%s mesh, reach %g" % (scene, reach), su.host_mesh(scene, U, pts, nrm, reach), ref)
        _well_formed(*ref)
    assert (ref[1][:, 3] == 1).mean() > 0.5


def test_surface_dtype_matches_header(tmp_path):
    import sdf_playground_amd as sp

    fields = ("material_id", "flags", "max_cost", "valid", "albedo", "alpha", "specular", "specular_power", "emissive", "optical_index", "unlit",
              "reserved0", "reflection", "reserved1", "refraction", "reserved2", "shading_normal", "reserved3")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdfr.h"\nint main(void) {\nprintf("%zu", sizeof(sdfr_surface));\n'
                   + "".join('printf(" %%zu", offsetof(sdfr_surface, %s));\n' % f for f in fields)
                   + 'printf(" %u %u\\n", SDFR_SURFACE_USE_HDR, SDFR_SURFACE_LIT);\nreturn 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I" + os.path.join(qu.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    dt = sp.SURFACE_DTYPE
    want = [dt.itemsize] + [dt.fields[k][1] for k in fields] + [sp.SURFACE_USE_HDR, sp.SURFACE_LIT]
    assert got == want == [128, 0, 4, 8, 12, 16, 28, 32, 44, 48, 60, 64, 76, 80, 92, 96, 108, 112, 124, 1, 2]


def test_obj_colours_and_gbuffer_arrays():
    import io

    import sdf_playground_amd as sp
    from sdf_playground_amd import cli, obj

    srf = np.zeros(4, sp.SURFACE_DTYPE)
    srf["valid"] = [1, 1, 0, -1]
    srf["flags"] = [sp.SURFACE_LIT | sp.SURFACE_USE_HDR, 0, 0, 0]
    srf["albedo"][0] = (0.25, 1.5, -0.5)
    srf["unlit"][0] = (9, 9, 9)
    srf["unlit"][1] = (0.125, np.nan, 0.75)
    rgb, missing = obj.surface_colors(srf)
    assert missing == 2 and rgb.dtype == np.float32
    assert rgb.tolist() == [[0.25, 1.0, 0.0], [0.125, 0.0, 0.75], list(obj.MISSING_COLOR), list(obj.MISSING_COLOR)]
    pos = np.arange(12, dtype=np.float32).reshape(4, 3)
    out = io.StringIO()
    obj.write_obj(out, pos, None, np.array([[0, 1, 2]], np.uint32), colors=rgb)
    lines = out.getvalue().splitlines()
    assert lines[0] == "v 0 1 2 0.25 1 0" and lines[3] == "v 9 10 11 0.5 0.5 0.5" and lines[4] == "f 1 2 3"
    with pytest.raises(ValueError):
        obj.write_obj(io.StringIO(), pos, None, [], colors=rgb[:3])
    plain = io.StringIO()
    obj.write_obj(plain, pos, None, [])  # without colours: the lines as before
    assert plain.getvalue().splitlines()[0] == "v 0 1 2"
    hits = np.zeros(4, sp.HIT_DTYPE)
    hits["t"] = [2.0, 3.0, 50.0, 0.0]
    srf["shading_normal"][1] = (0, 1, 0)
    g = cli.gbuffer_arrays(hits, srf, 2, 2)
    assert g["depth"].tolist() == [[2.0, 3.0], [np.inf, np.inf]] and g["valid"].tolist() == [[1, 1], [0, -1]]
    assert g["albedo"][0, 0].tolist() == [0.25, 1.5, -0.5] and g["normal"][0, 1].tolist() == [0, 1, 0] and g["material_id"].shape == (2, 2)

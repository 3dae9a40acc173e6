"""CPU tier of the scene queries (sdfr_query_distance, sdfr_query_rays, sdfr_pick): the library's query functions
(sdf_playground_amd/csrc/sdfr_query.h) built for the CPU (tests/cpp/query_host.cpp) against the oracle's definitions of the three
queries (tests/cpp/query_oracle.h), bit for bit, for every scene compiled ahead of time and the run-time scenes with an oracle
twin; and sdfr_hit's layout against the Python mirror HIT_DTYPE."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import query_util as qu

N_POINTS = 20000
N_RAYS = 2000
W, H = 64, 48


def _compare(scene, of, seed, shortcuts=False):
    U = qu.host_frame(of, shortcuts)
    pts = qu.point_samples(scene, of, seed, N_POINTS)
    d_ref, n_ref = qu.oracle_points(scene, of, pts)
    d, n = qu.host_points(scene, U, pts)
    qu.assert_same("%s distance" % scene, d, d_ref)
    qu.assert_same("%s normal" % scene, n, n_ref)
    o, dirs = qu.ray_samples(of, seed + 7, N_RAYS)
    h_ref = qu.oracle_rays(scene, of, o, dirs)
    qu.assert_same("%s rays" % scene, qu.host_rays(scene, U, o, dirs), h_ref)
    # a shorter reach than the range
    qu.assert_same("%s rays, max_distance 3" % scene, qu.host_rays(scene, U, o[:500], dirs[:500], 3.0), qu.oracle_rays(scene, of, o[:500], dirs[:500], 3.0))
    px = qu.pick_grid(W, H)
    p_ref = qu.oracle_pick(scene, of, px)
    qu.assert_same("%s pick" % scene, qu.host_pick(scene, U, W, H, px), p_ref)
    return h_ref


@pytest.mark.parametrize("stime", qu.TIMES)
@pytest.mark.parametrize("scene", qu.BUILTIN + qu.HLSL)
def test_queries_equal_oracle(scene, stime):
    of = qu.frame(scene, stime, W, H)
    h_ref = _compare(scene, of, seed=zlib.crc32(("%s %g" % (scene, stime)).encode()) & 0xffff)
    # the samples reach surfaces: the comparison is not one of misses alone
    assert (h_ref[:, 10] == 1).sum() > 0 or scene in ("basic_clouds",)


@pytest.mark.parametrize("scene", sorted(qu.MOVED_VARS))
def test_queries_with_moved_variables(scene):
    of = qu.frame(scene, 0.5, W, H, qu.MOVED_VARS[scene])
    _compare(scene, of, seed=11)


@pytest.mark.parametrize("scene", ["labyrinth", "lense", "normal_test", "dialect_tour"])
def test_debug_plane_hidden_objects_and_epsilons(scene):
    # the debug plane on (map_geometry's min with it, map_material's distance-plane id), objects hidden, other epsilons
    of = qu.frame(scene, 0.75, W, H, {"debug_nx": 0.3, "debug_ny": 1.0, "debug_y": 0.4})
    _compare(scene, of, seed=21)
    of = qu.frame(scene, 0.75, W, H, {"show_objects": 0.0, "debug_ny": 1.0})
    _compare(scene, of, seed=22)
    of = qu.frame(scene, 0.75, W, H)
    of.dist_eps, of.grad_eps = 0.002, 0.0007
    _compare(scene, of, seed=23)


@pytest.mark.parametrize("scene", ["labyrinth", "lense", "cube_sea", "gems"])
def test_step_shortcuts_keep_hits(scene):
    of = qu.frame(scene, 0.25, W, H)
    o, dirs = qu.ray_samples(of, 5, N_RAYS)
    exact = qu.host_rays(scene, qu.host_frame(of, False), o, dirs)
    short = qu.host_rays(scene, qu.host_frame(of, True), o, dirs)
    hit = exact[:, 10] == 1
    assert np.array_equal(short[:, 10], exact[:, 10])
    assert np.array_equal(short[hit], exact[hit])
    assert (short[~hit, 8] <= exact[~hit, 8]).all()


def test_hit_dtype_matches_header(tmp_path):
    import sdf_playground_amd as sp

    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdfr.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(sdfr_hit), offsetof(sdfr_hit, t), offsetof(sdfr_hit, distance),'
                   ' offsetof(sdfr_hit, pos), offsetof(sdfr_hit, normal), offsetof(sdfr_hit, iterations), offsetof(sdfr_hit, material_id),'
                   ' offsetof(sdfr_hit, hit), offsetof(sdfr_hit, reserved));\nreturn 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I" + os.path.join(qu.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    dt = sp.HIT_DTYPE
    want = [dt.itemsize] + [dt.fields[k][1] for k in ("t", "distance", "pos", "normal", "iterations", "material_id", "hit", "reserved")]
    assert got == want == [48, 0, 4, 8, 20, 32, 36, 40, 44]

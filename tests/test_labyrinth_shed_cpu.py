"""CPU tier: the labyrinth after its pixel kernel shed work that a frame or a result already fixes (SceneLabyrinth, sdfr_scenes.h;
ShadowHitsNeedMaterial, FrameSunDir, sdfr_scene_traits.h).  The sun's direction as prepare() stores it against the light loop's own
expression; then the whole pipeline, the host build of the product's headers (tests/hostsim: render_pixel with the unshaded shadow hits,
the stored sun and the walls' sums), against the oracle -- pixels and per-pixel counters bit for bit, step shortcuts on and off -- from
the sweep eyes of bench.py and from eyes near a vase and the torch, in corridors below the wall tops, inside a wall, below the floor,
in far cells, and with a zero of either sign in each component (tests/labyrinth_shed_cameras.py)."""
import ctypes
import os

import numpy as np
import pytest

import cppbuild
import labyrinth_shed_cameras as cams

SRC = os.path.join(cppbuild.HERE, "cpp", "labyrinth_shed_host.cpp")
F32 = np.float32
W, H = 40, 24


@pytest.fixture(scope="module")
def shed_lib():
    return ctypes.CDLL(cppbuild.csrc_lib("shed", SRC))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


ALL_EYES = [(c[0], c[2]) for c in cams.cameras()]


@pytest.mark.parametrize("dist_eps", [1e-4, 1e-3, 3e-5, 0.0])
def test_stored_sun_direction_is_the_light_loop_s(shed_lib, dist_eps):
    stored, formed = np.empty(3, F32), np.empty(3, F32)
    shed_lib.sun_dirs(ctypes.c_float(dist_eps), _ptr(stored), _ptr(formed))
    assert np.array_equal(stored.view(np.uint32), formed.view(np.uint32))
    assert abs(float(np.linalg.norm(stored.astype(np.float64))) - 1.0) < 1e-3 and stored[2] > 0 > stored[0]


@pytest.fixture(scope="module")
def oracle_frames(oracle):
    """the oracle's render of every camera, made once: {name: (frame, image, stats)}"""
    out = {}
    for cam in cams.cameras():
        f, _basis = cams.oracle_frame(oracle, cam, W, H)
        ref, rst, _ = oracle.render("labyrinth", f, stats=True)
        out[cam[0]] = (f, ref, rst)
    return out


@pytest.mark.parametrize("name", [n for n, _e in ALL_EYES])
def test_host_pipeline_matches_the_oracle(oracle_frames, name):
    """render_pixel compiled for the CPU: pixels and per-pixel counters against the oracle, every step marched and with step shortcuts"""
    import hostsim

    f, ref, rst = oracle_frames[name]
    hf = hostsim.frame_from_oracle(f)
    for shortcuts in (0, 1):
        hf.step_shortcuts = shortcuts
        img, st = hostsim.render("labyrinth", hf)
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), (name, shortcuts, int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum()))
        assert np.array_equal(st[..., 0], rst[..., 0]) and np.array_equal(st[..., 2], rst[..., 2]), (name, shortcuts)
        if shortcuts:
            assert (st[..., 1] <= rst[..., 1]).all(), name
        else:
            assert np.array_equal(st[..., 1], rst[..., 1]), name


def test_the_frames_show_what_the_changes_touch(oracle_frames):
    """no case passes by seeing nothing: over the cameras there are hits and misses, shadow rays that hit (rays that end in a hit beyond
    the first: hits > 1 in a pixel) and pixels that are a hit at the eye itself (inside a wall: one evaluation)"""
    hits = sum(int(rst[..., 2].sum()) for _f, _ref, rst in oracle_frames.values())
    rays = sum(int(rst[..., 0].sum()) for _f, _ref, rst in oracle_frames.values())
    assert 0 < hits < rays
    assert sum(int((rst[..., 2] >= 2).sum()) for _f, _ref, rst in oracle_frames.values()) > 1000
    _f, _ref, rst = oracle_frames["inside_wall1"]
    assert (rst[..., 1][rst[..., 0] >= 1] >= 1).all() and int((rst[..., 2] >= 1).sum()) == W * H

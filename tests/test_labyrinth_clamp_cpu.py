"""CPU tier: the labyrinth's walls with sums for clamps (SceneLabyrinth::sd_box_pair_min_adds, o' = q + |q| for o = max(q, 0), sdfr_scenes.h)
give the very bits of the form with max1 -- SceneLabyrinth::sd_box_pair_min, which stays for arbitrary boxes and which
tests/cpp/labyrinth_shed_host.cpp also holds written out as it stood for the walls -- and of the two sd_box calls.

The host build checks the algebra with the host's sqrtf; on the device sqrt1 is the correctly rounded root on the domain both forms
rely on (sdfr_math.h), and the GPU tier renders the labyrinth against the oracle."""
import ctypes
import os

import numpy as np
import pytest

import cppbuild

SRC = os.path.join(cppbuild.HERE, "cpp", "labyrinth_shed_host.cpp")
F32 = np.float32


@pytest.fixture(scope="module")
def shed_lib():
    lib = ctypes.CDLL(cppbuild.csrc_lib("shed", SRC))
    lib.clamp_check.restype = ctypes.c_int64
    lib.clamp_check.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p]
    lib.clamp_grid.restype = ctypes.c_int64
    return lib


def _check(lib, mode, seed, n):
    first = np.zeros(6, F32)
    bad = lib.clamp_check(mode, seed, n, first.ctypes.data)
    assert bad == 0, "%d of %d differ; first: point %s, sums %r, max1 %r, two boxes %r" % (bad, n, first[:3], first[3], first[4], first[5])


def _at(lib, p):
    p, out = np.array(p, F32), np.empty(3, F32)
    lib.clamp_at(p.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_points_of_the_folded_cell(shed_lib, seed):
    _check(shed_lib, 0, seed, 1_500_000)


@pytest.mark.parametrize("seed", [4, 5])
def test_faces_edges_corners_and_zero_components(shed_lib, seed):
    """coordinates on the faces of both walls, up to 3 ulps off them, and y = +-0: components q = +-0, and q a few ulps from zero"""
    _check(shed_lib, 1, seed, 1_000_000)


def test_every_face_edge_and_corner(shed_lib):
    bad, inside, on_face = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    n = shed_lib.clamp_grid(ctypes.byref(bad), ctypes.byref(inside), ctypes.byref(on_face))
    assert n == 6 * 3 * 5 * 7 ** 3
    assert bad.value == 0, bad.value
    assert inside.value > 1000 and on_face.value > 1000  # both kinds are among the points


def test_points_inside_each_wall(shed_lib):
    _check(shed_lib, 2, 6, 500_000)
    for p in ((3.5, 2.0, 3.0), (7.0, 2.0, 5.0), (4.5, 1.0, 4.0)):  # the centres, and a point of both walls' common face
        now, before, boxes = _at(shed_lib, p)
        assert now <= 0 and now.view(np.uint32) == before.view(np.uint32) == boxes.view(np.uint32), p


def test_heights_up_to_a_million(shed_lib):
    _check(shed_lib, 3, 7, 500_000)
    for y in (1e6, -1e6, 999999.9375):
        now, before, boxes = _at(shed_lib, (6.0, y, 3.0))
        assert now.view(np.uint32) == before.view(np.uint32) == boxes.view(np.uint32) and now > 9e5, y


def test_signed_zero_components_by_hand(shed_lib):
    """q.y = |y - 2| - 2 is +0 at y = +0, -0 and 4; q.x = +0 on the face x = 2 -- and -0 never: a difference of equal floats is +0"""
    for p in ((2.0, 0.0, 3.0), (2.0, -0.0, 3.0), (3.0, 4.0, 3.0), (10.0, -0.0, 6.0), (0.0, -0.0, 0.0), (-0.0, 2.0, -0.0)):
        now, before, boxes = _at(shed_lib, p)
        assert now.view(np.uint32) == before.view(np.uint32) == boxes.view(np.uint32), (p, now, before, boxes)


def test_a_nan_coordinate_marks_the_edge_of_the_domain(shed_lib):
    """outside the domain (finite points): max1 drops a NaN component -- the clamp becomes 0 --, the sum keeps it.  The root of a NaN
    is a NaN, and min1 with the inside term, itself built with max1 / min1, cannot bring it back: the sums' form says NaN where the
    form with max1 measured the distance in the two finite coordinates."""
    now, before, boxes = _at(shed_lib, (np.nan, 1.0, 8.0))
    assert np.isnan(now) and not np.isnan(before) and before.view(np.uint32) == boxes.view(np.uint32)
    assert before == F32(2.0)  # z = 8 is 2 from wall 2's face z = 6: x no longer counts

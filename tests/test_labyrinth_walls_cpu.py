"""CPU tier: the labyrinth's two walls with one square root (SceneLabyrinth::sd_box_pair_min, sdfr_scenes.h) give the very bits of
the two sd_box calls and the min1 they replace.

The host build (tests/cpp/labyrinth_walls_host.cpp, compiled the way tests/hostsim builds the product headers) checks the
algebra -- signed zeros, insides, outsides, overflow, NaN -- with the host's sqrtf.  On the device sqrt1 is the correctly rounded
square root on the domain both forms rely on (sdfr_math.h), which is all the proof beside the code needs of it; the GPU tier
renders the labyrinth against the oracle."""
import ctypes
import os

import numpy as np
import pytest

import cppbuild

SRC = os.path.join(cppbuild.HERE, "cpp", "labyrinth_walls_host.cpp")


@pytest.fixture(scope="module")
def walls_lib():
    lib = ctypes.CDLL(cppbuild.csrc_lib("walls", SRC))
    lib.walls_check.restype = ctypes.c_int64
    lib.walls_check.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p]
    lib.walls_grid.restype = ctypes.c_int64
    lib.walls_grid.argtypes = [ctypes.POINTER(ctypes.c_int64)]
    return lib


def _check(lib, mode, seed, n):
    first = np.zeros(8, np.float32)
    bad = lib.walls_check(mode, seed, n, first.ctypes.data)
    assert bad == 0, "%d of %d differ; first: points %s / %s, pair %r, two boxes %r" % (bad, n, first[:3], first[3:6], first[6], first[7])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_walls_match_the_two_boxes_in_and_around_the_cell(walls_lib, seed):
    """uniform points in and around the folded cell, and coordinates on, and a few ulps off, every face, edge and corner"""
    _check(walls_lib, 0, seed, 1_000_000)


def test_walls_match_the_two_boxes_on_every_face_edge_and_corner(walls_lib):
    bad = ctypes.c_int64(0)
    n = walls_lib.walls_grid(ctypes.byref(bad))
    assert n == 7 * 3 * 6 * 7 ** 3
    assert bad.value == 0, bad.value


@pytest.mark.parametrize("seed", [11, 12])
def test_pair_matches_two_boxes_anywhere(walls_lib, seed):
    """random boxes and points: inside both (nested, overlapping), inside one, outside both, on faces, +-0 and denormal offsets,
    tiny q, squares that overflow"""
    _check(walls_lib, 1, seed, 1_000_000)

"""CPU tier: the frames of labyrinth_step_cameras.fallback_cameras() do what they are for.  The labyrinth's pixel kernel reads the
gradients of snoise3 from a table in LDS and sends a lane whose lattice coordinates or gradient index leave the table's domain through
the formula a second time (sdfr_noise.h: NoiseGradTable, NoiseHashExact, the `ok` of snoise3 / turbulence3).  No built-in camera reaches
that second pass; these frames do, in some pixels and not in all.  Here the host build of the per-pixel pipeline with
NoiseGradTable<HostTab> as its gradient source and a counter on cleared `ok` (tests/cpp/labyrinth_fallback_host.cpp) counts them, and is
held to the oracle bit for bit; tests/test_gpu_labyrinth_step.py then renders the same frames on the kernels."""
import ctypes
import os

import numpy as np
import pytest

import cppbuild
import labyrinth_step_cameras as lsc

CAMERAS = lsc.fallback_cameras()


@pytest.fixture(scope="module")
def fallback_lib():
    so = cppbuild.compile(os.path.join(cppbuild.BUILD, "liblabyrinth_fallback.so"), [os.path.join(cppbuild.HERE, "cpp", "labyrinth_fallback_host.cpp")],
                          [os.path.join(cppbuild.HERE, "hostsim", "render_rows.h")] + cppbuild.csrc_headers(),
                          cppbuild.EXACT_FLAGS + ["-pthread", "-I" + cppbuild.CSRC, "-I" + os.path.join(cppbuild.HERE, "hostsim")])
    import hostsim

    L = ctypes.CDLL(so)
    assert L.lf_frame_size() == ctypes.sizeof(hostsim.FrameU)
    return L


@pytest.fixture(scope="module")
def frames(oracle):
    """{camera name: (frame, oracle image, oracle per-pixel counters)}: rendered once, shared, left unchanged"""
    out = {}
    for cam in CAMERAS:
        f, _basis = lsc.oracle_frame(oracle, cam)
        ref, rst, _ = oracle.render("labyrinth", f, stats=True)
        ref.setflags(write=False)
        rst.setflags(write=False)
        out[cam[0]] = (f, ref, rst)
    return out


def _render(lib, f, shortcuts):
    import hostsim

    hf = hostsim.frame_from_oracle(f)
    hf.step_shortcuts = shortcuts
    img = np.zeros((lsc.H, lsc.W, 4), np.float32)
    st = np.zeros((lsc.H, lsc.W, 3), np.uint32)
    noise = np.zeros((lsc.H, lsc.W, 2), np.uint32)
    vp = ctypes.c_void_p
    assert lib.lf_render(ctypes.byref(hf), vp(img.ctypes.data), vp(st.ctypes.data), vp(noise.ctypes.data), cppbuild.default_threads()) == 0
    return img, st, noise


@pytest.mark.parametrize("name", [c[0] for c in CAMERAS])
def test_some_pixels_fall_back_and_not_all(fallback_lib, frames, name, capsys):
    f, ref, rst = frames[name]
    # the oracle alone: the frame shows hits and misses, and more than a few colours
    no_hit = int((rst[..., 2] == 0).sum())
    assert lsc.W * lsc.H // 10 < no_hit < lsc.W * lsc.H * 9 // 10, (name, no_hit)
    assert len(np.unique(ref.reshape(-1, 4), axis=0)) > 500, name
    _img, _st, noise = _render(fallback_lib, f, 0)
    shaded = int((noise[..., 0] > 0).sum())  # pixels that read a gradient at all: marble, wood, fire or sky
    fell_back = int((noise[..., 1] > 0).sum())
    with capsys.disabled():
        print("\n%s: %d of %d pixels that evaluate noise fall back (%d of %d gradients read with `ok` cleared); %d pixels without a hit"
              % (name, fell_back, shaded, int(noise[..., 1].sum()), int(noise[..., 0].sum()), no_hit))
    assert shaded > lsc.W * lsc.H // 2
    assert 0 < fell_back < shaded, (name, fell_back, shaded)


def test_where_the_lattice_coordinates_leave_the_range():
    """what fallback_cameras() says of noise_mod289 (plain, as NoiseHashExact::corners reduces the lattice coordinates): for positive
    integers from 2^24 on it leaves [-1, 289] often; for the even integers of [-2^25, -2^24] -- every float there -- at 850 values of one
    band, where it gives 290; below that, down to -2^28, never."""
    c = np.float32(0.00346020761245674740484429065744)

    def outside(v):
        v = v.astype(np.float32)
        r = v - np.floor(v * c) * np.float32(289.0)
        return ~((r >= -1) & (r <= 289)), r

    x = np.arange(2 ** 24, 2 ** 25 + 1, 2, dtype=np.float64)
    assert outside(x)[0].mean() > 0.0015
    bad, r = outside(-x)
    assert int(bad.sum()) == 850 and (r[bad] == 290).all()
    assert (-x[bad]).max() == -17957882 and (-x[bad]).min() == -18939326 and (np.diff(x[bad]) == 1156).all()
    for lo in (25, 26, 27):
        assert not outside(-np.arange(2 ** lo, 2 ** (lo + 1) + 1, 2 ** (lo - 23), dtype=np.float64))[0].any()


@pytest.mark.parametrize("name", [c[0] for c in CAMERAS])
@pytest.mark.parametrize("shortcuts", [0, 1])
def test_host_pipeline_with_the_table_matches_the_oracle(fallback_lib, frames, name, shortcuts):
    f, ref, rst = frames[name]
    img, st, _noise = _render(fallback_lib, f, shortcuts)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), (name, int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum()))
    assert np.array_equal(st[..., 0], rst[..., 0]) and np.array_equal(st[..., 2], rst[..., 2]), name
    if shortcuts:
        assert (st[..., 1] <= rst[..., 1]).all(), name
    else:
        assert np.array_equal(st[..., 1], rst[..., 1]), name

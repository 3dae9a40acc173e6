"""GPU tier: one renderer handle through long mixed sequences of calls (tests/handle_sequences.py).

A handle carries state from frame to frame -- its workspace, the tile cursors and the row order a persistent launch learned,
the two lanes of two frames in flight, the host staging buffers, the strip split, the schedule, the launch mode, step
shortcuts, limits, variables and a scene compiled at run time.  Every step of a seeded sequence runs on ONE handle and is
compared with the same state rendered by a fresh handle (one frame in flight, the default launch mode, fresh buffers):
pixels and per-pixel {rays, evals, hits} bit for bit, getStats() read right after the step, no sentinel left in what the
call owns.  On about one step in eight the fresh handle's frame is checked against the oracle on a stride sample, so that
the reference is not only the library compared with itself.  Failed calls sit between valid frames: they must change
nothing, with one frame in flight or two."""
import ctypes
import math

import numpy as np
import pytest

import gpu_util as gu
import handle_sequences as hs
from gpu_util import FOVY
from handle_sequences import LAUNCH, NAN16, NAN32, SCHEDULE

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT, ERR_NO_SCENE = -1, -4


def _image_format(fmt):
    return hs.RGBA16F if fmt in (hs.RGBA16F, hs.STRIP_RGB16F_A8) else hs.RGBA32F


def _ready(t):
    """a buffer torch has written, finished: with two frames in flight the library renders on streams of its own, which do not
    wait for torch's"""
    import torch

    torch.cuda.synchronize()
    return t


def _sentinel_image(h, w, fmt):
    import torch

    if _image_format(fmt) == hs.RGBA16F:
        return _ready(torch.full((h, w, 4), NAN16, dtype=torch.int16, device="cuda").view(torch.float16))
    return _ready(torch.full((h, w, 4), NAN32, dtype=torch.int32, device="cuda").view(torch.float32))


def _sentinel_stats(h, w):
    import torch

    return _ready(torch.full((h, w, 3), -1, dtype=torch.int32, device="cuda"))


def _bits(a):
    """the raw bits of an image, numpy or torch"""
    if not isinstance(a, np.ndarray):
        a = a.cpu().numpy()
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _sentinel_bits(fmt):
    return NAN16 if _image_format(fmt) == hs.RGBA16F else NAN32


def _stat_sums(st, rows=None):
    st = np.asarray(st, np.int64)
    if rows is not None:
        st = st[rows]
    return (st.shape[0] * st.shape[1],) + tuple(int(st[..., k].sum()) for k in range(3))


class References:
    """Frames of a state as a fresh handle renders them: one frame in flight, the default launch mode, fresh buffers, cached
    by state.  The run-time scene is compiled once, on a handle kept for it and configured in full for every frame."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.cache = {}
        self.runtime = None
        self.oracle_checked = 0

    def close(self):
        if self.runtime is not None:
            self.runtime.close()

    def _handle(self, st):
        import sdf_playground_amd as sp

        if st["scene"] != hs.RUNTIME_SCENE:
            r = sp.SDFRenderer(0)
            r.initShader(st["scene"])
        else:
            if self.runtime is None:
                self.runtime = sp.SDFRenderer(0)
                gu.load(self.runtime, hs.RUNTIME_SCENE)
            r = self.runtime
            r.resetVariables()
            r.setLaunchMode(LAUNCH["auto"])
        r.setLimits(**hs.limits(st["limits"]))
        for name, v in sorted(st["vars"].items()):
            assert r.setValue(name, v)
        r.setParameters(st["stime"])
        r.setStepShortcuts(st["shortcuts"])
        r.setSchedule(SCHEDULE[st["schedule"]])
        return r

    def get(self, st, w, h, fmt):
        """(image as numpy, per-pixel stats [h, w, 3] uint32, getStats totals)"""
        import torch

        fmt = _image_format(fmt)
        key = (st["scene"], st["limits"], tuple(sorted(st["vars"].items())), st["t"], st["stime"], st["shortcuts"], st["schedule"], w, h, fmt)
        if key in self.cache:
            return self.cache[key]
        r = self._handle(st)
        try:
            gu.orbit_camera(r, st["scene"], st["t"], w, h)
            img = _sentinel_image(h, w, fmt)
            pst = _sentinel_stats(h, w)
            r.render(None, w, h, out=img, fmt=fmt, pixel_stats=pst)
            tot = gu.totals(r.getStats())
            r.sync()
            torch.cuda.synchronize()
        finally:
            if r is not self.runtime:
                r.close()
        img, pst = img.cpu().numpy(), pst.cpu().numpy().view(np.uint32)
        assert not (_bits(img) == _sentinel_bits(fmt)).any(), key
        assert tot == _stat_sums(pst) and tot[0] == w * h, (key, tot, _stat_sums(pst))
        self.cache[key] = (img, pst, tot)
        return self.cache[key]

    def check_oracle(self, st, w, h, fmt, phase):
        """a stride sample of the fresh handle's frame against the oracle (built-in scenes)"""
        oracle = self.oracle
        img, pst, _ = self.get(st, w, h, fmt)
        kind, eye, target = hs.camera(st["scene"], st["t"])
        aspect = np.float32(w) / np.float32(h)
        basis = (oracle.camera_lookat if kind == "lookat" else oracle.camera_direction)(eye, target, FOVY, aspect)
        f = oracle.default_frame(st["scene"], w, h, basis=basis, stime=st["stime"])
        for name, v in hs.limits(st["limits"]).items():
            setattr(f, name, v)
        slots = {row[0]: row[6] for row in oracle.var_table(st["scene"])}
        for name, v in st["vars"].items():
            f.scene_var[slots[name]] = v
        stride = max(1, int(math.ceil(math.sqrt(w * h / 1500.0))))
        x0, y0 = phase % stride, (phase // stride) % stride
        if x0 >= w or y0 >= h:
            x0 = y0 = 0
        ref, rst, _ = oracle.render(st["scene"], f, region=(x0, y0, w, h), step=(stride, stride), stats=True)
        ref, rst = ref[y0::stride, x0::stride], rst[y0::stride, x0::stride]
        if _image_format(fmt) == hs.RGBA16F:
            assert np.array_equal(_bits(img)[y0::stride, x0::stride], oracle.float_to_half(ref)), st
        else:
            assert np.array_equal(_bits(img)[y0::stride, x0::stride], ref.view(np.uint32)), st
        got = pst[y0::stride, x0::stride]
        assert np.array_equal(got[..., 0], rst[..., 0]) and np.array_equal(got[..., 2], rst[..., 2]), st
        if not st["shortcuts"]:
            assert np.array_equal(got[..., 1], rst[..., 1]), st
        else:
            assert (got[..., 1] <= rst[..., 1]).all(), st
        self.oracle_checked += 1


@pytest.fixture(scope="module")
def refs(oracle):
    r = References(oracle)
    yield r
    r.close()


def _fail(r, step, keep):
    """a call that must fail and change nothing: a bad format, or a frame of more than 2^30 pixels (raw sdfr_render: the
    wrapper asserts the size of the tensor)"""
    import torch

    w, h = (step["w"], step["h"]) if step["fail"] == "format" else (1, 4)
    target = _sentinel_image(h, w, hs.RGBA32F)
    keep.append(target)
    if step["fail"] == "format":
        rc, message = r._L.sdfr_render(r._h, w, h, ctypes.c_void_p(target.data_ptr()), 7, 0, None), "bad format"
    else:
        rc, message = r._L.sdfr_render(r._h, hs.HUGE_SIZE[0], hs.HUGE_SIZE[1], ctypes.c_void_p(target.data_ptr()), hs.RGBA32F, 0, None), "bad frame size"
    assert rc == ERR_INVALID_ARGUMENT, (step["i"], rc)
    assert r._L.sdfr_last_error(r._h).decode() == message, step["i"]
    return target


def _run_sequence(refs, seed):
    import torch
    import sdf_playground_amd as sp

    steps = hs.sequence(seed)
    r = sp.SDFRenderer(0)
    side = torch.cuda.Stream()
    last = None       # getStats of the last call that succeeded
    prev_bufs = {}    # the device image and statistics of the step before
    keep = []         # buffers of calls that failed, checked untouched at the end
    try:
        assert all(np.float32(getattr(r.getLimits(), k)) == np.float32(v) for k, v in hs.DEFAULT_LIMITS.items())
        for s in steps:
            i, st, w, h, fmt = s["i"], s["state"], s["w"], s["h"], s["fmt"]
            where = (seed, i, s["call"], st["scene"], w, h, fmt, st["fif"])
            gu.apply_changes(r, s["set"])
            if s["call"] == "failed":
                target = _fail(r, s, keep)
                # the frame submitted last is still the last one that succeeded
                assert gu.totals(r.getStats()) == last, where
                r.waitFrame(side.cuda_stream)
                r.sync()
                side.synchronize()
                assert (_bits(target) == NAN32).all(), where
                prev_bufs = {}
                continue
            gu.orbit_camera(r, st["scene"], st["t"], w, h)
            img_ref, pst_ref, tot_ref = refs.get(st, w, h, fmt)
            bufs = {}
            if s["call"] == "device":
                img = prev_bufs["img"] if s["reuse_image"] else _sentinel_image(h, w, fmt)
                pst = (prev_bufs["pst"] if s["reuse_stats"] else _sentinel_stats(h, w)) if s["stats"] else None
                r.render(None, w, h, out=img, fmt=fmt, pixel_stats=pst if pst is not None else False)
                last = gu.totals(r.getStats())
                r.sync()
                assert last == tot_ref, (where, last, tot_ref)
                got = _bits(img)
                assert np.array_equal(got, _bits(img_ref)), (where, int((got != _bits(img_ref)).any(axis=2).sum()))
                if pst is not None:
                    st_got = pst.cpu().numpy().view(np.uint32)
                    assert np.array_equal(st_got, pst_ref), where
                    assert _stat_sums(st_got) == last, where
                bufs = dict(img=img, pst=pst)
            elif s["call"] == "host":
                out = np.full((h, w, 4), NAN16 if fmt == hs.RGBA16F else NAN32, np.uint16 if fmt == hs.RGBA16F else np.uint32)
                out = out.view(np.float16 if fmt == hs.RGBA16F else np.float32)
                res = r.render(None, w, h, out=out, fmt=fmt, pixel_stats=s["stats"])
                last = gu.totals(r.getStats())
                assert last == tot_ref, (where, last, tot_ref)
                img = res[0] if s["stats"] else res
                assert img is out
                assert np.array_equal(_bits(img), _bits(img_ref)), (where, int((_bits(img) != _bits(img_ref)).any(axis=2).sum()))
                if s["stats"]:
                    assert np.array_equal(res[1], pst_ref), where
            elif s["call"] == "strips":
                last = _run_strips(r, s, where, img_ref, pst_ref) or last
            else:
                last = _run_private(r, s, where, img_ref, pst_ref)
            prev_bufs = bufs
            if i % 8 == seed % 8 and st["scene"] != hs.RUNTIME_SCENE:
                refs.check_oracle(st, w, h, fmt, phase=i)
        for target in keep:
            assert (_bits(target) == NAN32).all()
    finally:
        r.close()
    return steps


def _run_strips(r, s, where, img_ref, pst_ref):
    """renderStrips for every rank of an emulated world, then assembleStrips: the rows the shared strips own equal the fresh
    handle's frame, the private rows of the handle's split are left alone, rows of a strip buffer past the frame are zero"""
    import torch
    import sdf_playground_amd as sp

    w, h, fmt, world = s["w"], s["h"], s["fmt"], s["world"]
    split = s["state"]["split"]
    n = sp.strip_buffer_pixels(w, h, world, split)
    nbytes = sp.strip_buffer_bytes(w, h, world, fmt, split)
    fill = NAN32 if _image_format(fmt) == hs.RGBA32F else (NAN16 << 16) | NAN16
    fill = fill - (1 << 32) if fill >= 1 << 31 else fill
    img = _sentinel_image(h, w, fmt)
    last = None
    if nbytes > 0:  # (every strip private: nothing to render)
        bufs = []
        for rank in range(world):
            buf = _ready(torch.full((nbytes // 4,), fill, dtype=torch.int32, device="cuda"))
            r.renderStrips(w, h, rank, world, buf, fmt=fmt)
            last = gu.totals(r.getStats())
            rows = sp.strip_rows_of_rank(h, rank, world, split)
            assert last == _stat_sums(pst_ref, rows), (where, rank, last, _stat_sums(pst_ref, rows))
            bufs.append(buf)
        r.sync()
        r.assembleStrips(w, h, world, _ready(torch.cat(bufs)), img, fmt=fmt)
        r.sync()
        for rank, buf in enumerate(bufs):
            b = buf.cpu().numpy().view(np.uint8)
            k = len(sp.strip_rows_of_rank(h, rank, world, split)) * w
            if fmt in (hs.RGBA32F, hs.RGBA16F):
                px = 16 if fmt == hs.RGBA32F else 8
                tail = [b[px * k:px * n]]
            else:
                rgb = 12 if fmt == hs.STRIP_RGB32F_A8 else 6
                tail = [b[rgb * k:rgb * n], b[rgb * n + k:(rgb + 1) * n]]
            assert all(not t.any() for t in tail), (where, rank, "strip buffer rows past the frame are not zero")
    got, want = _bits(img), _bits(img_ref)
    private = np.zeros(h, bool)
    private[sp.private_rows_host(h, split)] = True
    assert np.array_equal(got[~private], want[~private]), (where, int((got[~private] != want[~private]).any(axis=-1).sum()))
    assert (got[private] == _sentinel_bits(fmt)).all(), (where, "assembly wrote a private row")
    return last


def _run_private(r, s, where, img_ref, pst_ref):
    """setStripSplit + renderPrivateStrips: the private rows equal the fresh handle's frame, no other row is written"""
    import sdf_playground_amd as sp

    w, h, fmt = s["w"], s["h"], s["fmt"]
    split = s["state"]["split"]
    img = _sentinel_image(h, w, fmt)
    r.renderPrivateStrips(w, h, img, fmt=fmt)
    last = gu.totals(r.getStats())
    r.sync()
    rows = sp.private_rows_host(h, split)
    assert rows and last == _stat_sums(pst_ref, rows), (where, last, _stat_sums(pst_ref, rows))
    got, want = _bits(img), _bits(img_ref)
    private = np.zeros(h, bool)
    private[rows] = True
    assert np.array_equal(got[private], want[private]), (where, int((got[private] != want[private]).any(axis=-1).sum()))
    assert (got[~private] == _sentinel_bits(fmt)).all(), (where, "a private launch wrote a shared row")
    return last


@pytest.mark.parametrize("seed", hs.SEEDS)
def test_one_handle_through_a_seeded_sequence(refs, seed):
    steps = _run_sequence(refs, seed)
    assert len(steps) == hs.STEPS


def test_a_call_before_any_scene_changes_nothing(refs):
    """'no scene' can only happen on a new handle: it fails with the right error, leaves nothing to report, and the frames after
    it (two in flight) are right"""
    import sdf_playground_amd as sp

    r = sp.SDFRenderer(0)
    try:
        r.setFramesInFlight(2)
        img = _sentinel_image(90, 160, hs.RGBA32F)
        with pytest.raises(sp.SdfrError) as e:
            r.render(None, 160, 90, out=img)
        assert e.value.code == ERR_NO_SCENE and r._L.sdfr_last_error(r._h).decode() == "no scene loaded"
        with pytest.raises(sp.SdfrError) as e:
            r.getStats()
        assert e.value.code == ERR_INVALID_ARGUMENT
        r.waitFrame(None)
        r.sync()
        assert (_bits(img) == NAN32).all()
        st = dict(scene="gems", limits="5", vars={}, t=0.4, stime=0.25, shortcuts=False, schedule="pixel")
        gu.apply_changes(r, dict(scene="gems", limits="5", stime=0.25, shortcuts=False))
        imgs = []
        for t in (0.4, 1.4):
            gu.orbit_camera(r, "gems", t, 160, 90)
            imgs.append(_sentinel_image(90, 160, hs.RGBA32F))
            r.render(None, 160, 90, out=imgs[-1])
            assert gu.totals(r.getStats()) == refs.get(dict(st, t=t), 160, 90, hs.RGBA32F)[2]
        r.sync()
        for t, im in zip((0.4, 1.4), imgs):
            assert np.array_equal(_bits(im), _bits(refs.get(dict(st, t=t), 160, 90, hs.RGBA32F)[0])), t
    finally:
        r.close()


def test_two_frames_in_flight_share_a_pixel_stats_buffer(refs):
    """Two frames in flight, each into its own image but into the SAME device pixel_stats tensor, nothing waited for: the
    statistics are the second frame's.  A failed call in between changes neither what getStats / waitFrame report nor the
    order of the frames: a third frame into the first frame's image (and the same statistics) lands after both."""
    import torch
    import sdf_playground_amd as sp

    w, h = 1920, 1080
    st = dict(scene="labyrinth", limits="3", vars={}, stime=0.5, shortcuts=True, schedule="pixel")
    ts = (0.3, 1.9, 3.6)
    want = [refs.get(dict(st, t=t), w, h, hs.RGBA32F) for t in ts]
    assert all(not np.array_equal(want[0][1], x[1]) for x in want[1:])
    r = sp.SDFRenderer(0)
    side = torch.cuda.Stream()
    try:
        gu.apply_changes(r, dict(scene="labyrinth", limits="3", stime=0.5, shortcuts=True, fif=2))
        for wait_between in (True, False):
            img1, img2 = _sentinel_image(h, w, hs.RGBA32F), _sentinel_image(h, w, hs.RGBA32F)
            pst = _sentinel_stats(h, w)
            for t, img in zip(ts[:2], (img1, img2)):
                gu.orbit_camera(r, "labyrinth", t, w, h)
                r.render(None, w, h, out=img, pixel_stats=pst)
            if wait_between:
                r.sync()
                assert np.array_equal(pst.cpu().numpy().view(np.uint32), want[1][1]), "statistics are not the second frame's"
                assert np.array_equal(_bits(img1), _bits(want[0][0])) and np.array_equal(_bits(img2), _bits(want[1][0]))
            _fail(r, dict(i=-1, fail="format", w=w, h=h), [])
            # what getStats and waitFrame describe is still the second frame
            assert gu.totals(r.getStats()) == want[1][2], wait_between
            r.waitFrame(side.cuda_stream)
            with torch.cuda.stream(side):
                copy2 = img2.clone()
            gu.orbit_camera(r, "labyrinth", ts[2], w, h)
            r.render(None, w, h, out=img1, pixel_stats=pst)
            assert gu.totals(r.getStats()) == want[2][2], wait_between
            r.sync()
            side.synchronize()
            assert np.array_equal(_bits(copy2), _bits(want[1][0])), (wait_between, "waitFrame did not wait for the second frame")
            assert np.array_equal(_bits(img1), _bits(want[2][0])), (wait_between, "the first image is not the third frame's")
            assert np.array_equal(_bits(img2), _bits(want[1][0])), wait_between
            assert np.array_equal(pst.cpu().numpy().view(np.uint32), want[2][1]), (wait_between, "statistics are not the third frame's")
    finally:
        r.close()

"""Shared by the anti-aliasing tests (test_aa_cpu.py, test_gpu_aa.py): the definition of sdfr_render_aa (include/sdfr.h) restated in
numpy from the header's words, np.float32 operations only; the pass plan restated from DESIGN.md 4.7; the library's stage functions
and planner built for the CPU (tests/cpp/resolve_host.cpp); compact strip buffers; the frames.  Test infrastructure: the product
never imports this."""
import ctypes
import functools

import numpy as np

import cppbuild
import query_util as qu

F = np.float32
STRIP_ROWS = 8
FACTORS = (2, 4, 8)
W, H = 37, 21  # odd and indivisible on purpose: K * H is a multiple of 8 for K = 8 only


# ---- the definition ---------------------------------------------------------------------------------------------------------------

def box2(a):
    """box2(A)[y][x] = ((A[2y][2x] + A[2y][2x+1]) + (A[2y+1][2x] + A[2y+1][2x+1])) * 0.25f, in fp32 and in that order"""
    a = np.asarray(a, np.float32)
    with np.errstate(all="ignore"):
        return ((a[0::2, 0::2] + a[0::2, 1::2]) + (a[1::2, 0::2] + a[1::2, 1::2])) * F(0.25)


def pyramid(s, factor):
    """box2 applied log2(factor) times to the frame S"""
    while factor > 1:
        s = box2(s)
        factor //= 2
    return np.ascontiguousarray(s, np.float32)


def sum_stats(st, factor):
    """[K * H, K * W, 3] uint32 -> [H, W, 3]: the sums over every pixel's K x K sub-samples"""
    h, w = st.shape[0] // factor, st.shape[1] // factor
    return st.reshape(h, factor, w, factor, 3).astype(np.uint64).sum(axis=(1, 3)).astype(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(u), b.view(u))


def same_bits_or_nan(a, b):
    """same_bits, except that where both are NaN any NaN will do: which of two NaN operands an addition hands on (its sign, its
    payload) is left open by IEEE 754 -- x86 keeps its first source operand, whichever the compiler made that, and a GPU returns
    one canonical NaN -- so a NaN's bits are not something the definition fixes.  Every other value, infinities and zeros' signs
    included, must have the definition's bits."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())


# ---- the pass plan, from the words of DESIGN.md 4.7 ---------------------------------------------------------------------------------

def plan(width, height, factor, budget):
    """-> (strips of S, passes, strips per pass): the fewest passes for which one pass's strips of 8 * K * W RGBA32F pixels fit the
    budget, at least one strip per pass"""
    strips = -(-factor * height // STRIP_ROWS)
    fit = max(1, budget // (STRIP_ROWS * factor * width * 16))
    passes = -(-strips // fit)
    return strips, passes, -(-strips // passes)


def budget_for(width, factor, strips_per_pass):
    """a budget that holds exactly that many strips of S"""
    return strips_per_pass * STRIP_ROWS * factor * width * 16


def compact(s, pass_, passes, strips_per_pass, fill):
    """pass `pass_`'s compact buffer of the frame S ([rows, cols, c]): local strip l is strip l * passes + pass_ of S; what lies past
    the frame is `fill` -- the library zero-fills it and must not read it, so the tests put something loud there"""
    rows, cols, c = s.shape
    out = np.full((strips_per_pass * STRIP_ROWS, cols, c), fill, s.dtype)
    for l in range(strips_per_pass):
        y0 = (l * passes + pass_) * STRIP_ROWS
        if y0 < rows:
            n = min(STRIP_ROWS, rows - y0)
            out[l * STRIP_ROWS:l * STRIP_ROWS + n] = s[y0:y0 + n]
    return out


# ---- the library's stage functions and planner, for the CPU -----------------------------------------------------------------------------

_host = None


def host_lib():
    global _host
    if _host is None:
        L = ctypes.CDLL(qu.build_lib("resolve_host", "resolve_host.cpp", ["-I" + qu.CSRC], cppbuild.csrc_headers()))
        vp, ci, cu, ull = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_ulonglong
        L.rh_plan.argtypes = [ci, ci, ci, ull, vp]
        L.rh_plan.restype = None
        L.rh_pass_rows.argtypes = [ci, ci, ci, ull, cu, vp]
        L.rh_half.argtypes = [vp, vp, ctypes.c_longlong]
        L.rh_half.restype = None
        L.rh_resolve.argtypes = [ci, ci, ci, ull, cu, vp, vp, ci, vp, vp]
        L.rh_resolve.restype = None
        _host = L
    return _host


def host_half(x):
    """the library's fp32 -> half conversion as the host compiler builds it: uint16 bits"""
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros(x.shape, np.uint16)
    host_lib().rh_half(qu._p(x), qu._p(out), x.size)
    return out


def host_plan(width, height, factor, budget):
    """the library's plan: dict of factor_log2, s_width, s_height, rows_per_strip, strips, passes, strips_per_pass, pass_pixels"""
    out = np.zeros(8, np.int64)
    host_lib().rh_plan(width, height, factor, budget, qu._p(out))
    return dict(zip(["factor_log2", "s_width", "s_height", "rows_per_strip", "strips", "passes", "strips_per_pass", "pass_pixels"], (int(v) for v in out)))


def host_pass_rows(width, height, factor, budget, pass_, strips_per_pass):
    """(strips the pass renders, [(row0, rows)] per local strip of its compact buffer)"""
    rows = np.zeros(2 * strips_per_pass, np.int32)
    n = host_lib().rh_pass_rows(width, height, factor, budget, pass_, qu._p(rows))
    return n, [(int(rows[2 * l]), int(rows[2 * l + 1])) for l in range(strips_per_pass)]


def host_resolve(s, st, width, height, factor, budget, fmt, canary=None):
    """Every pass of the plan for `budget` through the host build of the stage functions, each from its compact buffers.
    -> (image [H, W, 4] float32 or float16, stats [H, W, 3] or None)"""
    _strips, passes, spp = plan(width, height, factor, budget)
    img = np.zeros((height, width, 4), np.float32 if fmt == 0 else np.float16)
    if canary is not None:
        img.view(np.uint32 if fmt == 0 else np.uint16)[...] = canary
    out_st = None if st is None else np.full((height, width, 3), 0xDEADBEEF, np.uint32)
    for p in range(passes):
        c = compact(s, p, passes, spp, np.nan)  # rows past the frame: NaN colours, huge counters -- never to be read
        cs = None if st is None else compact(st, p, passes, spp, 0x7FFFFFFF)
        host_lib().rh_resolve(width, height, factor, budget, p, qu._p(c), None if cs is None else qu._p(cs), fmt, qu._p(img), None if st is None else qu._p(out_st))
    return img, out_st


# ---- frames -----------------------------------------------------------------------------------------------------------------------

def camera_of(oracle, scene):
    """the camera the parity tests give the scene (gpu_util.parity_cameras): (kind, eye, target, fovy, aspect, basis)"""
    import gpu_util as gu

    cams, fovy, asp = gu.parity_cameras()
    kind, eye, tgt = cams[scene]
    basis = (oracle.camera_lookat if kind == "lookat" else oracle.camera_direction)(eye, tgt, fovy, asp)
    return kind, eye, tgt, fovy, asp, basis


@functools.lru_cache(maxsize=None)
def _oracle_frame(scene, stime, width, height):
    from oracle import pyoracle as po

    f = po.default_frame(scene, width, height, basis=camera_of(po, scene)[5], stime=stime)
    img, st, tot = po.render(scene, f, stats=True)
    for a in (img, st, tot):
        a.setflags(write=False)
    return img, st, tot


def oracle_s(oracle, scene, stime, width, height, factor):
    """the oracle's frame S for a width x height image at `factor`: (rgba, stats, totals), computed once and read-only"""
    return _oracle_frame(scene, stime, width * factor, height * factor)

"""Shared by the span tests (test_span_cpu.py, test_gpu_span.py): the definition of the span queries (include/sdfr.h: sdfr_query_ray_spans)
restated in numpy from the header's words, np.float32 operations only, all rays in lockstep; the library's stage function built for the
CPU (tests/cpp/span_host.cpp); the pixels' primary rays from the oracle's driver (tests/cpp/span_oracle.cpp); and the checks every
result has to pass.  Test infrastructure: the product never imports this."""
import ctypes
import os

import numpy as np

import cppbuild
import query_util as qu

F = np.float32
STARTS_INSIDE, ENDS_INSIDE, OUT_OF_STEPS = 1, 2, 4
# sdfr_span_summary, word for word
SUMMARY_DTYPE = np.dtype([("crossings", np.uint32), ("spans", np.uint32), ("steps", np.uint32), ("valid", np.int32), ("inside_length", np.float32),
                          ("t_end", np.float32), ("flags", np.uint32), ("reserved", np.uint32)])
assert SUMMARY_DTYPE.itemsize == 32


def params(min_step, t_max, iso=0.0, max_steps=4096, max_spans=4):
    """t_max is the EFFECTIVE one: the entry points' 0 already replaced by limits.range"""
    return dict(t_max=float(t_max), min_step=float(min_step), iso=float(iso), max_steps=int(max_steps), max_spans=int(max_spans))


def march_spans(distance_fn, origins, dirs, p, valid=None):
    """The header's definition.  distance_fn: points [k, 3] float32 -> D [k] float32, called once per step on the rays still marching.
    valid: per item 1, or -1 for an item that is no ray (a pixel outside the frame).  -> (summaries [n] SUMMARY_DTYPE, spans [n, max_spans, 2])"""
    o, d = np.ascontiguousarray(origins, F).reshape(-1, 3), np.ascontiguousarray(dirs, F).reshape(-1, 3)
    n = len(o)
    t_max, min_step, iso, max_steps, max_spans = F(p["t_max"]), F(p["min_step"]), F(p["iso"]), p["max_steps"], p["max_spans"]
    S, spans = np.zeros(n, SUMMARY_DTYPE), np.zeros((n, max_spans, 2), F)
    ok = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)
    if valid is not None:
        ok &= np.asarray(valid) == 1
        S["valid"][np.asarray(valid) == -1] = -1
    S["valid"][ok] = 1
    t, t_prev, s_prev, t_in = (np.zeros(n, F) for _ in range(4))
    inside_prev, is_open = np.zeros(n, bool), np.zeros(n, bool)

    def close(idx, t_out):
        k = S["spans"][idx].astype(np.int64) - 1
        store = k < max_spans
        spans[idx[store], k[store], 0] = t_in[idx[store]]
        spans[idx[store], k[store], 1] = t_out[store]
        S["inside_length"][idx] = S["inside_length"][idx] + (t_out - t_in[idx])
        is_open[idx] = False

    a = np.nonzero(ok)[0]
    step = 0
    with np.errstate(all="ignore"):
        while len(a):
            pos = o[a] + t[a, None] * d[a]  # one multiply, then one add
            assert pos.dtype == F
            s = np.ascontiguousarray(distance_fn(pos), F) - iso
            inside = s < 0  # NaN: outside
            if step == 0:
                first = a[inside]
                is_open[first] = True
                S["flags"][first] |= STARTS_INSIDE
                S["spans"][first] += 1
            else:
                cross = inside != inside_prev[a]
                u = s_prev[a] / (s_prev[a] - s)
                u = np.where((u >= 0) & (u <= 1), u, F(0.5)).astype(F)
                tc = t_prev[a] + u * (t[a] - t_prev[a])
                S["crossings"][a[cross]] += 1
                enter, leave = cross & inside, cross & ~inside
                is_open[a[enter]] = True
                t_in[a[enter]] = tc[enter]
                S["spans"][a[enter]] += 1
                close(a[leave], tc[leave])
            S["steps"][a] += 1
            S["t_end"][a] = t[a]
            at_end = ~(t[a] < t_max)
            out_of = ~at_end & (step + 1 == max_steps)
            S["flags"][a[out_of]] |= OUT_OF_STEPS
            done = at_end | out_of
            last = a[done & is_open[a]]
            S["flags"][last] |= ENDS_INSIDE
            close(last, t[last])
            k = a[~done]
            mag = np.abs(s[~done])
            h = np.where(mag > min_step, mag, min_step).astype(F)  # NaN steps by min_step
            tn = t[k] + h
            tn = np.where(tn < t_max, tn, t_max).astype(F)
            s_prev[k], inside_prev[k], t_prev[k] = s[~done], inside[~done], t[k]
            t[k] = tn
            a = k
            step += 1
    return S, spans


def mesh_rays(positions, normals, reach):
    """sdfr_mesh_spans' rays: origin = positions + reach * normals (one multiply, then one add), dir = -normals"""
    pos, nrm = np.ascontiguousarray(positions, F).reshape(-1, 3), np.ascontiguousarray(normals, F).reshape(-1, 3)
    return (pos + F(reach) * nrm).astype(F), (-nrm).astype(F)


def thickness(S, spans):
    """meshThickness' rule: the length of the first stored span; inf where there is none or where it is closed only by ENDS_INSIDE"""
    out = np.full(len(S), np.inf, F)
    if spans.shape[1]:
        closed = (S["valid"] == 1) & (S["spans"] >= 1) & ~((S["spans"] == 1) & ((S["flags"] & ENDS_INSIDE) != 0))
        out[closed] = (spans[closed, 0, 1] - spans[closed, 0, 0]).astype(F)
    return out


# ---- the fields of the CPU tier --------------------------------------------------------------------------------------------------
def slab_field(c, r, nan_lo, nan_hi):
    """D = min_k(|x - c_k| - r_k), the minimum taken in the order of k by `v < D ? v : D` from +inf; NaN where nan_lo <= x <= nan_hi"""
    c, r = np.asarray(c, F), np.asarray(r, F)

    def distance(p):
        x = p[:, 0]
        D = np.full(len(x), np.inf, F)
        for ck, rk in zip(c, r):
            v = np.abs(x - ck) - rk
            D = np.where(v < D, v, D)
        return np.where((x >= F(nan_lo)) & (x <= F(nan_hi)), F(np.nan), D).astype(F)

    return distance


# ---- the library's stage function on the CPU -------------------------------------------------------------------------------------
class HostParams(ctypes.Structure):  # sdfr::SpanParams = sdfr_span_params
    _fields_ = [("t_max", ctypes.c_float), ("min_step", ctypes.c_float), ("iso", ctypes.c_float), ("max_steps", ctypes.c_int32), ("max_spans", ctypes.c_int32)]


_host = None


def host_lib():
    global _host
    if _host is None:
        L = ctypes.CDLL(cppbuild.csrc_lib("span_host", os.path.join(cppbuild.HERE, "cpp", "span_host.cpp")))
        assert L.sph_params_size() == ctypes.sizeof(HostParams) == 20 and L.sph_summary_words() == 8
        vp = ctypes.c_void_p
        L.sph_march_slabs.argtypes = [ctypes.c_int64, vp, vp, ctypes.POINTER(HostParams), ctypes.c_int, vp, vp, ctypes.c_float, ctypes.c_float, vp, vp]
        L.sph_march_sphere.argtypes = [ctypes.c_int64, vp, vp, ctypes.POINTER(HostParams), vp, ctypes.c_float, vp, vp]
        _host = L
    return _host


def _host_call(fn, origins, dirs, p, *field):
    o, d = np.ascontiguousarray(origins, F).reshape(-1, 3), np.ascontiguousarray(dirs, F).reshape(-1, 3)
    hp = HostParams(p["t_max"], p["min_step"], p["iso"], p["max_steps"], p["max_spans"])
    S, spans = np.full(len(o), -7, np.int32).repeat(8).view(SUMMARY_DTYPE), np.full((len(o), p["max_spans"], 2), -7.0, F)
    assert fn(len(o), qu._p(o), qu._p(d), ctypes.byref(hp), *field, qu._p(S), qu._p(spans) if p["max_spans"] else None) == 0
    return S, spans


def host_march_slabs(origins, dirs, p, c, r, nan_lo, nan_hi):
    c, r = np.ascontiguousarray(c, F), np.ascontiguousarray(r, F)
    return _host_call(host_lib().sph_march_slabs, origins, dirs, p, len(c), qu._p(c), qu._p(r), float(nan_lo), float(nan_hi))


def host_march_sphere(origins, dirs, p, centre, radius):
    centre = np.ascontiguousarray(centre, F)
    return _host_call(host_lib().sph_march_sphere, origins, dirs, p, qu._p(centre), float(radius))


# ---- the pixels' primary rays, as the oracle's driver makes them -----------------------------------------------------------------
_oracle = None


def pixel_rays(of, pixels):
    """-> (origins [n, 3], dirs [n, 3], valid [n]: 1, or -1 for a pixel outside the frame, whose ray is all zero)"""
    global _oracle
    if _oracle is None:
        deps = cppbuild.oracle_headers()
        _oracle = ctypes.CDLL(qu.build_lib("span_oracle", "span_oracle.cpp", ["-I" + cppbuild.ORACLE], deps))
        _oracle.spo_pixel_rays.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        assert _oracle.spo_frame_size() == ctypes.sizeof(type(of))
    px = np.ascontiguousarray(pixels, np.int32).reshape(-1, 2)
    o, d, valid = np.zeros((len(px), 3), F), np.zeros((len(px), 3), F), np.zeros(len(px), np.int32)
    assert _oracle.spo_pixel_rays(ctypes.byref(of), len(px), qu._p(px), qu._p(o), qu._p(d), qu._p(valid)) == 0
    return o, d, valid


# ---- what every result has to pass -----------------------------------------------------------------------------------------------
def check_invariants(S, spans, p):
    max_spans = p["max_spans"]
    assert S.dtype == SUMMARY_DTYPE and spans.shape == (len(S), max_spans, 2) and spans.dtype == F
    bad = S["valid"] != 1
    for name in SUMMARY_DTYPE.names:
        if name != "valid":
            assert not S[name][bad].view(np.uint32).any(), name
    assert not spans[bad].view(np.uint32).any() and not S["reserved"].any()
    ok = ~bad
    starts, ends = (S["flags"] & STARTS_INSIDE) != 0, (S["flags"] & ENDS_INSIDE) != 0
    assert (S["crossings"][ok] == (2 * S["spans"].astype(np.int64) - starts - ends)[ok]).all()
    assert (S["steps"][ok] >= 1).all() and (S["steps"] <= p["max_steps"]).all() and (S["flags"] < 8).all()
    assert (S["t_end"][ok] >= 0).all() and (S["t_end"][ok] <= F(p["t_max"])).all()
    out_of = (S["flags"] & OUT_OF_STEPS) != 0
    assert (S["steps"][out_of] == p["max_steps"]).all() and (S["t_end"][out_of] < F(p["t_max"])).all()
    assert (S["t_end"][ok & ~out_of] == F(p["t_max"])).all()
    stored = np.minimum(S["spans"], max_spans)
    for i in np.nonzero(ok)[0]:
        k = int(stored[i])
        assert not spans[i, k:].view(np.uint32).any(), i  # unused slots are zero
        flat = spans[i, :k].ravel()
        assert (np.diff(flat) >= 0).all() and (k == 0 or (flat[0] >= 0 and flat[-1] <= S["t_end"][i])), (i, flat, S[i])
        if starts[i] and k:
            assert spans[i, 0, 0] == 0
        if S["spans"][i] <= max_spans:  # all spans are stored: the running fp32 sum can be redone
            run = F(0)
            order = spans[i, :k]
            for t_in, t_out in order:
                run = F(run + F(t_out - t_in))
            assert run.view(np.uint32) == S["inside_length"][i].view(np.uint32), (i, run, S[i])
            if ends[i] and k:
                assert spans[i, k - 1, 1] == S["t_end"][i]

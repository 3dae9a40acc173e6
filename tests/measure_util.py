"""Shared by the measure tests (test_measure_cpu.py, test_gpu_measure.py): the definition of sdfr_measure and sdfr_measure_properties
(include/sdfr.h) restated in numpy from the header's words -- the march is span_util.march_spans, imported and called with room for every
span; the moments are np.float64 operations in the header's order; the reduction is the pairwise tree over 8 x 8 tiles and then over runs
of 64 --; the library's stage functions built for the CPU (tests/cpp/measure_host.cpp); and the comparison of two results bit for bit.
Test infrastructure: the product never imports this."""
import ctypes
import os

import numpy as np

import cppbuild
import query_util as qu
import span_util as su

F, D = np.float32, np.float64
COLUMN_DTYPE = np.dtype([("m0", D), ("m1", D), ("m2", D), ("spans", np.uint32), ("steps", np.uint32), ("flags", np.uint32), ("valid", np.int32)])
assert COLUMN_DTYPE.itemsize == 40
INTEGERS = ("columns_hit", "columns_open", "columns_out_of_steps", "columns_invalid", "steps", "spans", "crossings")
# The restatement against the closed forms of a sphere (tests/test_measure_cpu.py: sphere_errors), per rho / cell: the worst values it gave
# (recorded in DESIGN.md 4.16), as relative errors of the volume and of I_zz and the centroid's distance in cells
RECORDED_WORST = {8: (4.8e-3, 1.65e-2, 0.019), 16: (1.14e-3, 4.55e-3, 0.0104), 32: (1.82e-4, 8.83e-4, 0.0045)}


def grid(origin, du, dv, dw, nu, nv):
    return dict(origin=np.asarray(origin, F), du=np.asarray(du, F), dv=np.asarray(dv, F), dw=np.asarray(dw, F), nu=int(nu), nv=int(nv))


def box_grid(lo, hi, cell, axis="z"):
    """measureGrid's rule: columns through the centres of the cells on the box's lower face across `axis` -> (grid, t_max)"""
    w = "xyz".index(axis)
    u, v = (w + 1) % 3, (w + 2) % 3
    n = [max(1, int(np.ceil((hi[a] - lo[a]) / cell - 1e-6))) for a in (u, v)]
    origin, du, dv, dw = [float(x) for x in lo], [0.0] * 3, [0.0] * 3, [0.0] * 3
    origin[u], origin[v] = lo[u] + 0.5 * cell, lo[v] + 0.5 * cell
    du[u], dv[v], dw[w] = cell, cell, 1.0
    return grid(origin, du, dv, dw, n[0], n[1]), float(hi[w] - lo[w])


def column_rays(g):
    """-> origins, dirs [nu * nv, 3] float32, row-major i + nu * j: (origin + (float)i * du) + (float)j * dv per component, and dw"""
    j, i = np.mgrid[0:g["nv"], 0:g["nu"]]
    i, j = i.ravel().astype(F)[:, None], j.ravel().astype(F)[:, None]
    with np.errstate(all="ignore"):
        o = (g["origin"][None, :] + i * g["du"][None, :]) + j * g["dv"][None, :]
    assert o.dtype == F
    return o, np.broadcast_to(g["dw"], o.shape).copy()


def tree64(x):
    """the pairwise tree over the last axis (64 long), level by level x[m] = x[2m] + x[2m + 1]"""
    assert x.shape[-1] == 64 and x.dtype == D
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def reduce_records(rec):
    """records [n, 10] float64 -> the one record: runs of 64 by index, the last padded with +0.0, each replaced by its tree sum, until
    one remains; a single record is its own result.  -> (record [10], passes)"""
    rec = np.ascontiguousarray(rec, D)
    passes = 0
    while len(rec) > 1:
        runs = -(-len(rec) // 64)
        padded = np.zeros((runs * 64, rec.shape[1]), D)
        padded[: len(rec)] = rec
        rec = tree64(padded.reshape(runs, 64, rec.shape[1]).transpose(0, 2, 1))
        passes += 1
    return rec[0].copy(), passes


def columns_of(S, spans):
    """the header's per-column sums over the spans in the order they close -> COLUMN_DTYPE [n], (t_lo, t_hi) float32 [n]"""
    assert (S["spans"] <= spans.shape[1]).all(), "every span must be stored"
    n = len(S)
    col = np.zeros(n, COLUMN_DTYPE)
    t_lo, t_hi = np.full(n, np.inf, F), np.full(n, -np.inf, F)
    for k in range(spans.shape[1]):
        m = S["spans"] > k
        if not m.any():
            break
        a, b = spans[m, k, 0].astype(D), spans[m, k, 1].astype(D)
        col["m0"][m] = col["m0"][m] + (b - a)
        col["m1"][m] = col["m1"][m] + D(0.5) * (b * b - a * a)
        col["m2"][m] = col["m2"][m] + ((b * b) * b - (a * a) * a) / D(3.0)
        t_lo[m] = np.minimum(t_lo[m], spans[m, k, 0])
        t_hi[m] = np.maximum(t_hi[m], spans[m, k, 1])
    for name in ("spans", "steps", "flags", "valid"):
        col[name] = S[name]
    return col, t_lo, t_hi


def reduce_columns(g, col, crossings, t_lo, t_hi):
    """the header's reduction of the columns [nu * nv] -> the result as a dict"""
    nu, nv = g["nu"], g["nv"]
    tu, tv = -(-nu // 8), -(-nv // 8)
    ok = (col["valid"] == 1).reshape(nv, nu)
    u, v = np.broadcast_to(np.arange(nu, dtype=D)[None, :], (nv, nu)), np.broadcast_to(np.arange(nv, dtype=D)[:, None], (nv, nu))
    m0, m1, m2 = (np.where(ok, col[k].reshape(nv, nu), D(0.0)) for k in ("m0", "m1", "m2"))
    contributions = [m0, u * m0, v * m0, m1, (u * u) * m0, (v * v) * m0, m2, (u * v) * m0, v * m1, u * m1]
    lanes = np.zeros((tv * 8, tu * 8, 10), D)
    lanes[:nv, :nu] = np.where(ok[..., None], np.stack(contributions, -1), D(0.0))
    # tile (ti, tj), lane (i & 7) + 8 * (j & 7); tiles row-major ti + tu * tj
    tiles = tree64(lanes.reshape(tv, 8, tu, 8, 10).transpose(0, 2, 4, 1, 3).reshape(tv * tu, 10, 64))
    moments, passes = reduce_records(tiles)
    hit = (col["spans"] >= 1).reshape(nv, nu)
    jj, ii = np.nonzero(hit)
    with_span = col["spans"] >= 1
    return dict(moments=moments, passes=passes, tiles=tiles,
                columns_hit=int(hit.sum()), columns_open=int(((col["flags"] & 3) != 0).sum()), columns_out_of_steps=int(((col["flags"] & 4) != 0).sum()),
                columns_invalid=int((col["valid"] != 1).sum()), steps=int(col["steps"].astype(np.int64).sum()), spans=int(col["spans"].astype(np.int64).sum()),
                crossings=int(np.asarray(crossings, np.int64).sum()),
                hit_lo=(int(ii.min()), int(jj.min())) if len(ii) else (nu, nv), hit_hi=(int(ii.max()), int(jj.max())) if len(ii) else (-1, -1),
                t_lo=F(t_lo[with_span].min()) if with_span.any() else F(np.inf), t_hi=F(t_hi[with_span].max()) if with_span.any() else F(-np.inf))


def measure(distance_fn, g, p, max_spans=8):
    """The header's definition.  distance_fn as for span_util.march_spans; p: span_util.params with the EFFECTIVE t_max (max_spans is
    set here: room for every span).  -> (result dict, columns COLUMN_DTYPE [nv, nu])"""
    o, d = column_rays(g)
    while True:
        S, spans = su.march_spans(distance_fn, o, d, dict(p, max_spans=max_spans))
        if S["spans"].max(initial=0) <= max_spans:
            break
        max_spans = int(S["spans"].max())
    col, t_lo, t_hi = columns_of(S, spans)
    res = reduce_columns(g, col, S["crossings"], t_lo, t_hi)
    res["summaries"] = S
    return res, col.reshape(g["nv"], g["nu"])


def properties(g, res, density=1.0):
    """sdfr_measure_properties restated: Python floats are IEEE doubles and every operation below is separate, in the header's order"""
    M = [float(x) for x in res["moments"]]
    if not M[0] > 0.0:
        return dict(volume=0.0, mass=0.0, centroid=(0.0, 0.0, 0.0), inertia=(0.0,) * 6)
    A = [[float(g["du"][r]), float(g["dv"][r]), float(g["dw"][r])] for r in range(3)]
    cx, cy, cz = A[1][1] * A[2][2] - A[2][1] * A[1][2], A[2][1] * A[0][2] - A[0][1] * A[2][2], A[0][1] * A[1][2] - A[1][1] * A[0][2]
    det = (A[0][0] * cx + A[1][0] * cy) + A[2][0] * cz
    scale = abs(det)
    volume = M[0] * scale
    cu, cv, cw = M[1] / M[0], M[2] / M[0], M[3] / M[0]
    centroid = tuple(((float(g["origin"][r]) + cu * A[r][0]) + cv * A[r][1]) + cw * A[r][2] for r in range(3))
    foot = M[0] / 12.0
    C = [[0.0] * 3 for _ in range(3)]
    C[0][0], C[1][1], C[2][2] = (M[4] - cu * M[1]) + foot, (M[5] - cv * M[2]) + foot, M[6] - cw * M[3]
    C[0][1] = C[1][0] = M[7] - cu * M[2]
    C[1][2] = C[2][1] = M[8] - cv * M[3]
    C[2][0] = C[0][2] = M[9] - cw * M[1]
    T = [[(C[k][0] * A[s][0] + C[k][1] * A[s][1]) + C[k][2] * A[s][2] for s in range(3)] for k in range(3)]
    P = [[(A[r][0] * T[0][s] + A[r][1] * T[1][s]) + A[r][2] * T[2][s] for s in range(3)] for r in range(3)]
    k = float(density) * scale
    inertia = (k * (P[1][1] + P[2][2]), k * (P[2][2] + P[0][0]), k * (P[0][0] + P[1][1]), -(k * P[0][1]), -(k * P[1][2]), -(k * P[2][0]))
    return dict(volume=volume, mass=float(density) * volume, centroid=centroid, inertia=inertia)


def bits64(x):
    return np.ascontiguousarray(x, D).view(np.uint64)


def assert_same_result(what, got, want):
    """got: anything with the fields of sdfr_measure_result as attributes or keys; want: reduce_columns' dict"""
    get = (lambda n: got[n]) if isinstance(got, dict) else (lambda n: getattr(got, n))
    gm, wm = bits64(list(get("moments"))), bits64(want["moments"])
    assert (gm == wm).all(), (what, "moments", list(get("moments")), list(want["moments"]))
    for name in INTEGERS:
        assert int(get(name)) == want[name], (what, name, int(get(name)), want[name])
    assert tuple(get("hit_lo")) == tuple(want["hit_lo"]) and tuple(get("hit_hi")) == tuple(want["hit_hi"]), (what, tuple(get("hit_lo")), tuple(get("hit_hi")), want["hit_lo"], want["hit_hi"])
    for name in ("t_lo", "t_hi"):
        assert F(get(name)).view(np.uint32) == F(want[name]).view(np.uint32), (what, name, get(name), want[name])


def assert_same_columns(what, got, want):
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    assert got.dtype == COLUMN_DTYPE and want.dtype == COLUMN_DTYPE and got.shape == want.shape, what
    qu.assert_same("%s columns" % (what,), got.view(np.uint32).reshape(-1, 10), want.view(np.uint32).reshape(-1, 10))


# ---- the library's stage functions on the CPU ------------------------------------------------------------------------------------
class HostGrid(ctypes.Structure):  # sdfr::MeasureGrid = sdfr_measure_grid
    _fields_ = [("origin", ctypes.c_float * 3), ("du", ctypes.c_float * 3), ("dv", ctypes.c_float * 3), ("dw", ctypes.c_float * 3), ("nu", ctypes.c_int32), ("nv", ctypes.c_int32)]


class HostResult(ctypes.Structure):  # sdfr::MeasureResult = sdfr_measure_result
    _fields_ = [("moments", ctypes.c_double * 10), ("columns_hit", ctypes.c_int64), ("columns_open", ctypes.c_int64), ("columns_out_of_steps", ctypes.c_int64),
                ("columns_invalid", ctypes.c_int64), ("steps", ctypes.c_int64), ("spans", ctypes.c_int64), ("crossings", ctypes.c_int64),
                ("hit_lo", ctypes.c_int32 * 2), ("hit_hi", ctypes.c_int32 * 2), ("t_lo", ctypes.c_float), ("t_hi", ctypes.c_float)]


class HostProperties(ctypes.Structure):  # sdfr::SolidProperties = sdfr_solid_properties
    _fields_ = [("volume", ctypes.c_double), ("mass", ctypes.c_double), ("centroid", ctypes.c_double * 3), ("inertia", ctypes.c_double * 6)]


_host = None


def host_lib():
    global _host
    if _host is None:
        L = ctypes.CDLL(cppbuild.csrc_lib("measure_host", os.path.join(cppbuild.HERE, "cpp", "measure_host.cpp")))
        assert [L.msh_sizes(k) for k in range(4)] == [ctypes.sizeof(HostGrid), 40, ctypes.sizeof(HostResult), ctypes.sizeof(HostProperties)] == [56, 40, 160, 88]
        vp = ctypes.c_void_p
        L.msh_measure_slabs.argtypes = [ctypes.POINTER(HostGrid), ctypes.POINTER(su.HostParams), ctypes.c_int, vp, vp, ctypes.c_float, ctypes.c_float, vp, vp, ctypes.POINTER(HostResult)]
        L.msh_measure_sphere.argtypes = [ctypes.POINTER(HostGrid), ctypes.POINTER(su.HostParams), vp, ctypes.c_float, vp, vp, ctypes.POINTER(HostResult)]
        L.msh_reduce_records.argtypes = [vp, ctypes.c_int64]
        L.msh_properties.argtypes = [ctypes.POINTER(HostGrid), ctypes.POINTER(HostResult), ctypes.c_double, ctypes.POINTER(HostProperties)]
        L.msh_properties.restype = None
        L.msh_order_key.argtypes, L.msh_order_key.restype = [ctypes.c_float], ctypes.c_uint32
        L.msh_order_value.argtypes, L.msh_order_value.restype = [ctypes.c_uint32], ctypes.c_float
        _host = L
    return _host


def host_grid(g, cls=HostGrid):
    f3 = lambda a: (ctypes.c_float * 3)(*[float(x) for x in a])  # noqa: E731
    return cls(f3(g["origin"]), f3(g["du"]), f3(g["dv"]), f3(g["dw"]), g["nu"], g["nv"])


def host_result(res, cls=HostResult):
    out = cls()
    out.moments[:] = [float(x) for x in res["moments"]]
    return out


def _host_measure(fn, g, p, *field):
    hp = su.HostParams(p["t_max"], p["min_step"], p["iso"], p["max_steps"], 0)
    n = g["nu"] * g["nv"]
    col, extras, out = np.zeros(n, COLUMN_DTYPE), np.zeros((n, 3), np.uint32), HostResult()
    assert fn(ctypes.byref(host_grid(g)), ctypes.byref(hp), *field, qu._p(col), qu._p(extras), ctypes.byref(out)) == 0
    return out, col.reshape(g["nv"], g["nu"]), extras


def host_measure_slabs(g, p, c, r, nan_lo, nan_hi):
    c, r = np.ascontiguousarray(c, F), np.ascontiguousarray(r, F)
    return _host_measure(host_lib().msh_measure_slabs, g, p, len(c), qu._p(c), qu._p(r), float(nan_lo), float(nan_hi))


def host_measure_sphere(g, p, centre, radius):
    centre = np.ascontiguousarray(centre, F)
    return _host_measure(host_lib().msh_measure_sphere, g, p, qu._p(centre), float(radius))


def host_reduce_records(rec):
    rec = np.ascontiguousarray(rec, D).copy()
    passes = host_lib().msh_reduce_records(qu._p(rec), len(rec))
    return rec[0].copy(), passes


def host_properties(g, res, density):
    out = HostProperties()
    host_lib().msh_properties(ctypes.byref(host_grid(g)), ctypes.byref(host_result(res)), float(density), ctypes.byref(out))
    return dict(volume=out.volume, mass=out.mass, centroid=tuple(out.centroid), inertia=tuple(out.inertia))


def sphere_field(centre, radius):
    """tests/cpp's Sphere, operation for operation in float32"""
    c, radius = np.asarray(centre, F), F(radius)

    def distance(p):
        x, y, z = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
        return (np.sqrt((x * x + y * y) + z * z) - radius).astype(F)

    return distance

"""Shared by the slice tests (test_slice_cpu.py, test_gpu_slice.py): the definition of sdfr_slice_extract (include/sdfr.h) restated in
numpy from the header's words, np.float32 operations only; the library's stage functions built for the CPU (tests/cpp/slice_host.cpp);
and the checks every result has to pass.  Test infrastructure: the product never imports this."""
import ctypes
import os

import numpy as np

import cppbuild
import query_util as qu

F = np.float32
# the boxes of the GPU tier's slice and span tests, per scene: time, the low corner (x, z), the cell, the height of layer 0 and the
# step between layers -- a box the scene's solid crosses in every layer
CASES = {"fast_sphere": (0.0, (-0.92, -0.72), 0.05, 0.62, 0.17), "labyrinth": (1.25, (-5.35, -2.55), 0.05, 0.37, 0.23),
         "gyroid": (0.5, (-0.92, -0.72), 0.05, -0.2, 0.23), "sierpinski": (0.5, (-0.75, -0.55), 0.04, 1.02, 0.11),
         "noise_lod": (0.5, (-0.92, -0.72), 0.05, 0.4, 0.4)}


def _f3(v):
    return np.asarray(v, np.float32).reshape(3)


def lattice_points(origin, du, dv, dw, dims, layers):
    """[points, 3] in the order of the linear index i + (nu + 1) * (j + (nv + 1) * l):
    ((origin + (float)i * du) + (float)j * dv) + (float)l * dw per component, every operation in fp32"""
    nu, nv = int(dims[0]), int(dims[1])
    l, j, i = np.meshgrid(np.arange(layers), np.arange(nv + 1), np.arange(nu + 1), indexing="ij")
    i, j, l = (a.ravel().astype(np.float32) for a in (i, j, l))
    o, du, dv, dw = _f3(origin), _f3(du), _f3(dv), _f3(dw)
    return np.stack([((o[c] + i * du[c]) + j * dv[c]) + l * dw[c] for c in range(3)], 1).astype(np.float32)


def marching_squares(D, origin, du, dv, dw, dims, layers, iso):
    """The header's definition.  D: the distances at lattice_points().  -> positions [v, 3] float32, coords [v, 2] float32,
    segments [s, 2] uint32, layer_vertices [layers + 1] int64, layer_segments [layers + 1] int64"""
    nu, nv, layers = int(dims[0]), int(dims[1]), int(layers)
    shape = (layers, nv + 1, nu + 1)  # [l, j, i]
    P = lattice_points(origin, du, dv, dw, dims, layers).reshape(shape + (3,))
    with np.errstate(invalid="ignore"):
        s = (np.asarray(D, np.float32) - F(iso)).reshape(shape)
        inside = s < 0  # NaN: outside
    J, I = np.meshgrid(np.arange(nv + 1), np.arange(nu + 1), indexing="ij")
    I, J = np.broadcast_to(I, shape).astype(np.float32), np.broadcast_to(J, shape).astype(np.float32)

    # vertices: the u-edge of a point, then its v-edge, points in linear order
    has = np.zeros((2,) + shape, bool)
    has[0][:, :, :nu] = inside[:, :, :-1] != inside[:, :, 1:]
    has[1][:, :nv, :] = inside[:, :-1, :] != inside[:, 1:, :]
    per_point = has[0].astype(np.int64) + has[1]
    first = (np.cumsum(per_point.ravel()) - per_point.ravel()).reshape(shape)
    index = np.stack([first, first + has[0]])  # [edge axis][l, j, i]
    total = int(per_point.sum())
    pos, uv = np.zeros((total, 3), np.float32), np.zeros((total, 2), np.float32)
    for axis in range(2):
        # the upper endpoint's values, rolled onto the lower endpoint (what wraps around is masked by `has`)
        sb, Pb = np.roll(s, -1, 2 - axis), np.roll(P, -1, 2 - axis)
        with np.errstate(all="ignore"):
            t = s / (s - sb)
            t = np.where((t >= 0) & (t <= 1), t, F(0.5)).astype(np.float32)
            p = P + t[..., None] * (Pb - P)
        m = has[axis]
        pos[index[axis][m]] = p[m]
        uv[index[axis][m], 0] = (I + t)[m] if axis == 0 else I[m]
        uv[index[axis][m], 1] = J[m] if axis == 0 else (J + t)[m]

    # segments: cells in linear order, in a cell by OUT side
    def corner(a, di, dj):
        return a[:, dj:dj + nv, di:di + nu]

    offs = ((0, 0), (1, 0), (1, 1), (0, 1))  # c0 .. c3, counter-clockwise
    sk = [corner(s, di, dj) for di, dj in offs]
    ik = [corner(inside, di, dj) for di, dj in offs]
    out = np.stack([ik[k] & ~ik[(k + 1) % 4] for k in range(4)], -1)  # [l, j, i, side]
    into = np.stack([~ik[k] & ik[(k + 1) % 4] for k in range(4)], -1)
    # the vertex on each side: side 0 the u-edge of (i, j), 1 the v-edge of (i + 1, j), 2 the u-edge of (i, j + 1), 3 the v-edge of (i, j)
    side_vertex = np.stack([corner(index[0], 0, 0), corner(index[1], 1, 0), corner(index[0], 0, 1), corner(index[1], 0, 0)], -1)
    n_out = out.sum(-1)
    assert (n_out == into.sum(-1)).all() and n_out.max(initial=0) <= 2
    with np.errstate(all="ignore"):
        m = ((sk[0] + sk[1]) + (sk[2] + sk[3])) * F(0.25)
        centre_inside = m < 0  # NaN is not
    the_in = np.argmax(into, -1)  # where there is one IN side: that one
    partner = np.empty(out.shape, np.int64)
    for k in range(4):
        partner[..., k] = np.where(n_out == 2, np.where(centre_inside, (k + 1) % 4, (k + 3) % 4), the_in)
    start = side_vertex
    end = np.take_along_axis(side_vertex, partner, -1)
    seg = np.stack([start[out], end[out]], 1).astype(np.uint32)  # boolean selection in C order: cell by cell, then side by side

    layer_v = np.concatenate([[0], np.cumsum(per_point.reshape(layers, -1).sum(1))]).astype(np.int64)
    layer_s = np.concatenate([[0], np.cumsum(n_out.reshape(layers, -1).sum(1))]).astype(np.int64)
    return pos, uv, seg, layer_v, layer_s


# ---- the library's stage functions on the CPU ------------------------------------------------------------------------------------
class HostGrid(ctypes.Structure):  # sdfr::SliceGrid
    _fields_ = [("origin", ctypes.c_float * 3), ("du", ctypes.c_float * 3), ("dv", ctypes.c_float * 3), ("dw", ctypes.c_float * 3),
                ("nu", ctypes.c_int32), ("nv", ctypes.c_int32), ("layers", ctypes.c_int32), ("iso", ctypes.c_float)]


_host = None


def host_lib():
    global _host
    if _host is None:
        L = ctypes.CDLL(cppbuild.csrc_lib("slice_host", os.path.join(cppbuild.HERE, "cpp", "slice_host.cpp")))
        assert L.sh_grid_size() == ctypes.sizeof(HostGrid) == 64
        vp = ctypes.c_void_p
        L.sh_extract.argtypes = [ctypes.POINTER(HostGrid), vp, ctypes.c_int64, ctypes.c_int64, vp, vp, vp, vp, vp, vp]
        L.sh_points.argtypes = [ctypes.POINTER(HostGrid), vp]
        L.sh_points.restype = None
        _host = L
    return _host


def host_grid(origin, du, dv, dw, dims, layers, iso):
    f3 = lambda v: (ctypes.c_float * 3)(*[float(x) for x in v])  # noqa: E731
    return HostGrid(f3(origin), f3(du), f3(dv), f3(dw), int(dims[0]), int(dims[1]), int(layers), float(iso))


def host_points(origin, du, dv, dw, dims, layers):
    g = host_grid(origin, du, dv, dw, dims, layers, 0.0)
    out = np.empty(((dims[0] + 1) * (dims[1] + 1) * layers, 3), np.float32)
    host_lib().sh_points(ctypes.byref(g), qu._p(out))
    return out


def host_extract(D, origin, du, dv, dw, dims, layers, iso, coords=True):
    """counting call, then filling call -> positions, coords, segments, layer_vertices, layer_segments"""
    L = host_lib()
    g = host_grid(origin, du, dv, dw, dims, layers, iso)
    D = np.ascontiguousarray(D, np.float32)
    counts, lv, ls = np.zeros(2, np.int64), np.zeros(layers + 1, np.int64), np.zeros(layers + 1, np.int64)
    assert L.sh_extract(ctypes.byref(g), qu._p(D), 0, 0, None, None, None, qu._p(lv), qu._p(ls), qu._p(counts)) == 0
    pos = np.empty((counts[0], 3), np.float32)
    uv = np.empty((counts[0], 2), np.float32) if coords else None
    seg = np.empty((counts[1], 2), np.uint32)
    if counts[0]:
        assert L.sh_extract(ctypes.byref(g), qu._p(D), counts[0], counts[1], qu._p(pos), qu._p(uv) if coords else None, qu._p(seg), qu._p(lv), qu._p(ls),
                            qu._p(counts)) == 0
    return pos, uv, seg, lv, ls


# ---- what every result has to pass -----------------------------------------------------------------------------------------------
def vertex_edges(D, dims, layers, iso):
    """per vertex, in the vertices' order: (axis of its edge -- 0: u, 1: v --, i, j of the point that owns the edge)"""
    nu, nv = dims
    shape = (layers, nv + 1, nu + 1)
    with np.errstate(invalid="ignore"):
        inside = (np.asarray(D, np.float32) - F(iso)).reshape(shape) < 0
    has = np.zeros(shape + (2,), bool)  # [l, j, i, axis]: C order is the vertices' order
    has[:, :, :nu, 0] = inside[:, :, :-1] != inside[:, :, 1:]
    has[:, :nv, :, 1] = inside[:, :-1, :] != inside[:, 1:, :]
    _l, j, i, axis = np.nonzero(has)
    return axis, i, j


def check_invariants(D, iso, uv, seg, layer_v, layer_s, dims, layers):
    """Every vertex is used; a vertex on an edge interior to its layer starts exactly one segment and ends exactly one, a vertex on a
    layer's border edge has exactly one use; no segment crosses a layer; the layer arrays are the running counts"""
    nu, nv = dims
    n = len(uv)
    seg = np.asarray(seg, np.int64).reshape(-1, 2)
    assert layer_v[0] == 0 and layer_s[0] == 0 and layer_v[-1] == n and layer_s[-1] == len(seg)
    assert len(layer_v) == len(layer_s) == layers + 1 and (np.diff(layer_v) >= 0).all() and (np.diff(layer_s) >= 0).all()
    assert seg.min(initial=0) >= 0 and seg.max(initial=-1) < n
    starts, ends = np.bincount(seg[:, 0], minlength=n), np.bincount(seg[:, 1], minlength=n)
    axis, i, j = vertex_edges(D, dims, layers, iso)
    assert len(axis) == n
    border = np.where(axis == 0, (j == 0) | (j == nv), (i == 0) | (i == nu))  # a u-edge on the first or last row, a v-edge on the first or last column
    assert ((starts + ends) >= 1).all(), "a vertex no segment uses"
    assert (starts[~border] == 1).all() and (ends[~border] == 1).all()
    assert ((starts + ends)[border] == 1).all()
    layer_of_vertex = np.searchsorted(layer_v, np.arange(n), side="right") - 1
    layer_of_segment = np.searchsorted(layer_s, np.arange(len(seg)), side="right") - 1
    assert (layer_of_vertex[seg[:, 0]] == layer_of_segment).all() and (layer_of_vertex[seg[:, 1]] == layer_of_segment).all()


def shoelace(uv, chain):
    """the signed area of a closed chain in lattice units: positive counter-clockwise"""
    p = np.asarray(uv, np.float64)[chain]
    q = np.roll(p, -1, 0)
    return 0.5 * float((p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]).sum())

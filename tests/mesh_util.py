"""Shared by the mesh tests (test_mesh_cpu.py, test_gpu_mesh.py): the definition of sdfr_mesh_extract (include/sdfr.h) restated in
numpy from the header's words, np.float32 operations only; the library's stage functions built for the CPU (tests/cpp/mesh_host.cpp);
the lattice points; and the topology checks.  Test infrastructure: the product never imports this."""
import ctypes

import numpy as np

import cppbuild
import query_util as qu

F = np.float32


def lattice_axes(origin, cell, dims):
    """per axis: origin + (float)i * cell -- one multiply, then one add, in fp32"""
    return [F(origin[a]) + np.arange(dims[a] + 1, dtype=np.float32) * F(cell) for a in range(3)]


def lattice_points(origin, cell, dims):
    """[points, 3] in the order of the linear index i + (nx + 1) * (j + (ny + 1) * k)"""
    x, y, z = lattice_axes(origin, cell, dims)
    k, j, i = np.meshgrid(np.arange(dims[2] + 1), np.arange(dims[1] + 1), np.arange(dims[0] + 1), indexing="ij")
    return np.stack([x[i.ravel()], y[j.ravel()], z[k.ravel()]], 1).astype(np.float32)


def surface_nets(D, origin, cell, dims, iso):
    """The header's definition.  D: the distances at lattice_points().  -> positions [v, 3] float32, indices [t, 3] uint32."""
    n = [int(d) for d in dims]
    shape = (n[2] + 1, n[1] + 1, n[0] + 1)  # [k, j, i]
    with np.errstate(invalid="ignore"):
        s = (np.asarray(D, np.float32) - F(iso)).reshape(shape)
        inside = s < 0  # NaN: outside
    axes = lattice_axes(origin, cell, dims)

    def corner(a, d):
        """array `a` over the lattice, at offset d = (di, dj, dk) from every cell"""
        return a[d[2]:d[2] + n[2], d[1]:d[1] + n[1], d[0]:d[0] + n[0]]

    def coord(axis, off):
        """coordinate `axis` of the points at offset `off` on that axis from every cell, broadcast over the cells"""
        sh = [1, 1, 1]
        sh[2 - axis] = n[axis]
        return np.broadcast_to(axes[axis][off:off + n[axis]].reshape(sh), (n[2], n[1], n[0]))

    # active cells and their vertex indices
    count = np.zeros((n[2], n[1], n[0]), np.int32)
    for c in range(8):
        count += corner(inside, (c & 1, (c >> 1) & 1, c >> 2))
    active = (count > 0) & (count < 8)
    vertex_of = (np.cumsum(active.ravel()) - active.ravel()).reshape(active.shape)  # exclusive: consecutive in linear order
    # vertex positions: the running sum over the 12 edges in the header's order
    total = [np.zeros(active.shape, np.float32) for _ in range(3)]
    crossings = np.zeros(active.shape, np.int32)
    for axis in range(3):
        b, c = [(1, 2), (0, 2), (0, 1)][axis]
        for e in range(4):
            da = [0, 0, 0]
            da[b], da[c] = e & 1, e >> 1
            db = list(da)
            db[axis] += 1
            sa, sb = corner(s, da), corner(s, db)
            with np.errstate(all="ignore"):
                cross = (sa < 0) != (sb < 0)
                t = sa / (sa - sb)
                p = [coord(m, da[m]) for m in range(3)]
                p[axis] = p[axis] + t * (coord(axis, db[axis]) - p[axis])
                for m in range(3):
                    total[m] = np.where(cross, total[m] + p[m], total[m])
            crossings += cross
    with np.errstate(all="ignore"):
        pos = np.stack([(total[m] / crossings.astype(np.float32))[active] for m in range(3)], 1).astype(np.float32)
    # quads: per lattice point in linear order, then axis x, y, z
    K, J, I = np.meshgrid(np.arange(n[2] + 1), np.arange(n[1] + 1), np.arange(n[0] + 1), indexing="ij")
    P = [I, J, K]
    emits = np.zeros(shape + (3,), bool)
    tris = np.zeros(shape + (3, 6), np.int64)
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        ok = (P[a] < n[a]) & (P[b] >= 1) & (P[b] <= n[b] - 1) & (P[c] >= 1) & (P[c] <= n[c] - 1)
        Q = list(P)
        Q[a] = np.minimum(P[a] + 1, n[a])
        emits[..., a] = ok & (inside != inside[Q[2], Q[1], Q[0]])
        q = []
        for ob, oc in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            C = list(P)
            C[b] = np.clip(P[b] + ob, 0, n[b] - 1)
            C[c] = np.clip(P[c] + oc, 0, n[c] - 1)
            C[a] = np.minimum(P[a], n[a] - 1)
            q.append(vertex_of[C[2], C[1], C[0]])
        fwd = np.stack([q[0], q[1], q[2], q[0], q[2], q[3]], -1)
        rev = np.stack([q[3], q[2], q[1], q[3], q[1], q[0]], -1)
        tris[..., a, :] = np.where(inside[..., None], fwd, rev)
    idx = tris.reshape(-1, 6)[emits.ravel()].reshape(-1, 3).astype(np.uint32)
    return pos, idx


# ---- the library's stage functions on the CPU ------------------------------------------------------------------------------------
class HostGrid(ctypes.Structure):  # sdfr::MeshGrid
    _fields_ = [("origin", ctypes.c_float * 3), ("cell", ctypes.c_float), ("n", ctypes.c_int32 * 3), ("iso", ctypes.c_float)]


_host = None


def host_lib():
    global _host
    if _host is None:
        L = ctypes.CDLL(qu.build_lib("mesh_host", "mesh_host.cpp", ["-I" + qu.CSRC], cppbuild.csrc_headers()))
        assert L.mh_grid_size() == ctypes.sizeof(HostGrid)
        vp = ctypes.c_void_p
        L.mh_extract.argtypes = [ctypes.POINTER(HostGrid), vp, ctypes.c_int64, ctypes.c_int64, vp, vp, vp]
        _host = L
    return _host


def host_extract(D, origin, cell, dims, iso):
    """counting call, then filling call -> positions, indices"""
    L = host_lib()
    g = HostGrid((ctypes.c_float * 3)(*[float(v) for v in origin]), float(cell), (ctypes.c_int32 * 3)(*[int(d) for d in dims]), float(iso))
    D = np.ascontiguousarray(D, np.float32)
    counts = np.zeros(2, np.int64)
    assert L.mh_extract(ctypes.byref(g), qu._p(D), 0, 0, None, None, qu._p(counts)) == 0
    pos = np.empty((counts[0], 3), np.float32)
    idx = np.empty((counts[1], 3), np.uint32)
    if counts[0]:
        assert L.mh_extract(ctypes.byref(g), qu._p(D), counts[0], counts[1], qu._p(pos), qu._p(idx), qu._p(counts)) == 0
    return pos, idx


# ---- topology --------------------------------------------------------------------------------------------------------------------
def directed_edges(idx):
    t = np.asarray(idx, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def check_closed_oriented(idx, n_vertices, euler):
    """every undirected edge in exactly two triangles, every directed edge (a, b) matched by one (b, a), V - E + F = euler"""
    e = directed_edges(idx)
    assert (e[:, 0] != e[:, 1]).all()
    key = e[:, 0] * n_vertices + e[:, 1]
    back = e[:, 1] * n_vertices + e[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    assert (cnt == 1).all(), "a directed edge is used twice"
    assert np.array_equal(uniq, np.unique(back)), "a directed edge has no opposite"
    und = np.minimum(e[:, 0], e[:, 1]) * n_vertices + np.maximum(e[:, 0], e[:, 1])
    _, ucnt = np.unique(und, return_counts=True)
    assert (ucnt == 2).all()
    assert len(np.unique(idx)) == n_vertices, "a vertex no triangle uses"
    assert n_vertices - len(ucnt) + len(idx) == euler


def face_normals_and_centroids(pos, idx):
    p = np.asarray(pos, np.float64)
    a, b, c = p[idx[:, 0]], p[idx[:, 1]], p[idx[:, 2]]
    return np.cross(b - a, c - a), (a + b + c) / 3.0


# ---- the two analytic scenes of the topology tests ---------------------------------------------------------------------------------
# exact 1-Lipschitz distances, centred off the lattice so that no lattice point sits on the surface; cell 1/8, boxes with more than
# three cells of margin on every side
CENTRE = (0.03, 0.05, 0.07)
TOPOLOGY = {
    # name: (origin, cell, dims, Euler characteristic)
    "sphere": ((-1.5, -1.5, -1.5), 0.125, (24, 24, 24), 2),   # radius 1
    "torus": ((-2.0, -1.0, -2.0), 0.125, (32, 16, 32), 0),    # R = 1, r = 0.4, axis y
}


def analytic_distance(name, p):
    q = np.asarray(p, np.float64) - np.array(CENTRE)
    if name == "sphere":
        return np.linalg.norm(q, axis=1) - 1.0
    return np.hypot(np.hypot(q[:, 0], q[:, 2]) - 1.0, q[:, 1]) - 0.4


def analytic_normal(name, p):
    q = np.asarray(p, np.float64) - np.array(CENTRE)
    if name == "torus":
        ring = np.hypot(q[:, 0], q[:, 2])[:, None]
        q = q - np.stack([q[:, 0], np.zeros(len(q)), q[:, 2]], 1) / ring
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def check_surface(name, pos, idx, cell, distance, normal_at):
    """the conditions of a closed, outward-oriented mesh near the surface.  distance: at the vertices; normal_at(points): the
    scene's normals"""
    check_closed_oriented(idx, len(pos), TOPOLOGY[name][3])
    fn, fc = face_normals_and_centroids(pos, idx)
    solid = np.linalg.norm(fn, axis=1) > 0
    assert solid.any() and ((fn[solid] * np.asarray(normal_at(fc[solid]), np.float64)).sum(1) > 0).all()
    assert (np.abs(distance) <= np.sqrt(3.0) * cell).all()

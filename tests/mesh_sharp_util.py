"""Shared by the sharp-mesh tests (test_mesh_sharp_cpu.py, test_gpu_mesh_sharp.py): the definition of sdfr_mesh_extract_sharp
(include/sdfr.h) restated in numpy from the header's words -- np.float32 operations only, in the stated order, vectorised over the
vertices and fed by a distance-and-normal function --, the library's stage functions built for the CPU with the scene bound to a
callback (tests/cpp/mesh_sharp_host.cpp), the analytic scenes of that file, and the geometry measures.  Test infrastructure: the
product never imports this."""
import ctypes
import os
import subprocess

import numpy as np

import cppbuild
import mesh_util as mu
import query_util as qu

F = np.float32

# the grid of the CPU tier: cell 1/8, the analytic shapes centred at (0.03, 0.05, 0.07), off the lattice
GRID = ((-0.75, -0.6, -0.65), 0.125, (12, 10, 11))
BOX_CENTRE = np.array([0.03, 0.05, 0.07])
BOX_HALF = np.array([0.6, 0.45, 0.5])
ANALYTIC = {"box": 0, "rotated_box": 1, "sphere": 2, "torus": 3, "cliff": 4}  # msh_analytic's scenes


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def sharp_nets(D, origin, cell, dims, iso, f):
    """The header's definition of the vertices.  D: the distances at mesh_util.lattice_points(); f(points [n, 3] float32, normals: bool) ->
    (distance [n] float32, normals [n, 3] float32 or None), what sdfr_query_distance returns.  -> positions [v, 3] float32 and a dict:
    cells [v, 3] (i, j, k of each vertex's cell), m (the mass points), lo / hi (the clamp's bounds), planes (c per vertex), crossings."""
    n = [int(d) for d in dims]
    iso = F(iso)
    shape = (n[2] + 1, n[1] + 1, n[0] + 1)  # [k, j, i]
    with np.errstate(invalid="ignore"):
        s_lat = (np.asarray(D, np.float32) - iso).reshape(shape)
        inside = s_lat < 0
    axes = mu.lattice_axes(origin, cell, dims)
    count = np.zeros((n[2], n[1], n[0]), np.int32)
    for c in range(8):
        d = (c & 1, (c >> 1) & 1, c >> 2)
        count += inside[d[2]:d[2] + n[2], d[1]:d[1] + n[1], d[0]:d[0] + n[0]]
    kji = np.argwhere((count > 0) & (count < 8))  # in the order of the cells' linear index
    cells = kji[:, ::-1].copy()                   # (i, j, k)
    V = len(cells)
    cross = np.zeros((12, V), bool)
    plane = np.zeros((12, V), bool)
    P, N, S = np.zeros((12, V, 3), np.float32), np.zeros((12, V, 3), np.float32), np.zeros((12, V), np.float32)
    half = F(0.5)
    with np.errstate(all="ignore"):
        for e in range(12):
            axis = e >> 2
            b, c = [(1, 2), (0, 2), (0, 1)][axis]
            A = [cells[:, 0].copy(), cells[:, 1].copy(), cells[:, 2].copy()]
            A[b] += e & 1
            A[c] += (e >> 1) & 1
            B = [a.copy() for a in A]
            B[axis] += 1
            s_lo, s_hi = s_lat[A[2], A[1], A[0]], s_lat[B[2], B[1], B[0]]
            sel = np.nonzero((s_lo < 0) != (s_hi < 0))[0]
            if not len(sel):
                continue
            s_lo, s_hi = s_lo[sel], s_hi[sel]
            p = np.stack([axes[m][A[m][sel]] for m in range(3)], 1).astype(np.float32)
            pa, pb = p[:, axis].copy(), axes[axis][B[axis][sel]]
            lo, hi = np.zeros(len(sel), np.float32), np.ones(len(sel), np.float32)
            for _ in range(4):
                mid = half * (lo + hi)
                p[:, axis] = pa + mid * (pb - pa)
                s = f(p.copy(), False)[0].astype(np.float32) - iso
                same = (s < 0) == (s_lo < 0)
                lo, s_lo = np.where(same, mid, lo), np.where(same, s, s_lo)
                hi, s_hi = np.where(same, hi, mid), np.where(same, s_hi, s)
            t = lo + (s_lo / (s_lo - s_hi)) * (hi - lo)
            t = np.where((t >= lo) & (t <= hi), t, half * (lo + hi))
            p[:, axis] = pa + t * (pb - pa)
            d, nn = f(p.copy(), True)
            nn = np.asarray(nn, np.float32)
            si = np.asarray(d, np.float32) - iso
            cross[e, sel] = True
            plane[e, sel] = np.isfinite(nn).all(1) & np.isfinite(si) & ~(nn == 0).all(1)
            P[e, sel], N[e, sel], S[e, sel] = p, nn, si
        assert P.dtype == N.dtype == S.dtype == np.float32
        # the mass point
        m = np.zeros((V, 3), np.float32)
        for e in range(12):
            m = np.where(cross[e][:, None], m + P[e], m)
        m = m / cross.sum(0).astype(np.float32)[:, None]
        # the normal equations
        H = np.zeros((V, 3, 3), np.float32)
        G = np.zeros((V, 3), np.float32)
        for e in range(12):
            nn, pp = N[e], P[e]
            bi = ((nn[:, 0] * (pp[:, 0] - m[:, 0]) + nn[:, 1] * (pp[:, 1] - m[:, 1])) + nn[:, 2] * (pp[:, 2] - m[:, 2])) - S[e]
            for a in range(3):
                for b in range(a, 3):
                    H[:, a, b] = np.where(plane[e], H[:, a, b] + nn[:, a] * nn[:, b], H[:, a, b])
                G[:, a] = np.where(plane[e], G[:, a] + nn[:, a] * bi, G[:, a])
        planes = plane.sum(0)
        ridge = F(2.0 ** -8) * planes.astype(np.float32)
        for a in range(3):
            H[:, a, a] = H[:, a, a] + ridge
        H[:, 1, 0], H[:, 2, 0], H[:, 2, 1] = H[:, 0, 1], H[:, 0, 2], H[:, 1, 2]

        def dot(u, w):
            return (u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1]) + u[:, 2] * w[:, 2]

        # three steps of conjugate gradients from y = 0; a vertex that stops stays stopped
        y, r, d = np.zeros((V, 3), np.float32), G.copy(), G.copy()
        rr = dot(r, r)
        alive = planes > 0
        for _ in range(3):
            alive = alive & (rr > 0)
            Hd = np.stack([(H[:, a, 0] * d[:, 0] + H[:, a, 1] * d[:, 1]) + H[:, a, 2] * d[:, 2] for a in range(3)], 1)
            dHd = dot(d, Hd)
            alive = alive & (dHd > 0)
            alpha = rr / dHd
            go = alive[:, None]
            y = np.where(go, y + alpha[:, None] * d, y)
            r = np.where(go, r - alpha[:, None] * Hd, r)
            rr2 = dot(r, r)
            beta = rr2 / rr
            d = np.where(go, r + beta[:, None] * d, d)
            rr = np.where(alive, rr2, rr)
        x = m + y
        x = np.where(np.isfinite(x).all(1)[:, None], x, m)
        h = half * F(cell)
        lo = np.stack([axes[a][cells[:, a]] - h for a in range(3)], 1)
        hi = np.stack([axes[a][cells[:, a] + 1] + h for a in range(3)], 1)
        x = np.minimum(np.maximum(x, lo), hi)
    assert x.dtype == np.float32 and m.dtype == np.float32 and lo.dtype == np.float32
    return x, dict(cells=cells, m=m, lo=lo, hi=hi, planes=planes, crossings=cross.sum(0))


# ---- the library's stage functions on the CPU ------------------------------------------------------------------------------------
CALLBACK = ctypes.CFUNCTYPE(None, ctypes.POINTER(ctypes.c_float), ctypes.c_int, ctypes.POINTER(ctypes.c_float))
SOURCE = os.path.join(cppbuild.HERE, "cpp", "mesh_sharp_host.cpp")
_host = None


def host_lib():
    global _host
    if _host is None:
        L = ctypes.CDLL(qu.build_lib("mesh_sharp_host", "mesh_sharp_host.cpp", ["-I" + qu.CSRC], cppbuild.csrc_headers()))
        assert L.msh_grid_size() == ctypes.sizeof(mu.HostGrid)
        vp = ctypes.c_void_p
        L.msh_extract.argtypes = [ctypes.POINTER(mu.HostGrid), vp, CALLBACK, ctypes.c_int64, ctypes.c_int64, vp, vp, vp]
        L.msh_analytic.argtypes = [ctypes.c_int, ctypes.c_int64, vp, vp, vp]
        L.msh_analytic.restype = None
        _host = L
    return _host


def analytic(name):
    """f of sharp_nets for one of ANALYTIC: exact distances and normals, computed in double and rounded once"""
    scene = ANALYTIC[name]

    def f(points, normals):
        p = np.ascontiguousarray(points, np.float32)
        d = np.empty(len(p), np.float32)
        nn = np.empty((len(p), 3), np.float32) if normals else None
        host_lib().msh_analytic(scene, len(p), qu._p(p), qu._p(d), qu._p(nn) if normals else None)
        return d, nn

    return f


def host_extract(D, origin, cell, dims, iso, f):
    """the stand-in with f behind its callback: the counting call, then the filling call -> positions, indices"""
    L = host_lib()
    g = mu.HostGrid((ctypes.c_float * 3)(*[float(v) for v in origin]), float(cell), (ctypes.c_int32 * 3)(*[int(d) for d in dims]), float(iso))
    D = np.ascontiguousarray(D, np.float32)

    def one(p, want_normal, out):
        d, nn = f(np.array([[p[0], p[1], p[2]]], np.float32), bool(want_normal))
        out[0] = d[0]
        if want_normal:
            out[1], out[2], out[3] = nn[0]

    cb = CALLBACK(one)
    counts = np.zeros(2, np.int64)
    assert L.msh_extract(ctypes.byref(g), qu._p(D), cb, 0, 0, None, None, qu._p(counts)) == 0
    pos = np.empty((counts[0], 3), np.float32)
    idx = np.empty((counts[1], 3), np.uint32)
    if counts[0]:
        assert L.msh_extract(ctypes.byref(g), qu._p(D), cb, counts[0], counts[1], qu._p(pos), qu._p(idx), qu._p(counts)) == 0
    return pos, idx


def program(sanitize):
    """the stand-alone program of mesh_sharp_host.cpp, plain or under the address and undefined-behaviour sanitizers -> its path"""
    flags = cppbuild.EXACT_FLAGS + ["-w", "-DMESH_SHARP_MAIN", "-I" + qu.CSRC]
    if sanitize:
        flags += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    return cppbuild.compile(os.path.join(cppbuild.BUILD, "mesh_sharp_program" + ("_san" if sanitize else "")), [SOURCE], cppbuild.csrc_headers(), flags, shared=False)


def run_program(sanitize):
    """-> {scene: (positions, indices)} as the program wrote them"""
    raw = subprocess.run([program(sanitize)], check=True, stdout=subprocess.PIPE).stdout
    out, at = {}, 0
    for name, _k in sorted(ANALYTIC.items(), key=lambda kv: kv[1]):
        v, t = (int(c) for c in np.frombuffer(raw, np.int64, 2, at))
        at += 16
        pos = np.frombuffer(raw, np.float32, 3 * v, at).reshape(v, 3)
        at += 12 * v
        idx = np.frombuffer(raw, np.uint32, 3 * t, at).reshape(t, 3)
        at += 12 * t
        out[name] = (pos, idx)
    assert at == len(raw)
    return out


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
def box_corners():
    s = np.array([[(c & 1) * 2 - 1, ((c >> 1) & 1) * 2 - 1, (c >> 2) * 2 - 1] for c in range(8)], np.float64)
    return BOX_CENTRE[None] + s * BOX_HALF[None]


def triangles(pos, idx):
    """-> unit normals [t, 3], areas [t], centroids [t, 3], in float64"""
    fn, fc = mu.face_normals_and_centroids(pos, idx)
    length = np.linalg.norm(fn, axis=1)
    with np.errstate(all="ignore"):
        return fn / length[:, None], 0.5 * length, fc


def in_clamp(pos, info):
    return bool(((pos >= info["lo"]) & (pos <= info["hi"])).all())

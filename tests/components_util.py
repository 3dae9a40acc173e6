"""Shared by the component tests (test_components_cpu.py, test_gpu_components.py): the definition of sdfr_components_label
(include/sdfr.h) restated in numpy from the header's words; the library's union, rules and plan built for the CPU
(tests/cpp/components_host.cpp, tests/cpp/components_plan_host.cpp); the synthetic lattices; and the scenes and grids whose counts the
issue tables.  Test infrastructure: the product never imports this."""
import ctypes
import math
import os
import subprocess

import numpy as np

import cppbuild
import mesh_util as mu
import query_util as qu

F = np.float32
INSIDE, FACE_SHIFT, FACES = 1, 8, 0x3F00
COUNT_KEYS = ("components", "solids", "voids", "closed_solids", "closed_voids", "inside_points", "largest_solid_points", "largest_void_points")
RECORD_DTYPE = np.dtype([("root", np.uint32), ("flags", np.uint32), ("points", np.int64), ("lo", np.int32, (3,)), ("hi", np.int32, (3,))])
INVALID, NO_SCENE = -1, -4
NULL_POINTER, BAD_FLAG, BAD_GRID, NEGATIVE, NULL_ARRAY = "null pointer", "on_host must be 0 or 1", "bad mesh grid", "negative capacity", "null array with a capacity"


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def inside_of(D, iso):
    """[pz, py, px] bool: s = D - iso < 0 in float32 (NaN, and -0.0, are not inside)"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(D, np.float32) - F(iso)) < 0


def label(D, dims, iso=0.0):
    """sdfr_components_label's definition.  D: the distances at mesh_util.lattice_points(), in any shape.  -> (counts dict, records
    RECORD_DTYPE [C], labels uint32 [pz, py, px]).  Min-label hooking over the joined edges with full path compression between the
    rounds: a root is the smallest index of its class by construction."""
    px, py, pz = (int(n) + 1 for n in dims)
    inside = inside_of(np.asarray(D, np.float32).reshape(pz, py, px), iso)
    N = px * py * pz
    index = np.arange(N, dtype=np.int64).reshape(pz, py, px)
    ends = []
    for axis in range(3):  # the edges along k, j, i: both ends inside or both not
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        joined = inside[tuple(lo)] == inside[tuple(hi)]
        ends.append((index[tuple(lo)][joined], index[tuple(hi)][joined]))
    A, B = np.concatenate([e[0] for e in ends]), np.concatenate([e[1] for e in ends])
    parent = np.arange(N, dtype=np.int64)
    while True:
        ra, rb = parent[A], parent[B]
        differ = ra != rb
        if not differ.any():
            break
        np.minimum.at(parent, np.maximum(ra, rb)[differ], np.minimum(ra, rb)[differ])
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    roots = np.nonzero(parent == np.arange(N))[0]  # ascending
    number = np.zeros(N, np.int64)
    number[roots] = np.arange(len(roots))
    labels = number[parent]
    C = len(roots)
    records = np.zeros(C, RECORD_DTYPE)
    records["root"] = roots
    records["points"] = np.bincount(labels, minlength=C)
    k, j, i = np.unravel_index(np.arange(N), (pz, py, px))
    faces = np.zeros(N, np.uint32)
    for a, (c, last) in enumerate(((i, px - 1), (j, py - 1), (k, pz - 1))):
        faces |= np.where(c == 0, 1 << (FACE_SHIFT + 2 * a), 0).astype(np.uint32) | np.where(c == last, 1 << (FACE_SHIFT + 2 * a + 1), 0).astype(np.uint32)
        lo, hi = np.full(C, np.iinfo(np.int32).max, np.int64), np.full(C, -1, np.int64)
        np.minimum.at(lo, labels, c)
        np.maximum.at(hi, labels, c)
        records["lo"][:, a], records["hi"][:, a] = lo, hi
    flags = inside.reshape(-1)[roots].astype(np.uint32) * INSIDE
    np.bitwise_or.at(flags, labels, faces)
    records["flags"] = flags
    return counts_of(records), records, labels.astype(np.uint32).reshape(pz, py, px)


def counts_of(records):
    solid = (records["flags"] & INSIDE) != 0
    closed = (records["flags"] & FACES) == 0
    pts = records["points"]
    return dict(components=len(records), solids=int(solid.sum()), voids=int((~solid).sum()), closed_solids=int((solid & closed).sum()),
                closed_voids=int((~solid & closed).sum()), inside_points=int(pts[solid].sum()),
                largest_solid_points=int(pts[solid].max()) if solid.any() else 0, largest_void_points=int(pts[~solid].max()) if (~solid).any() else 0)


def assert_same(what, got, want):
    """(counts, records, labels) against the definition's, every field equal"""
    assert got[0] == want[0], (what, got[0], want[0])
    g = np.asarray(got[1])
    if g.dtype != RECORD_DTYPE:  # the device form: [C, 10] words
        g = np.ascontiguousarray(g).view(np.uint32).reshape(-1).view(RECORD_DTYPE)
    assert g.shape == want[1].shape, (what, g.shape, want[1].shape)
    for field in RECORD_DTYPE.names:
        assert np.array_equal(g[field], want[1][field]), (what, field)
    if got[2] is not None:
        assert np.array_equal(np.asarray(got[2]).view(np.uint32), want[2]), what


def fault(dims, iso=0.0, cell=1.0, capacity=0, grid=True, counts=True, lattice=True, records=False, on_host=1):
    """the text of the argument fault that wins, or None"""
    if not grid or not counts or not lattice:
        return NULL_POINTER
    if on_host not in (0, 1):
        return BAD_FLAG
    c = float(F(cell))
    if not (all(math.isfinite(float(F(v))) for v in (c, iso)) and c > 0 and all(1 <= n <= 1024 for n in dims) and (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1) <= 1 << 30):
        return BAD_GRID
    if capacity < 0:
        return NEGATIVE
    if capacity > 0 and not records:
        return NULL_ARRAY
    return None


# ---- the synthetic lattices, [pz, py, px] float32; None where the lattice is too small for the shape --------------------------------
SYNTHETIC = ("all_inside", "all_outside", "all_nan", "checkerboard", "serpentine", "comb", "hollow_box", "drilled_box", "diagonal", "noise", "zeros", "iso")
SYNTHETIC_DIMS = ((1, 1, 1), (7, 1, 1), (8, 8, 8), (33, 9, 5))  # cells: around the brick edges -- 9 points: a one-point slab of second bricks


def serpentine(shape):
    """one long thin solid: every second row of every second layer, the rows joined at alternating ends and the layers at alternating ends
    of the layer's path, so that the solid is one path"""
    pz, py, px = shape
    inside = np.zeros(shape, bool)
    rows = list(range(0, py, 2))
    end = (rows[-1], px - 1 if (len(rows) - 1) % 2 == 0 else 0)  # where a layer's path ends; it starts at (0, 0)
    for k in range(0, pz, 2):
        for r, j in enumerate(rows):
            inside[k, j, :] = True
            if j + 2 < py:
                inside[k, j + 1, px - 1 if r % 2 == 0 else 0] = True
        if k + 2 < pz:
            inside[(k + 1,) + (end if (k // 2) % 2 == 0 else (0, 0))] = True
    return inside


def synthetic(name, dims, seed=7):
    """-> (lattice, iso) or None"""
    shape = tuple(int(n) + 1 for n in reversed(dims))
    pz, py, px = shape
    k, j, i = np.indices(shape)
    iso = 0.0
    if name == "all_inside":
        D = np.full(shape, -1.0)
    elif name == "all_outside":
        D = np.full(shape, 1.0)
    elif name == "all_nan":
        D = np.full(shape, np.nan)
    elif name == "checkerboard":
        D = np.where((i + j + k) & 1, -1.0, 1.0)
    elif name == "serpentine":
        D = np.where(serpentine(shape), -0.5, 0.5)
    elif name == "comb":  # a spine with teeth in every second layer
        D = np.where(((j == 0) | (i % 2 == 0)) & (k % 2 == 0), -0.5, 0.5)
    elif name in ("hollow_box", "drilled_box"):
        if min(shape) < 6:
            return None
        box = (i >= 1) & (i <= px - 2) & (j >= 1) & (j <= py - 2) & (k >= 1) & (k <= pz - 2)
        cavity = (i >= 2) & (i <= px - 3) & (j >= 2) & (j <= py - 3) & (k >= 2) & (k <= pz - 3)
        solid = box & ~cavity
        if name == "drilled_box":
            solid[pz // 2, py // 2, 1] = False  # a one-point channel through the wall i = 1
        D = np.where(solid, -0.5, 0.5)
    elif name == "diagonal":  # two bodies that touch only across a lattice diagonal
        if min(shape) < 6:
            return None
        a = (i >= 1) & (i <= 2) & (j >= 1) & (j <= 2) & (k >= 1) & (k <= 2)
        b = (i >= 3) & (i <= 4) & (j >= 3) & (j <= 4) & (k >= 1) & (k <= 2)
        D = np.where(a | b, -0.5, 0.5)
    elif name == "noise":
        rng = np.random.default_rng(seed)
        D = np.where(rng.random(shape) < 0.5, -1.0, 1.0) * (0.25 + rng.random(shape))
    elif name == "zeros":  # -0.0 is not < 0
        rng = np.random.default_rng(seed + 1)
        D = np.array([-0.0, 0.0, -1e-30, 1e-30], np.float32)[rng.integers(0, 4, shape)]
    elif name == "iso":  # s == 0 exactly where D == iso
        rng = np.random.default_rng(seed + 2)
        D, iso = np.array([0.25, 0.5, 0.75], np.float32)[rng.integers(0, 3, shape)], 0.5
    else:
        raise KeyError(name)
    return np.ascontiguousarray(D, np.float32), iso


def synthetic_cases(dims_list=SYNTHETIC_DIMS):
    """[(name, dims)] of the lattices that exist"""
    return [(name, dims) for dims in dims_list for name in SYNTHETIC if synthetic(name, dims) is not None]


# ---- the scenes and grids whose counts the issue tables: (scene, time, origin, cell, dims, iso, variables) -> what must come out ------
W, H = 64, 48
_O, _D = (-1.85, -0.3, -1.05), (37, 29, 21)
TABLE = {
    "fast_sphere": (("fast_sphere", 0.0, _O, 0.1, _D, 0.0, None), dict(solids=2, closed_solids=1, voids=1, closed_voids=0), (2508, 536)),
    "labyrinth": (("labyrinth", 1.25, (-5.35, -0.3, -2.55), 0.1, _D, 0.0, None), dict(solids=2, closed_solids=0, voids=1, closed_voids=0), (4680, 2508)),
    "gyroid": (("gyroid", 0.5, _O, 0.1, _D, 0.0, None), dict(solids=331, closed_solids=305, voids=1, closed_voids=0), (5, 4, 4)),
    "sierpinski": (("sierpinski", 0.5, _O, 0.1, _D, 0.0, None), dict(solids=19, closed_solids=18, voids=1, closed_voids=0), (2508, 8, 4)),
    "cube_sea": (("cube_sea", 0.5, _O, 0.1, _D, 0.0, None), dict(solids=4, closed_solids=0, voids=1, closed_voids=0), (2508, 891, 344, 198)),
    "noise_lod": (("noise_lod", 0.5, _O, 0.1, _D, 0.0, None), dict(solids=4, closed_solids=3, voids=1, closed_voids=0), (4191, 2508, 1, 1)),
    "cube": (("cube", 0.5, (-1.82, 0.31, -0.98), 0.1, _D, 0.0, {"size": 0.8, "xpos": 0.03, "ypos": 0.55, "zpos": 0.07}),
             dict(solids=1, closed_solids=1, voids=1, closed_voids=0), (4096,)),
    "sierpinski_iso": (("sierpinski", 0.5, (-1.5, 0.0, -1.5), 0.0625, (48, 40, 44), 0.05, None), dict(solids=2, closed_solids=1, voids=11, closed_voids=10), (2205, 1084)),
}
_oracle = {}


def oracle_case(key):
    """-> (the oracle frame, the oracle's distances [pz, py, px], the definition's (counts, records, labels)) of a row of TABLE, once"""
    if key not in _oracle:
        (scene, stime, origin, cell, dims, iso, variables), _counts, _largest = TABLE[key]
        of = qu.frame(scene, stime, W, H, variables)
        D = qu.oracle_points(scene, of, mu.lattice_points(origin, cell, dims), normals=False)[0]
        D = np.ascontiguousarray(D, np.float32).reshape(dims[2] + 1, dims[1] + 1, dims[0] + 1)
        _oracle[key] = (of, D, label(D, dims, iso))
    return _oracle[key]


# ---- the library's text on the CPU ---------------------------------------------------------------------------------------------------
_host = None


def _source(name):
    return os.path.join(cppbuild.HERE, "cpp", name)


def host_lib():
    global _host
    if _host is None:
        L = ctypes.CDLL(qu.build_lib("components_host", "components_host.cpp", ["-I" + qu.CSRC], cppbuild.csrc_headers()))
        vp = ctypes.c_void_p
        L.cmp_label.restype = ctypes.c_int64
        L.cmp_label.argtypes = [vp, vp, vp, ctypes.c_int64, vp, vp, vp]
        L.cmp_sizes.restype = ctypes.c_int
        L.cmp_sizes.argtypes = [ctypes.c_int]
        _host = L
    return _host


def edge_count(dims):
    return 3 * (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1)


def host_label(D, dims, iso=0.0, order=None):
    """the stand-in: sdfr_components.h's union with the plain min over the edge slots in `order` (None: lattice order; slot 3 x + a is
    the edge from point x along axis a, skipped where there is none), then flatten, number and tally -> (counts, records, labels)"""
    import sdf_playground_amd as sp

    L = host_lib()
    assert [L.cmp_sizes(k) for k in range(3)] == [ctypes.sizeof(sp.MeshGrid), RECORD_DTYPE.itemsize, ctypes.sizeof(sp.ComponentCounts)]
    g = sp.MeshGrid((ctypes.c_float * 3)(0.0, 0.0, 0.0), 1.0, int(dims[0]), int(dims[1]), int(dims[2]), float(iso))
    D = np.ascontiguousarray(D, np.float32)
    N = D.size
    records, labels, counts = np.zeros(N, RECORD_DTYPE), np.zeros(N, np.uint32), sp.ComponentCounts()
    if order is not None:
        order = np.ascontiguousarray(order, np.int64)
    C = L.cmp_label(ctypes.addressof(g), qu._p(D), qu._p(order) if order is not None else None, 0 if order is None else len(order), qu._p(records), qu._p(labels),
                    ctypes.addressof(counts))
    return counts.as_dict(), records[:C].copy(), labels.reshape(D.shape)


def sanitizer_program():
    """the stand-alone program of components_plan_host.cpp under the address and undefined-behaviour sanitizers -> its path"""
    return cppbuild.plan_program("components_plan_host", "components_plan_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def run_plan(lines, program=None):
    """the plan program over request lines -> its answer lines"""
    program = program or cppbuild.plan_program("components_plan_host")
    return subprocess.run([program], input="".join(line + "\n" for line in lines), check=True, capture_output=True, text=True).stdout.splitlines()

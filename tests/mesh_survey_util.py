"""Shared by the survey tests (test_mesh_survey_cpu.py, test_gpu_mesh_survey.py): the definitions of sdfr_mesh_survey and sdfr_mesh_fit
(include/sdfr.h) restated in numpy from the header's words; the library's predicates, plans and fit loop built for the CPU
(tests/cpp/mesh_survey_host.cpp); the analytic distances; and the scenes and boxes of the GPU fit cases, which the CPU tier admits
first.  Test infrastructure: the product never imports this."""
import ctypes
import math
import os

import numpy as np

import cppbuild
import mesh_util as mu
import query_util as qu
from handle_sequences import DEFAULT_LIMITS

F = np.float32
EMPTY, FOUND, TOO_LARGE = 0, 1, 2
INVALID = -1  # SDFR_ERR_INVALID_ARGUMENT
NULL_POINTER, BAD_GRID, BAD_BAND = "null pointer", "bad mesh grid", "band must be finite and >= 0"
BAD_SEARCH, BAD_LEVELS, BAD_MARGIN = "bad search grid", "levels must be 0..10 and cell * 2^levels finite", "margin must be 0..8"
SURVEY_KEYS = ("active_cells", "quads", "near_cells", "inside_points", "active_lo", "active_hi", "near_lo", "near_hi", "face_active")


# ---- the definitions ---------------------------------------------------------------------------------------------------------------
def grid_ok(origin, cell, dims, iso):
    """a grid sdfr_mesh_extract takes"""
    cell = float(F(cell))
    return (all(math.isfinite(float(F(v))) for v in tuple(origin) + (cell, iso)) and cell > 0 and all(1 <= n <= 1024 for n in dims)
            and (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1) <= 1 << 30)


def survey(D, dims, iso, band):
    """sdfr_mesh_survey's definition.  D: the distances at mesh_util.lattice_points().  -> the dict SDFRenderer.surveyMesh returns"""
    n = [int(d) for d in dims]
    with np.errstate(invalid="ignore"):
        s = (np.asarray(D, np.float32) - F(iso)).reshape(n[2] + 1, n[1] + 1, n[0] + 1)  # [k, j, i]
        inside = s < 0  # NaN: outside
        close = np.abs(s) <= F(band)  # NaN: not near

    def corners(a):
        return [a[dk:dk + n[2], dj:dj + n[1], di:di + n[0]] for dk in (0, 1) for dj in (0, 1) for di in (0, 1)]

    count = sum(c.astype(np.int32) for c in corners(inside))
    active = (count > 0) & (count < 8)
    near = active | np.logical_or.reduce(corners(close))
    quads = 0
    for a in range(3):  # edges along axis a from the points whose two other coordinates are 1 .. n - 1
        lower, upper = [slice(1, n[m]) for m in range(3)], [slice(1, n[m]) for m in range(3)]
        lower[a], upper[a] = slice(0, n[a]), slice(1, n[a] + 1)
        quads += int((inside[lower[2], lower[1], lower[0]] != inside[upper[2], upper[1], upper[0]]).sum())

    def bounds(flags):
        k, j, i = np.nonzero(flags)
        if not len(i):
            return tuple(n), (-1, -1, -1)
        return (int(i.min()), int(j.min()), int(k.min())), (int(i.max()), int(j.max()), int(k.max()))

    faces = (active[:, :, 0], active[:, :, n[0] - 1], active[:, 0, :], active[:, n[1] - 1, :], active[0], active[n[2] - 1])
    out = dict(active_cells=int(active.sum()), quads=quads, near_cells=int(near.sum()), inside_points=int(inside.sum()),
               face_active=tuple(int(f.sum()) for f in faces))
    out["active_lo"], out["active_hi"] = bounds(active)
    out["near_lo"], out["near_hi"] = bounds(near)
    return out


def level_grid(origin, cell, lo, hi, level):
    """the grid of a level over the window: origin + (float)lo * c per axis -- one multiply, then one add --, cells of 2^level"""
    step = 1 << level
    o = tuple(float(F(origin[a]) + F(lo[a]) * F(cell)) for a in range(3))
    return o, float(F(cell) * F(step)), tuple(-(-(hi[a] - lo[a]) // step) for a in range(3))


def fit(distance, origin, cell, dims, iso, levels, margin):
    """sdfr_mesh_fit's definition.  distance(origin, cell, dims) -> the distances at that lattice's points.  -> the dict
    SDFRenderer.fitMesh returns"""
    lo, hi = [0, 0, 0], [int(d) for d in dims]
    surveys, last = 0, None

    def result(state, level):
        found = state == FOUND
        o, _c, n = level_grid(origin, cell, lo, hi, 0)
        return dict(state=state, level=level, surveys=surveys, lo=tuple(lo), hi=tuple(hi), origin=o if found else None, dims=n if found else None, survey=last)

    for level in range(levels, -1, -1):
        step = 1 << level
        o, c, n = level_grid(origin, cell, lo, hi, level)
        if not grid_ok(o, c, n, iso):
            return result(TOO_LARGE, level)
        band = F(1.75) * F(c) if level >= 1 else F(0)
        last = survey(distance(o, c, n), n, iso, band)
        surveys += 1
        which = "near" if level >= 1 else "active"
        if last[which + "_cells"] == 0:
            return result(EMPTY, level)
        g = 1 if level >= 1 else margin
        b_lo, b_hi = last[which + "_lo"], last[which + "_hi"]
        lo, hi = ([max(lo[a] + (b_lo[a] - g) * step, 0) for a in range(3)], [min(lo[a] + (b_hi[a] + 1 + g) * step, dims[a]) for a in range(3)])
    return result(FOUND, 0)


def survey_fault(origin, cell, dims, iso, band, grid=True, out=True):
    """the text of the fault that wins, or None"""
    if not grid or not out:
        return NULL_POINTER
    if not grid_ok(origin, cell, dims, iso):
        return BAD_GRID
    if not (math.isfinite(float(F(band))) and band >= 0):
        return BAD_BAND
    return None


def fit_fault(origin, cell, dims, iso, levels, margin, grid=True, out=True):
    if not grid or not out:
        return NULL_POINTER
    c = float(F(cell))
    if not (all(math.isfinite(float(F(v))) for v in tuple(origin) + (c, iso)) and c > 0 and all(1 <= n <= 1 << 20 for n in dims)):
        return BAD_SEARCH
    with np.errstate(over="ignore"):
        if not 0 <= levels <= 10 or not np.isfinite(F(cell) * F(1 << levels)):
            return BAD_LEVELS
    if not 0 <= margin <= 8:
        return BAD_MARGIN
    return None


def default_levels(dims):
    """the smallest L with max ceil(n / 2^L) <= 64, capped at 10"""
    return next((L for L in range(10) if max(-(-n // (1 << L)) for n in dims) <= 64), 10)


# ---- the library's text on the CPU ---------------------------------------------------------------------------------------------------
_host = None
LATTICE_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p)


def _source():
    return os.path.join(cppbuild.HERE, "cpp", "mesh_survey_host.cpp")


def host_lib():
    global _host
    if _host is None:
        import sdf_playground_amd as sp

        L = ctypes.CDLL(qu.build_lib("mesh_survey_host", "mesh_survey_host.cpp", ["-I" + qu.CSRC], cppbuild.csrc_headers()))
        # the ctypes mirrors of include/sdfr.h are the C++ structs
        assert [L.msh_sizes(k) for k in range(3)] == [ctypes.sizeof(sp.MeshGrid), ctypes.sizeof(sp.MeshSurvey), ctypes.sizeof(sp.MeshFit)]
        vp = ctypes.c_void_p
        L.msh_survey.argtypes = [vp, vp, ctypes.c_float, vp, ctypes.c_char_p]
        L.msh_fit.argtypes = [vp, ctypes.c_int, ctypes.c_int, LATTICE_FN, vp, ctypes.c_char_p]
        _host = L
    return _host


def sanitizer_program():
    """the stand-alone program of mesh_survey_host.cpp under the address and undefined-behaviour sanitizers -> its path"""
    return cppbuild.compile(os.path.join(cppbuild.BUILD, "mesh_survey_san"), [_source()], cppbuild.csrc_headers(),
                            cppbuild.EXACT_FLAGS + ["-I" + qu.CSRC, "-DMESH_SURVEY_MAIN", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                            shared=False)


def _grid(origin, cell, dims, iso):
    import sdf_playground_amd as sp

    return sp.MeshGrid((ctypes.c_float * 3)(*[float(v) for v in origin]), float(cell), int(dims[0]), int(dims[1]), int(dims[2]), float(iso))


def fit_dict(out):
    """sdfr_mesh_fit_result -> what SDFRenderer.fitMesh makes of it"""
    found = out.state == FOUND
    return dict(state=int(out.state), level=int(out.level), surveys=int(out.surveys), lo=tuple(out.lo), hi=tuple(out.hi),
                origin=tuple(float(v) for v in out.grid.origin) if found else None, dims=(out.grid.nx, out.grid.ny, out.grid.nz) if found else None,
                survey=out.last.as_dict() if out.surveys else None)


def host_survey(D, origin, cell, dims, iso, band, grid=True, out=True):
    """-> (status, error text, the survey or None)"""
    import sdf_playground_amd as sp

    g, s, err = _grid(origin, cell, dims, iso), sp.MeshSurvey(), ctypes.create_string_buffer(64)
    D = np.ascontiguousarray(D, np.float32)
    rc = host_lib().msh_survey(ctypes.addressof(g) if grid else None, qu._p(D), float(band), ctypes.addressof(s) if out else None, err)
    return rc, err.value.decode(), s.as_dict() if rc == 0 else None


def host_fit(distance, origin, cell, dims, iso, levels, margin, grid=True, out=True):
    """-> (status, error text, the fit or None)"""
    import sdf_playground_amd as sp

    keep = []

    def lattice(level):
        lg = ctypes.cast(level, ctypes.POINTER(sp.MeshGrid)).contents
        keep.append(np.ascontiguousarray(distance(tuple(lg.origin), lg.cell, (lg.nx, lg.ny, lg.nz)), np.float32))
        return keep[-1].ctypes.data

    g, f, err = _grid(origin, cell, dims, iso), sp.MeshFit(), ctypes.create_string_buffer(64)
    rc = host_lib().msh_fit(ctypes.addressof(g) if grid else None, levels, margin, LATTICE_FN(lattice), ctypes.addressof(f) if out else None, err)
    return rc, err.value.decode(), fit_dict(f) if rc == 0 else None


# ---- analytic distances (exact, so never overestimating), float64 then rounded ------------------------------------------------------
def shape_distance(shape, centre, size):
    """-> distance(origin, cell, dims) of a sphere of radius `size`, a torus (R = size, r = size / 3, axis y) or a box of half-edges
    size * (1, 0.75, 0.5) about `centre`"""
    def at(origin, cell, dims):
        q = mu.lattice_points(origin, cell, dims).astype(np.float64) - np.asarray(centre, np.float64)
        if shape == "sphere":
            d = np.linalg.norm(q, axis=1) - size
        elif shape == "torus":
            d = np.hypot(np.hypot(q[:, 0], q[:, 2]) - size, q[:, 1]) - size / 3.0
        else:
            e = np.abs(q) - size * np.array([1.0, 0.75, 0.5])
            d = np.linalg.norm(np.maximum(e, 0.0), axis=1) + np.minimum(e.max(1), 0.0)
        return d.astype(np.float32)
    return at


def scaled(distance, factor):
    return lambda origin, cell, dims: (distance(origin, cell, dims) * F(factor)).astype(np.float32)


def contains_active(fit_result, full_survey, dims, margin):
    """the fit's window holds the full grid's active bounds plus the margin, clipped to the search window"""
    if fit_result["state"] != FOUND:
        return False
    return all(fit_result["lo"][a] <= max(full_survey["active_lo"][a] - margin, 0) and fit_result["hi"][a] >= min(full_survey["active_hi"][a] + 1 + margin, dims[a])
               for a in range(3))


# ---- the scenes and search grids of the GPU fit test, admitted by the CPU tier first (test_mesh_survey_cpu.py) ------------------------
# dyadic origins and cell, so that the fitted lattice's points are the search lattice's bit for bit.  scene: (time, origin)
FIT_CELL, FIT_DIMS = 0.0625, (64, 48, 56)
FIT_SCENES = {"fast_sphere": (0.0, (-2.0, -0.5, -1.75)), "labyrinth": (1.25, (-5.5, -0.25, -3.5))}


def oracle_distance(scene, of):
    """-> distance(origin, cell, dims) by the oracle's definition of the scene"""
    return lambda origin, cell, dims: qu.oracle_points(scene, of, mu.lattice_points(origin, cell, dims), normals=False)[0]


# ---- the run-time probe scene of the GPU tier's survey, slice, span and measure tests ----------------------------------------------
# By `kind` a sphere with its centre and radius in variables, the plane y = height, or that plane with NaN
# where x > split.  setValue does not clamp, so the ranges below bind nothing.
PROBE = """struct Scene
{
	static SDF_HD void prepare(FrameU &) {}
	struct RayInv {};
	static SDF_HD RayInv ray_setup(const FrameU &, vec3, const RayFlags &) { return RayInv(); }
	static SDF_HD float dist(const FrameU &U, const RayInv &, vec3 p, vec3, bool)
	{
		const float kind = VAR_kind(min = 0, max = 2, start = 0);
		const vec3 c = V3(VAR_cx(min = -100, max = 100, start = 0), VAR_cy(min = -100, max = 100, start = 0), VAR_cz(min = -100, max = 100, start = 0));
		const float radius = VAR_radius(min = 0, max = 10, start = 1), height = VAR_height(min = -10, max = 10, start = 0.25);
		const float split = VAR_split(min = -10, max = 10, start = 0.3);
		if (kind < 0.5f) return sd_sphere(p - c, radius);
		if (kind > 1.5f && p.x > split) return bits_f32(0x7fc00000u);
		return p.y - height;
	}
	static SDF_HD void material(const FrameU &, const SurfacePoint &, Material &) {}
	static SDF_HD bool light(const FrameU &, int i, Light &L) { return sun_light(i, L); }
	static SDF_HD float ambient() { return 0.1f; }
	static SDF_HD vec3 background(const FrameU &U, vec3 dir, uint32_t) { return sky_color(dir, U.sky_s, U.sky_c); }
};
"""
PROBE_DEFAULTS = dict(kind=0.0, cx=0.0, cy=0.0, cz=0.0, radius=1.0, height=0.25, split=0.3)


def load_probe(r, name, defaults, loaded=None, **values):
    """the probe scene, compiled as `name` unless it is the handle's scene already (loaded: the caller knows; None: ask the handle),
    with its variables at `defaults` but for `values`"""
    if not (r.currentScene() == name if loaded is None else loaded):
        r.initShaderSource(name, PROBE)
        r.setLimits(**DEFAULT_LIMITS)
    for variable, v in dict(defaults, **values).items():
        assert r.setValue(variable, v)

"""The C ABI of libsdfr.so as Python sees it (include/sdfr.h): its constants, the ctypes mirrors of its structs, the numpy dtypes of its
records, one table of its functions, and the loader that applies the table.  tests/test_abi.py holds every row and every mirror
against the header."""
import ctypes
import os
import sys
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SDFR_LIBRARY") or os.path.join(_HERE, "libsdfr.so")  # SDFR_LIBRARY: developer builds (tools/phase_clocks.py)

SDFR_OK = 0
SCHEDULE_WAVEFRONT = 0
SCHEDULE_PIXEL = 1
LAUNCH_AUTO, LAUNCH_PER_TILE, LAUNCH_PERSISTENT = 0, 1, 2
RGBA32F = 0
RGBA16F = 1
STRIP_RGB32F_A8 = 2  # strips only: rgb float triples + one flag byte per pixel (lossless, 13 B/pixel)
STRIP_RGB16F_A8 = 3  # strips only: rgb half triples + one flag byte per pixel (the reference's RGBA16F target in 7 B/pixel)
COMM_ID_BYTES = 128
STRIP_ROWS = 8

_STATUS = {
    0: "SDFR_OK", -1: "SDFR_ERR_INVALID_ARGUMENT", -2: "SDFR_ERR_UNKNOWN_SCENE", -3: "SDFR_ERR_UNKNOWN_VARIABLE",
    -4: "SDFR_ERR_NO_SCENE", -5: "SDFR_ERR_HIP", -6: "SDFR_ERR_NO_DEVICE", -7: "SDFR_ERR_COMPILE", -8: "SDFR_ERR_COMM", -9: "SDFR_ERR_INTERNAL",
}


class SdfrError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("%s: %s" % (_STATUS.get(code, str(code)), message))
        self.code = code


class _CVariable(ctypes.Structure):  # sdfr_variable
    _fields_ = [("name", ctypes.c_char * 48), ("minval", c_float), ("maxval", c_float), ("start", c_float), ("step", c_float), ("value", c_float)]


class _CTiming(ctypes.Structure):  # sdfr_timing
    _fields_ = [("name", ctypes.c_char * 32), ("ms", c_double)]


class Limits(ctypes.Structure):
    """sdfr_limits: the driver's compile-time limits (pshader_sdf.hlsl:60-64,350) at run time."""

    _fields_ = [("iter_count", c_int), ("bounce_count", c_int), ("ray_count", c_int), ("light_count", c_int),
                ("range", c_float), ("max_cost_default", c_int), ("extension_lights", c_int),
                ("extension_marble_reflection", c_float),
                # pshader_sdf.hlsl:31-35 at run time; defaults 1e-4, 1e-4, 1e-3, 1e-3, 3e-4 (anything else: extension)
                ("dist_eps", c_float), ("grad_eps", c_float), ("reflect_eps", c_float), ("refract_eps", c_float),
                ("shadow_eps", c_float)]


class Stats(ctypes.Structure):  # sdfr_stats
    _fields_ = [("ms_gpu", c_double), ("ms_march", c_double), ("ms_shade", c_double), ("pixels", c_uint64),
                ("rays", c_uint64), ("march_evals", c_uint64), ("hits", c_uint64), ("march_launches", c_uint32),
                ("shade_launches", c_uint32)]


class MeshGrid(ctypes.Structure):  # sdfr_mesh_grid
    _fields_ = [("origin", c_float * 3), ("cell", c_float), ("nx", c_int32), ("ny", c_int32), ("nz", c_int32), ("iso", c_float)]


class MeshCounts(ctypes.Structure):  # sdfr_mesh_counts
    _fields_ = [("vertices", c_int64), ("triangles", c_int64)]


class SliceGrid(ctypes.Structure):  # sdfr_slice_grid
    _fields_ = [("origin", c_float * 3), ("du", c_float * 3), ("dv", c_float * 3), ("dw", c_float * 3),
                ("nu", c_int32), ("nv", c_int32), ("layers", c_int32), ("iso", c_float)]


class SliceCounts(ctypes.Structure):  # sdfr_slice_counts
    _fields_ = [("vertices", c_int64), ("segments", c_int64)]


class MeshSurvey(ctypes.Structure):  # sdfr_mesh_survey_result
    _fields_ = [("active_cells", c_int64), ("quads", c_int64), ("near_cells", c_int64), ("inside_points", c_int64),
                ("active_lo", c_int32 * 3), ("active_hi", c_int32 * 3), ("near_lo", c_int32 * 3), ("near_hi", c_int32 * 3),
                ("face_active", c_int64 * 6)]

    def as_dict(self):
        return {name: (int(getattr(self, name)) if name.endswith(("cells", "quads", "points")) else tuple(int(v) for v in getattr(self, name)))
                for name, _type in self._fields_}


FIT_EMPTY, FIT_FOUND, FIT_TOO_LARGE = 0, 1, 2  # SDFR_FIT_*


class MeshFit(ctypes.Structure):  # sdfr_mesh_fit_result
    _fields_ = [("state", c_int32), ("level", c_int32), ("surveys", c_int32), ("lo", c_int32 * 3), ("hi", c_int32 * 3),
                ("grid", MeshGrid), ("last", MeshSurvey)]


class ComponentCounts(ctypes.Structure):  # sdfr_component_counts
    _fields_ = [("components", c_int64), ("solids", c_int64), ("voids", c_int64), ("closed_solids", c_int64), ("closed_voids", c_int64),
                ("inside_points", c_int64), ("largest_solid_points", c_int64), ("largest_void_points", c_int64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _type in self._fields_}


# sdfr_component (include/sdfr.h): one part or void of the lattice, 40 bytes
COMPONENT_DTYPE = np.dtype([("root", np.uint32), ("flags", np.uint32), ("points", np.int64), ("lo", np.int32, (3,)), ("hi", np.int32, (3,))])
assert COMPONENT_DTYPE.itemsize == 40 and ctypes.sizeof(ComponentCounts) == 64
COMPONENT_INSIDE, COMPONENT_FACE_SHIFT, COMPONENT_FACES = 1, 8, 0x3F00  # SDFR_COMPONENT_*


class Atlas(ctypes.Structure):  # sdfr_atlas
    _fields_ = [("triangles", c_int64), ("quads", c_int64), ("tile", c_int32), ("width", c_int32), ("height", c_int32),
                ("tiles_per_row", c_int32), ("rows", c_int32), ("reserved", c_int32)]


ATLAS_LAYERS = {"albedo": 1, "normal": 2, "lit": 4}  # SDFR_ATLAS_*

# sdfr_hit (include/sdfr.h): the answer of a ray query or a pick, 48 bytes
HIT_DTYPE = np.dtype([("t", np.float32), ("distance", np.float32), ("pos", np.float32, (3,)), ("normal", np.float32, (3,)),
                      ("iterations", np.uint32), ("material_id", np.uint32), ("hit", np.int32), ("reserved", np.uint32)])
assert HIT_DTYPE.itemsize == 48
# sdfr_surface (include/sdfr.h): what the surface looks like at a hit, 128 bytes
SURFACE_DTYPE = np.dtype([("material_id", np.uint32), ("flags", np.uint32), ("max_cost", np.uint32), ("valid", np.int32),
                          ("albedo", np.float32, (3,)), ("alpha", np.float32), ("specular", np.float32, (3,)), ("specular_power", np.float32),
                          ("emissive", np.float32, (3,)), ("optical_index", np.float32), ("unlit", np.float32, (3,)), ("reserved0", np.float32),
                          ("reflection", np.float32, (3,)), ("reserved1", np.float32), ("refraction", np.float32, (3,)), ("reserved2", np.float32),
                          ("shading_normal", np.float32, (3,)), ("reserved3", np.float32)])
assert SURFACE_DTYPE.itemsize == 128
SURFACE_USE_HDR = 1
SURFACE_LIT = 2
# sdfr_occlusion (include/sdfr.h): which of 64 fixed directions above a point are blocked within a radius, 16 bytes
OCCLUSION_DTYPE = np.dtype([("mask_lo", np.uint32), ("mask_hi", np.uint32), ("occluded", np.uint32), ("valid", np.int32)])
assert OCCLUSION_DTYPE.itemsize == 16
# sdfr_lighting (include/sdfr.h): how the scene's lights fall on a hit, 64 bytes; sdfr_light_sample: one light slot of it, 80 bytes, [n, 8]
LIGHTING_DTYPE = np.dtype([("valid", np.int32), ("used_mask", np.uint32), ("traced_mask", np.uint32), ("visible_mask", np.uint32),
                           ("own", np.float32, (3,)), ("ambient_factor", np.float32), ("direct", np.float32, (3,)), ("segments", np.uint32),
                           ("lit", np.float32, (3,)), ("reserved", np.float32)])
assert LIGHTING_DTYPE.itemsize == 64
LIGHT_SAMPLE_DTYPE = np.dtype([("state", np.int32), ("flags", np.uint32), ("segments", np.uint32), ("reserved0", np.uint32),
                               ("dir", np.float32, (3,)), ("distance", np.float32), ("color", np.float32, (3,)), ("light_dot", np.float32),
                               ("influenced", np.float32, (3,)), ("specular_factor", np.float32), ("delivered", np.float32, (3,)),
                               ("reserved1", np.float32)])
assert LIGHT_SAMPLE_DTYPE.itemsize == 80
LIGHT_DIRECTIONAL = 1
LIGHT_UNUSED, LIGHT_NO_CHAIN, LIGHT_BLOCKED, LIGHT_ESCAPED = 0, 1, 2, 3
# sdfr_span_summary (include/sdfr.h): what a ray passes through, 32 bytes; its spans are [n, max_spans, 2] float32 (t_in, t_out)
SPAN_SUMMARY_DTYPE = np.dtype([("crossings", np.uint32), ("spans", np.uint32), ("steps", np.uint32), ("valid", np.int32), ("inside_length", np.float32),
                               ("t_end", np.float32), ("flags", np.uint32), ("reserved", np.uint32)])
assert SPAN_SUMMARY_DTYPE.itemsize == 32
SPAN_STARTS_INSIDE, SPAN_ENDS_INSIDE, SPAN_OUT_OF_STEPS = 1, 2, 4


class SpanParams(ctypes.Structure):  # sdfr_span_params
    _fields_ = [("t_max", c_float), ("min_step", c_float), ("iso", c_float), ("max_steps", c_int32), ("max_spans", c_int32)]


class MeasureGrid(ctypes.Structure):  # sdfr_measure_grid
    _fields_ = [("origin", c_float * 3), ("du", c_float * 3), ("dv", c_float * 3), ("dw", c_float * 3),
                ("nu", c_int32), ("nv", c_int32)]


class MeasureResult(ctypes.Structure):  # sdfr_measure_result
    _fields_ = [("moments", c_double * 10), ("columns_hit", c_int64), ("columns_open", c_int64), ("columns_out_of_steps", c_int64),
                ("columns_invalid", c_int64), ("steps", c_int64), ("spans", c_int64), ("crossings", c_int64),
                ("hit_lo", c_int32 * 2), ("hit_hi", c_int32 * 2), ("t_lo", c_float), ("t_hi", c_float)]

    def as_dict(self):
        return {name: (tuple(getattr(self, name)) if name in ("moments", "hit_lo", "hit_hi") else getattr(self, name)) for name, _type in self._fields_}


class SolidProperties(ctypes.Structure):  # sdfr_solid_properties
    _fields_ = [("volume", c_double), ("mass", c_double), ("centroid", c_double * 3), ("inertia", c_double * 6)]

    def as_dict(self):
        return {"volume": self.volume, "mass": self.mass, "centroid": tuple(self.centroid), "inertia": tuple(self.inertia)}


assert ctypes.sizeof(MeasureGrid) == 56 and ctypes.sizeof(MeasureResult) == 160 and ctypes.sizeof(SolidProperties) == 88
# sdfr_measure_column: a column's integrals of 1, t and t^2 over its inside part and the words of its span summary, 40 bytes
MEASURE_COLUMN_DTYPE = np.dtype([("m0", np.float64), ("m1", np.float64), ("m2", np.float64), ("spans", np.uint32), ("steps", np.uint32), ("flags", np.uint32),
                                 ("valid", np.int32)])
assert MEASURE_COLUMN_DTYPE.itemsize == 40

# Every function include/sdfr.h declares: name -> (restype, argtypes).  A new entry point is one row here and one method that calls it;
# load_library applies the rows, the tests check that the library exports each (EXPORTED_SYMBOLS) and hold each against its prototype.
_vp, _ci, _cf, _i64, _str, _f3 = c_void_p, c_int, c_float, c_int64, c_char_p, POINTER(c_float)
ABI = {
    "sdfr_create": (_ci, [_ci, POINTER(_vp)]),
    "sdfr_destroy": (None, [_vp]),
    "sdfr_last_error": (_str, [_vp]),
    "sdfr_set_stream": (_ci, [_vp, _vp]),
    "sdfr_scene_count": (_ci, []),
    "sdfr_scene_name": (_str, [_ci]),
    "sdfr_load_scene": (_ci, [_vp, _str]),
    "sdfr_current_scene": (_str, [_vp]),
    "sdfr_load_scene_source": (_ci, [_vp, _str, _str]),
    "sdfr_check_scene_source": (_ci, [_str, _str, _str, c_size_t]),
    "sdfr_load_scene_hlsl": (_ci, [_vp, _str, _str]),
    "sdfr_check_scene_hlsl": (_ci, [_str, _str, _str, c_size_t]),
    "sdfr_translate_scene_hlsl": (_ci, [_str, _str, c_size_t]),
    "sdfr_var_count": (_ci, [_vp]),
    "sdfr_var_info": (_ci, [_vp, _ci, POINTER(_CVariable)]),
    "sdfr_var_set": (_ci, [_vp, _str, _cf]),
    "sdfr_var_get": (_ci, [_vp, _str, _f3]),
    "sdfr_vars_reset": (_ci, [_vp]),
    "sdfr_set_camera": (_ci, [_vp, _f3, _f3, _f3, _f3]),
    "sdfr_set_camera_lookat": (_ci, [_vp, _f3, _f3, _cf, _cf, _cf]),
    "sdfr_set_camera_direction": (_ci, [_vp, _f3, _f3, _cf, _cf, _cf]),
    "sdfr_get_camera": (_ci, [_vp, _f3]),
    "sdfr_set_time": (_ci, [_vp, _cf]),
    "sdfr_get_limits": (_ci, [_vp, POINTER(Limits)]),
    "sdfr_set_limits": (_ci, [_vp, POINTER(Limits)]),
    "sdfr_set_schedule": (_ci, [_vp, _ci]),
    "sdfr_set_launch_mode": (_ci, [_vp, _ci]),
    "sdfr_set_step_shortcuts": (_ci, [_vp, _ci]),
    "sdfr_set_profiling": (_ci, [_vp, _ci]),
    "sdfr_render": (_ci, [_vp, _ci, _ci, _vp, _ci, _ci, _vp]),
    "sdfr_render_aa": (_ci, [_vp, _ci, _ci, _ci, _vp, _ci, _ci, _vp]),
    "sdfr_register_host_target": (_ci, [_vp, _vp, c_size_t]),
    "sdfr_strip_buffer_pixels": (_i64, [_ci, _ci, _ci]),
    "sdfr_strip_buffer_bytes": (_i64, [_ci, _ci, _ci, _ci]),
    "sdfr_set_strip_split": (_ci, [_vp, _ci, _ci]),
    "sdfr_strip_buffer_pixels_split": (_i64, [_ci, _ci, _ci, _ci, _ci]),
    "sdfr_strip_buffer_bytes_split": (_i64, [_ci, _ci, _ci, _ci, _ci, _ci]),
    "sdfr_render_private_strips": (_ci, [_vp, _ci, _ci, _vp, _ci]),
    "sdfr_render_strips": (_ci, [_vp, _ci, _ci, _ci, _ci, _vp, _ci]),
    "sdfr_assemble_strips": (_ci, [_vp, _ci, _ci, _ci, _vp, _vp, _ci]),
    "sdfr_comm_unique_id": (_ci, [_vp]),
    "sdfr_comm_create": (_ci, [_vp, _ci, _ci, _ci, POINTER(_vp)]),
    "sdfr_comm_create_all": (_ci, [POINTER(_ci), _ci, POINTER(_vp)]),
    "sdfr_comm_close": (_ci, [_vp]),
    "sdfr_comm_destroy": (None, [_vp]),
    "sdfr_comm_library_info": (_ci, [_str, c_size_t, POINTER(_ci), POINTER(_ci)]),
    "sdfr_comm_rank": (_ci, [_vp]),
    "sdfr_comm_world": (_ci, [_vp]),
    "sdfr_comm_last_error": (_str, [_vp]),
    "sdfr_comm_selftest": (_ci, [_vp, c_size_t, _vp]),
    "sdfr_render_gather": (_ci, [_vp, _vp, _ci, _ci, _vp, _ci, _ci]),
    "sdfr_render_gather_all": (_ci, [POINTER(_vp), POINTER(_vp), _ci, _ci, _ci, _vp, _ci, _ci]),
    "sdfr_postprocess": (_ci, [_vp, _ci, _ci, _vp, _vp, _vp]),
    "sdfr_sync": (_ci, [_vp]),
    "sdfr_query_distance": (_ci, [_vp, _i64, _vp, _vp, _vp, _ci]),
    "sdfr_query_rays": (_ci, [_vp, _i64, _vp, _vp, _cf, _vp, _ci]),
    "sdfr_pick": (_ci, [_vp, _ci, _ci, _i64, _vp, _vp, _ci]),
    "sdfr_query_ray_surfaces": (_ci, [_vp, _i64, _vp, _vp, _cf, _vp, _vp, _ci]),
    "sdfr_pick_surfaces": (_ci, [_vp, _ci, _ci, _i64, _vp, _vp, _vp, _ci]),
    "sdfr_mesh_surfaces": (_ci, [_vp, _i64, _vp, _vp, _cf, _vp, _vp, _ci]),
    "sdfr_query_ray_lighting": (_ci, [_vp, _i64, _vp, _vp, _cf, _vp, _vp, _vp, _ci]),
    "sdfr_pick_lighting": (_ci, [_vp, _ci, _ci, _i64, _vp, _vp, _vp, _vp, _ci]),
    "sdfr_mesh_lighting": (_ci, [_vp, _i64, _vp, _vp, _cf, _vp, _vp, _vp, _ci]),
    "sdfr_occlusion_directions": (_ci, [_vp]),
    "sdfr_query_occlusion": (_ci, [_vp, _i64, _vp, _vp, _cf, _cf, _vp, _ci]),
    "sdfr_hit_occlusion": (_ci, [_vp, _i64, _vp, _cf, _cf, _vp, _ci]),
    "sdfr_mesh_extract": (_ci, [_vp, POINTER(MeshGrid), _i64, _i64, _vp, _vp, _vp, POINTER(MeshCounts), _ci]),
    "sdfr_mesh_get_timings": (_ci, [_vp, POINTER(c_double * 4)]),
    "sdfr_mesh_extract_sharp": (_ci, [_vp, POINTER(MeshGrid), _i64, _i64, _vp, _vp, _vp, POINTER(MeshCounts), _ci]),
    "sdfr_mesh_survey": (_ci, [_vp, POINTER(MeshGrid), _cf, POINTER(MeshSurvey)]),
    "sdfr_mesh_fit": (_ci, [_vp, POINTER(MeshGrid), _ci, _ci, POINTER(MeshFit)]),
    "sdfr_components_label": (_ci, [_vp, POINTER(MeshGrid), _i64, _vp, _vp, POINTER(ComponentCounts), _ci]),
    "sdfr_components_label_lattice": (_ci, [_vp, POINTER(MeshGrid), _vp, _i64, _vp, _vp, POINTER(ComponentCounts), _ci]),
    "sdfr_slice_extract": (_ci,[_vp, POINTER(SliceGrid), _i64, _i64, _vp, _vp, _vp, _vp, _vp, POINTER(SliceCounts), _ci]),
    "sdfr_query_ray_spans": (_ci, [_vp, _i64, _vp, _vp, POINTER(SpanParams), _vp, _vp, _ci]),
    "sdfr_pick_spans": (_ci, [_vp, _ci, _ci, _i64, _vp, POINTER(SpanParams), _vp, _vp, _ci]),
    "sdfr_mesh_spans": (_ci, [_vp, _i64, _vp, _vp, _cf, POINTER(SpanParams), _vp, _vp, _ci]),
    "sdfr_measure": (_ci, [_vp, POINTER(MeasureGrid), POINTER(SpanParams), POINTER(MeasureResult), _vp, _ci]),
    "sdfr_measure_properties": (_ci, [POINTER(MeasureGrid), POINTER(MeasureResult), c_double, POINTER(SolidProperties)]),
    "sdfr_atlas_layout": (_ci, [_i64, _ci, _ci, POINTER(Atlas)]),
    "sdfr_atlas_uvs": (_ci, [POINTER(Atlas), _vp]),
    "sdfr_atlas_texels": (_ci, [_vp, POINTER(Atlas), _i64, _vp, _vp, _vp, _vp, _vp, _vp, _ci]),
    "sdfr_atlas_bake": (_ci, [_vp, POINTER(Atlas), _i64, _vp, _vp, _vp, _cf, c_uint32, _vp, _vp, _vp, _vp, _ci]),
    "sdfr_set_frames_in_flight": (_ci, [_vp, _ci]),
    "sdfr_wait_frame": (_ci, [_vp, _vp]),
    "sdfr_get_stats": (_ci, [_vp, POINTER(Stats)]),
    "sdfr_get_timings": (_ci, [_vp, POINTER(_CTiming), _ci]),
    "sdfr_selftest_math": (_ci, [_vp, _ci, _cf, POINTER(c_uint64)]),
    "sdfr_selftest_exception": (_ci, [_vp, _ci]),
}
EXPORTED_SYMBOLS = list(ABI)

_lib = None


def load_library():
    """dlopen libsdfr.so and give every function of ABI its types.  torch (when installed) is imported first so that both share one
    HIP runtime (same SONAME, libamdhip64.so.7)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SdfrError(-5, "libsdfr.so is not built: run `python -m sdf_playground_amd.buildlib` (needs hipcc)")
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in ABI.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L

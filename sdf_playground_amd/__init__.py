"""sdf_playground_amd -- MI355X-native SDF raymarch renderer (hot path of Gotbread/sdf-playground).

Python host side above the C ABI (include/sdfr.h, libsdfr.so).  The classes mirror the
reference's host interface for this path so that code written against the reference reads
the same here:

    SDFRenderer   Engine/SDFRenderer.h:17-44   init / initShader / setParameters /
                                               getVariableMap / render
    Camera        Engine/Camera.h:5-64         SetEye / SetLookat / SetDirection / SetAspect /
                                               SetFOVY / SetRoll  (FPS mode)
    Variable      Engine/ShaderVariable.h:6-12 minval / maxval / start / step / value

All pixels come from the HIP kernels; if libsdfr.so cannot be loaded or no GPU is present
the calls raise -- there is no CPU fallback.

The package's names live in four modules: _abi (the C ABI: constants, structs, records, the table of functions, the loader), _renderer
(SDFRenderer, Camera, Variable, HDR and the functions that need no handle), _comm (Comm) and _strips (the strip layout restated in numpy).
"""
from ._abi import (ATLAS_LAYERS, COMM_ID_BYTES, COMPONENT_DTYPE, COMPONENT_FACE_SHIFT, COMPONENT_FACES, COMPONENT_INSIDE, EXPORTED_SYMBOLS,  # noqa: F401
                   ComponentCounts, FIT_EMPTY, FIT_FOUND, FIT_TOO_LARGE, HIT_DTYPE, LAUNCH_AUTO, LAUNCH_PER_TILE,
                   LAUNCH_PERSISTENT, LIB_PATH, LIGHT_BLOCKED, LIGHT_DIRECTIONAL, LIGHT_ESCAPED, LIGHT_NO_CHAIN, LIGHT_SAMPLE_DTYPE, LIGHT_UNUSED,
                   LIGHTING_DTYPE, MEASURE_COLUMN_DTYPE, OCCLUSION_DTYPE, RGBA16F, RGBA32F, SCHEDULE_PIXEL, SCHEDULE_WAVEFRONT, SDFR_OK,
                   SPAN_ENDS_INSIDE, SPAN_OUT_OF_STEPS, SPAN_STARTS_INSIDE, SPAN_SUMMARY_DTYPE, STRIP_RGB16F_A8, STRIP_RGB32F_A8, STRIP_ROWS,
                   SURFACE_DTYPE, SURFACE_LIT, SURFACE_USE_HDR, Atlas, Limits, MeasureGrid, MeasureResult, MeshCounts, MeshFit, MeshGrid, MeshSurvey,
                   SdfrError, SliceCounts, SliceGrid, SolidProperties, SpanParams, Stats, load_library)
from ._comm import Comm  # noqa: F401
from ._renderer import (HDR, Camera, SDFRenderer, Variable, atlasDefaultWidth, atlasLayout, atlasUVs, chainContours, check_scene_hlsl,  # noqa: F401
                        check_scene_source, default_fit_levels, measureGrid, measureProperties, occlusionDirections, scene_names,
                        strip_buffer_bytes, strip_buffer_pixels, to_radian, translate_scene_hlsl)
from ._strips import (assemble_strips_host, pack_strip16_host, pack_strip_host, private_rows_host, strip_buffer_pixels_host,  # noqa: F401
                      strip_rows_of_rank, unpack_strip16_host, unpack_strip_host)


def build(force=False):
    """Compile the HIP sources for gfx950 into libsdfr.so (in-tree)."""
    from . import buildlib as _build

    return _build.build(force=force)

"""CPU tier: the C-ABI library builds for gfx950, loads, exports every symbol that
include/sdfr.h declares, and refuses to work without a GPU (no CPU fallback).  The Python binding's table of functions agrees with the
header's prototypes, and its mirrors of the header's structs agree with what the host compiler lays out."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import cppbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import sdf_playground_amd as sp

    sp.build()
    return sp.load_library()


def test_header_symbols_are_exported(lib):
    import sdf_playground_amd as sp

    header = open(os.path.join(ROOT, "include", "sdfr.h")).read()
    declared = sorted(set(re.findall(r"^(?:int|void|int64_t|const char \*)\s*(sdfr_[a-z_0-9]+)\(", header, re.M)))
    assert declared == sorted(sp.EXPORTED_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name


def _header():
    """include/sdfr.h without its comments"""
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "sdfr.h")).read(), flags=re.S)


def _c_class(text, returned=False):
    """what a prototype passes in a parameter, or returns: pointer, int32, int64, size_t, float, double, void"""
    if "*" in text or "[" in text:  # (an array parameter is a pointer)
        return "pointer"
    words = [w for w in text.split() if w != "const"]
    return {"int": "int32", "int32_t": "int32", "uint32_t": "int32", "int64_t": "int64", "size_t": "size_t", "float": "float", "double": "double",
            "void": "void"}[" ".join(words if returned else words[:-1])]  # (without the parameter's name)


def _ctypes_class(t):
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "pointer"
    return {ctypes.c_int: "int32", ctypes.c_uint32: "int32", ctypes.c_int64: "int64", ctypes.c_size_t: "size_t", ctypes.c_float: "float",
            ctypes.c_double: "double"}[t]


def test_table_rows_match_the_header_prototypes(lib):
    """every prototype of the header against its row of the binding's table: the number of parameters, what each one passes, what comes back"""
    from sdf_playground_amd import _abi

    assert ctypes.sizeof(ctypes.c_int) == 4 and ctypes.sizeof(ctypes.c_int64) == 8 and ctypes.c_int64 is not ctypes.c_size_t
    prototypes = re.findall(r"^(int|void|int64_t|const char \*)\s*(sdfr_[a-z_0-9]+)\(([^;{]*?)\)\s*;", _header(), re.M)
    assert sorted(name for _ret, name, _params in prototypes) == sorted(_abi.ABI)
    for ret, name, params in prototypes:
        restype, argtypes = _abi.ABI[name]
        declared = [] if params.strip() == "void" else [_c_class(p) for p in params.split(",")]
        assert [_ctypes_class(t) for t in argtypes] == declared, name
        assert _ctypes_class(restype) == _c_class(ret, returned=True), name
        fn = getattr(lib, name)  # load_library gave the function its row
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def _mirrors():
    """every struct the header defines -> the package's mirror of it: a ctypes Structure or a numpy record dtype"""
    import sdf_playground_amd as sp
    from sdf_playground_amd import _abi

    return {"sdfr_variable": _abi._CVariable, "sdfr_timing": _abi._CTiming, "sdfr_limits": sp.Limits, "sdfr_stats": sp.Stats,
            "sdfr_mesh_grid": sp.MeshGrid, "sdfr_mesh_counts": sp.MeshCounts, "sdfr_mesh_survey_result": sp.MeshSurvey, "sdfr_mesh_fit_result": sp.MeshFit,
            "sdfr_slice_grid": sp.SliceGrid, "sdfr_slice_counts": sp.SliceCounts, "sdfr_atlas": sp.Atlas, "sdfr_span_params": sp.SpanParams,
            "sdfr_measure_grid": sp.MeasureGrid, "sdfr_measure_result": sp.MeasureResult, "sdfr_solid_properties": sp.SolidProperties,
            "sdfr_hit": sp.HIT_DTYPE, "sdfr_surface": sp.SURFACE_DTYPE, "sdfr_occlusion": sp.OCCLUSION_DTYPE, "sdfr_lighting": sp.LIGHTING_DTYPE,
            "sdfr_light_sample": sp.LIGHT_SAMPLE_DTYPE, "sdfr_span_summary": sp.SPAN_SUMMARY_DTYPE, "sdfr_measure_column": sp.MEASURE_COLUMN_DTYPE,
            # (the binding has no record for a span: spans are float32 arrays [n, max_spans, 2])
            "sdfr_span": np.dtype([("t_in", np.float32), ("t_out", np.float32)])}


def _python_layout(mirror):
    """[size, then (offset, size) of every field in order]"""
    if isinstance(mirror, np.dtype):
        return [mirror.itemsize] + [(mirror.fields[f][1], mirror.fields[f][0].itemsize) for f in mirror.names]
    return [ctypes.sizeof(mirror)] + [(getattr(mirror, f).offset, getattr(mirror, f).size) for f, _type in mirror._fields_]


def test_mirrors_match_the_compiler_s_layout_of_the_header():
    """one C++ program, generated from the mirrors' field lists and compiled against include/sdfr.h, prints sizeof of every struct and
    offsetof and sizeof of every field"""
    mirrors = _mirrors()
    assert sorted(re.findall(r"^typedef struct (sdfr_\w+)\s*\{", _header(), re.M)) == sorted(mirrors)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "sdfr.h"', 'int main()', '{']
    for name, mirror in mirrors.items():
        fields = mirror.names if isinstance(mirror, np.dtype) else [f for f, _type in mirror._fields_]
        lines.append('\tprintf("%s %%zu", sizeof(%s));' % (name, name))
        lines += ['\tprintf(" %%zu %%zu", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (name, f, name, f) for f in fields]
        lines.append('\tprintf("\\n");')
    lines += ['\treturn 0;', '}', '']
    source = cppbuild.write_if_changed(os.path.join(cppbuild.BUILD, "abi_layout.cpp"), "\n".join(lines))
    header = os.path.join(ROOT, "include", "sdfr.h")
    program = cppbuild.compile(os.path.join(cppbuild.BUILD, "abi_layout"), [source], [header], cppbuild.PLAIN_FLAGS + ["-I" + os.path.dirname(header)],
                               shared=False)
    printed = subprocess.run([program], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(printed) == len(mirrors)
    for line in printed:
        name, size, *pairs = line.split()
        compiled = [int(size)] + [(int(o), int(s)) for o, s in zip(pairs[0::2], pairs[1::2])]
        assert _python_layout(mirrors[name]) == compiled, name


def test_scene_list_matches_reference_stems(lib):
    import sdf_playground_amd as sp

    assert sp.scene_names() == ["fast_sphere", "cube_sea", "labyrinth", "fractal", "lense", "gems", "light_shadows", "cube", "gyroid",
                                "basic_transparency", "basic_clouds", "coordinate_material", "distortion", "table", "sierpinski", "neon",
                                "fractal2", "shell", "spiral", "terrain", "tiling", "tree"]
    # every name is a stem of the reference's scenes directory (SceneManager.cpp:142-158), as recorded in the fixture read from it
    with open(os.path.join(ROOT, "tests", "golden", "reference", "var_tags.json")) as fh:
        stems = set(json.load(fh)["scenes"])
    assert set(sp.scene_names()) == stems  # all 22 scenes of the reference


def test_no_cpu_fallback_without_gpu(lib):
    import torch
    import sdf_playground_amd as sp

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(sp.SdfrError) as e:
        sp.SDFRenderer(0)
    assert e.value.code in (-6, -5)


def test_strip_layout_host_statement():
    import numpy as np
    import sdf_playground_amd as sp

    w, h, world = 5, 29, 3
    n = sp.strip_buffer_pixels_host(w, h, world)
    assert n == 2 * 8 * w  # 4 strips -> 2 per rank
    img = np.arange(h * w * 2, dtype=np.float32).reshape(h, w, 2)
    gathered = np.zeros((world, n // w, w, 2), np.float32)
    for rank in range(world):
        for k, row in enumerate(sp.strip_rows_of_rank(h, rank, world)):
            strip = row // 8
            gathered[rank, (strip // world) * 8 + row % 8] = img[row]
    assert np.array_equal(sp.assemble_strips_host(w, h, world, gathered.reshape(world, n, 2)), img)


def test_no_cpp_exception_crosses_the_c_boundary(lib):
    """every C entry point with a body runs inside guarded() (csrc/sdfr_handle.h): an exception thrown inside the library -- the
    self-test throws a std::runtime_error, a std::bad_alloc and a non-std object on purpose -- comes back as SDFR_ERR_INTERNAL;
    a ctypes (or C) caller would otherwise die of std::terminate.  Needs no device."""
    for what in (0, 1, 2):
        assert lib.sdfr_selftest_exception(None, what) == -9
    assert lib.sdfr_selftest_exception(None, 3) == 0

"""CPU tier: the one list of query kernel kinds (sdf_playground_amd/csrc/sdfr_query_args.h: SDFR_FOR_EACH_QUERY_KERNEL) and what is generated from
it -- the QUERY_KERNEL_* enum, the kernels' argument type, the kernel lines and symbols of a run-time scene's query module (sdfr_jit_unit.h) --
through the stand-alone program tests/cpp/query_kernels_host.cpp, which is built without a HIP header on the include path.  The built-in
scenes' unit is generated from the same list by the preprocessor (sdfr_query_scene.hip); the GPU tier compares the two
(test_gpu_query_kernels.py)."""
import re
import subprocess

import pytest

import cppbuild
import query_kernels_util as ku

# the list, in its order: a kind's number is part of nothing persistent, but the plan table and the tools name kinds and kernels by these
ROWS = [("POINTS", "query_points", "query_points_kernel", "QueryArgs"),
        ("RAYS", "query_rays", "query_rays_kernel", "QueryArgs"),
        ("LATTICE", "query_lattice", "query_lattice_kernel", "LatticeArgs"),
        ("SURFACES", "query_surfaces", "query_surfaces_kernel", "QueryArgs"),
        ("OCCLUSION", "query_occlusion", "query_occlusion_kernel", "QueryArgs"),
        ("LIGHTING", "query_lighting", "query_lighting_kernel", "QueryArgs"),
        ("ATLAS", "bake_atlas", "atlas_bake_kernel", "AtlasArgs"),
        ("MESH_SHARP", "mesh_sharp", "mesh_sharp_kernel", "MeshSharpArgs"),
        ("SLICES", "query_slices", "query_slices_kernel", "SliceArgs"),
        ("SPANS", "query_spans", "query_spans_kernel", "SpanArgs"),
        ("MEASURE", "query_measure", "query_measure_kernel", "MeasureArgs")]
# sizeof each arguments struct, as sdfr_query_args.h pins it with a static_assert
PINNED = {"QueryArgs": 112, "LatticeArgs": 40, "MeshSharpArgs": 56, "AtlasArgs": 104, "SliceArgs": 72, "SpanArgs": 72, "MeasureArgs": 96}


@pytest.fixture(scope="module")
def rep():
    return ku.report()


def test_the_kinds_are_numbered_in_the_lists_order(rep):
    assert rep.kinds == 11 == len(rep.rows)
    assert [r.index for r in rep.rows] == list(range(11))
    assert [(r.name, r.stem, r.body, r.args) for r in rep.rows] == ROWS


def test_every_kernel_of_the_plan_table_names_a_row(rep):
    """k_query_kinds[].kernel (sdfr_query_plan.h), as query_plan_host prints it for a plain request of each kind of query"""
    exe = cppbuild.plan_program("query_plan_host")
    # kind n on_host reach bias width height want_surfaces range, then pos dir pixels distance normals hits surfaces hit_items occlusion
    requests = {"POINTS": "0 1 0 0 0 0 0 0 9  1 0 0 2 0 0 0 0 0", "RAYS": "1 1 0 0 0 0 0 0 9  1 2 0 0 0 3 0 0 0", "PICK": "2 1 0 0 0 4 4 0 9  0 0 1 0 0 3 0 0 0",
                "FRAME": "3 16 0 0 0 4 4 0 9  0 0 0 0 0 3 0 0 0", "MESH": "4 1 0 1 0 0 0 0 9  1 2 0 0 0 3 0 0 0", "OCCLUSION": "5 1 0 1 0 0 0 0 9  1 2 0 0 0 0 0 0 5",
                "HIT_OCCLUSION": "6 1 0 1 0 0 0 0 9  0 0 0 0 0 0 0 6 5"}
    out = subprocess.run([exe], input="".join(v + "\n" for v in requests.values()), check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(requests) == 7
    named = {}
    for what, line in zip(requests, out):
        fields = line.split(";")
        assert fields[0] == "0" and fields[1] == "", (what, line)
        named[what] = rep.rows[int(fields[2])].name  # (an index past the list fails here)
    assert named == {"POINTS": "POINTS", "RAYS": "RAYS", "PICK": "RAYS", "FRAME": "RAYS", "MESH": "RAYS", "OCCLUSION": "OCCLUSION", "HIT_OCCLUSION": "OCCLUSION"}


LINE = re.compile(r'extern "C" __global__ SDFR_PIXEL_KERNEL_ATTRS\(Scene\) void (\w+)\((.+) (\w+)\) \{ (\w+)<Scene, (true|false)>\((\w+)\); \}$')


def test_the_query_unit_has_two_kernels_per_row(rep):
    assert len(rep.query) == 2 * len(rep.rows)
    got = []
    for line in rep.query:
        m = LINE.match(line)
        assert m, line
        symbol, type_, param, body, dbg, passed = m.groups()
        assert param == passed
        got.append((symbol, type_, body, dbg))
    assert len({g[0] for g in got}) == len(got)
    # of every kind the plain kernel, then the debug one, in the list's order
    want = []
    for r in rep.rows:
        want.append(("sdfr_jit_" + r.stem, "SceneKernelArgs<%s>" % r.args, r.body, "false"))
        want.append(("sdfr_jit_" + r.stem + "_debug", "SceneKernelArgs<%s>" % r.args, r.body, "true"))
    assert got == want


def test_the_pixel_unit_has_its_three_kernels(rep):
    assert len(rep.pixel) == 3
    assert rep.pixel[0].startswith('extern "C" __global__ void sdfr_jit_prepare(FrameU *U) ')
    got = [LINE.match(line).groups() for line in rep.pixel[1:]]
    assert got == [("sdfr_jit_pixel", "PixelKernelArgs", "args", "pixel_kernel", "false", "args"),
                   ("sdfr_jit_pixel_debug", "PixelKernelArgs", "args", "pixel_kernel", "true", "args")]


def test_a_kernels_argument_is_the_frame_then_the_arguments(rep):
    assert rep.frame % 8 == 0  # the arguments, which hold pointers, follow the frame without padding
    for r in rep.rows:
        assert r.align == 8, r
        assert r.size == (rep.frame + PINNED[r.args] + r.align - 1) // r.align * r.align, r

"""CPU tier: how one device buffer is cut into the stand-ins of a caller's host arrays (sdf_playground_amd/csrc/sdfr_stage.h, built as
the stand-alone program tests/cpp/stage_host.cpp).  The offsets and totals of the header against the formulas the entry points
carried before they shared it (query_impl, mesh_impl and atlas_impl), spelled out here a second time."""
import subprocess

import pytest

import cppbuild
POINTS, RAYS, PICK = 0, 1, 2
HIT_BYTES = 48


@pytest.fixture(scope="module")
def exe():
    return cppbuild.plan_program("stage_host")


def carve(exe, lists):
    """[[bytes of each piece]] -> [(offsets, total)]"""
    text = "".join(" ".join(str(b) for b in pieces) + "\n" for pieces in lists)
    lines = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(lists)
    return [([int(x) for x in l.split()[:-1]], int(l.split()[-1])) for l in lines]


def up(b):
    return (b + 255) & ~255


def test_query_staging(exe):
    """query_impl: inputs, then answers -- in0, in1, out0, out1"""
    cases, want = [], []
    for kind in (POINTS, RAYS, PICK):
        for normals in (False, True):
            for n in (1, 21, 64, 65, 1000):
                in0 = n * 8 if kind == PICK else n * 12
                in1 = n * 12 if kind == RAYS else 0
                out0 = n * 4 if kind == POINTS else n * HIT_BYTES
                out1 = n * 12 if kind == POINTS and normals else 0
                cases.append([in0, in1, out0, out1])
                d_in1 = up(in0)
                d_out0 = d_in1 + up(in1)
                d_out1 = d_out0 + up(out0)
                want.append(([0, d_in1, d_out0, d_out1], up(in0) + up(in1) + up(out0) + up(out1)))
    assert len(cases) == 30
    assert carve(exe, cases) == want


def test_mesh_staging(exe):
    """mesh_impl's host arrays: positions, normals (or none), indices"""
    cases, want = [], []
    for V, T in ((1, 0), (5, 6), (1000, 1996)):
        for normals in (False, True):
            b_pos = up(V * 12)
            b_nrm = up(V * 12) if normals else 0
            cases.append([V * 12, V * 12 if normals else 0, T * 12])
            want.append(([0, b_pos, b_pos + b_nrm], b_pos + b_nrm + up(T * 12)))
    assert carve(exe, cases) == want


def test_an_empty_piece_takes_no_room(exe):
    assert carve(exe, [[100, 0, 300], [256, 0, 0, 1], [0, 0, 7], []]) == [([0, 256, 256], 768), ([0, 256, 256, 256], 512), ([0, 0, 0], 256), ([], 0)]


def test_atlas_staging(exe):
    """atlas_impl's host arrays: positions, normals, indices, then the answers -- of a bake the planes of its layers and valid, of the
    texel call the texels' positions, normals and valid, and no seventh"""
    cases, want = [], []
    for V, T in ((5, 6), (1000, 1996)):
        for width, height in ((8, 8), (64, 16)):
            texels = width * height
            answers = [[texels * 12, texels * 12, texels * 4, 0]]  # sdfr_atlas_texels
            for layers in range(1, 8):  # sdfr_atlas_bake: albedo 1, normal 2, lit 4
                answers.append([texels * 16 if layers & bit else 0 for bit in (1, 2, 4)] + [texels * 4])
            for out in answers:
                pieces = [V * 12, V * 12, T * 12] + out
                cases.append(pieces)
                d_normals = up(V * 12)
                d_indices = d_normals + up(V * 12)
                d_out0 = d_indices + up(T * 12)
                d_out1 = d_out0 + up(out[0])
                d_out2 = d_out1 + up(out[1])
                d_out3 = d_out2 + up(out[2])
                want.append(([0, d_normals, d_indices, d_out0, d_out1, d_out2, d_out3], d_out3 + up(out[3])))
    assert len(cases) == 2 * 2 * 8 and all(len(c) == 7 for c in cases)
    assert carve(exe, cases) == want
    # written out: V = 5, T = 6 at 8 x 8 texels, the texel call and a bake of albedo and lit
    assert carve(exe, [[60, 60, 72, 768, 768, 256, 0], [60, 60, 72, 1024, 0, 1024, 256]]) == [([0, 256, 512, 768, 1536, 2304, 2560], 2560),
                                                                                            ([0, 256, 512, 768, 1792, 1792, 2816], 3072)]

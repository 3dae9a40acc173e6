"""CPU tier: the plan of the lighting entries (sdf_playground_amd/csrc/sdfr_query_plan.h with QueryRequest::want_lighting, built as the
stand-alone program tests/cpp/lighting_plan_host.cpp): `lighting` required, `hits` and `lights` optional, `surfaces` never taken, the
six staging sizes, the lighting kernel, one launch of a block per 64 items or per 8 x 8 tile of the frame, and the argument errors in the
order of the other queries.  tests/test_query_plan_cpu.py keeps checking the requests that existed before, through its own program."""
import struct
import subprocess

import pytest

import cppbuild

RAYS, PICK, FRAME, MESH = 1, 2, 3, 4
KERNEL_LIGHTING = 5
MEMBERS = ("pos", "dir", "pixels", "hits", "surfaces", "lighting", "lights")
BYTES = dict(pos=12, dir=12, pixels=8, hits=48, surfaces=128, lighting=64, lights=640)
INVALID = -1
RANGE = "37.5"


@pytest.fixture(scope="module")
def exe():
    return cppbuild.plan_program("lighting_plan_host")


def plans(exe, requests):
    """requests: (kind, n, on_host, reach, width, height, {member: code}) -> the program's answers, split at ';'"""
    text = "".join("%d %d %d %s %d %d %s %s\n" % (k, n, host, reach, w, h, RANGE, " ".join(str(arrays.get(m, 0)) for m in MEMBERS))
                   for k, n, host, reach, w, h, arrays in requests)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(requests)
    return [line.split(";") for line in out]


def entry(kind, n, arrays, reach="0", width=0, height=0, on_host=0):
    return (kind, n, on_host, reach, width, height, arrays)


INPUTS = {RAYS: dict(pos=1, dir=2), PICK: dict(pixels=3), FRAME: {}, MESH: dict(pos=1, dir=2)}


def valid(kind, n, hits=True, lights=True, on_host=0):
    arrays = dict(INPUTS[kind], lighting=6)
    if hits:
        arrays["hits"] = 4
    if lights:
        arrays["lights"] = 7
    if kind == FRAME:
        return entry(kind, n, arrays, width=n, height=1, on_host=on_host)
    return entry(kind, n, arrays, reach="0.25" if kind == MESH else "0", width=9 if kind == PICK else 0, height=7 if kind == PICK else 0, on_host=on_host)


@pytest.mark.parametrize("kind", [RAYS, PICK, FRAME, MESH])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2000])
def test_valid_requests(exe, kind, n):
    for hits in (False, True):
        for lights in (False, True):
            req = valid(kind, n, hits, lights, on_host=1)
            (ans,) = plans(exe, [req])
            arrays = req[6]
            assert ans[0] == "0" and ans[1] == "" and int(ans[2]) == KERNEL_LIGHTING
            w, h = (req[4], req[5]) if kind in (PICK, FRAME) else (1, 1)
            assert ans[3] == "%d %d" % (w, h)
            ins = [m for m in ("pos", "dir", "pixels") if m in arrays] + [None, None]
            sizes = [n * BYTES[m] if m else 0 for m in ins[:2]] + [n * 48 if hits else 0, 0, n * 64, n * 640 if lights else 0]
            assert [int(x) for x in ans[4].split()] == sizes
            dist_max = {RAYS: float(RANGE), PICK: float(RANGE), FRAME: float(RANGE), MESH: 0.25}[kind]
            assert ans[5] == "%d %08x" % (n, struct.unpack("I", struct.pack("f", dist_max))[0])
            want_ptrs = [arrays.get(m, 0) << 44 for m in MEMBERS]
            assert [int(x, 16) for x in ans[6].split()] == want_ptrs
            # one launch: a block per 64 items, or per 8 x 8 tile of the frame; the arrays as they are
            assert len(ans) == 8
            first, count, blocks, ln, *ptrs = ans[7].split()
            blocks_want = ((w + 7) // 8) * ((h + 7) // 8) if kind == FRAME else (n + 63) // 64
            assert (int(first), int(count), int(blocks), int(ln)) == (0, n, blocks_want, n)
            assert [int(x, 16) for x in ptrs] == want_ptrs


def test_frame_grid(exe):
    for w, h in ((61, 45), (8, 8), (9, 1), (3840, 2160)):
        (ans,) = plans(exe, [entry(FRAME, w * h, dict(lighting=6), width=w, height=h)])
        assert ans[0] == "0" and int(ans[7].split()[2]) == ((w + 7) // 8) * ((h + 7) // 8)
    wrong = plans(exe, [entry(FRAME, n, dict(lighting=6), width=8, height=8) for n in (1, 63, 65)])
    assert all(a[:2] == [str(INVALID), "without a pixel list n must be width * height"] for a in wrong)


def test_surfaces_are_not_taken(exe):
    # a surfaces pointer in a lighting request is dropped: not staged, not handed to the kernel, and the kernel is the lighting kernel
    (ans,) = plans(exe, [entry(RAYS, 5, dict(pos=1, dir=2, surfaces=5, lighting=6), on_host=1)])
    assert ans[0] == "0" and int(ans[2]) == KERNEL_LIGHTING and ans[4].split()[3] == "0" and int(ans[6].split()[4], 16) == 0


def test_errors_and_their_order(exe):
    nothing = plans(exe, [entry(k, 0, {}, reach="0.5" if k == MESH else "0", width=4, height=4) for k in (RAYS, PICK, FRAME, MESH)])
    assert all(a == ["0", ""] for a in nothing)  # n = 0: nothing to do, null pointers allowed
    null = "null pointer"
    cases = [
        (valid(RAYS, 3)[:6] + (dict(pos=1, dir=2, hits=4, lights=7),), null),  # no lighting
        (valid(PICK, 3)[:6] + (dict(pixels=3, hits=4, surfaces=5),), null),  # surfaces do not stand in for it
        (valid(FRAME, 3)[:6] + (dict(hits=4),), null),
        (valid(MESH, 3)[:6] + (dict(pos=1, lighting=6),), null),  # no normals
        (valid(RAYS, 3)[:6] + (dict(dir=2, lighting=6),), null),
        (valid(PICK, 3)[:6] + (dict(lighting=6),), null),  # the pick kind needs its pixels
        (entry(RAYS, -1, dict(pos=1, dir=2, lighting=6)), "bad item count"),
        (entry(RAYS, 2 ** 31, dict(pos=1, dir=2, lighting=6)), "bad item count"),
        (entry(RAYS, 3, dict(pos=1, dir=2, lighting=6), on_host=2), "on_host must be 0 or 1"),
        (entry(RAYS, 3, dict(pos=1, dir=2, lighting=6), reach="-1"), "max_distance must be finite and >= 0"),
        (entry(RAYS, 3, dict(pos=1, dir=2, lighting=6), reach="nan"), "max_distance must be finite and >= 0"),
        (entry(MESH, 3, dict(pos=1, dir=2, lighting=6), reach="0"), "reach must be finite and > 0"),
        (entry(MESH, 3, dict(pos=1, dir=2, lighting=6), reach="inf"), "reach must be finite and > 0"),
        (entry(PICK, 3, dict(pixels=3, lighting=6), width=0, height=4), "bad frame size"),
        # the order: the count before on_host before the reach before the frame before the pointers
        (entry(MESH, -1, {}, reach="0", on_host=7), "bad item count"),
        (entry(MESH, 1, {}, reach="0", on_host=7), "on_host must be 0 or 1"),
        (entry(PICK, 1, {}, reach="-1", width=0, height=0), "max_distance must be finite and >= 0"),
        (entry(PICK, 1, {}, width=0, height=0), "bad frame size"),
    ]
    for (req, text), ans in zip(cases, plans(exe, [c[0] for c in cases])):
        assert ans == [str(INVALID), text], (req, ans)

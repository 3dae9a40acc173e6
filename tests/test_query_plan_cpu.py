"""CPU tier: the table of query kinds and the plan of one query call (sdf_playground_amd/csrc/sdfr_query_plan.h, built as the stand-alone
program tests/cpp/query_plan_host.cpp).  The rules query_impl and launch_query carried as chains of conditionals before they shared the
table are spelled out here a second time (parent_rules: the statuses, the error texts, the sizes, the kernel, the grids and the split of
an occlusion query into launches), and the plan has to agree with them for every kind, every argument fault and every size below.
The split of more than 2^25 occlusion items into several launches is checked here as arithmetic only: no device has run it."""
import math
import struct
import subprocess

import pytest

import cppbuild


POINTS, RAYS, PICK, FRAME, MESH, OCCLUSION, HIT_OCCLUSION = range(7)
KERNEL_POINTS, KERNEL_RAYS, KERNEL_LATTICE, KERNEL_SURFACES, KERNEL_OCCLUSION = range(5)
MEMBERS = ("pos", "dir", "pixels", "distance", "normals", "hits", "surfaces", "hit_items", "occlusion")
INVALID = -1  # SDFR_ERR_INVALID_ARGUMENT
RANGE = "37.5"
PER_LAUNCH = 1 << 25
INT32_MAX = 2 ** 31 - 1


def _exe(name, flags):
    return cppbuild.plan_program("query_plan_host", name, flags)


@pytest.fixture(scope="module")
def exe():
    return _exe("query_plan_host", [])


# ---- requests, as the entry points of sdfr_api.cpp make them ----------------------------------------------------------------------
def request(kind, n=1, on_host=0, reach="0", bias="0", width=0, height=0, want=0, **arrays):
    """arrays: member -> 1 .. 6 (an address); every other member is null"""
    assert set(arrays) <= set(MEMBERS)
    return dict(kind=kind, n=n, on_host=on_host, reach=reach, bias=bias, width=width, height=height, want=want, arrays=dict(arrays))


def entry_requests(n=1, optional=True):
    """{entry point: a valid request of n items}; optional: with the optional answer"""
    opt = 3 if optional else 0
    return {
        "sdfr_query_distance": request(POINTS, n, pos=1, distance=2, normals=opt),
        "sdfr_query_rays": request(RAYS, n, reach="2.5", pos=1, dir=2, hits=3),
        "sdfr_pick": request(PICK, n, width=9, height=7, pixels=1, hits=3),
        "sdfr_query_ray_surfaces": request(RAYS, n, reach="0", want=1, pos=1, dir=2, hits=opt, surfaces=4),
        "sdfr_pick_surfaces": request(PICK, n, width=9, height=7, want=1, pixels=1, hits=opt, surfaces=4),
        "sdfr_pick_surfaces (frame)": request(FRAME, n, width=n, height=1, want=1, hits=opt, surfaces=4),
        "sdfr_mesh_surfaces": request(MESH, n, reach="0.25", want=1, pos=1, dir=2, hits=opt, surfaces=4),
        "sdfr_query_occlusion": request(OCCLUSION, n, reach="1.5", bias="0.01", pos=1, dir=2, occlusion=5),
        "sdfr_hit_occlusion": request(HIT_OCCLUSION, n, reach="1.5", bias="0", hit_items=6, occlusion=5),
    }


def changed(req, **fields):
    out = dict(req, arrays=dict(req["arrays"]))
    for k, v in fields.items():
        if k in MEMBERS:
            out["arrays"][k] = v
        else:
            out[k] = v
    return out


def line_of(req):
    a = req["arrays"]
    return "%d %d %d %s %s %d %d %d %s %s" % (req["kind"], req["n"], req["on_host"], req["reach"], req["bias"], req["width"], req["height"], req["want"],
                                              RANGE, " ".join(str(a.get(m, 0)) for m in MEMBERS))


def f32(text):
    return struct.unpack("f", struct.pack("f", float(text)))[0]


def f32_bits(v):
    return struct.unpack("I", struct.pack("f", v))[0]


# ---- the rules of the code before the table: query_impl (sdfr_api.cpp) and launch_query (sdfr_kernels.hip) ---------------------------
def parent_rules(req):
    """-> (status, text, plan or None); plan: kernel, frame, bytes [4], q (kind, n, dist_max, reach, bias, pointers by member as byte
    addresses), launches [(first, count, blocks, pointers)], host (the members a host call points at staging pieces)"""
    kind, n, w, h = req["kind"], req["n"], req["width"], req["height"]
    p = {m: req["arrays"].get(m, 0) << 44 for m in MEMBERS}
    reach, bias = f32(req["reach"]), f32(req["bias"])
    of_occlusion = kind in (OCCLUSION, HIT_OCCLUSION)
    of_pixels = kind in (PICK, FRAME)
    of_rays = kind in (RAYS, MESH, OCCLUSION)
    if n < 0 or n > INT32_MAX:
        return INVALID, "bad item count", None
    if req["on_host"] not in (0, 1):
        return INVALID, "on_host must be 0 or 1", None
    if kind == MESH or of_occlusion:
        bad = not (math.isfinite(reach) and reach > 0)
    else:
        bad = not math.isfinite(reach) or reach < 0
    if bad:
        return INVALID, ("radius must be finite and > 0" if of_occlusion else "reach must be finite and > 0" if kind == MESH else "max_distance must be finite and >= 0"), None
    if of_occlusion and not (math.isfinite(bias) and bias >= 0):
        return INVALID, "bias must be finite and >= 0", None
    if of_pixels and not (w >= 1 and h >= 1 and w * h <= 1 << 30):
        return INVALID, "bad frame size", None
    if n == 0:
        return 0, "", None
    if kind == FRAME and n != w * h:
        return INVALID, "without a pixel list n must be width * height", None
    if kind == POINTS:
        inputs_ok = p["pos"] != 0
    elif of_rays:
        inputs_ok = p["pos"] != 0 and p["dir"] != 0
    elif kind == HIT_OCCLUSION:
        inputs_ok = p["hit_items"] != 0
    else:
        inputs_ok = kind == FRAME or p["pixels"] != 0
    outputs_ok = p["distance"] != 0 if kind == POINTS else p["occlusion"] != 0 if of_occlusion else p["surfaces"] != 0 if req["want"] else p["hits"] != 0
    if not inputs_ok or not outputs_ok:
        return INVALID, "null pointer", None

    in0 = 0 if kind == FRAME else n * 8 if kind == PICK else n * 48 if kind == HIT_OCCLUSION else n * 12
    in1 = n * 12 if of_rays else 0
    out0 = n * 4 if kind == POINTS else n * 16 if of_occlusion else n * 48 if p["hits"] else 0
    out1 = (n * 12 if p["normals"] else 0) if kind == POINTS else n * 128 if p["surfaces"] else 0
    kernel = KERNEL_OCCLUSION if of_occlusion else KERNEL_POINTS if kind == POINTS else KERNEL_SURFACES if p["surfaces"] else KERNEL_RAYS
    frame = (w, h) if of_pixels else (1, 1)
    q = dict(p, kind=kind, n=n, dist_max=f32(RANGE) if reach == 0 else reach, reach=reach, bias=bias)
    # the members the nine lines of the host path pointed at staging pieces; every other one they set to null
    host = set()
    if not (of_pixels or kind == HIT_OCCLUSION):
        host.add("pos")
    if kind == HIT_OCCLUSION:
        host.add("hit_items")
    if kind == PICK:
        host.add("pixels")
    if in1:
        host.add("dir")
    if kind == POINTS:
        host.add("distance")
    if kind == POINTS and out1:
        host.add("normals")
    if kind != POINTS and not of_occlusion and out0:
        host.add("hits")
    if of_occlusion:
        host.add("occlusion")
    if kind != POINTS and out1:
        host.add("surfaces")

    launches = []
    if of_occlusion:
        for first in range(0, n, PER_LAUNCH):
            count = min(n - first, PER_LAUNCH)
            at = dict(p)
            for member, per_item in (("pos", 12), ("dir", 12), ("hit_items", 48)):
                at[member] = p[member] + per_item * first if p[member] else 0
            at["occlusion"] = p["occlusion"] + 16 * first
            launches.append((first, count, count, at))
    else:
        blocks = ((n + 63) & 0xFFFFFFFF) // 64
        if kind == FRAME:
            blocks = ((frame[0] + 7) >> 3) * ((frame[1] + 7) >> 3)
        launches.append((0, n, blocks, dict(p)))
    return 0, "", dict(kernel=kernel, frame=frame, bytes=[in0, in1, out0, out1], q=q, launches=launches, host=host)


def expected_line(req):
    status, text, plan = parent_rules(req)
    out = "%d;%s" % (status, text)
    if plan:
        q = plan["q"]
        ptrs = lambda a: "".join(" %x" % a[m] for m in MEMBERS)  # noqa: E731
        out += ";%d;%d %d;%d %d %d %d;%d %d %08x %08x %08x;" % ((plan["kernel"],) + plan["frame"] + tuple(plan["bytes"])
                                                                 + (q["kind"], q["n"], f32_bits(q["dist_max"]), f32_bits(q["reach"]), f32_bits(q["bias"])))
        out += ptrs(q)
        for first, count, blocks, at in plan["launches"]:
            out += ";%d %d %d %d" % (first, count, blocks, count) + ptrs(at)
    return out


def run(exe, reqs):
    text = "".join(line_of(r) + "\n" for r in reqs)
    lines = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(reqs)
    return lines


def parse_launches(line):
    """[(first, count, blocks, n, {member: address})] of an answer line"""
    out = []
    for part in line.split(";")[7:]:
        w = part.split()
        out.append((int(w[0]), int(w[1]), int(w[2]), int(w[3]), dict(zip(MEMBERS, (int(x, 16) for x in w[4:])))))
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def fault_cases():
    """every entry point x every argument fault query_impl knows, at n = 1 and n = 0"""
    cases = []
    for name, ok in entry_requests().items():
        kind = ok["kind"]
        takes_zero = kind in (POINTS, RAYS, PICK, FRAME)
        for n in (1, 0):
            base = changed(ok, n=n, width=ok["width"] if kind != FRAME or n else 1)
            faults = [dict(n=-1), dict(n=2 ** 31), dict(on_host=2), dict(on_host=-1), dict(on_host=1)]
            faults += [dict(reach=v) for v in ("0", "-1", "inf", "nan", "-inf", "-0.0")]
            faults += [dict(bias=v) for v in ("-0.5", "inf", "nan", "0")]
            faults += [dict(width=0, height=1), dict(width=1, height=0), dict(width=2 ** 15, height=2 ** 15 + 1), dict(width=2 ** 15, height=2 ** 15)]
            faults += [dict(n=n + 1), dict(width=3, height=5, n=14), dict(width=3, height=5, n=15)]  # a frame's n != width * height
            faults += [{m: 0} for m in MEMBERS if ok["arrays"].get(m)]  # each pointer the entry passes, null in turn (required or optional)
            # two faults at once: the one that wins is part of the behaviour
            faults += [dict(n=-1, on_host=2), dict(on_host=2, reach="nan"), dict(reach="nan", bias="nan"), dict(bias="nan", width=0), dict(width=0, pos=0, pixels=0, hit_items=0)]
            for f in faults:
                cases.append(("%s n=%d %r" % (name, n, f), changed(base, **f)))
            assert takes_zero or parent_rules(changed(base, reach="0"))[0] == INVALID
    return cases


def valid_cases():
    cases = []
    for optional in (True, False):
        for n in (1, 21, 64, 65, 1000):
            for name, r in entry_requests(n, optional).items():
                for on_host in (0, 1):
                    cases.append(("%s n=%d optional=%d on_host=%d" % (name, n, optional, on_host), changed(r, on_host=on_host)))
    return cases


def grid_cases():
    cases = [(n, request(kind, n, reach=reach, want=want, **arrays)) for n in (1, 63, 64, 65, INT32_MAX)
             for kind, reach, want, arrays in ((POINTS, "0", 0, dict(pos=1, distance=2)), (RAYS, "0", 0, dict(pos=1, dir=2, hits=3)),
                                               (MESH, "1", 1, dict(pos=1, dir=2, surfaces=4)))]
    cases += [(n, request(PICK, n, width=16, height=16, pixels=1, hits=3)) for n in (1, 63, 64, 65, INT32_MAX)]
    return cases


FRAMES = ((1, 1, 1), (8, 8, 1), (9, 7, 2), (3840, 2160, 480 * 270))
SPLIT_N = (1, PER_LAUNCH - 1, PER_LAUNCH, PER_LAUNCH + 1, 2 * PER_LAUNCH, 2 * PER_LAUNCH + 5, INT32_MAX)


def split_cases():
    return [request(OCCLUSION, n, reach="1", bias="0", pos=1, dir=2, occlusion=5) for n in SPLIT_N] + \
           [request(HIT_OCCLUSION, n, reach="1", bias="0", hit_items=6, occlusion=5) for n in SPLIT_N]


def frame_cases():
    return [request(FRAME, w * h, width=w, height=h, want=1, hits=3, surfaces=4) for w, h, _tiles in FRAMES]


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
def test_argument_faults(exe):
    """the same status and the same text as query_impl gave, whichever fault wins; n = 0 is fine only once the scalars are"""
    cases = fault_cases()
    assert len(cases) > 500
    got = run(exe, [r for _what, r in cases])
    texts = set()
    for (what, r), line in zip(cases, got):
        assert line == expected_line(r), what
        texts.add(line.split(";")[1])
    assert texts == {"", "bad item count", "on_host must be 0 or 1", "max_distance must be finite and >= 0", "reach must be finite and > 0",
                     "radius must be finite and > 0", "bias must be finite and >= 0", "bad frame size", "without a pixel list n must be width * height",
                     "null pointer"}
    # a bad radius with n = 0 is still an error; an optional pointer may be null
    assert run(exe, [request(OCCLUSION, 0, reach="0", pos=1, dir=2, occlusion=5)]) == ["-1;radius must be finite and > 0"]
    assert run(exe, [request(OCCLUSION, 0, reach="1", pos=1, dir=2, occlusion=5)]) == ["0;"]
    assert run(exe, [request(RAYS, 1, want=1, pos=1, dir=2, surfaces=4)])[0].startswith("0;;%d;" % KERNEL_SURFACES)
    assert run(exe, [request(RAYS, 1, want=1, pos=1, dir=2, hits=3)]) == ["-1;null pointer"]


def test_valid_requests(exe):
    """sizes in staging order, kernel, dist_max and the kernel's arguments: the caller's pointers where the kind takes them, null elsewhere"""
    cases = valid_cases()
    assert len(cases) == 2 * 5 * 9 * 2
    got = run(exe, [r for _what, r in cases])
    for (what, r), line in zip(cases, got):
        assert line == expected_line(r), what
        plan = parent_rules(r)[2]
        # what a host call stages -- the arrays with a size -- are the members the host path used to re-point, and no other is non-null
        sizes = [int(x) for x in line.split(";")[4].split()]
        pointers = dict(zip(MEMBERS, (int(x, 16) for x in line.split(";")[6].split())))
        assert {m for m in MEMBERS if pointers[m]} == plan["host"], what
        assert sum(1 for b in sizes if b) == len(plan["host"]), what
    # spot values, written out
    by_name = {what: line for (what, _r), line in zip(cases, got)}
    assert by_name["sdfr_query_rays n=21 optional=1 on_host=1"].split(";")[2:5] == ["1", "1 1", "252 252 1008 0"]
    assert by_name["sdfr_query_ray_surfaces n=21 optional=0 on_host=0"].split(";")[2:5] == ["3", "1 1", "252 252 0 2688"]
    assert by_name["sdfr_pick_surfaces n=65 optional=1 on_host=0"].split(";")[2:5] == ["3", "9 7", "520 0 3120 8320"]
    assert by_name["sdfr_hit_occlusion n=1000 optional=1 on_host=1"].split(";")[2:5] == ["4", "1 1", "48000 0 16000 0"]
    assert by_name["sdfr_query_distance n=64 optional=0 on_host=0"].split(";")[2:5] == ["0", "1 1", "768 0 256 0"]
    # dist_max: the range for max_distance 0, else the reach
    assert by_name["sdfr_query_ray_surfaces n=1 optional=1 on_host=0"].split(";")[5].split()[2] == "%08x" % f32_bits(f32(RANGE))
    assert by_name["sdfr_query_rays n=1 optional=1 on_host=0"].split(";")[5].split()[2] == "%08x" % f32_bits(2.5)


def test_grids(exe):
    """a block per 64 items; of a whole frame a block per 8 x 8 tile; of occlusion a block per item"""
    cases = grid_cases()
    got = run(exe, [r for _n, r in cases])
    for (n, r), line in zip(cases, got):
        assert line == expected_line(r)
        assert parse_launches(line) == [(0, n, (n + 63) // 64, n, {m: r["arrays"].get(m, 0) << 44 for m in MEMBERS})]
    assert [parse_launches(l)[0][2] for (n, r), l in zip(cases, got) if r["kind"] == POINTS] == [1, 1, 1, 2, 1 << 25]
    frames = frame_cases()
    got = run(exe, frames)
    for (w, h, tiles), r, line in zip(FRAMES, frames, got):
        assert line == expected_line(r)
        (first, count, blocks, n, _p), = parse_launches(line)
        assert (first, count, blocks, n) == (0, w * h, tiles, w * h)
    for r, line in zip(split_cases(), run(exe, split_cases())):
        assert all(blocks == count for _first, count, blocks, _n, _p in parse_launches(line))


def test_occlusion_split(exe):
    """more than 2^25 items go in several launches: their ranges tile [0, n) in order, and every array is advanced to the launch's
    first item, in 64 bits"""
    cases = split_cases()
    got = run(exe, cases)
    per_item = {"pos": 12, "dir": 12, "hit_items": 48, "occlusion": 16}
    for r, line in zip(cases, got):
        assert line == expected_line(r)
        n, at = r["n"], 0
        launches = parse_launches(line)
        assert len(launches) == (n + PER_LAUNCH - 1) // PER_LAUNCH
        for first, count, blocks, launch_n, pointers in launches:
            assert first == at and 1 <= count <= PER_LAUNCH and count * 64 < 2 ** 32 and launch_n == count and blocks == count
            at += count
            for m in MEMBERS:
                code = r["arrays"].get(m, 0)
                assert pointers[m] == ((code << 44) + per_item[m] * first if code else 0)
        assert at == n
    # the last launch of the largest query of hit records starts past 2^36 bytes
    last = parse_launches(got[-1])[-1]
    assert last[0] == 63 * PER_LAUNCH and last[1] == PER_LAUNCH - 1 and last[4]["hit_items"] - (6 << 44) == 48 * 63 * PER_LAUNCH > 2 ** 36


def test_under_sanitizers(exe):
    """the same program built with the address and undefined-behaviour sanitizers, over every request above: the same answers"""
    reqs = [r for _w, r in fault_cases()] + [r for _w, r in valid_cases()] + [r for _n, r in grid_cases()] + frame_cases() + split_cases()
    checked = _exe("query_plan_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert run(checked, reqs) == run(exe, reqs)

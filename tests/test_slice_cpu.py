"""CPU tier of sdfr_slice_extract: the stage functions of sdf_playground_amd/csrc/sdfr_slice.h, built for the host
(tests/cpp/slice_host.cpp), against the header's definition restated in numpy (tests/slice_util.py), every word equal; chainContours;
the SVG writer; the plan (sdfr_slice_plan.h, built as the stand-alone program tests/cpp/slice_plan_host.cpp, also under the address and
undefined-behaviour sanitizers); the struct layouts; the command line's argument faults."""
import ctypes
import math
import re
import struct
import subprocess

import numpy as np
import pytest

import cppbuild
import query_util as qu
import slice_util as su

F = np.float32
NAN, INF = float("nan"), float("inf")
# (nu, nv, layers): ragged against a wave of 64 and against a block of 256
SHAPES = [(1, 1, 1), (1, 5, 3), (7, 1, 2), (13, 9, 4), (70, 3, 2), (37, 29, 5)]
# an oblique stack: du and dv neither axis-aligned nor of equal length, dw not orthogonal to them
OBLIQUE = dict(origin=(-0.7, 0.31, 1.9), du=(0.11, 0.02, -0.03), dv=(-0.015, 0.09, 0.04), dw=(0.05, -0.02, 0.13))


def _random_lattices(dims, layers, rng):
    """(what, D, iso): special values on a dyadic ladder -- the sums and quotients of the definition are then exact, m == 0 and t on the
    ends of [0, 1] happen, and two diagonal corners inside are common --; a smooth field; that field with the ladder sown in; noise"""
    points = (dims[0] + 1) * (dims[1] + 1) * layers
    iso = 0.125
    ladder = np.array([-0.5, -0.25, -0.0, 0.0, 0.25, 0.5, 0.75, NAN, INF, -INF], np.float32)
    D = (ladder[rng.integers(0, len(ladder), points)] + F(iso)).astype(np.float32)
    yield "ladder", D, iso
    l, j, i = np.meshgrid(np.arange(layers), np.arange(dims[1] + 1), np.arange(dims[0] + 1), indexing="ij")
    p = np.stack([i.ravel(), j.ravel(), l.ravel()], 1).astype(np.float64)
    centre = np.array([dims[0] * 0.45, dims[1] * 0.55, layers * 0.5])
    smooth = (np.linalg.norm((p - centre) * np.array([1.0, 1.0, 2.0]), axis=1) - 0.35 * max(dims)).astype(np.float32)
    sown = smooth.copy()
    where = rng.integers(0, points, max(1, points // 7))
    sown[where] = ladder[rng.integers(0, len(ladder), len(where))]
    yield "smooth", smooth, 0.0
    yield "smooth with special values", sown, 0.0
    yield "noise", rng.normal(0.0, 0.3, points).astype(np.float32), 0.05


def _situations(D, dims, layers, iso):
    """how often the definition's corner cases occur: cells with two OUT sides, such cells with m == 0, clamped t, NaN corners"""
    nu, nv = dims
    with np.errstate(all="ignore"):
        s = (D - F(iso)).reshape(layers, nv + 1, nu + 1)
        inside = s < 0
        c = [a[:, dj:dj + nv, di:di + nu] for a in (s, inside) for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1))]
        two_out = (c[4] == c[6]) & (c[5] == c[7]) & (c[4] != c[5])
        m = ((c[0] + c[1]) + (c[2] + c[3])) * F(0.25)
        clamped = 0
        for axis in (2, 1):
            a, b = np.moveaxis(s, axis, 0)[:-1], np.moveaxis(s, axis, 0)[1:]
            t = a / (a - b)
            clamped += int((((a < 0) != (b < 0)) & ~((t >= 0) & (t <= 1))).sum())
    return int(two_out.sum()), int((two_out & (m == 0)).sum()), clamped, int(np.isnan(s).sum())


def test_host_text_equals_the_definition():
    rng = np.random.default_rng(31)
    seen = np.zeros(4, np.int64)
    for nu, nv, layers in SHAPES:
        dims = (nu, nv)
        for what, D, iso in _random_lattices(dims, layers, rng):
            case = (nu, nv, layers, what)
            want = su.marching_squares(D, dims=dims, layers=layers, iso=iso, **OBLIQUE)
            got = su.host_extract(D, dims=dims, layers=layers, iso=iso, **OBLIQUE)
            for name, g, w in zip(("positions", "coords", "segments", "layer_vertices", "layer_segments"), got, want):
                assert g.shape == w.shape and g.dtype == w.dtype, (case, name)
                if g.dtype == np.float32:
                    qu.assert_same("%s %s" % (case, name), g, w)
                else:
                    assert np.array_equal(g, w), (case, name)
            # coords not wanted: the same positions and segments
            pos, none, seg, _lv, _ls = su.host_extract(D, dims=dims, layers=layers, iso=iso, coords=False, **OBLIQUE)
            assert none is None and np.array_equal(seg, want[2])
            qu.assert_same("%s positions without coords" % (case,), pos, want[0])
            su.check_invariants(D, iso, want[1], want[2], want[3], want[4], dims, layers)
            su.check_invariants(D, iso, got[1], got[2], got[3], got[4], dims, layers)
            if what == "ladder":
                seen += _situations(D, dims, layers, iso)
    two_out, m_zero, clamped, nan_corners = seen
    assert two_out > 100 and m_zero > 5 and clamped > 100 and nan_corners > 100, seen


def test_lattice_points_are_the_definition_s():
    for nu, nv, layers in SHAPES:
        qu.assert_same((nu, nv, layers), su.host_points(dims=(nu, nv), layers=layers, **OBLIQUE), su.lattice_points(dims=(nu, nv), layers=layers, **OBLIQUE))


def test_single_cells():
    """the sixteen corner masks of one cell, with the centre value on either side of zero for the two diagonal ones"""
    axes = dict(origin=(0, 0, 0), du=(1, 0, 0), dv=(0, 1, 0), dw=(0, 0, 1))
    for mask in range(16):
        for strong in (1.0, 3.0):
            # D in point order: (0,0), (1,0), (0,1), (1,1) = c0, c1, c3, c2
            s = {k: (-strong if (mask >> k) & 1 else 1.0) for k in range(4)}
            D = np.array([s[0], s[1], s[3], s[2]], np.float32)
            pos, uv, seg, lv, ls = su.host_extract(D, dims=(1, 1), layers=1, iso=0.0, **axes)
            want = su.marching_squares(D, dims=(1, 1), layers=1, iso=0.0, **axes)
            assert np.array_equal(seg, want[2]) and np.array_equal(uv, want[1])
            inside = [(mask >> k) & 1 for k in range(4)]
            outs = [k for k in range(4) if inside[k] and not inside[(k + 1) % 4]]
            assert len(seg) == len(outs) and list(ls) == [0, len(outs)]
            # a segment keeps the inside on its left: the cross product of its direction with the way to an inside corner is positive
            corners = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float64)
            for a, b in seg:
                d = uv[b].astype(np.float64) - uv[a]
                mid = 0.5 * (uv[a].astype(np.float64) + uv[b])
                side = [d[0] * (c[1] - mid[1]) - d[1] * (c[0] - mid[0]) for c in corners]
                if len(outs) == 1:
                    assert all((sd > 0) == bool(i) for sd, i in zip(side, inside) if abs(sd) > 1e-9), (mask, strong)
            if len(outs) == 2:
                m = sum(s.values()) * 0.25
                ends = {int(a): int(b) for a, b in seg}
                side_vertex = {0: 0, 3: 1, 1: 2, 2: 3}  # side -> vertex: the u-edge and v-edge of (0,0), the v-edge of (1,0), the u-edge of (0,1)
                for k in outs:
                    assert ends[side_vertex[k]] == side_vertex[(k + 1) % 4 if m < 0 else (k + 3) % 4], (mask, strong)


# ---- chainContours and the SVG writer -------------------------------------------------------------------------------------------
def _rings(dims, layers, radii, centre=None):
    """a stack over the unit lattice whose every layer holds concentric rings: inside between radii[0] and radii[1], between [2] and [3] ..."""
    nu, nv = dims
    axes = dict(origin=(0, 0, 0), du=(1, 0, 0), dv=(0, 1, 0), dw=(0, 0, 1))
    p = su.lattice_points(dims=dims, layers=layers, **axes).astype(np.float64)
    c = np.array(centre if centre is not None else (nu * 0.5 + 0.13, nv * 0.5 - 0.21))
    r = np.hypot(p[:, 0] - c[0], p[:, 1] - c[1])
    d = np.full(len(p), np.inf)
    for lo, hi in zip(radii[::2], radii[1::2]):
        d = np.minimum(d, np.maximum(lo - r, r - hi))
    return d.astype(np.float32), axes


def test_chain_contours_nested_loops():
    import sdf_playground_amd as sp

    dims, layers = (40, 36), 2
    D, axes = _rings(dims, layers, (3.0, 7.0, 10.0, 15.0))
    pos, uv, seg, lv, ls = su.marching_squares(D, dims=dims, layers=layers, iso=0.0, **axes)
    chains = sp.chainContours(seg, ls)
    assert len(chains) == layers
    for l, layer in enumerate(chains):
        assert len(layer) == 4 and all(closed for _c, closed in layer)
        areas = [su.shoelace(uv, c) for c, _closed in layer]
        # outer boundaries (radius 7 and 15) run counter-clockwise, the holes (3 and 10) clockwise; each within a ring of one cell
        want = sorted([-math.pi * 9, math.pi * 49, -math.pi * 100, math.pi * 225])
        for a, w in zip(sorted(areas), want):
            r = math.sqrt(abs(w) / math.pi)
            assert math.pi * (r - 1) ** 2 <= abs(a) <= math.pi * (r + 1) ** 2 and (a > 0) == (w > 0)
        used = np.concatenate([c for c, _closed in layer])
        assert len(used) == len(set(used)) == lv[l + 1] - lv[l] and used.min() >= lv[l] and used.max() < lv[l + 1]
        # each loop starts at its lowest segment, and the loops are ordered by it
        first_segments = []
        for c, _closed in layer:
            members = [k for k in range(ls[l], ls[l + 1]) if seg[k, 0] in set(c)]
            assert seg[min(members), 0] == c[0]
            first_segments.append(min(members))
            nxt = {int(a): int(b) for a, b in seg[members]}
            assert all(nxt[int(a)] == int(b) for a, b in zip(c, np.roll(c, -1)))
        assert first_segments == sorted(first_segments)


def test_chain_contours_open_chains():
    import sdf_playground_amd as sp

    # a disc larger than the lattice's width: the contour leaves through the left and right borders, two open chains; and a small ring inside
    dims = (20, 40)
    D, axes = _rings(dims, 1, (0.0, 14.0), centre=(10.2, 20.3))
    D2, _ = _rings(dims, 1, (0.0, 2.5), centre=(10.2, 20.3))
    D = np.maximum(D, -D2)  # the disc with a hole
    pos, uv, seg, lv, ls = su.marching_squares(D, dims=dims, layers=1, iso=0.0, **axes)
    (layer,) = sp.chainContours(seg, ls)
    assert [closed for _c, closed in layer] == [False, False, True]
    ended = set(int(b) for b in seg[:, 1])
    started = set(int(a) for a in seg[:, 0])
    firsts = []
    for c, closed in layer[:2]:
        assert int(c[0]) not in ended and int(c[-1]) not in started  # from the vertex no segment ends at to the one none starts at
        assert {float(uv[c[0], 0]), float(uv[c[-1], 0])} == {0.0, 20.0}  # both ends on the border
        firsts.append(int(np.nonzero(seg[:, 0] == c[0])[0][0]))
    assert firsts == sorted(firsts)
    assert su.shoelace(uv, layer[2][0]) < 0  # the hole runs clockwise
    assert sum(len(c) for c, _closed in layer) == len(uv)
    # nothing at all
    assert sp.chainContours(np.zeros((0, 2), np.uint32), np.zeros(4, np.int64)) == [[], [], []]
    with pytest.raises(ValueError):
        sp.chainContours(np.array([[0, 1], [0, 2]], np.uint32), [0, 2])


def test_svg_writer(tmp_path):
    from sdf_playground_amd import svg

    uv = np.array([[0.0, 0.0], [2.5, 0.0], [2.5, 3.0], [0.0, 3.0], [1.0, 1.5], [4.0, 1.25]], np.float32)
    layers = [[(np.array([4, 5]), False), (np.array([0, 1, 2, 3]), True)], []]
    text = svg.svg_text(uv, layers, (4, 3), 0.5, title="a <scene>")
    assert text.startswith('<?xml version="1.0"') and text.rstrip().endswith("</svg>")
    assert 'width="2" height="1.5" viewBox="0 0 2 1.5"' in text and "<title>a &lt;scene&gt;</title>" in text
    assert len(re.findall(r"<g ", text)) == 2 and len(re.findall(r"<path ", text)) == 2
    assert text.count('fill-rule="evenodd"') == 2 and 'id="layer0"' in text and 'id="layer1"' in text
    paths = re.findall(r'<path d="([^"]*)"/>', text)
    # lattice units times the cell size; v points up: y = (nv - v) * cell
    assert paths[0] == "M 0.5 0.75 L 2 0.875"
    assert paths[1] == "M 0 1.5 L 1.25 1.5 L 1.25 0 L 0 0 Z"
    out = tmp_path / "s.svg"
    svg.write_svg(str(out), uv, layers, (4, 3), 0.5, title="a <scene>")
    assert out.read_text() == text
    import xml.dom.minidom

    doc = xml.dom.minidom.parseString(text)
    assert len(doc.getElementsByTagName("path")) == 2
    with pytest.raises(ValueError):
        svg.svg_text(uv, layers, (4, 3), 0.0)


# ---- the plan -------------------------------------------------------------------------------------------------------------------
INVALID = -1  # SDFR_ERR_INVALID_ARGUMENT
NULL_POINTER, BAD_ON_HOST, BAD_GRID = "null pointer", "on_host must be 0 or 1", "bad slice grid"
NEGATIVE_CAPACITY, NULL_ARRAY = "negative capacity", "null array with a capacity"


def _exe(name, flags):
    return cppbuild.plan_program("slice_plan_host", name, flags)


@pytest.fixture(scope="module")
def exe():
    return _exe("slice_plan_host", [])


def request(origin=(-0.5, 0.25, -0.5), du=(0.1, 0.0, 0.0), dv=(0.0, 0.0, 0.1), dw=(0.0, 0.05, 0.0), dims=(8, 9), layers=3, iso=0.0, grid=True, vcap=0, scap=0,
            positions=False, coords=False, segments=False, counts=True, on_host=0, V=0, S=0):
    return dict(origin=origin, du=du, dv=dv, dw=dw, dims=dims, layers=layers, iso=iso, grid=grid, vcap=vcap, scap=scap, positions=positions, coords=coords,
                segments=segments, counts=counts, on_host=on_host, V=V, S=S)


def line_of(r):
    f = lambda v: repr(float(v))  # noqa: E731
    floats = [f(v) for k in ("origin", "du", "dv", "dw") for v in r[k]]
    return " ".join([str(int(r["grid"]))] + floats + [str(r["dims"][0]), str(r["dims"][1]), str(r["layers"]), f(r["iso"]), str(r["vcap"]), str(r["scap"])]
                    + [str(int(r[a])) for a in ("positions", "coords", "segments", "counts")] + [str(r["on_host"]), str(r["V"]), str(r["S"])])


def f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def f32_bits(v):
    return struct.unpack("I", struct.pack("f", v))[0]


def scan_sum_words(n):
    words = 0
    while n > 256:
        n = (n + 255) // 256
        words += n
    return words


def rules(r):
    """the issue's rules, in the order their errors win -> (status, text, plan or None)"""
    if not r["grid"] or not r["counts"]:
        return INVALID, NULL_POINTER, None
    if r["on_host"] not in (0, 1):
        return INVALID, BAD_ON_HOST, None
    nu, nv = r["dims"]
    layers = r["layers"]
    ok = all(math.isfinite(f32(v)) for k in ("origin", "du", "dv", "dw") for v in r[k]) and math.isfinite(f32(r["iso"]))
    ok = ok and any(f32(v) != 0 for v in r["du"]) and any(f32(v) != 0 for v in r["dv"])
    ok = ok and 1 <= nu <= 16384 and 1 <= nv <= 16384 and 1 <= layers <= 65536
    if not ok or (nu + 1) * (nv + 1) * layers > 1 << 30:
        return INVALID, BAD_GRID, None
    if r["vcap"] < 0 or r["scap"] < 0:
        return INVALID, NEGATIVE_CAPACITY, None
    if (r["vcap"] > 0 and not r["positions"]) or (r["scap"] > 0 and not r["segments"]):
        return INVALID, NULL_ARRAY, None
    points = (nu + 1) * (nv + 1) * layers
    work = [points * 4, (points + 1) * 4, (points + 1) * 4, 2 * scan_sum_words(points + 1) * 4, 2 * (layers + 1) * 4]
    V, S = r["V"], r["S"]
    fill = V <= r["vcap"] and S <= r["scap"] and V != 0
    blocks = (-(-(nu + 1) // 8) * -(-(nv + 1) // 8) * layers, -(-points // 64))
    return 0, "", dict(points=points, work=work, fill=fill, blocks=blocks, bytes=[V * 12, V * 8 if r["coords"] else 0, S * 8])


def expected_line(r):
    status, text, plan = rules(r)
    out = "%d;%s" % (status, text)
    if plan:
        nu, nv = r["dims"]
        floats = " ".join("%08x" % f32_bits(v) for k in ("origin", "du", "dv", "dw") for v in r[k])
        out += ";%s %08x %d %d %d" % (floats, f32_bits(r["iso"]), nu, nv, r["layers"])
        out += ";%s %d %d %d %d %d" % ((floats, nu + 1, nv + 1, r["layers"]) + plan["blocks"])
        out += ";%d;%d %d %d %d %d" % ((plan["points"],) + tuple(plan["work"]))
        out += ";%d %d %d;%d %d %d" % ((int(plan["fill"]), r["V"], r["S"]) + tuple(plan["bytes"]))
    return out


def run(exe, reqs):
    text = "".join(line_of(r) + "\n" for r in reqs)
    lines = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(reqs)
    return lines


BAD_GRIDS = [dict(origin=(NAN, 0.0, 0.0)), dict(origin=(0.0, INF, 0.0)), dict(du=(NAN, 0.0, 0.0)), dict(dv=(0.0, -INF, 0.0)), dict(dw=(0.0, 0.0, INF)), dict(iso=NAN),
             dict(iso=INF), dict(du=(0.0, 0.0, 0.0)), dict(dv=(0.0, -0.0, 0.0)), dict(dims=(0, 8)), dict(dims=(8, -1)), dict(dims=(16385, 8)), dict(dims=(8, 16385)),
             dict(layers=0), dict(layers=65537), dict(dims=(16384, 16384), layers=4), dict(dims=(1023, 1023), layers=1025)]


def fault_cases():
    """(what, request, the text that wins)"""
    cases = [("bad grid %r" % g, request(**g), BAD_GRID) for g in BAD_GRIDS]
    cases += [("null grid", request(grid=False), NULL_POINTER), ("null counts", request(counts=False), NULL_POINTER),
              ("on_host -1", request(on_host=-1), BAD_ON_HOST), ("on_host 2", request(on_host=2), BAD_ON_HOST),
              ("vertex capacity -1", request(vcap=-1), NEGATIVE_CAPACITY), ("segment capacity -1", request(scap=-1), NEGATIVE_CAPACITY),
              ("positions null", request(vcap=1), NULL_ARRAY), ("segments null", request(scap=1), NULL_ARRAY),
              ("segments null, positions there", request(vcap=4096, scap=1, positions=True), NULL_ARRAY)]
    # two faults at once, one request per adjacent pair of checks: the earlier text wins
    cases += [("null grid + on_host 2", request(grid=False, on_host=2), NULL_POINTER),
              ("on_host 2 + bad grid", request(on_host=2, layers=0), BAD_ON_HOST),
              ("bad grid + negative capacity", request(dims=(0, 8), vcap=-1), BAD_GRID),
              ("negative capacity + null array", request(vcap=-1, scap=1), NEGATIVE_CAPACITY),
              ("null array + negative capacity", request(vcap=1, scap=-1), NEGATIVE_CAPACITY)]
    return cases


def good_cases():
    return [("2^30 points exactly", request(dims=(1023, 1023), layers=1024)), ("the widest layer", request(dims=(16384, 16384), layers=3)),
            ("the tallest stack", request(dims=(1, 1), layers=65536)), ("dw zero: layers on top of each other", request(dw=(0.0, 0.0, 0.0))),
            ("coords null with a capacity", request(vcap=4096, scap=8192, positions=True, segments=True)), ("the counting call", request()),
            ("a host call", request(on_host=1, vcap=1, scap=1, positions=True, coords=True, segments=True)),
            ("arrays without a capacity", request(positions=True, coords=True, segments=True)),
            ("oblique steps and iso", request(dims=(37, 29), layers=5, iso=0.05, **OBLIQUE))]


WORKSPACE_SHAPES = [(1, 1, 1), (1, 1, 64), (15, 15, 1), (15, 16, 1), (300, 250, 1), (37, 29, 5), (1, 1, 65536), (4096, 4096, 1)]


def fill_cases():
    """capacities 100 vertices and 50 segments: the counts within, at and one past each; no vertex; coords wanted or not"""
    cases = []
    for coords in (False, True):
        for V, S in ((99, 10), (100, 10), (101, 10), (10, 49), (10, 50), (10, 51), (100, 50), (101, 51), (0, 0), (1, 1)):
            cases.append(request(vcap=100, scap=50, positions=True, coords=coords, segments=True, on_host=1, V=V, S=S))
    cases += [request(V=5, S=3), request(dims=(1023, 1023), layers=1024, vcap=1 << 31, scap=1 << 31, positions=True, coords=True, segments=True, V=1 << 31, S=1 << 31)]
    return cases


def test_argument_faults(exe):
    cases = fault_cases()
    got = run(exe, [r for _what, r, _text in cases])
    for (what, r, text), line in zip(cases, got):
        assert line == "%d;%s" % (INVALID, text), what
        assert line == expected_line(r), what
    assert {text for _w, _r, text in cases} == {NULL_POINTER, BAD_ON_HOST, BAD_GRID, NEGATIVE_CAPACITY, NULL_ARRAY}


def test_good_requests(exe):
    cases = good_cases()
    got = run(exe, [r for _what, r in cases])
    for (what, r), line in zip(cases, got):
        assert line.startswith("0;;"), what
        assert line == expected_line(r), what
    assert got[0].split(";")[4] == str(1 << 30)
    assert got[8].split(";")[3].split()[12:] == ["38", "30", "5", str(5 * 4 * 5), str(-(-38 * 30 * 5 // 64))]


def test_workspace_sizes(exe):
    """the five pieces, about 12 bytes per lattice point, through every branch of the scan's recursion on its block totals"""
    reqs = [request(dims=(nu, nv), layers=layers) for nu, nv, layers in WORKSPACE_SHAPES]
    got = run(exe, reqs)
    sums = {}
    for shape, r, line in zip(WORKSPACE_SHAPES, reqs, got):
        assert line == expected_line(r), shape
        points = (shape[0] + 1) * (shape[1] + 1) * shape[2]
        work = [int(x) for x in line.split(";")[5].split()]
        assert work[:3] == [points * 4, points * 4 + 4, points * 4 + 4] and work[4] == 8 * (shape[2] + 1)
        sums[shape] = work[3] // 8
    assert sums[(1, 1, 1)] == 0 and sums[(1, 1, 64)] == 2  # 5 elements: one block; 257: two
    assert sums[(15, 15, 1)] == 2 and sums[(15, 16, 1)] == 2  # 257 and 273 elements
    assert sums[(300, 250, 1)] == 296 + 2  # 75552 elements: 296 blocks, whose totals take 2 more
    assert sums[(4096, 4096, 1)] == 65569 + 257 + 2  # three levels
    big = [int(x) for x in got[-1].split(";")[5].split()]
    assert 12.0 <= sum(big) / (4097 * 4097) < 12.1


def test_second_phase(exe):
    cases = fill_cases()
    got = run(exe, cases)
    for r, line in zip(cases, got):
        assert line == expected_line(r), r
    decided = {(r["V"], r["S"], r["coords"]): line.split(";")[6:] for r, line in zip(cases[:20], got)}
    assert decided[(100, 50, True)] == ["1 100 50", "1200 800 400"]
    assert decided[(100, 50, False)] == ["1 100 50", "1200 0 400"]
    assert decided[(101, 10, True)][0] == "0 101 10" and decided[(10, 51, True)][0] == "0 10 51" and decided[(0, 0, True)][0] == "0 0 0"
    assert got[-2].split(";")[6] == "0 5 3"
    assert got[-1].split(";")[6:] == ["1 %d %d" % (1 << 31, 1 << 31), "%d %d %d" % (24 << 30, 16 << 30, 16 << 30)]


def test_under_sanitizers(exe):
    """the same program built with the address and undefined-behaviour sanitizers, over every request above: the same answers"""
    reqs = ([r for _w, r, _t in fault_cases()] + [r for _w, r in good_cases()] + [request(dims=(nu, nv), layers=layers) for nu, nv, layers in WORKSPACE_SHAPES]
            + fill_cases())
    checked = _exe("slice_plan_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert run(checked, reqs) == run(exe, reqs)


# ---- layouts and the command line -----------------------------------------------------------------------------------------------
def test_struct_layouts():
    import sdf_playground_amd as sp

    for S in (sp.SliceGrid, su.HostGrid):
        assert ctypes.sizeof(S) == 64
        assert [(getattr(S, n).offset, getattr(S, n).size) for n, _t in S._fields_] == [(0, 12), (12, 12), (24, 12), (36, 12), (48, 4), (52, 4), (56, 4), (60, 4)]
    assert [n for n, _t in sp.SliceGrid._fields_] == ["origin", "du", "dv", "dw", "nu", "nv", "layers", "iso"]
    assert su.host_lib().sh_grid_size() == 64
    assert ctypes.sizeof(sp.SliceCounts) == 16 and sp.SliceCounts.vertices.offset == 0 and sp.SliceCounts.segments.offset == 8
    assert "sdfr_slice_extract" in sp.EXPORTED_SYMBOLS
    # the header declares the same fields in the same order
    header = open(cppbuild.ROOT + "/include/sdfr.h").read()
    body = re.search(r"typedef struct sdfr_slice_grid\s*\{(.*?)\}\s*sdfr_slice_grid;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(origin|du|dv|dw|nu|nv|layers|iso)\b", body) == ["origin", "du", "dv", "dw", "nu", "nv", "layers", "iso"]
    assert re.search(r"float origin\[3\];\s*float du\[3\], dv\[3\];\s*float dw\[3\];\s*int32_t nu, nv, layers;\s*float iso;", body)


def test_cli_slice_arguments(capsys):
    from sdf_playground_amd import cli

    # the default axis is y: (u, v, w) = (z, x, y); one layer through the middle of the box
    origin, du, dv, dw, dims, layers = cli.slice_grid_from_box((-6, 0, -3, 0, 2, 3), 0.01)
    assert (origin, dims, layers) == ((-6, 1.0, -3), (600, 600), 1) and du == (0.0, 0.0, 0.01) and dv == (0.01, 0.0, 0.0) and dw == (0.0, 2, 0.0)
    origin, du, dv, dw, dims, layers = cli.slice_grid_from_box((-6, 0, -3, 0, 2, 3), 0.25, "x", step=0.5)
    assert (origin, dims, layers) == ((-5.75, 0, -3), (8, 24), 12) and du == (0.0, 0.25, 0.0) and dv == (0.0, 0.0, 0.25) and dw == (0.5, 0.0, 0.0)
    origin, du, dv, dw, dims, layers = cli.slice_grid_from_box((0, 0, 0, 1, 2, 4), 0.3, "z", layers=8)
    assert (origin, dims, layers) == ((0, 0, 0.25), (4, 7), 8) and du == (0.3, 0.0, 0.0) and dv == (0.0, 0.3, 0.0) and dw == (0.0, 0.0, 0.5)
    with pytest.raises(ValueError, match="x0 < x1"):
        cli.slice_grid_from_box((0, 0, 0, 1, 0, 1), 0.1)
    with pytest.raises(ValueError, match="at most 16384 per axis"):
        cli.slice_grid_from_box((0, 0, 0, 1, 1, 1), 1e-5)

    def refused(args, text):
        with pytest.raises(SystemExit) as e:
            cli.main(args)
        assert e.value.code == 2 and text in capsys.readouterr().err, args

    box = ["--slice-box", "-6", "0", "-3", "0", "2", "3", "--slice-cell", "0.01"]
    refused(["--scene", "labyrinth", "--slice", "s.svg"], "--slice needs --slice-box and --slice-cell")
    refused(["--scene", "labyrinth", "--slice", "s.svg", "--slice-cell", "0.01"], "--slice needs --slice-box and --slice-cell")
    refused(["--scene", "labyrinth"] + box, "need --slice")
    refused(["--scene", "labyrinth", "--slice-step", "0.1"], "need --slice")
    refused(["--scene", "labyrinth", "--slice", "s.svg", "--slice-axis", "w"] + box, "invalid choice")
    refused(["--scene", "labyrinth", "--slice", "s.svg", "--slice-step", "0.1", "--slice-layers", "4"] + box, "exclude each other")
    refused(["--scene", "labyrinth", "--slice", "s.svg", "--slice-step", "0"] + box, "--slice-step must be > 0")
    refused(["--scene", "labyrinth", "--slice", "s.svg", "--slice-step", "1e-6"] + box, "at most 65536")
    refused(["--scene", "labyrinth", "--slice", "s.svg", "--slice-layers", "0"] + box, "--slice-layers must be 1..65536")
    refused(["--scene", "labyrinth", "--slice", "s.svg", "--slice-box", "0", "0", "0", "1", "1", "1", "--slice-cell", "1e-5"], "at most 16384 per axis")
    refused(["--scene", "labyrinth", "--slice", "s.svg", "--slice-box", "0", "0", "0", "1", "1", "1", "--slice-cell", "-1"], "--slice-cell > 0")
    refused(["--scene", "labyrinth", "--slice", "s.svg", "--slice-box", "0", "0", "0", "1", "1", "1", "--slice-cell", "1e-4", "--slice-layers", "20"], "more than 2^30 lattice points")

"""CPU tier: the pixel launch plan (sdf_playground_amd/csrc/sdfr_launch_plan.h, built for the CPU by tests/cpp/launch_plan_host.cpp).

The plan decides what a launch of the pixel kernel hands out (tile rows or squares of tiles), to how many blocks, under which
feedback key, and what the fold that follows is told.  Most of it cannot be seen in a rendered picture -- a wrong key or grid
renders the right pixels, only slower -- so it is checked here, as arithmetic.

Three kinds of check over one grid of inputs: equality with a second spelling of the arithmetic (`parent_run_pixel`,
`parent_jit_launch_pixel` below: written from the two launchers of commit 880a4f7, run_pixel of sdfr_kernels_scene.hip and
jit_launch_pixel of sdfr_jit.cpp, each as it stood there) -- a characterisation that pins those numbers without arguing that they
are right --, the invariants the kernels rely on, and a few literal rows for the benchmark's configurations.  The row maps of that
grid are a second spelling too (`row_maps`, written from render_impl of commit ce3740b): frame_rows, which render_impl calls, is checked
against it."""
import ctypes
import itertools
import os

import pytest

import cppbuild

I32, U32, U64 = ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64
IN_FIELDS = ["persistent_tiles", "retire_after", "square_units", "scene_key", "knob_persistent", "knob_blocks_per_cu", "knob_retire_after",
             "knob_square_units", "launch_mode", "width", "local_rows", "rank", "world", "tile_w_log2", "priv_count", "priv_period", "direct",
             "resident_blocks_per_cu", "cus", "capacity"]
OUT_FIELDS = ["fits", "tile_cursors", "tiles_x", "tiles_x_magic", "unit_log2", "units_x", "units_x_magic", "units", "retire_after", "feedback_key",
              "n_work", "blocks", "feedback_rows", "work_items", "capacity_items", "frame_pixels"]


class LpIn(ctypes.Structure):
    _fields_ = [(n, U64 if n == "capacity" else U32 if n == "scene_key" else I32) for n in IN_FIELDS]


class LpOut(ctypes.Structure):
    _fields_ = [(n, U64 if n == "frame_pixels" else I32 if n in ("fits", "tile_cursors") else U32) for n in OUT_FIELDS]


# lp_frame_rows: FrIn, and FrameRows (sdfr_launch_plan.h) = RowMap (sdfr_frame.h) word by word, then the pixels the output spans
FRAME_FIELDS = ["mode", "width", "height", "rank", "world", "tile_w_log2", "priv_count", "priv_period"]
ROW_MAP_INTS = ["local_rows", "rank", "world", "tile_w_log2", "priv_count", "priv_period", "direct"]
ROW_MAP_WORDS = ["tiles_x", "tiles_x_magic", "unit_log2", "units_x", "units_x_magic", "units", "retire_after", "feedback_key"]
RENDER_FULL, RENDER_STRIPS, RENDER_PRIVATE = 0, 1, 2


class FrIn(ctypes.Structure):
    _fields_ = [(n, I32) for n in FRAME_FIELDS]


class FrameRows(ctypes.Structure):
    _fields_ = [(n, I32) for n in ROW_MAP_INTS] + [(n, U32) for n in ROW_MAP_WORDS] + [("local_pixels", U64)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        # the plan is host arithmetic: no HIP header on the include path
        so = cppbuild.compile(os.path.join(cppbuild.BUILD, "liblaunch_plan_host.so"), [os.path.join(cppbuild.HERE, "cpp", "launch_plan_host.cpp")],
                              cppbuild.csrc_headers(), cppbuild.PLAIN_FLAGS + ["-fPIC", "-Wno-unknown-pragmas", "-I" + cppbuild.CSRC])
        _lib = ctypes.CDLL(so)
        _lib.lp_plan.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        _lib.lp_plan.restype = None
        _lib.lp_frame_rows.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        _lib.lp_frame_rows.restype = None
    return _lib


def plan(cases):
    """[{IN_FIELDS}] -> [{OUT_FIELDS}]"""
    n = len(cases)
    a, o = (LpIn * n)(), (LpOut * n)()
    for k, c in enumerate(cases):
        for f in IN_FIELDS:
            setattr(a[k], f, c[f])
    lib().lp_plan(n, a, o)
    return [{f: getattr(o[k], f) for f in OUT_FIELDS} for k in range(n)]


# ---- the second spelling: commit 880a4f7 ------------------------------------------------------------------------------------------
M32 = 0xFFFFFFFF
FEEDBACK_MAX = 512
BLOCK = 64
UNSET = dict(knob_persistent=-1, knob_blocks_per_cu=0, knob_retire_after=-1, knob_square_units=-1)


def cdiv(a, b):
    return (a + b - 1) // b


def parent_work_items(width, c):
    tw, th = c["tile_w_log2"], 6 - c["tile_w_log2"]
    return (cdiv(width, 1 << tw) * cdiv(c["local_rows"], 1 << th) * 64) & M32


def parent_row_map_units(width, c):
    """row_map_units(rows, 512) -> (unit_log2, units_x, units_x_magic, units)"""
    if c["world"] != 1 or c["priv_count"] != 0 or c["direct"] != 0:
        return 0, 0, 0, 0
    tiles_x, tiles_y = cdiv(width, 1 << c["tile_w_log2"]), cdiv(c["local_rows"], 64 >> c["tile_w_log2"])
    for l in range(1, 9):
        ux, uy = cdiv(tiles_x, 1 << l), cdiv(tiles_y, 1 << l)
        if ux * uy <= FEEDBACK_MAX:
            return l, ux, (1 << 32) // ux if ux > 1 else M32, ux * uy
    return 0, 0, 0, 0


def parent_launch_mode(c, default_persistent, scene_retire_after):
    """pixel_launch_mode, the environment as the knob values -> (persistent, blocks_per_cu, retire_after)"""
    persistent = c["launch_mode"] == 2 or (c["launch_mode"] == 0 and default_persistent)
    if c["knob_persistent"] >= 0:
        persistent = c["knob_persistent"] != 0
    return persistent, c["knob_blocks_per_cu"], c["knob_retire_after"] if c["knob_retire_after"] >= 0 else scene_retire_after


def parent_launch_blocks(persistent, retire_after, tiles, resident):
    if not persistent:
        return tiles
    blocks = resident
    if retire_after > 0:
        blocks = resident // 2 + tiles // retire_after
    blocks = max(blocks, resident)
    return min(blocks, tiles)


def parent_feedback_key(scene_key, width, c, unit_log2, feedback_rows):
    if feedback_rows > FEEDBACK_MAX:
        return 0
    h = 2166136261
    for w in (scene_key, width, c["local_rows"], c["rank"], c["world"], c["tile_w_log2"], c["priv_count"], c["priv_period"], c["direct"], unit_log2):
        for b in range(4):
            h = ((h ^ ((w >> (8 * b)) & 0xFF)) * 16777619) & M32
    h = (h & ~1023 & M32) | feedback_rows
    return h if h else 1024


def parent_run_pixel(c):
    """run_pixel<Scene, DBG> of sdfr_kernels_scene.hip; the scene's traits and `2 * index + DBG` are the case's"""
    width = c["width"]
    n_work = parent_work_items(width, c)
    if n_work > c["capacity"]:
        return None
    tiles_blocks = cdiv(n_work, BLOCK)
    persistent, cap_per_cu, retire_after = parent_launch_mode(c, bool(c["persistent_tiles"]), c["retire_after"])
    per_cu = c["resident_blocks_per_cu"]
    if 0 < cap_per_cu < per_cu:
        per_cu = cap_per_cu
    units = (0, 0, 0, 0)
    hand_out = n_work
    if persistent and c["square_units"] and c["knob_square_units"] != 0:
        units = parent_row_map_units(width, c)
        if units[0]:
            hand_out = ((units[3] << (2 * units[0])) * 64) & M32
    if hand_out > c["capacity"]:
        return None
    blocks = parent_launch_blocks(persistent, retire_after, cdiv(hand_out, BLOCK), (c["cus"] * per_cu) & M32)
    tiles_x = cdiv(width, 1 << c["tile_w_log2"])
    feedback_rows = 0 if not persistent else units[3] if units[0] else tiles_blocks // tiles_x
    key = parent_feedback_key(c["scene_key"], width, c, units[0], feedback_rows) if persistent else 0
    return dict(unit_log2=units[0], units_x=units[1], units_x_magic=units[2], units=units[3], retire_after=retire_after if persistent else 0,
                feedback_key=key, n_work=hand_out, blocks=blocks, tile_cursors=int(persistent), feedback_rows=feedback_rows,
                frame_pixels=(1 << 56) - 1 if units[0] else n_work)


def parent_jit_launch_pixel(c):
    """jit_launch_pixel of sdfr_jit.cpp; `0x80000000 | fnv1a(name) | DBG` is the case's scene_key"""
    width = c["width"]
    n_work = parent_work_items(width, c)
    if n_work > c["capacity"]:
        return None
    persistent, cap_per_cu, retire_after = parent_launch_mode(c, False, 8)
    per_cu = c["resident_blocks_per_cu"]
    if 0 < cap_per_cu < per_cu:
        per_cu = cap_per_cu
    blocks = parent_launch_blocks(persistent, retire_after, cdiv(n_work, BLOCK), c["cus"] * per_cu)
    tiles_x = cdiv(width, 1 << c["tile_w_log2"])
    feedback_rows = cdiv(n_work, BLOCK) // tiles_x if persistent else 0
    key = parent_feedback_key(c["scene_key"], width, c, 0, feedback_rows) if persistent else 0
    return dict(unit_log2=0, units_x=0, units_x_magic=0, units=0, retire_after=retire_after if persistent else 0, feedback_key=key, n_work=n_work,
                blocks=blocks, tile_cursors=int(persistent), feedback_rows=feedback_rows, frame_pixels=n_work)


# ---- the grid ---------------------------------------------------------------------------------------------------------------------
WIDTHS = [8, 64, 333, 1000, 1283, 1920, 2050, 3840]
HEIGHTS = [3, 8, 40, 721, 1080, 1203, 2160, 3000]
CUS = 256
JIT_KEY = 0x80000000 | 0x1234ABC0
# (persistent_tiles, retire_after, square_units, scene_key, run-time scene): the shapes the scene headers declare, and a run-time scene
SCENES = [(1, 4, 0, 2 * 2, False), (1, 1, 1, 2 * 3 + 1, False), (0, 8, 0, 2 * 0, False), (1, 0, 1, 2 * 5, False), (0, 8, 0, JIT_KEY | 1, True)]
KNOBS_SET = [dict(knob_persistent=0), dict(knob_persistent=1), dict(knob_blocks_per_cu=1), dict(knob_blocks_per_cu=5), dict(knob_retire_after=0),
             dict(knob_retire_after=3), dict(knob_retire_after=16), dict(knob_square_units=0), dict(knob_square_units=1)]


def private_strip_count(strips, priv_count, priv_period):
    if priv_count <= 0:
        return 0
    return (strips // priv_period) * priv_count + min(strips % priv_period, priv_count)


def row_maps(height, empty=False):
    """the row maps render_impl (sdfr_api.cpp) makes: the full frame, strips of world 1..8, a strip split, its private strips"""
    strips = cdiv(height, 8)
    maps = [dict(local_rows=height, rank=0, world=1, priv_count=0, priv_period=1, direct=0)]
    for world in range(1, 9):
        maps.append(dict(local_rows=cdiv(strips, world) * 8, rank=world // 2, world=world, priv_count=0, priv_period=1, direct=0))
    for world, pc, pp in ((2, 1, 4), (8, 3, 5)):
        shared = strips - private_strip_count(strips, pc, pp)
        maps.append(dict(local_rows=cdiv(shared, world) * 8, rank=world - 1, world=world, priv_count=pc, priv_period=pp, direct=0))
        maps.append(dict(local_rows=private_strip_count(strips, pc, pp) * 8, rank=0, world=world, priv_count=pc, priv_period=pp, direct=1))
    return [m for m in maps if empty or m["local_rows"] > 0]  # (no rows: the API launches nothing)


def grid():
    """every width x height x tile shape x launch mode x row map x scene; with the knobs unset every residency 1..8 and three workspace
    sizes (what the API allocates, exactly the frame's items, one tile less), and every knob set to each of its values at one residency"""
    k = 0
    for width, height, tw, mode in itertools.product(WIDTHS, HEIGHTS, (3, 4, 5, 6), (0, 1, 2)):
        for rm in row_maps(height):
            shape = dict(rm, width=width, tile_w_log2=tw, launch_mode=mode, cus=CUS)
            items = parent_work_items(width, shape)
            pixels = width * (height if rm["direct"] else rm["local_rows"])
            for pt, ra, sq, key, jit in SCENES:
                base = dict(shape, persistent_tiles=pt, retire_after=ra, square_units=sq, scene_key=key, jit=jit)
                for per_cu in range(1, 9):
                    yield dict(base, **UNSET, resident_blocks_per_cu=per_cu, capacity=None, pixels=pixels)
                for capacity in (items, items - 64):
                    yield dict(base, **UNSET, resident_blocks_per_cu=1 + k % 8, capacity=capacity)
                for knob in KNOBS_SET:
                    k += 1
                    yield dict(base, **dict(UNSET, **knob), resident_blocks_per_cu=1 + k % 8, capacity=None, pixels=pixels)


@pytest.fixture(scope="module")
def planned():
    cases = list(grid())
    # capacity None: what render_impl asks ensure_workspace for -- launch_capacity_items, or the image's pixels where that is more
    probe = plan([dict(c, capacity=0) for c in cases])
    for c, o in zip(cases, probe):
        if c["capacity"] is None:
            c["capacity"] = max(o["capacity_items"], c["pixels"])
    return cases, plan(cases)


def test_plan_equals_the_parent_launchers(planned):
    cases, outs = planned
    assert len(cases) > 500000
    fitted = 0
    for c, o in zip(cases, outs):
        want = parent_jit_launch_pixel(c) if c["jit"] else parent_run_pixel(c)
        if want is None:
            assert not o["fits"], c
            continue
        fitted += 1
        got = {f: o[f] for f in want}
        assert o["fits"] and got == want, (c, got, want)
        assert o["work_items"] == parent_work_items(c["width"], c), c
    assert fitted > 0.9 * len(cases)


def test_plan_keeps_what_the_kernels_rely_on(planned):
    cases, outs = planned
    assert lib().lp_row_feedback_max() == FEEDBACK_MAX
    squares = 0
    for c, o in zip(cases, outs):
        tw, th = c["tile_w_log2"], 6 - c["tile_w_log2"]
        tiles_x, tiles_y = cdiv(c["width"], 1 << tw), cdiv(c["local_rows"], 1 << th)
        assert o["work_items"] == tiles_x * tiles_y * 64 and o["capacity_items"] >= o["work_items"], c
        assert (o["tiles_x"], o["tiles_x_magic"]) == (tiles_x, (1 << 32) // tiles_x if tiles_x > 1 else M32), c
        if not o["fits"]:
            assert c["capacity"] < o["work_items"] or (c["capacity"] < o["capacity_items"] and c["square_units"]), (c, o)
            continue
        # the workspace: one counter record per block, at most one block per tile handed out; what the API allocates is enough
        assert o["n_work"] % 64 == 0 and o["work_items"] <= o["n_work"] <= c["capacity"] and o["n_work"] <= o["capacity_items"], (c, o)
        assert 1 <= o["blocks"] <= o["n_work"] // 64, (c, o)
        assert o["units"] <= FEEDBACK_MAX, (c, o)
        if o["unit_log2"]:
            squares += 1
            ul, units_y = o["unit_log2"], o["units"] // o["units_x"]
            assert o["units"] == o["units_x"] * units_y and o["tile_cursors"] and c["square_units"] and not c["jit"], (c, o)
            assert (o["units_x"] << ul) >= tiles_x and (units_y << ul) >= tiles_y, (c, o)  # every tile of the frame lies in a square
            assert o["n_work"] == (o["units"] << (2 * ul)) * 64 and o["feedback_rows"] == o["units"], (c, o)
            assert o["units_x_magic"] == ((1 << 32) // o["units_x"] if o["units_x"] > 1 else M32), (c, o)
            assert o["frame_pixels"] == (1 << 56) - 1, (c, o)
        else:
            assert o["n_work"] == o["work_items"] == o["frame_pixels"] and o["units"] == o["units_x"] == 0, (c, o)
        if o["tile_cursors"]:  # a persistent launch
            assert (o["feedback_key"] != 0) == (o["feedback_rows"] <= FEEDBACK_MAX), (c, o)
            if o["feedback_key"]:
                assert o["feedback_key"] & 1023 == o["feedback_rows"], (c, o)
            if not o["unit_log2"]:
                assert o["feedback_rows"] == tiles_y, (c, o)
        else:
            assert o["feedback_key"] == 0 and o["feedback_rows"] == 0 and o["retire_after"] == 0 and o["unit_log2"] == 0, (c, o)
            assert o["blocks"] == o["n_work"] // 64, (c, o)
    assert squares > 10000


def test_frame_rows_are_the_row_maps_of_the_grid():
    """frame_rows, which render_impl calls, against `row_maps`: every row map of the grid, the empty ones included.  A full frame is
    asked for on a handle that carries a strip split, which it ignores."""
    cases, want = [], []
    for width, height, tw in itertools.product(WIDTHS, HEIGHTS, (3, 4, 5, 6)):
        for k, m in enumerate(row_maps(height, empty=True)):
            mode = RENDER_FULL if k == 0 else RENDER_PRIVATE if m["direct"] else RENDER_STRIPS
            split = (3, 5) if mode == RENDER_FULL else (m["priv_count"], m["priv_period"])
            cases.append(dict(mode=mode, width=width, height=height, rank=m["rank"], world=m["world"], tile_w_log2=tw, priv_count=split[0],
                              priv_period=split[1]))
            want.append(m)
    n = len(cases)
    assert n == len(WIDTHS) * len(HEIGHTS) * 4 * 13 and any(m["local_rows"] == 0 for m in want)
    assert {c["mode"] for c in cases} == {RENDER_FULL, RENDER_STRIPS, RENDER_PRIVATE}
    assert ctypes.sizeof(FrameRows) == 72
    a, o = (FrIn * n)(), (FrameRows * n)()
    for k, c in enumerate(cases):
        for f in FRAME_FIELDS:
            setattr(a[k], f, c[f])
    lib().lp_frame_rows(n, a, o)
    for c, m, got in zip(cases, want, o):
        assert {f: getattr(got, f) for f in m} == m, (c, m)
        tiles_x = cdiv(c["width"], 1 << c["tile_w_log2"])
        assert (got.tile_w_log2, got.tiles_x, got.tiles_x_magic) == (c["tile_w_log2"], tiles_x, (1 << 32) // tiles_x if tiles_x > 1 else M32), c
        assert (got.unit_log2, got.units_x, got.units_x_magic, got.units, got.retire_after, got.feedback_key) == (0, 0, 0, 0, 0, 0), c
        assert got.local_pixels == c["width"] * (c["height"] if c["mode"] == RENDER_PRIVATE else m["local_rows"]), (c, m)


def test_keys_tell_launches_apart():
    """what a row order depends on changes the key: scene, debug variant, frame size, tile shape, which rows the launch renders"""
    base = dict(UNSET, persistent_tiles=1, retire_after=4, square_units=0, scene_key=4, launch_mode=0, width=1920, local_rows=1080, rank=0, world=1,
                tile_w_log2=3, priv_count=0, priv_period=1, direct=0, resident_blocks_per_cu=28, cus=CUS, capacity=1 << 24)
    others = [dict(scene_key=5), dict(scene_key=6), dict(width=1921), dict(local_rows=1072), dict(tile_w_log2=4), dict(world=2), dict(world=2, rank=1),
              dict(priv_count=1, priv_period=4, world=2), dict(priv_count=1, priv_period=4, world=2, direct=1), dict(square_units=1)]
    keys = [o["feedback_key"] for o in plan([base] + [dict(base, **d) for d in others])]
    assert all(keys) and len(set(k >> 10 for k in keys)) == len(keys), keys


def test_benchmark_configurations():
    """The benchmark's launches on a 256-CU MI355X, scene traits as the scene headers declare them (sdfr_scenes.h) and the residency the
    occupancy query reports for their kernels (28 blocks of one wave per CU at 7 waves per SIMD).  The headline's grid is the one recorded in
    profiles/r04_cfg3_rocprofv3_kernel_trace_head.csv: Grid_Size_X 2302976 = 35984 blocks of 64."""
    def case(pt, ra, sq, index, width, height, tw, per_cu=28, mode=0):
        rm = dict(local_rows=height, rank=0, world=1, priv_count=0, priv_period=1, direct=0)
        return dict(UNSET, **rm, persistent_tiles=pt, retire_after=ra, square_units=sq, scene_key=2 * index, launch_mode=mode, width=width,
                    tile_w_log2=tw, resident_blocks_per_cu=per_cu, cus=CUS, capacity=1 << 24)
    rows = [
        # configuration 2, cube_sea 1920x1080: 240 x 135 tiles in tile rows, waves retire after 4
        (case(1, 4, 0, 1, 1920, 1080, 3), dict(n_work=2073600, blocks=11684, unit_log2=0, units=0, feedback_rows=135, retire_after=4, frame_pixels=2073600)),
        # configuration 3, labyrinth 3840x2160: 480 x 270 tiles, 7168 resident / 2 + 129600 / 4
        (case(1, 4, 0, 2, 3840, 2160, 3), dict(n_work=8294400, blocks=35984, unit_log2=0, units=0, feedback_rows=270, retire_after=4, frame_pixels=8294400)),
        # configuration 4, fractal 3840x2160: 480 x 270 tiles in 30 x 17 squares of 16 x 16 tiles, a wave per tile handed out (retire after 1)
        (case(1, 1, 1, 3, 3840, 2160, 3), dict(n_work=8355840, blocks=130560, unit_log2=4, units_x=30, units=510, feedback_rows=510, retire_after=1,
                                               frame_pixels=(1 << 56) - 1)),
        # configuration 5g, gems 3840x2160 in 16 x 4 tiles: 240 x 540 tiles in 15 x 34 squares
        (case(1, 1, 1, 5, 3840, 2160, 4), dict(n_work=8355840, blocks=130560, unit_log2=4, units_x=15, units=510, feedback_rows=510, retire_after=1,
                                               frame_pixels=(1 << 56) - 1)),
        # fast_sphere 3840x2160: one wave per tile
        (case(0, 8, 0, 0, 3840, 2160, 3), dict(n_work=8294400, blocks=129600, tile_cursors=0, feedback_key=0, feedback_rows=0, retire_after=0)),
        # the same asked to be persistent: resident / 2 + 129600 / 8
        (case(0, 8, 0, 0, 3840, 2160, 3, mode=2), dict(n_work=8294400, blocks=19784, tile_cursors=1, feedback_rows=270, retire_after=8)),
    ]
    for (c, want), o in zip(rows, plan([c for c, _ in rows])):
        assert o["fits"] and {f: o[f] for f in want} == want, (c, o)

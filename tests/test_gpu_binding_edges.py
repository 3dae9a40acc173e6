"""GPU tier of the Python binding at its edge shapes: every family of SDFRenderer calls, on the host and on the device path, against the
raw C entry point called through r._L.sdfr_*(r._h, ...) with buffers this test makes itself.  The binding's answer must have the
documented shape and element type and equal the raw call's bytes.  Empty inputs, one item, one full wave plus a ragged lane, a pixel
outside the frame, the whole-frame pick, span slots of zero, a lattice that misses the surface, uploads made for the caller.  All on
fast_sphere (the floor and a sphere of radius 0.5 about (0, 1, 0)), the cheapest scene."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FW, FH = 9, 7  # the frame of the picks: 63 pixels, no multiple of a tile
PIXELS = np.array([[4, 3], [0, 6], [9, 2]], np.int32)  # (9, 2) lies outside the frame
CELL = 0.1
ACROSS, MISS = (0.33, 0.83, -0.17), (3.0, 3.0, 3.0)  # origins of a 4 x 4 x 4 lattice through the sphere's surface at x = 0.5, and of one in the open
SPAN = dict(min_step=0.05, t_max=6.0, iso=0.0, max_steps=256)

# an answer array: (numpy dtype's name in the package, numpy shape after n, device shape after n, device dtype)
ANSWERS = {"distance": ("float32", (), (), "float32"), "normals": ("float32", (3,), (3,), "float32"), "hits": ("HIT_DTYPE", (), (12,), "float32"),
           "surfaces": ("SURFACE_DTYPE", (), (32,), "float32"), "occlusion": ("OCCLUSION_DTYPE", (), (4,), "int32"),
           "lighting": ("LIGHTING_DTYPE", (), (16,), "float32"), "lights": ("LIGHT_SAMPLE_DTYPE", (8,), (160,), "float32"),
           "summaries": ("SPAN_SUMMARY_DTYPE", (), (8,), "int32")}


@pytest.fixture(scope="module")
def sp():
    import sdf_playground_amd

    return sdf_playground_amd


@pytest.fixture(scope="module")
def renderer(sp):
    r = sp.SDFRenderer(0)
    r.initShader("fast_sphere")
    r.setParameters(0.0)
    cam = sp.Camera()  # eye (0, 2, -3) looking at (0, 1, 0): the sphere in the middle of the frame
    cam.SetAspect(FW / FH)
    r.setCamera(cam)
    yield r
    r.close()


def _cuda():
    import torch

    return torch.device("cuda", 0)


def _zeros(dev, shape, dtype):
    """a zeroed buffer of the test's own: numpy, or (dev) a device tensor; dtype a numpy dtype or its name"""
    if not dev:
        return np.zeros(shape, dtype)
    import torch

    return torch.zeros(shape, dtype=getattr(torch, dtype), device=_cuda())


def _out(sp, dev, n, kind):
    name, host_tail, dev_tail, dev_dtype = ANSWERS[kind]
    return _zeros(dev, (n,) + dev_tail, dev_dtype) if dev else _zeros(False, (n,) + host_tail, getattr(sp, name, name))


def _to(dev, a):
    if not dev or a is None:
        return a
    import torch

    return torch.from_numpy(a).to(_cuda())


def _p(a):
    if a is None:
        return None
    return ctypes.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else a.ctypes.data_as(ctypes.c_void_p)


def _raw(r, rc):
    assert rc == 0, r._L.sdfr_last_error(r._h)


def _same(r, what, got, want):
    """the binding's array against the raw call's buffer: the same side, shape, element type and bytes"""
    if want is None:
        assert got is None, what
        return
    assert type(got) is type(want), (what, type(got), type(want))
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if hasattr(got, "data_ptr"):
        r.sync()
        got, want = got.cpu().numpy(), want.cpu().numpy()
    assert got.tobytes() == want.tobytes(), what


def _items(n):
    """n points about the sphere with unit normals, and n rays from about the camera towards it: some hit it, some the floor, some nothing"""
    g = np.random.default_rng(20 + n)
    points = (g.uniform(-1.0, 1.0, (n, 3)) + (0.0, 1.0, 0.0)).astype(np.float32)
    normals = g.normal(size=(n, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(np.float32)
    origins = ((0.0, 2.0, -3.0) + g.uniform(-0.2, 0.2, (n, 3))).astype(np.float32)
    dirs = ((0.0, -1.0, 3.0) + g.uniform(-1.5, 1.5, (n, 3))).astype(np.float32)
    return points, normals, origins, dirs


@pytest.mark.parametrize("n", [0, 1, 65])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_queries(sp, renderer, dev, n):
    r, L, h, on_host = renderer, renderer._L, renderer._h, 0 if dev else 1
    P, N, O, D = [_to(dev, a) for a in _items(n)]
    out = lambda kind: _out(sp, dev, n, kind)  # noqa: E731

    d = out("distance")
    _raw(r, L.sdfr_query_distance(h, n, _p(P), _p(d), None, on_host))
    _same(r, "queryDistance", r.queryDistance(P), d)
    d, nr = out("distance"), out("normals")
    _raw(r, L.sdfr_query_distance(h, n, _p(P), _p(d), _p(nr), on_host))
    got = r.queryDistance(P, normals=True)
    _same(r, "queryDistance distance", got[0], d)
    _same(r, "queryDistance normals", got[1], nr)

    hits = out("hits")
    _raw(r, L.sdfr_query_rays(h, n, _p(O), _p(D), 0.0, _p(hits), on_host))
    _same(r, "queryRays", r.queryRays(O, D), hits)

    hs, s = out("hits"), out("surfaces")
    _raw(r, L.sdfr_query_ray_surfaces(h, n, _p(O), _p(D), 0.0, _p(hs), _p(s), on_host))
    got = r.queryRaySurfaces(O, D, hits=True)
    _same(r, "queryRaySurfaces hits", got[0], hs)
    _same(r, "queryRaySurfaces surfaces", got[1], s)
    _same(r, "the hits of the surface query", hs, hits)

    hl, g, ls = out("hits"), out("lighting"), out("lights")
    _raw(r, L.sdfr_query_ray_lighting(h, n, _p(O), _p(D), 0.0, _p(hl), _p(g), _p(ls), on_host))
    got = r.queryRayLighting(O, D, hits=True, lights=True)
    for k, (what, want) in enumerate((("hits", hl), ("lighting", g), ("lights", ls))):
        _same(r, "queryRayLighting " + what, got[k], want)

    o = out("occlusion")
    _raw(r, L.sdfr_query_occlusion(h, n, _p(P), _p(N), 0.01, 0.8, _p(o), on_host))
    _same(r, "queryOcclusion", r.queryOcclusion(P, N, 0.01, 0.8), o)
    o = out("occlusion")
    _raw(r, L.sdfr_hit_occlusion(h, n, _p(hits), 0.01, 0.8, _p(o), on_host))
    _same(r, "hitOcclusion", r.hitOcclusion(hits, 0.01, 0.8), o)
    if n == 65 and not dev:
        assert 0 < int((hits["hit"] == 1).sum()) < n  # the items do meet the scene, and not all of them


def _span_params(sp, max_spans):
    return sp.SpanParams(SPAN["t_max"], SPAN["min_step"], SPAN["iso"], SPAN["max_steps"], max_spans)


def _raw_picks(sp, r, dev, n, px):
    """the four pick entry points with the test's buffers -> {name: buffers}"""
    L, h, on_host = r._L, r._h, 0 if dev else 1
    out = lambda kind: _out(sp, dev, n, kind)  # noqa: E731
    want = {}
    if px is not None:
        want["pick"] = (out("hits"),)
        _raw(r, L.sdfr_pick(h, FW, FH, n, _p(px), _p(want["pick"][0]), on_host))
    want["surfaces"] = (out("hits"), out("surfaces"))
    _raw(r, L.sdfr_pick_surfaces(h, FW, FH, n, _p(px), _p(want["surfaces"][0]), _p(want["surfaces"][1]), on_host))
    want["lighting"] = (out("hits"), out("lighting"), out("lights"))
    _raw(r, L.sdfr_pick_lighting(h, FW, FH, n, _p(px), *[_p(a) for a in want["lighting"]], on_host))
    want["spans"] = (out("summaries"), _zeros(dev, (n, 2, 2), "float32"))
    _raw(r, L.sdfr_pick_spans(h, FW, FH, n, _p(px), ctypes.byref(_span_params(sp, 2)), _p(want["spans"][0]), _p(want["spans"][1]), on_host))
    return want


def _check_picks(r, want, got):
    for name, arrays in want.items():
        assert len(got[name]) == len(arrays), name
        for k, a in enumerate(arrays):
            _same(r, "pick %s [%d]" % (name, k), got[name][k], a)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_picks_of_a_pixel_list(sp, renderer, dev):
    r, px = renderer, _to(dev, PIXELS)
    want = _raw_picks(sp, r, dev, len(PIXELS), px)
    got = {"pick": (r.pick(px, FW, FH),), "surfaces": r.pickSurfaces(px, FW, FH, hits=True), "lighting": r.pickLighting(px, FW, FH, hits=True, lights=True),
           "spans": r.pickSpans(px, FW, FH, max_spans=2, **SPAN)}
    _check_picks(r, want, got)
    if not dev:
        assert got["pick"][0]["hit"][0] == 1 and got["pick"][0]["hit"][2] == -1 and got["spans"][0]["valid"][2] == -1  # the sphere; outside the frame


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_picks_of_the_whole_frame(sp, renderer, dev):
    r = renderer
    want = _raw_picks(sp, r, dev, FW * FH, None)
    got = {"surfaces": r.pickSurfaces(None, FW, FH, hits=True, device=dev), "lighting": r.pickLighting(None, FW, FH, hits=True, lights=True, device=dev),
           "spans": r.pickSpans(None, FW, FH, max_spans=2, device=dev, **SPAN)}
    _check_picks(r, want, got)
    # without the extras the answer is the one array, not a tuple
    _same(r, "pickSurfaces", r.pickSurfaces(None, FW, FH, device=dev), want["surfaces"][1])
    _same(r, "pickLighting", r.pickLighting(None, FW, FH, device=dev), want["lighting"][1])


@pytest.mark.parametrize("max_spans", [0, 1])
@pytest.mark.parametrize("n", [0, 65])
@pytest.mark.parametrize("mode", ["host", "device", "uploaded"])
def test_spans(sp, renderer, mode, n, max_spans):
    """mode "uploaded": numpy inputs with device=True, which the binding uploads itself and must let go of when the call is over"""
    import torch

    r, L, h, dev = renderer, renderer._L, renderer._h, mode != "host"
    _points, _normals, origins, dirs = _items(n)
    O, D = _to(dev, origins), _to(dev, dirs)
    s, spans = _out(sp, dev, n, "summaries"), _zeros(dev, (n, max_spans, 2), "float32")
    if not (dev and n == 0):  # (an empty tensor has no address, and the entry point refuses a null pointer: the binding answers that case itself)
        _raw(r, L.sdfr_query_ray_spans(h, n, _p(O), _p(D), ctypes.byref(_span_params(sp, max_spans)), _p(s), _p(spans) if max_spans else None,
                                       0 if dev else 1))
    if mode != "uploaded":
        got = r.querySpans(O, D, max_spans=max_spans, **SPAN)
        _same(r, "querySpans summaries", got[0], s)
        _same(r, "querySpans spans", got[1], spans)
        return
    r.sync()
    held = torch.cuda.memory_allocated(0)
    first = r.querySpans(origins, dirs, max_spans=max_spans, device=True, **SPAN)
    second = r.querySpans(origins, dirs, max_spans=max_spans, device=True, **SPAN)
    for got in (first, second):
        _same(r, "querySpans summaries", got[0], s)
        _same(r, "querySpans spans", got[1], spans)
    del got, first, second
    assert torch.cuda.memory_allocated(0) == held  # neither call's uploads are still held
    if n and max_spans:
        assert int((s.cpu().numpy()[:, 1] >= 1).sum()) > 0  # some rays do pass through the solid


def _mesh_grid(sp, origin):
    return sp.MeshGrid((ctypes.c_float * 3)(*origin), CELL, 4, 4, 4, 0.0)


def _raw_mesh(sp, r, dev, origin, normals, sharp):
    extract = r._L.sdfr_mesh_extract_sharp if sharp else r._L.sdfr_mesh_extract
    grid, counts, on_host = _mesh_grid(sp, origin), sp.MeshCounts(), 0 if dev else 1
    _raw(r, extract(r._h, ctypes.byref(grid), 0, 0, None, None, None, ctypes.byref(counts), on_host))
    v, t = int(counts.vertices), int(counts.triangles)
    pos, nrm, idx = _zeros(dev, (v, 3), "float32"), _zeros(dev, (v, 3), "float32") if normals else None, _zeros(dev, (t, 3), "int32" if dev else "uint32")
    if v:
        _raw(r, extract(r._h, ctypes.byref(grid), v, t, _p(pos), _p(nrm), _p(idx), ctypes.byref(counts), on_host))
        assert (int(counts.vertices), int(counts.triangles)) == (v, t)
    return pos, nrm, idx


@pytest.mark.parametrize("normals", [True, False], ids=["normals", "bare"])
@pytest.mark.parametrize("sharp", [False, True], ids=["plain", "sharp"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_mesh(sp, renderer, dev, sharp, normals):
    r = renderer
    for origin in (ACROSS, MISS):
        want = _raw_mesh(sp, r, dev, origin, normals, sharp)
        assert (want[0].shape[0] > 0) == (origin is ACROSS)
        got = r.extractMesh(origin, CELL, (4, 4, 4), normals=normals, device=dev, sharp=sharp)
        for what, g, w in zip(("positions", "normals", "indices"), got, want):
            _same(r, "extractMesh %s" % what, g, w)


@pytest.mark.parametrize("coords", [True, False], ids=["coords", "bare"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_slices(sp, renderer, dev, coords):
    r, L, h, on_host = renderer, renderer._L, renderer._h, 0 if dev else 1
    f3 = lambda *v: (ctypes.c_float * 3)(*v)  # noqa: E731
    for origin in (ACROSS, MISS):
        grid, counts = sp.SliceGrid(f3(*origin), f3(CELL, 0, 0), f3(0, CELL, 0), f3(0, 0, 2 * CELL), 4, 4, 2, 0.0), sp.SliceCounts()
        lv, ls = np.zeros(3, np.int64), np.zeros(3, np.int64)
        _raw(r, L.sdfr_slice_extract(h, ctypes.byref(grid), 0, 0, None, None, None, _p(lv), _p(ls), ctypes.byref(counts), on_host))
        v, s = int(counts.vertices), int(counts.segments)
        assert (v > 0) == (origin is ACROSS)
        pos, uv, seg = _zeros(dev, (v, 3), "float32"), _zeros(dev, (v, 2), "float32") if coords else None, _zeros(dev, (s, 2), "int32" if dev else "uint32")
        if v:
            _raw(r, L.sdfr_slice_extract(h, ctypes.byref(grid), v, s, _p(pos), _p(uv), _p(seg), _p(lv), _p(ls), ctypes.byref(counts), on_host))
        got = r.extractSlices(origin, (CELL, 0, 0), (0, CELL, 0), (0, 0, 2 * CELL), dims=(4, 4), layers=2, coords=coords, device=dev)
        for what, g, w in zip(("positions", "coords", "segments", "layer_vertices", "layer_segments"), got, (pos, uv, seg, lv, ls)):
            _same(r, "extractSlices %s" % what, g, w)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_measure_columns(sp, renderer, dev):
    r = renderer
    grid, depth = sp.measureGrid((-0.1, 0.4, -0.15), (0.1, 1.6, 0.15), CELL, axis="y")  # columns along y through the sphere: u = z, v = x
    assert (grid.nu, grid.nv) == (3, 2)
    want, cols = sp.MeasureResult(), _zeros(True, (2, 3, 10), "int32") if dev else _zeros(False, (2, 3), sp.MEASURE_COLUMN_DTYPE)
    params = sp.SpanParams(depth, SPAN["min_step"], 0.0, SPAN["max_steps"], 0)
    _raw(r, r._L.sdfr_measure(r._h, ctypes.byref(grid), ctypes.byref(params), ctypes.byref(want), _p(cols), 0 if dev else 1))
    got, got_cols = r.measure(grid, SPAN["min_step"], t_max=depth, max_steps=SPAN["max_steps"], columns=True, device=dev)
    assert bytes(got) == bytes(want) and want.columns_hit == 6
    _same(r, "measure columns", got_cols, cols)
    assert bytes(r.measure(grid, SPAN["min_step"], t_max=depth, max_steps=SPAN["max_steps"], device=dev)) == bytes(want)


@pytest.mark.parametrize("mode", ["host", "uploaded", "device"])
def test_atlas(sp, renderer, mode):
    """numpy inputs (host arrays back), numpy inputs with device=True and device inputs (device tensors back)"""
    r, L, h, dev = renderer, renderer._L, renderer._h, mode != "host"
    pos, nrm, idx = r.extractMesh(ACROSS, CELL, (4, 4, 4))
    assert len(idx) >= 2
    v, on_host, reach = len(pos), 0 if dev else 1, 2 * CELL
    atlas = sp.atlasLayout(len(idx), 4)
    hw = (atlas.height, atlas.width)
    P, N, I = _to(dev, pos), _to(dev, nrm), _to(dev, idx.view(np.int32) if dev else idx)
    tp, tn, valid = _zeros(dev, hw + (3,), "float32"), _zeros(dev, hw + (3,), "float32"), _zeros(dev, hw, "int32")
    _raw(r, L.sdfr_atlas_texels(h, ctypes.byref(atlas), v, _p(P), _p(N), _p(I), _p(tp), _p(tn), _p(valid), on_host))
    albedo, lit, bvalid = _zeros(dev, hw + (4,), "float32"), _zeros(dev, hw + (4,), "float32"), _zeros(dev, hw, "int32")
    _raw(r, L.sdfr_atlas_bake(h, ctypes.byref(atlas), v, _p(P), _p(N), _p(I), reach, 1 | 4, _p(albedo), None, _p(lit), _p(bvalid), on_host))
    ins = (P, N, I) if mode == "device" else (pos, nrm, idx)
    kw = dict(device=True) if mode == "uploaded" else {}
    got = r.atlasTexels(*ins, tile=4, **kw)
    assert bytes(got[0]) == bytes(atlas)
    for what, g, w in zip(("positions", "normals", "valid"), got[1:], (tp, tn, valid)):
        _same(r, "atlasTexels %s" % what, g, w)
    baked = r.bakeAtlas(*ins, tile=4, reach=reach, layers=("albedo", "lit"), **kw)
    assert sorted(baked) == ["albedo", "atlas", "lit", "valid"] and bytes(baked["atlas"]) == bytes(atlas)
    for what, w in (("albedo", albedo), ("lit", lit), ("valid", bvalid)):
        _same(r, "bakeAtlas %s" % what, baked[what], w)
    if not dev:
        assert (bvalid == 1).any()


@pytest.mark.parametrize("aa", [False, True], ids=["render", "renderAA"])
def test_render(sp, renderer, aa):
    import torch

    r, L, h, W, H = renderer, renderer._L, renderer._h, 16, 8

    def raw(out, on_host, stats=None):
        if aa:
            _raw(r, L.sdfr_render_aa(h, W, H, 2, _p(out), sp.RGBA32F, on_host, _p(stats)))
        else:
            _raw(r, L.sdfr_render(h, W, H, _p(out), sp.RGBA32F, on_host, _p(stats)))
        return out

    def bound(**kw):
        return r.renderAA(None, W, H, factor=2, **kw) if aa else r.render(None, W, H, **kw)

    img, st = _zeros(False, (H, W, 4), "float32"), _zeros(False, (H, W, 3), "uint32")
    raw(img, 1, st)
    assert img[..., :3].max() > 0 and st[..., 0].min() >= 1
    _same(r, "host return", bound(), img)
    mine = np.zeros((H, W, 4), np.float32)
    assert bound(out=mine) is mine
    _same(r, "host out", mine, img)
    got = bound(pixel_stats=True)
    _same(r, "host image with pixel_stats", got[0], img)
    _same(r, "host pixel_stats", got[1], st)

    dimg, dst = _zeros(True, (H, W, 4), "float32"), _zeros(True, (H, W, 3), "int32")
    raw(dimg, 0, dst)
    mine, mine_st = torch.zeros((H, W, 4), dtype=torch.float32, device=_cuda()), _zeros(True, (H, W, 3), "int32")
    assert bound(out=mine) is mine
    _same(r, "device out", mine, dimg)
    _same(r, "device against host", mine.cpu().numpy(), img)
    mine.zero_()
    assert bound(out=mine, pixel_stats=mine_st) is mine
    _same(r, "device out with pixel_stats", mine, dimg)
    _same(r, "device pixel_stats", mine_st, dst)
    _same(r, "device pixel_stats against host", mine_st.cpu().numpy().view(np.uint32), st)

"""SDFRenderer, Camera, Variable and HDR: the classes above the C ABI, and the free functions that need no handle."""
import ctypes
import os

import numpy as np

from ._abi import (ATLAS_LAYERS, COMPONENT_DTYPE, ComponentCounts, FIT_FOUND, HIT_DTYPE, LIGHT_SAMPLE_DTYPE, LIGHTING_DTYPE, MEASURE_COLUMN_DTYPE, OCCLUSION_DTYPE, RGBA32F, SDFR_OK,
                   SPAN_ENDS_INSIDE, SPAN_SUMMARY_DTYPE, STRIP_RGB16F_A8, STRIP_RGB32F_A8, SURFACE_DTYPE, Atlas, Limits, MeasureGrid, MeasureResult,
                   MeshCounts, MeshFit, MeshGrid, MeshSurvey, SdfrError, SliceCounts, SliceGrid, SolidProperties, SpanParams, Stats, _CTiming,
                   _CVariable, load_library)


def _f3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


def _mesh_grid(origin, cell, dims, iso):
    return MeshGrid(_f3(origin), float(cell), int(dims[0]), int(dims[1]), int(dims[2]), float(iso))


def _source_text(source):
    """`source` is a scene's text, or the path of a file that holds it"""
    if os.path.exists(source):
        with open(source) as f:
            source = f.read()
    return source


class _Side:
    """Where the arrays of one call live: on the host (numpy), or on GPU `device` (torch, which only a device side imports)."""

    def __init__(self, device=None):
        self.host = device is None
        if not self.host:
            import torch

            self._torch, self._where = torch, torch.device("cuda", device)

    def new(self, shape, kind=np.float32, zero=False):
        """A new array, zeroed or uninitialised.  kind: a numpy dtype; a device tensor is float32 for np.float32 and int32 for anything
        else (np.int32, and np.uint32: the same 32 bits)."""
        if self.host:
            return (np.zeros if zero else np.empty)(shape, kind)
        make = self._torch.zeros if zero else self._torch.empty
        return make(shape, dtype=self._torch.float32 if kind is np.float32 else self._torch.int32, device=self._where)

    def put(self, a, kind):
        """An input on this side: a device tensor as it is; anything else as a contiguous numpy array of `kind`, uploaded if the side is a
        GPU (np.uint32 as int32: the same 32 bits)."""
        if hasattr(a, "data_ptr"):
            return a
        a = np.ascontiguousarray(a, kind)
        return a if self.host else self._torch.from_numpy(a.view(np.int32) if kind is np.uint32 else a).to(self._where)


_HOST = _Side()


def _ptr(a, empty=False):
    """The address of a numpy array or a device tensor; None for no array and for an empty one -- unless `empty`: an empty numpy array
    has an address, for the entry points that refuse a null pointer whatever the item count."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return ctypes.c_void_p(a.data_ptr()) if a.numel() else None
    return a.ctypes.data_as(ctypes.c_void_p) if a.size or empty else None


def default_fit_levels(dims):
    """fitMesh's levels=None: the smallest L with ceil(n / 2^L) <= 64 on every axis, 10 at the most"""
    levels = 0
    while levels < 10 and max(-(-int(n) // (1 << levels)) for n in dims) > 64:
        levels += 1
    return levels


def measureGrid(box_lo, box_hi, cell, axis="z"):
    """The measure grid of a box: columns along `axis` ('x', 'y' or 'z'; dw is its unit vector) through the centres of square cells of
    edge `cell` on the box's lower face across it, ceil(extent / cell) per axis (u, v, w are a cyclic permutation of x, y, z).
    -> (MeasureGrid, t_max: the box's depth along the axis)"""
    if axis not in ("x", "y", "z"):
        raise ValueError("the measure axis must be x, y or z")
    w = "xyz".index(axis)
    u, v = (w + 1) % 3, (w + 2) % 3
    lo, hi, cell = [float(x) for x in box_lo], [float(x) for x in box_hi], float(cell)
    if not (cell > 0 and all(h > l for l, h in zip(lo, hi))):
        raise ValueError("the measure box needs lo < hi on every axis and a cell > 0")
    n = [max(1, int(np.ceil((hi[a] - lo[a]) / cell - 1e-6))) for a in (u, v)]
    if max(n) > 8192 or n[0] * n[1] > 1 << 24:
        raise ValueError("the measure box and cell give %dx%d columns: at most 8192 per axis and 2^24 in all" % tuple(n))
    origin, du, dv, dw = list(lo), [0.0] * 3, [0.0] * 3, [0.0] * 3
    origin[u], origin[v] = lo[u] + 0.5 * cell, lo[v] + 0.5 * cell
    du[u], dv[v], dw[w] = cell, cell, 1.0
    return MeasureGrid(_f3(origin), _f3(du), _f3(dv), _f3(dw), n[0], n[1]), hi[w] - lo[w]


def measureProperties(grid, result, density=1.0):
    """sdfr_measure_properties: volume, mass, centroid (world space) and the inertia tensor about the centroid (xx, yy, zz, xy, yz, zx) of a
    measure, as a dict; host arithmetic in fp64, no GPU"""
    out = SolidProperties()
    rc = load_library().sdfr_measure_properties(ctypes.byref(grid), ctypes.byref(result), float(density), ctypes.byref(out))
    if rc != SDFR_OK:
        raise SdfrError(rc, "bad arguments to sdfr_measure_properties")
    return out.as_dict()


def scene_names():
    L = load_library()
    return [L.sdfr_scene_name(i).decode() for i in range(L.sdfr_scene_count())]


def occlusionDirections():
    """The 64 directions of the occlusion queries (sdfr_occlusion_directions): [64, 3] float32 unit vectors, cosine-distributed over the
    hemisphere z > 0.  Bit k of a record's mask belongs to row k turned into the frame of the item's normal (include/sdfr.h)."""
    d = np.empty((64, 3), np.float32)
    rc = load_library().sdfr_occlusion_directions(d.ctypes.data_as(ctypes.c_void_p))
    if rc != 0:
        raise SdfrError(rc, "sdfr_occlusion_directions")
    return d


def chainContours(segments, layer_segments):
    """The segments of extractSlices joined into polylines, layer by layer: a list with one entry per layer, each a list of
    (vertex indices int64 [k], closed) in contour direction (the inside on the left).  Integer matching only: every vertex starts at most
    one segment and ends at most one.  Open chains come first, ordered by their first segment's index, each beginning at the vertex no
    segment ends at; closed loops follow, each starting at its lowest segment index (closed: the first vertex is not repeated)."""
    seg = np.asarray(segments).reshape(-1, 2).astype(np.int64)
    offsets = [int(v) for v in np.asarray(layer_segments).reshape(-1)]
    layers = []
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        part = seg[lo:hi]
        starts_at = {int(a): k for k, a in enumerate(part[:, 0])}  # vertex -> the segment that starts there
        ended = set(int(b) for b in part[:, 1])
        if len(starts_at) != len(part) or len(ended) != len(part):
            raise ValueError("chainContours: a vertex starts or ends more than one segment")
        used = np.zeros(len(part), bool)
        chains = []
        for closed in (False, True):
            for k in range(len(part)):
                if used[k] or (not closed and int(part[k, 0]) in ended):
                    continue
                chain = [int(part[k, 0])]
                while k is not None and not used[k]:
                    used[k] = True
                    chain.append(int(part[k, 1]))
                    k = starts_at.get(chain[-1])
                if closed:
                    chain.pop()  # (the loop came back to its first vertex)
                chains.append((np.asarray(chain, np.int64), closed))
        layers.append(chains)
    return layers


def atlasLayout(triangles, tile=8, width=None):
    """The texture atlas of a mesh of `triangles` triangles (sdfr_atlas_layout): one tile x tile square of texels per quad, `width`
    texels wide (default: atlasDefaultWidth).  -> Atlas (triangles, quads, tile, width, height, tiles_per_row, rows)."""
    a = Atlas()
    if width is None:
        width = atlasDefaultWidth(int(triangles) // 2, tile)
    rc = load_library().sdfr_atlas_layout(int(triangles), int(tile), int(width), ctypes.byref(a))
    if rc != 0:
        raise SdfrError(rc, "sdfr_atlas_layout: tile must be 4, 8, 16 or 32, width a multiple of 8 and of the tile up to 16384, triangles even")
    return a


def atlasDefaultWidth(quads, tile=8):
    """The smallest allowed atlas width >= tile * ceil(sqrt(quads)): a square-ish image."""
    tile, quads = int(tile), max(int(quads), 0)
    side = int(np.ceil(np.sqrt(quads)))
    while side * side < quads:
        side += 1
    step = max(8, tile)
    return min(max(step, (tile * side + step - 1) // step * step), 16384)


def atlasUVs(atlas):
    """The texture coordinates of the atlas (sdfr_atlas_uvs): [triangles, 3, 2] float32, one (u, v) per triangle corner in the order
    of the triangle's indices, origin top-left, every corner on the centre of its quad's corner texel."""
    uvs = np.empty((int(atlas.triangles), 3, 2), np.float32)
    rc = load_library().sdfr_atlas_uvs(ctypes.byref(atlas), uvs.ctypes.data_as(ctypes.c_void_p))
    if rc != 0:
        raise SdfrError(rc, "sdfr_atlas_uvs")
    return uvs


def check_scene_source(source, arch="gfx950"):
    """Compile a run-time scene without a device; returns (ok, compiler messages)."""
    log = ctypes.create_string_buffer(1 << 16)
    rc = load_library().sdfr_check_scene_source(_source_text(source).encode(), arch.encode(), log, len(log))
    return rc == SDFR_OK, log.value.decode(errors="replace")


def check_scene_hlsl(source, arch="gfx950"):
    """Compile a scene written in the reference's dialect (an .hlsl scene file's text, or its path) without a device;
    returns (ok, compiler messages).  sdfr_check_scene_hlsl."""
    log = ctypes.create_string_buffer(1 << 16)
    rc = load_library().sdfr_check_scene_hlsl(_source_text(source).encode(), arch.encode(), log, len(log))
    return rc == SDFR_OK, log.value.decode(errors="replace")


def translate_scene_hlsl(source):
    """The C++ the library generates from a scene in the reference's dialect (sdfr_translate_scene_hlsl): `struct UserScene`
    + the `Scene` typedef, to stand inside namespace sdfr after #include "sdfr_hlsl.h"."""
    L, text = load_library(), _source_text(source).encode()
    n = L.sdfr_translate_scene_hlsl(text, None, 0)
    buf = ctypes.create_string_buffer(n)
    L.sdfr_translate_scene_hlsl(text, buf, n)
    return buf.value.decode()


def strip_buffer_pixels(width, height, world, split=(0, 1)):
    return int(load_library().sdfr_strip_buffer_pixels_split(width, height, world, split[0], split[1]))


def strip_buffer_bytes(width, height, world, fmt, split=(0, 1)):
    """Bytes of one rank's compact strip buffer in format `fmt` (RGBA32F, RGBA16F or STRIP_RGB32F_A8);
    split = (priv_count, priv_period) of setStripSplit."""
    return int(load_library().sdfr_strip_buffer_bytes_split(width, height, world, fmt, split[0], split[1]))


def to_radian(deg):
    """Math3D::ToRadian (Math3D.h:299-303) in fp32."""
    return float(np.float32(deg) * np.float32(3.14159265358979) / np.float32(180.0))


class Camera:
    """First-person camera of the reference (Engine/Camera.h), parameters only: the basis
    arithmetic runs in the C++ host library (sdfr_set_camera_lookat / _direction)."""

    def __init__(self):
        # Application.cpp:214-224
        self.eye = (0.0, 2.0, -3.0)
        self.target = (0.0, 1.0, 0.0)
        self.target_is_direction = False
        self.fovy = to_radian(60.0)
        self.aspect = float(np.float32(1200.0) / np.float32(800.0))
        self.roll = 0.0

    def SetEye(self, eye):
        self.eye = tuple(float(x) for x in eye)

    def SetLookat(self, lookat):
        self.target = tuple(float(x) for x in lookat)
        self.target_is_direction = False

    def SetDirection(self, direction):
        self.target = tuple(float(x) for x in direction)
        self.target_is_direction = True

    def SetAspect(self, aspect):
        self.aspect = float(aspect)

    def SetFOVY(self, fovy):
        self.fovy = float(fovy)

    def SetRoll(self, roll):
        self.roll = float(roll)


class Variable:
    """One shader variable; assigning .value updates the renderer (the reference's UI
    writes through a raw pointer into the map, VariableManager.cpp:105,157)."""

    def __init__(self, owner, name, c):
        self._owner, self.name = owner, name
        self.minval, self.maxval, self.start, self.step = c.minval, c.maxval, c.start, c.step

    @property
    def value(self):
        out = ctypes.c_float()
        self._owner._check(self._owner._L.sdfr_var_get(self._owner._h, self.name.encode(), ctypes.byref(out)))
        return out.value

    @value.setter
    def value(self, v):
        self._owner._check(self._owner._L.sdfr_var_set(self._owner._h, self.name.encode(), float(v)))

    def __repr__(self):
        return "Variable(%s: min=%g max=%g start=%g step=%g value=%g)" % (self.name, self.minval, self.maxval, self.start, self.step, self.value)


class SDFRenderer:
    """The SDF render stage.  Mirrors Engine/SDFRenderer.h:17-44."""

    def __init__(self, device=0):
        self._L = load_library()
        self._h = ctypes.c_void_p()
        self._stime = 0.0
        self.init(device)

    # bool init(Graphics&) -- here: bind to a GPU
    def init(self, device=0):
        if self._h:
            self._L.sdfr_destroy(self._h)
            self._h = ctypes.c_void_p()
        rc = self._L.sdfr_create(int(device), ctypes.byref(self._h))
        if rc != SDFR_OK:
            raise SdfrError(rc, "sdfr_create(device=%d) failed" % device)
        self.device = int(device)
        self._frames_in_flight = 1
        return True

    def close(self):
        if self._h:
            self._L.sdfr_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != SDFR_OK:
            raise SdfrError(rc, self._L.sdfr_last_error(self._h).decode())

    # bool initShader(ShaderIncluder&) with the scene substitution of Application::loadScene
    def initShader(self, scene):
        self._check(self._L.sdfr_load_scene(self._h, scene.encode()))
        return True

    loadScene = initShader

    # the reference's edit-and-reload: compile a scene from its source text (hiprtc).  `source`
    # is the text or a path to it; on a compile error the previous scene stays active and
    # SdfrError carries the compiler's messages (SceneManager.cpp:118-127)
    def initShaderSource(self, name, source):
        self._check(self._L.sdfr_load_scene_source(self._h, name.encode(), _source_text(source).encode()))
        return True

    def initShaderHlsl(self, name, source):
        """A scene in the reference's own dialect: the text (or path) of an .hlsl scene file with map / map_normal / map_light /
        map_background, as Application::loadScene would substitute it into the shader (sdfr_load_scene_hlsl)."""
        self._check(self._L.sdfr_load_scene_hlsl(self._h, name.encode(), _source_text(source).encode()))
        return True

    def currentScene(self):
        s = self._L.sdfr_current_scene(self._h)
        return s.decode() if s else None

    # void setParameters(float stime)
    def setParameters(self, stime):
        self._stime = float(stime)
        self._check(self._L.sdfr_set_time(self._h, self._stime))

    # VariableMap &getVariableMap(): ordered like std::map
    def getVariableMap(self):
        out = {}
        for i in range(self._L.sdfr_var_count(self._h)):
            c = _CVariable()
            self._check(self._L.sdfr_var_info(self._h, i, ctypes.byref(c)))
            out[c.name.decode()] = Variable(self, c.name.decode(), c)
        return out

    def setValue(self, name, value):
        """ShaderVariableManager::setValue: unknown names are ignored (returns False)."""
        rc = self._L.sdfr_var_set(self._h, name.encode(), float(value))
        if rc == -3:
            return False
        self._check(rc)
        return True

    def resetVariables(self):
        self._check(self._L.sdfr_vars_reset(self._h))

    def setCamera(self, camera):
        fn = self._L.sdfr_set_camera_direction if camera.target_is_direction else self._L.sdfr_set_camera_lookat
        self._check(fn(self._h, _f3(camera.eye), _f3(camera.target), camera.fovy, camera.aspect, camera.roll))

    def setCameraBasis(self, eye, front, right, top):
        """The raw constant-buffer form (SDFRenderer.h:29-34)."""
        self._check(self._L.sdfr_set_camera(self._h, _f3(eye), _f3(front), _f3(right), _f3(top)))

    def getCameraBasis(self):
        out = (ctypes.c_float * 12)()
        self._check(self._L.sdfr_get_camera(self._h, out))
        return np.array(out, np.float32).reshape(4, 3)

    def getLimits(self):
        l = Limits()
        self._check(self._L.sdfr_get_limits(self._h, ctypes.byref(l)))
        return l

    def setLimits(self, **kw):
        l = self.getLimits()
        for k, v in kw.items():
            if not hasattr(l, k):
                raise AttributeError(k)
            setattr(l, k, v)
        self._check(self._L.sdfr_set_limits(self._h, ctypes.byref(l)))

    def setSchedule(self, schedule):
        self._check(self._L.sdfr_set_schedule(self._h, int(schedule)))

    def setLaunchMode(self, mode):
        """LAUNCH_AUTO (the scene's own choice), LAUNCH_PER_TILE or LAUNCH_PERSISTENT (sdfr_set_launch_mode)."""
        self._check(self._L.sdfr_set_launch_mode(self._h, int(mode)))

    def setStepShortcuts(self, enabled):
        """sdfr_set_step_shortcuts: rays their scene knows to be misses already stop marching (same pixels, fewer steps
        counted); off = every step marched, step counters equal the reference's."""
        self._check(self._L.sdfr_set_step_shortcuts(self._h, 1 if enabled else 0))

    def setProfiling(self, enabled):
        self._check(self._L.sdfr_set_profiling(self._h, 1 if enabled else 0))

    def setStream(self, stream_handle):
        self._check(self._L.sdfr_set_stream(self._h, ctypes.c_void_p(stream_handle)))

    # bool render(FullscreenQuad&, GPUProfiler&, Camera&)
    def render(self, camera=None, width=1200, height=800, out=None, fmt=RGBA32F, pixel_stats=False):
        """Renders one frame.  `out` may be a CUDA/HIP torch tensor ([H,W,4] float32 or
        float16) -> device-to-device, asynchronous on the renderer's stream; otherwise a host
        numpy array is returned (synchronous).  pixel_stats: True (host path) also returns
        [H,W,3] uint32 {rays, march evaluations, hits}; with a device `out` it may be a device
        int32/uint32 tensor [H,W,3] that receives them."""
        return self._render(self._L.sdfr_render, camera, (width, height), out, fmt, pixel_stats)

    def renderAA(self, camera=None, width=1200, height=800, factor=2, out=None, fmt=RGBA32F, pixel_stats=False):
        """Renders one anti-aliased frame (sdfr_render_aa): factor x factor sub-samples per pixel (factor 1, 2, 4 or 8), rendered and
        box-filtered on the GPU in passes of bounded memory.  Arguments and results as render(); alpha comes back as the share of a
        pixel's sub-samples that carry the tone-map flag, pixel_stats as the sums over them."""
        return self._render(self._L.sdfr_render_aa, camera, (width, height, factor), out, fmt, pixel_stats)

    def _render(self, call, camera, frame, out, fmt, pixel_stats):
        """render and renderAA: frame = (width, height) or (width, height, factor), the arguments of `call` after the handle"""
        if camera is not None:
            self.setCamera(camera)
        width, height = frame[0], frame[1]
        if out is not None and hasattr(out, "data_ptr"):
            assert out.is_cuda and out.is_contiguous() and out.numel() == width * height * 4
            pst = None
            if pixel_stats is not False and pixel_stats is not None:
                assert hasattr(pixel_stats, "data_ptr") and pixel_stats.is_cuda and pixel_stats.is_contiguous()
                assert pixel_stats.numel() == width * height * 3 and pixel_stats.element_size() == 4
                pst = ctypes.c_void_p(pixel_stats.data_ptr())
            self._check(call(self._h, *frame, ctypes.c_void_p(out.data_ptr()), fmt, 0, pst))
            return out
        dt = np.float32 if fmt == RGBA32F else np.float16
        img = np.zeros((height, width, 4), dt) if out is None else out
        st = np.zeros((height, width, 3), np.uint32) if pixel_stats else None
        self._check(call(self._h, *frame, img.ctypes.data_as(ctypes.c_void_p), fmt, 1, _ptr(st)))
        return (img, st) if pixel_stats else img

    # ---- questions put to the loaded scene (sdfr_query_distance / sdfr_query_rays / sdfr_pick; DESIGN.md "Queries") -------------
    # numpy arrays: the host path, answers returned as new arrays.  Contiguous device torch tensors: the device path, enqueued on the
    # handle's stream, answers written into the caller's tensors (`out`, like render(out=...)); a hit record is a row of an [n, 12]
    # float32 tensor whose integer fields (iterations, material_id, hit, reserved: columns 8-11) are read with .view(torch.int32).

    def _dev(self, t, numel, what, ints=False, hits=False):
        """the device pointer of a query tensor, after checking what the kernels will read or write through it: a contiguous tensor
        on the handle's GPU of `numel` float32 elements (int32 for pixels; hit records float32 or int32).  Raises, also under -O."""
        import torch

        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()):
            raise TypeError("%s: a contiguous device tensor is needed" % what)
        if t.device.index is not None and t.device.index != self.device:
            raise ValueError("%s: on %s, the renderer is on device %d" % (what, t.device, self.device))
        allowed = (torch.float32, torch.int32) if hits else ((torch.int32,) if ints else (torch.float32,))
        if t.dtype not in allowed:
            raise TypeError("%s: dtype %s, expected %s" % (what, t.dtype, " or ".join(str(d) for d in allowed)))
        if t.numel() != numel:
            raise ValueError("%s: %d elements, expected %d" % (what, t.numel(), numel))
        return ctypes.c_void_p(t.data_ptr())

    def _inputs(self, *specs):
        """The input arrays of a query, specs (array, dtype, columns, name): numpy arrays (made contiguous, of equal length) or, if the
        first is a device tensor, device tensors (checked: _dev).  -> (n, pointers, the side they are on)"""
        first, _dtype, columns, _name = specs[0]
        if hasattr(first, "data_ptr"):
            n, dev = first.numel() // columns, self._dev
            return n, [dev(a, c * n, name, dt is np.int32, dt is HIT_DTYPE) for a, dt, c, name in specs], _Side(self.device)
        arrays = []
        for a, dt, c, _name in specs:
            a = np.ascontiguousarray(a) if dt is HIT_DTYPE else np.ascontiguousarray(a, dt).reshape(-1, c)
            if dt is HIT_DTYPE and a.dtype != HIT_DTYPE:  # [n, 12] words
                a = np.ascontiguousarray(a.view(np.uint32).reshape(-1, c)).view(HIT_DTYPE).reshape(-1)
            assert not arrays or a.shape == arrays[0].shape
            arrays.append(a)
        return arrays[0].shape[0], [a.ctypes.data_as(ctypes.c_void_p) for a in arrays], _HOST

    # the answers of the queries: (numpy dtype, numpy columns, device tensor columns, device tensor is int32, hit records)
    _DISTANCE = (np.float32, 0, 0, False, False)
    _NORMALS = (np.float32, 3, 3, False, False)
    _HITS = (HIT_DTYPE, 0, 12, False, True)
    _SURFACES = (SURFACE_DTYPE, 0, 32, False, False)
    _OCCLUSION = (OCCLUSION_DTYPE, 0, 4, True, False)
    _LIGHTING = (LIGHTING_DTYPE, 0, 16, False, False)
    _LIGHT_SAMPLES = (LIGHT_SAMPLE_DTYPE, 8, 160, False, False)

    def _side(self, device):
        return _Side(self.device) if device else _HOST

    def _answer(self, n, side, kind, name, given=None):
        """One answer array of a query on the side of its inputs: a new numpy array, zeroed ([n] records, [n, columns] or [n] float32), or
        a device tensor -- the caller's `given`, checked, or a new one: [n, columns] or [n], float32 or int32.  -> (array, pointer)"""
        dtype, columns, words, ints, hits = kind
        if side.host:
            a = side.new((n, columns) if columns else n, dtype, zero=True)
            return a, _ptr(a)
        if given is None:
            given = side.new((n, words) if words else n, np.int32 if ints else np.float32)
        return given, self._dev(given, n * (words or 1), name, ints, hits)

    def _pixels(self, pixels_xy, width, height, device=False, upload=False):
        """The items of a pick: pixels [n, 2] as _span_inputs takes them (uploaded only if `upload`), or None: every pixel of the frame in
        row-major order, answered on the host or, with `device`, on the GPU.
        -> ((width, height, n, pointer or None): these arguments of the entry point, side, uploads)"""
        width, height = int(width), int(height)
        if pixels_xy is None:
            return (width, height, width * height, None), self._side(device), None
        n, (px,), side, uploads = self._span_inputs(upload and device, (pixels_xy, np.int32, 2, "pixels_xy"))
        return (width, height, n, px), side, uploads

    def queryDistance(self, points, normals=False, out=None, out_normals=None):
        """Scene distance at points [n, 3] (and the normal there if `normals`): distance [n] or (distance [n], normals [n, 3])."""
        n, (p,), side = self._inputs((points, np.float32, 3, "points"))
        d, pd = self._answer(n, side, self._DISTANCE, "out", out)
        nr, pn = self._answer(n, side, self._NORMALS, "out_normals", out_normals) if normals else (None, None)
        self._check(self._L.sdfr_query_distance(self._h, n, p, pd, pn, side.host))
        return (d, nr) if normals else d

    def queryRays(self, origins, dirs, max_distance=0.0, out=None):
        """First hit along rays origins [n, 3] + t * dirs [n, 3] (dirs as given, not normalised; max_distance 0 = limits.range):
        a HIT_DTYPE array [n], or the [n, 12] device tensor `out`."""
        n, (o, d), side = self._inputs((origins, np.float32, 3, "origins"), (dirs, np.float32, 3, "dirs"))
        hits, ph = self._answer(n, side, self._HITS, "out", out)
        self._check(self._L.sdfr_query_rays(self._h, n, o, d, float(max_distance), ph, side.host))
        return hits

    def pick(self, pixels_xy, width, height, camera=None, out=None):
        """What lies under pixels [n, 2] (x, y; row 0 = top) of a width x height frame of the current camera: a HIT_DTYPE array [n]
        (hit = -1 for a pixel outside the frame), or the [n, 12] device tensor `out`."""
        if camera is not None:
            self.setCamera(camera)
        frame, side, _uploads = self._pixels(pixels_xy, width, height)
        hits, ph = self._answer(frame[2], side, self._HITS, "out", out)
        self._check(self._L.sdfr_pick(self._h, *frame, ph, side.host))
        return hits

    # ---- what the surface looks like at a hit (sdfr_query_ray_surfaces / sdfr_pick_surfaces / sdfr_mesh_surfaces; DESIGN.md "Surface
    # queries").  numpy arrays in: SURFACE_DTYPE records out (and HIT_DTYPE records with hits=True).  Device tensors in: [n, 32] (and
    # [n, 12]) float32 device tensors out, whose integer fields (columns 0-3 of a surface) are read with .view(torch.int32).
    def _surfaces(self, call, n, side, hits, *scalars_and_inputs):
        h, ph = self._answer(n, side, self._HITS, "hits") if hits else (None, None)
        s, ps = self._answer(n, side, self._SURFACES, "surfaces")
        self._check(call(self._h, *scalars_and_inputs, ph, ps, side.host))
        return (h, s) if hits else s

    def queryRaySurfaces(self, origins, dirs, max_distance=0.0, hits=False):
        """The surface at the first hit along rays (as queryRays): SURFACE_DTYPE records [n], or (hits, surfaces) with hits=True."""
        n, (o, d), side = self._inputs((origins, np.float32, 3, "origins"), (dirs, np.float32, 3, "dirs"))
        return self._surfaces(self._L.sdfr_query_ray_surfaces, n, side, hits, n, o, d, float(max_distance))

    def pickSurfaces(self, pixels_xy, width, height, hits=False, device=False):
        """The surface under pixels [n, 2] of a width x height frame of the current camera (as pick).  pixels_xy=None: the G-buffer,
        every pixel of the frame in row-major order (height * width records; device=True: as device tensors)."""
        frame, side, _uploads = self._pixels(pixels_xy, width, height, device)
        return self._surfaces(self._L.sdfr_pick_surfaces, frame[2], side, hits, *frame)

    def meshSurfaces(self, positions, normals, reach, hits=False):
        """The surface at mesh vertices positions [n, 3] with normals [n, 3], each looked at from `reach` outside it along its normal
        (sdfr_mesh_surfaces); valid = 0 where that ray misses."""
        n, (p, nr), side = self._inputs((positions, np.float32, 3, "positions"), (normals, np.float32, 3, "normals"))
        return self._surfaces(self._L.sdfr_mesh_surfaces, n, side, hits, n, p, nr, float(reach))

    # ---- how the scene's lights fall on a hit (sdfr_query_ray_lighting / sdfr_pick_lighting / sdfr_mesh_lighting; DESIGN.md "Lighting
    # queries").  numpy arrays in: LIGHTING_DTYPE records out; hits=True adds HIT_DTYPE records in front, lights=True LIGHT_SAMPLE_DTYPE
    # records [n, 8] behind.  Device tensors in: [n, 16] (and [n, 12], [n, 160]) float32 device tensors out, whose integer fields are
    # read with .view(torch.int32).
    def _lighting(self, call, n, side, hits, lights, *scalars_and_inputs):
        h, ph = self._answer(n, side, self._HITS, "hits") if hits else (None, None)
        g, pg = self._answer(n, side, self._LIGHTING, "lighting")
        s, ps = self._answer(n, side, self._LIGHT_SAMPLES, "lights") if lights else (None, None)
        self._check(call(self._h, *scalars_and_inputs, ph, pg, ps, side.host))
        out = ((h,) if hits else ()) + (g,) + ((s,) if lights else ())
        return out if len(out) > 1 else g

    def queryRayLighting(self, origins, dirs, max_distance=0.0, hits=False, lights=False):
        """The direct lighting at the first hit along rays (as queryRays): LIGHTING_DTYPE records [n]; with hits and / or lights a tuple
        (hits, lighting, light samples [n, 8]) of those asked for."""
        n, (o, d), side = self._inputs((origins, np.float32, 3, "origins"), (dirs, np.float32, 3, "dirs"))
        return self._lighting(self._L.sdfr_query_ray_lighting, n, side, hits, lights, n, o, d, float(max_distance))

    def pickLighting(self, pixels_xy, width, height, hits=False, lights=False, device=False):
        """The direct lighting under pixels [n, 2] of a width x height frame of the current camera (as pick).  pixels_xy=None: every pixel
        of the frame in row-major order (height * width records; device=True: as device tensors)."""
        frame, side, _uploads = self._pixels(pixels_xy, width, height, device)
        return self._lighting(self._L.sdfr_pick_lighting, frame[2], side, hits, lights, *frame)

    def meshLighting(self, positions, normals, reach, hits=False, lights=False):
        """The direct lighting at mesh vertices positions [n, 3] with normals [n, 3], each looked at from `reach` outside it along its
        normal (sdfr_mesh_lighting); valid = 0 where that ray misses."""
        n, (p, nr), side = self._inputs((positions, np.float32, 3, "positions"), (normals, np.float32, 3, "normals"))
        return self._lighting(self._L.sdfr_mesh_lighting, n, side, hits, lights, n, p, nr, float(reach))

    # ---- ambient occlusion (sdfr_query_occlusion / sdfr_hit_occlusion; DESIGN.md "Occlusion queries").  numpy arrays in:
    # OCCLUSION_DTYPE records out.  Device tensors in: an [n, 4] int32 device tensor out (mask_lo, mask_hi, occluded, valid), enqueued
    # on the handle's stream.
    def queryOcclusion(self, points, normals, bias, radius):
        """Which of the 64 directions (occlusionDirections) above points [n, 3] with normals [n, 3] meet the scene within `radius`,
        the rays starting `bias` off each point along its normal: OCCLUSION_DTYPE records [n]; openness is 1 - occluded / 64."""
        n, (p, nr), side = self._inputs((points, np.float32, 3, "points"), (normals, np.float32, 3, "normals"))
        out, po = self._answer(n, side, self._OCCLUSION, "occlusion")
        self._check(self._L.sdfr_query_occlusion(self._h, n, p, nr, float(bias), float(radius), po, side.host))
        return out

    def hitOcclusion(self, hits, bias, radius):
        """queryOcclusion at the hits of queryRays, pick or the surface queries -- HIT_DTYPE records [n], or an [n, 12] device tensor --:
        valid = 0 where the ray missed, -1 where the item was invalid."""
        n, (h,), side = self._inputs((hits, HIT_DTYPE, 12, "hits"))
        out, po = self._answer(n, side, self._OCCLUSION, "occlusion")
        self._check(self._L.sdfr_hit_occlusion(self._h, n, h, float(bias), float(radius), po, side.host))
        return out

    # ---- the loaded scene as a triangle mesh (sdfr_mesh_extract; DESIGN.md "Mesh extraction") ------------------------------------
    def extractMesh(self, origin, cell, dims, iso=0.0, normals=True, device=False, surfaces=False, reach=None, occlusion=False, ao_radius=None,
                    ao_bias=None, lighting=False, atlas=None, sharp=False):
        """Surface nets over the lattice origin + (i, j, k) * cell, dims = (nx, ny, nz) cells: (positions [v, 3] float32, normals [v, 3]
        float32 or None, indices [t, 3]) -- numpy arrays (indices uint32), or with device=True torch tensors on the renderer's GPU
        (indices int32: the same 32 bits), enqueued on the handle's stream.  The counting call, then the filling call.
        sharp=True: sdfr_mesh_extract_sharp -- the same indices, every vertex moved onto the scene's planes at its cell's edge crossings, so
        that the scene's edges and corners stay sharp; everything below composes with it unchanged.
        surfaces=True: a fourth element, the surface at every vertex (meshSurfaces with `reach`, default 2 * cell; needs the normals) --
        the mesh is made on the GPU and looked at there, whatever `device` says about where the results go.
        occlusion=True: one more element, after the surfaces if both are asked for: the ambient occlusion at every vertex
        (queryOcclusion with ao_bias, default 1 cell, and ao_radius, default 8 cells; needs the normals), looked at on the GPU likewise.
        lighting=True: one more element, the last: the direct lighting at every vertex (meshLighting with `reach`; needs the normals).
        atlas=dict(tile=8, width=None, layers=("albedo",), occlusion=False): one more element after all of those: the mesh's texture atlas
        baked with `reach` -- bakeAtlas's dict with "uvs" [t, 3, 2] added (atlasUVs), and with occlusion=True an "openness" plane [H, W]
        (atlasTexels + queryOcclusion with ao_bias and ao_radius: 1 - occluded / 64 where that is answered, else 0)."""
        if surfaces or occlusion or lighting or atlas is not None:
            if not normals:
                raise ValueError("surfaces=True, occlusion=True, lighting=True and atlas need the normals")
            pos, nrm, idx = self.extractMesh(origin, cell, dims, iso, True, device=True, sharp=sharp)
            baked = None
            if atlas is not None:
                unknown = set(atlas) - {"tile", "width", "layers", "occlusion"}
                if unknown:
                    raise ValueError("atlas: unknown keys %s" % sorted(unknown))
                tile, width = atlas.get("tile", 8), atlas.get("width")
                baked = self.bakeAtlas(pos, nrm, idx, tile, width, 2.0 * float(cell) if reach is None else reach, atlas.get("layers", ("albedo",)))
                baked["uvs"] = atlasUVs(baked["atlas"])
                if atlas.get("occlusion"):
                    import torch

                    _a, tp, tn, tv = self.atlasTexels(pos, nrm, idx, tile, baked["atlas"].width)
                    ao = self.queryOcclusion(tp.reshape(-1, 3), tn.reshape(-1, 3), float(cell) if ao_bias is None else ao_bias,
                                             8.0 * float(cell) if ao_radius is None else ao_radius)
                    if self._frames_in_flight == 2:
                        self.sync()  # the handle's stream is then its own: torch's does not wait for the records and states it reads next
                    answered = (ao[:, 3] == 1) & (tv.reshape(-1) == 1)
                    baked["openness"] = torch.where(answered, 1.0 - ao[:, 2].to(torch.float32) / 64.0, torch.zeros((), device=ao.device)).reshape(tv.shape)
            extra = []
            if surfaces:
                extra.append(self.meshSurfaces(pos, nrm, 2.0 * float(cell) if reach is None else reach))
            if occlusion:
                extra.append(self.queryOcclusion(pos, nrm, float(cell) if ao_bias is None else ao_bias, 8.0 * float(cell) if ao_radius is None else ao_radius))
            if lighting:
                extra.append(self.meshLighting(pos, nrm, 2.0 * float(cell) if reach is None else reach))
            if device:
                return (pos, nrm, idx) + tuple(extra) + ((baked,) if baked is not None else ())
            self.sync()
            if baked is not None:
                baked = {k: (a.cpu().numpy() if hasattr(a, "data_ptr") else a) for k, a in baked.items()}
            if surfaces:
                extra[0] = extra[0].cpu().numpy().view(np.uint32).reshape(-1).view(SURFACE_DTYPE)
            if occlusion:
                k = 1 if surfaces else 0
                extra[k] = extra[k].cpu().numpy().view(np.uint32).reshape(-1).view(OCCLUSION_DTYPE)
            if lighting:
                extra[-1] = extra[-1].cpu().numpy().view(np.uint32).reshape(-1).view(LIGHTING_DTYPE)
            return (pos.cpu().numpy(), nrm.cpu().numpy(), idx.cpu().numpy().view(np.uint32)) + tuple(extra) + ((baked,) if baked is not None else ())
        extract = self._L.sdfr_mesh_extract_sharp if sharp else self._L.sdfr_mesh_extract
        return self._extract(extract, _mesh_grid(origin, cell, dims, iso), MeshCounts(), device, (3, 3, 3), normals, "mesh")

    def _extract(self, call, grid, counts, device, columns, with_second, what, *host_arrays):
        """The two calls of sdfr_mesh_extract and sdfr_slice_extract: the counting call, which fills `counts` (vertices, then triangles or
        segments), and -- unless there is no vertex -- the filling call into new arrays of those sizes, which must count the same.
        -> ([vertices, columns[0]] float32, [vertices, columns[1]] float32 or, without `with_second`, None, [counts' second, columns[2]]
        uint32 on the host, int32 on the device)"""
        side = self._side(device)
        self._check(call(self._h, ctypes.byref(grid), 0, 0, None, None, None, *host_arrays, ctypes.byref(counts), side.host))
        v, k = (int(getattr(counts, name)) for name, _type in counts._fields_)
        first = side.new((v, columns[0]))
        second = side.new((v, columns[1])) if with_second else None
        index = side.new((k, columns[2]), np.uint32)
        if v:
            again = type(counts)()
            self._check(call(self._h, ctypes.byref(grid), v, k, _ptr(first), _ptr(second), _ptr(index), *host_arrays, ctypes.byref(again), side.host))
            if bytes(again) != bytes(counts):
                raise SdfrError(-9, "the %s changed between the counting and the filling call" % what)
        return first, second, index

    # ---- the loaded scene's contours on a stack of planes (sdfr_slice_extract; DESIGN.md "Slices") ---------------------------------------
    def extractSlices(self, origin, du, dv, dw=(0.0, 0.0, 0.0), dims=(1, 1), layers=1, iso=0.0, coords=True, device=False):
        """Marching squares over `layers` plane lattices: point (i, j) of layer l at origin + i * du + j * dv + l * dw, dims = (nu, nv)
        cells.  -> (positions [v, 3] float32, coords [v, 2] float32 lattice coordinates or None, segments [s, 2] (start vertex, end vertex:
        the inside on the left), layer_vertices [layers + 1] int64, layer_segments [layers + 1] int64: layer l's vertices and segments are
        the rows layer_*[l] .. layer_*[l + 1]).  numpy arrays (segments uint32), or with device=True torch tensors on the renderer's GPU
        (segments int32: the same 32 bits), enqueued on the handle's stream; the two layer arrays are numpy either way.  The counting call,
        then the filling call.  chainContours joins the segments into polylines."""
        grid = SliceGrid(_f3(origin), _f3(du), _f3(dv), _f3(dw), int(dims[0]), int(dims[1]), int(layers), float(iso))
        n_layers = max(int(layers), 0) + 1
        layer_v, layer_s = np.zeros(n_layers, np.int64), np.zeros(n_layers, np.int64)
        pos, uv, seg = self._extract(self._L.sdfr_slice_extract, grid, SliceCounts(), device, (3, 2, 2), coords, "slices",
                                     layer_v.ctypes.data_as(ctypes.c_void_p), layer_s.ctypes.data_as(ctypes.c_void_p))
        return pos, uv, seg, layer_v, layer_s

    # ---- what a ray passes through (sdfr_query_ray_spans / sdfr_pick_spans / sdfr_mesh_spans; DESIGN.md "Spans") ----------------------------
    # -> (summaries, spans): numpy, SPAN_SUMMARY_DTYPE records [n] and float32 [n, max_spans, 2] (t_in, t_out); with device tensors in, or
    # device=True, device tensors: int32 [n, 8] (inside_length and t_end, columns 4 and 5, are read with .view(torch.float32)) and float32
    # [n, max_spans, 2], enqueued on the handle's stream.
    def _spans(self, call, n, side, uploads, min_step, t_max, iso, max_steps, max_spans, *scalars_and_inputs):
        params = SpanParams(float(t_max), float(min_step), float(iso), int(max_steps), int(max_spans))
        slots = min(max(int(max_spans), 0), 64)  # (a count the library refuses still gets its error from the library)
        if n == 0 and not side.host:  # (an empty tensor has no address)
            return side.new((0, 8), np.int32, zero=True), side.new((0, slots, 2), zero=True)
        # (on the device the kernel writes every word of every summary and every span slot)
        s = side.new(n, SPAN_SUMMARY_DTYPE, zero=True) if side.host else side.new((n, 8), np.int32)
        sp = side.new((n, slots, 2), zero=side.host)
        self._check(call(self._h, *scalars_and_inputs, ctypes.byref(params), _ptr(s, empty=True), _ptr(sp, empty=slots > 0), side.host))
        if uploads:  # made for this call: they may go only when the launch, which runs on the handle's stream, has read them
            self.sync()
        return s, sp

    def _span_inputs(self, device, *specs):
        """_inputs; with device=True numpy inputs are uploaded first.  -> (n, pointers, side, the uploads or None): the call that made
        uploads keeps them until it has synchronised (_spans)"""
        uploads = None
        if device and not hasattr(specs[0][0], "data_ptr"):
            side = self._side(True)
            uploads = [side.put(a, dt).reshape(-1, c) for a, dt, c, _name in specs]
            specs = [(up,) + spec[1:] for up, spec in zip(uploads, specs)]
        return self._inputs(*specs) + (uploads,)

    def querySpans(self, origins, dirs, min_step, t_max=0.0, iso=0.0, max_steps=4096, max_spans=4, device=False):
        """The intervals of rays origins [n, 3] + t * dirs [n, 3], 0 <= t <= t_max (0: limits.range; dirs as given, t in units of |dir|),
        that lie inside the solid (distance < iso), marched on the GPU in steps of max(|distance - iso|, min_step) -> (summaries, spans)."""
        n, (o, d), side, uploads = self._span_inputs(device, (origins, np.float32, 3, "origins"), (dirs, np.float32, 3, "dirs"))
        return self._spans(self._L.sdfr_query_ray_spans, n, side, uploads, min_step, t_max, iso, max_steps, max_spans, n, o, d)

    def pickSpans(self, pixels_xy, width, height, min_step, t_max=0.0, iso=0.0, max_steps=4096, max_spans=4, device=False):
        """querySpans along the primary rays of pixels [n, 2] of a width x height frame of the current camera (as pick; valid = -1 outside the
        frame).  pixels_xy=None: every pixel of the frame in row-major order (height * width items)."""
        frame, side, uploads = self._pixels(pixels_xy, width, height, device, upload=True)
        return self._spans(self._L.sdfr_pick_spans, frame[2], side, uploads, min_step, t_max, iso, max_steps, max_spans, *frame)

    def meshSpans(self, positions, normals, reach, min_step, t_max=0.0, iso=0.0, max_steps=4096, max_spans=4, device=False):
        """querySpans along sdfr_mesh_surfaces' rays: from positions [n, 3] + reach * normals [n, 3] along -normals.  The first span is the
        wall under the vertex."""
        n, (p, nr), side, uploads = self._span_inputs(device, (positions, np.float32, 3, "positions"), (normals, np.float32, 3, "normals"))
        return self._spans(self._L.sdfr_mesh_spans, n, side, uploads, min_step, t_max, iso, max_steps, max_spans, n, p, nr, float(reach))

    def meshThickness(self, positions, normals, reach, min_step, t_max=0.0, iso=0.0, max_steps=4096):
        """The wall thickness under mesh vertices: the length of meshSpans' first span, float32 [n] in units of |normal|; inf where there is
        none (the ray meets no solid, or the item is invalid) or where that span is closed only by the end of the march (ENDS_INSIDE)."""
        s, sp = self.meshSpans(positions, normals, reach, min_step, t_max, iso, max_steps, max_spans=1)
        if hasattr(s, "data_ptr"):
            self.sync()
            s, sp = s.cpu().numpy().view(SPAN_SUMMARY_DTYPE).reshape(-1), sp.cpu().numpy()
        out = np.full(len(s), np.inf, np.float32)
        closed = (s["valid"] == 1) & (s["spans"] >= 1) & ~((s["spans"] == 1) & ((s["flags"] & SPAN_ENDS_INSIDE) != 0))
        out[closed] = sp[closed, 0, 1] - sp[closed, 0, 0]
        return out

    # ---- how much solid there is (sdfr_measure; DESIGN.md "Measure") ---------------------------------------------------------------------
    def measure(self, grid, min_step, t_max=0.0, iso=0.0, max_steps=4096, columns=False, device=False):
        """The moments of the solid over the columns of `grid` (a MeasureGrid: measureGrid, or made by hand), each marched as querySpans
        marches a ray from its origin along grid.dw, integrated and summed on the GPU in a defined order -> a MeasureResult; with
        columns=True (result, columns): MEASURE_COLUMN_DTYPE records [nv, nu], or with device=True an int32 tensor [nv, nu, 10] on the
        renderer's GPU holding the same words."""
        params = SpanParams(float(t_max), float(min_step), float(iso), int(max_steps), 0)
        out, cols, side = MeasureResult(), None, self._side(device)
        n = (max(int(grid.nv), 0), max(int(grid.nu), 0))
        if columns:
            cols = side.new(n, MEASURE_COLUMN_DTYPE, zero=True) if side.host else side.new(n + (10,), np.int32)
        self._check(self._L.sdfr_measure(self._h, ctypes.byref(grid), ctypes.byref(params), ctypes.byref(out), _ptr(cols), side.host))
        return (out, cols) if columns else out


    measureProperties = staticmethod(measureProperties)

    def measureSolid(self, box_lo, box_hi, cell, axis="z", density=1.0, min_step=None, iso=0.0, max_steps=4096):
        """The one-call form: measureGrid over the box, measure with min_step (default cell / 2) over the box's depth, measureProperties
        -> a dict of the properties, with the MeasureResult as `result` and the grid as `grid`."""
        grid, depth = measureGrid(box_lo, box_hi, cell, axis)
        res = self.measure(grid, 0.5 * float(cell) if min_step is None else min_step, t_max=depth, iso=iso, max_steps=max_steps)
        props = measureProperties(grid, res, density)
        props["result"], props["grid"] = res, grid
        return props

    # ---- the texture atlas of a mesh (sdfr_atlas_texels / sdfr_atlas_bake; DESIGN.md "Texture atlas") -------------------------------
    def _atlas_inputs(self, positions, normals, indices, device):
        """The mesh of an atlas call on the GPU -- device tensors in, or device=True: numpy arrays are uploaded -- or else on the host.
        -> (vertex count, triangle count, pointers, side, the arrays: the caller keeps them for the length of its call)"""
        side = self._side(device or hasattr(positions, "data_ptr"))
        pos, nrm, idx = (side.put(a, kind).reshape(-1, 3) for a, kind in ((positions, np.float32), (normals, np.float32), (indices, np.uint32)))
        v, t = pos.shape[0], idx.shape[0]
        if side.host:
            if nrm.shape != pos.shape:
                raise ValueError("positions and normals differ in shape")
            return v, t, [_ptr(a) for a in (pos, nrm, idx)], side, (pos, nrm, idx)
        ptrs = [self._dev(pos, 3 * v, "positions") if v else None, self._dev(nrm, 3 * v, "normals") if v else None,
                self._dev(idx, 3 * t, "indices", ints=True) if t else None]
        return v, t, ptrs, side, (pos, nrm, idx)

    def atlasTexels(self, positions, normals, indices, tile=8, width=None, device=False):
        """The surface point and unit normal of every texel of the mesh's atlas (sdfr_atlas_texels): (atlas, positions [H, W, 3],
        normals [H, W, 3], valid [H, W] int32 -- 1, 0 for a degenerate texel, -1 for a texel of no well-formed quad, zeros there).
        numpy arrays, or torch tensors on the renderer's GPU with device tensors in or device=True.  Needs no scene."""
        v, t, ptrs, side, _keep = self._atlas_inputs(positions, normals, indices, device)
        atlas = atlasLayout(t, tile, width)
        h, w = atlas.height, atlas.width
        P, N, valid = side.new((h, w, 3)), side.new((h, w, 3)), side.new((h, w), np.int32)
        self._check(self._L.sdfr_atlas_texels(self._h, ctypes.byref(atlas), v, *ptrs, _ptr(P), _ptr(N), _ptr(valid), side.host))
        return atlas, P, N, valid

    def bakeAtlas(self, positions, normals, indices, tile=8, width=None, reach=None, layers=("albedo",), device=False):
        """Bake the loaded scene's surface into the mesh's atlas (sdfr_atlas_bake): every texel is looked at as meshSurfaces /
        meshLighting look at a vertex, from `reach` outside it along its normal.  layers: any of "albedo" (rgb + alpha), "normal"
        (the shading normal, 0) and "lit" (the direct lighting, 1).  -> {"atlas": Atlas, "valid": [H, W] int32 (1 hit, 0 miss or
        degenerate, -1 no quad), and one [H, W, 4] float32 plane per layer}: numpy arrays, or torch tensors on the renderer's GPU
        with device tensors in or device=True (enqueued on the handle's stream)."""
        if reach is None:
            raise ValueError("bakeAtlas needs a reach (a cell or two of the mesh's lattice)")
        layers = (layers,) if isinstance(layers, str) else tuple(layers)
        mask = 0
        for name in layers:
            if name not in ATLAS_LAYERS:
                raise ValueError("unknown atlas layer %r: one of %s" % (name, ", ".join(sorted(ATLAS_LAYERS))))
            mask |= ATLAS_LAYERS[name]
        v, t, ptrs, side, _keep = self._atlas_inputs(positions, normals, indices, device)
        atlas = atlasLayout(t, tile, width)
        h, w = atlas.height, atlas.width
        out = {"atlas": atlas}
        for name in ATLAS_LAYERS:
            if name in layers:
                out[name] = side.new((h, w, 4))
        out["valid"] = side.new((h, w), np.int32)
        self._check(self._L.sdfr_atlas_bake(self._h, ctypes.byref(atlas), v, *ptrs, float(reach), mask, *[_ptr(out.get(name)) for name in ATLAS_LAYERS],
                                            _ptr(out["valid"]), side.host))
        return out

    # ---- where the surface is (sdfr_mesh_survey / sdfr_mesh_fit; DESIGN.md "Mesh survey and fit") -----------------------------------
    def surveyMesh(self, origin, cell, dims, iso=0.0, band=0.0):
        """What the lattice of extractMesh(origin, cell, dims, iso) holds (sdfr_mesh_survey), counted on the GPU in integers: a dict of
        active_cells (the mesh's vertices), quads (half its triangles), near_cells (active, or a corner with |distance - iso| <= band),
        inside_points, the inclusive bounds active_lo / active_hi / near_lo / near_hi (none: lo = dims, hi = -1) and face_active, the
        active cells on the box's six faces -- non-zero where the surface leaves the box and the mesh is open."""
        grid = _mesh_grid(origin, cell, dims, iso)
        out = MeshSurvey()
        self._check(self._L.sdfr_mesh_survey(self._h, ctypes.byref(grid), float(band), ctypes.byref(out)))
        return out.as_dict()

    def fitMesh(self, origin, cell, dims, iso=0.0, levels=None, margin=1):
        """Shrink the search grid (origin, cell, dims) -- up to 2^20 cells per axis -- onto the surface, coarse to fine (sdfr_mesh_fit).
        levels=None: the smallest number of levels whose coarsest grid has at most 64 cells per axis (10 at the most).  -> a dict:
        state (FIT_EMPTY, FIT_FOUND, FIT_TOO_LARGE), level, surveys, the window lo / hi in search cells, survey (the last one run, or
        None), and for FIT_FOUND origin and dims of the fitted grid (else None), to hand to extractMesh with the same cell and iso.
        Coarse levels rest on the scene's distance never overestimating (what sphere tracing needs too); levels=0 rests on nothing."""
        if levels is None:
            levels = default_fit_levels(dims)
        grid = _mesh_grid(origin, cell, dims, iso)
        out = MeshFit()
        self._check(self._L.sdfr_mesh_fit(self._h, ctypes.byref(grid), int(levels), int(margin), ctypes.byref(out)))
        found = out.state == FIT_FOUND
        return dict(state=int(out.state), level=int(out.level), surveys=int(out.surveys), lo=tuple(out.lo), hi=tuple(out.hi),
                    origin=tuple(float(v) for v in out.grid.origin) if found else None,
                    dims=(int(out.grid.nx), int(out.grid.ny), int(out.grid.nz)) if found else None,
                    survey=out.last.as_dict() if out.surveys else None)

    # ---- whether the solid is in one piece (sdfr_components_label / sdfr_components_label_lattice; DESIGN.md "Components") ---------
    def _components(self, call, grid, lattice, want_labels, side):
        """The two calls of a labelling: the counting call, then the filling call into records of that size (and the labels), which must
        count the same.  -> (counts dict, records, labels or None)"""
        shape = (grid.nz + 1, grid.ny + 1, grid.nx + 1)
        counts = ComponentCounts()
        self._check(call(self._h, ctypes.byref(grid), *lattice, 0, None, None, ctypes.byref(counts), side.host))
        c = int(counts.components)
        records = side.new(c, COMPONENT_DTYPE, zero=True) if side.host else side.new((c, 10), np.int32)
        labels = side.new(shape, np.uint32) if want_labels else None
        again = ComponentCounts()
        self._check(call(self._h, ctypes.byref(grid), *lattice, c, _ptr(records), _ptr(labels), ctypes.byref(again), side.host))
        if bytes(again) != bytes(counts):
            raise SdfrError(-9, "the components changed between the counting and the filling call")
        return counts.as_dict(), records, labels

    def labelComponents(self, origin, cell, dims, iso=0.0, labels=False, device=False):
        """The parts and the enclosed voids of the loaded scene on the lattice of extractMesh(origin, cell, dims, iso)
        (sdfr_components_label): 6-connected components of the inside points (solids) and of the others (voids), numbered by their
        smallest linear index.  -> (counts, records, labels): counts a dict of components, solids, voids, closed_solids, closed_voids,
        inside_points, largest_solid_points and largest_void_points; records COMPONENT_DTYPE [components] (root, flags, points, lo,
        hi); labels uint32 [nz + 1, ny + 1, nx + 1] with labels=True, else None.  With device=True records are an int32 tensor
        [components, 10] holding the same words and labels an int32 tensor, on the renderer's GPU.  The call is synchronous."""
        return self._components(self._L.sdfr_components_label, _mesh_grid(origin, cell, dims, iso), (), labels, self._side(device))

    def labelLattice(self, lattice, iso=0.0, labels=False, device=False):
        """labelComponents of the caller's distances (sdfr_components_label_lattice): lattice [pz, py, px] float32, each at least 2
        points -- a numpy array, uploaded first if `device`, or a device tensor.  Needs no scene."""
        side = self._side(device or hasattr(lattice, "data_ptr"))
        if not hasattr(lattice, "data_ptr"):
            lattice = np.asarray(lattice, np.float32)
        if len(lattice.shape) != 3:
            raise ValueError("lattice: [pz, py, px] distances are needed")
        pz, py, px = (int(n) for n in lattice.shape)
        D = side.put(lattice, np.float32)
        pointer = _ptr(D, empty=True) if side.host else self._dev(D, px * py * pz, "lattice")
        return self._components(self._L.sdfr_components_label_lattice, _mesh_grid((0.0, 0.0, 0.0), 1.0, (px - 1, py - 1, pz - 1), iso), (pointer,), labels, side)

    def getMeshTimings(self):
        """GPU ms of the last extractMesh's filling call, if setProfiling(True) was on: {sample, classify_scan, emit, normals}."""
        ms = (ctypes.c_double * 4)()
        self._check(self._L.sdfr_mesh_get_timings(self._h, ctypes.byref(ms)))
        return dict(zip(("sample", "classify_scan", "emit", "normals"), [float(x) for x in ms]))

    def registerHostTarget(self, array):
        """Page-lock a numpy image that render(out=array) will fill every frame (sdfr_register_host_target); None
        unregisters.  The array must stay alive and unmoved while registered."""
        if array is None:
            self._check(self._L.sdfr_register_host_target(self._h, None, 0))
            self._host_target = None
        else:
            assert array.flags["C_CONTIGUOUS"]
            self._check(self._L.sdfr_register_host_target(self._h, array.ctypes.data_as(ctypes.c_void_p), array.nbytes))
            self._host_target = array  # keeps it alive

    def setStripSplit(self, priv_count, priv_period):
        """Of every priv_period strips the first priv_count are private to the root (renderPrivateStrips),
        the others are shared round-robin (renderStrips / assembleStrips).  (0, 1) = plain round-robin."""
        self._check(self._L.sdfr_set_strip_split(self._h, int(priv_count), int(priv_period)))
        self._split = (int(priv_count), int(priv_period))

    def renderPrivateStrips(self, width, height, out, fmt=RGBA32F):
        """Root only: render the private strips straight into the full-size device image `out`."""
        assert out.is_cuda and out.is_contiguous() and out.numel() == width * height * 4
        self._check(self._L.sdfr_render_private_strips(self._h, width, height, ctypes.c_void_p(out.data_ptr()), fmt))
        return out

    def renderStrips(self, width, height, rank, world, out, fmt=RGBA32F):
        """Multi-GPU: render this rank's 8-row strips into the compact device tensor `out`."""
        assert out.is_cuda and out.is_contiguous()
        assert out.numel() * out.element_size() == strip_buffer_bytes(width, height, world, fmt, getattr(self, "_split", (0, 1)))
        self._check(self._L.sdfr_render_strips(self._h, width, height, rank, world, ctypes.c_void_p(out.data_ptr()), fmt))
        return out

    def assembleStrips(self, width, height, world, gathered, out, fmt=RGBA32F):
        self._check(self._L.sdfr_assemble_strips(self._h, width, height, world, ctypes.c_void_p(gathered.data_ptr()),
                                                 ctypes.c_void_p(out.data_ptr()), fmt))
        return out

    def renderGather(self, comm, width, height, out=None, fmt=RGBA32F, wire=None):
        """Multi-GPU frame through the library's own RCCL gather (sdfr_render_gather): every rank renders
        its strips, rank 0 receives them and assembles `out` (a device tensor of the full frame; None
        on the other ranks).  wire: strip format on the links (default: the packed one that matches fmt)."""
        if wire is None:
            wire = STRIP_RGB32F_A8 if fmt == RGBA32F else STRIP_RGB16F_A8
        ptr = None
        if out is not None:
            assert out.is_cuda and out.is_contiguous() and out.numel() == width * height * 4
            assert out.element_size() == (4 if fmt == RGBA32F else 2)
            ptr = ctypes.c_void_p(out.data_ptr())
        self._check(self._L.sdfr_render_gather(self._h, comm._c, width, height, ptr, fmt, wire))
        return out

    def getTimings(self):
        """GPUProfiler::getResults: {name: ms} of the last render and the last postprocess, in frame order."""
        buf = (_CTiming * 48)()
        n = self._L.sdfr_get_timings(self._h, buf, 48)
        if n < 0:
            self._check(n)
        return {buf[i].name.decode(): buf[i].ms for i in range(min(n, 48))}

    def postprocess(self, scene16, bloom_scratch, out8):
        """HDR::process on device tensors: scene16/bloom_scratch [H,W,4] float16, out8 [H,W,4] uint8."""
        H, W = scene16.shape[0], scene16.shape[1]
        assert scene16.is_cuda and scene16.is_contiguous() and bloom_scratch.is_contiguous() and out8.is_contiguous()
        assert bloom_scratch.numel() == scene16.numel() == out8.numel()
        self._check(self._L.sdfr_postprocess(self._h, W, H, ctypes.c_void_p(scene16.data_ptr()), ctypes.c_void_p(bloom_scratch.data_ptr()),
                                             ctypes.c_void_p(out8.data_ptr())))
        return out8

    def selftestMath(self, what, constant=1.0):
        """Exhaustive GPU check of the fast exact sqrt (what=0) / constant division (what=1); returns mismatches."""
        n = ctypes.c_uint64()
        self._check(self._L.sdfr_selftest_math(self._h, int(what), float(constant), ctypes.byref(n)))
        return int(n.value)

    def sync(self):
        self._check(self._L.sdfr_sync(self._h))

    def setFramesInFlight(self, n):
        """sdfr_set_frames_in_flight: 2 = render() alternates between two internal streams and workspaces, so that a frame starts
        while the one before drains (render into two images in turn; sync() waits for both); 1 = the default."""
        self._check(self._L.sdfr_set_frames_in_flight(self._h, int(n)))
        self._frames_in_flight = int(n)

    def waitFrame(self, stream=None):
        """sdfr_wait_frame: `stream` (a raw hipStream_t / torch stream's .cuda_stream; None = the default stream) waits on the
        device for the frame submitted last"""
        self._check(self._L.sdfr_wait_frame(self._h, ctypes.c_void_p(stream)))

    def getStats(self):
        s = Stats()
        self._check(self._L.sdfr_get_stats(self._h, ctypes.byref(s)))
        return s


class HDR:
    """The post-processing stage that consumes the render target.  Mirrors the reference's
    `class HDR` (Engine/Postprocessing.h:12-43): init / getRenderTarget / process.  The three
    RGBA16F textures of the reference become two device tensors (render target + one bloom
    buffer; the second bloom texture is never materialised, see sdfr_post.hip)."""

    def __init__(self, renderer):
        self._r = renderer
        self.width = self.height = 0

    def init(self, width, height):
        import torch

        self.width, self.height = int(width), int(height)
        self._target = torch.zeros((self.height, self.width, 4), dtype=torch.float16, device="cuda")
        self._bloom = torch.empty_like(self._target)
        self._ldr = torch.empty((self.height, self.width, 4), dtype=torch.uint8, device="cuda")
        return True

    def getRenderTarget(self):
        """The RGBA16F tensor SDFRenderer.render(..., out=..., fmt=RGBA16F) draws into."""
        return self._target

    def process(self, scene=None):
        """bloom + tone map of the render target (or of `scene`, an [H,W,4] float16 cuda
        tensor) -> [H,W,4] uint8 cuda tensor (R8G8B8A8_UNORM)."""
        src = self._target if scene is None else scene
        return self._r.postprocess(src, self._bloom, self._ldr)

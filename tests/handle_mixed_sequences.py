"""Seeded sequences of MIXED calls on ONE renderer handle: renders, anti-aliased frames, post-processing, every query family, mesh
extraction (plain and sharp), atlas calls, surveys and fits, slices, span queries, measures and component labellings, interleaved.
tests/handle_sequences.py drives what a handle carries from frame to frame; this module drives the state the handle has gained
since: the staging of host queries (`query`, cut per call and released past 64 MiB), the extraction workspace (`mesh`, cut two to
six ways by the mesh, the survey, the slices, the measure and the labelling, which cuts it again in the middle of its call once the
components are counted, reused across lanes behind an event, released past 64 MiB), the
supersampling buffers, and the per-handle query kernels in their DBG and non-DBG variants, on built-in scenes and on one compiled
at run time.

No torch, no GPU: the CPU tier (tests/test_handle_mixed_cpu.py) proves what the committed seeds cover, the GPU tier
(tests/test_gpu_handle_mixed.py) runs them.  A step is one call on the handle, with the settings changed just before it (`set`) and
the whole state a fresh handle needs to answer it (`state`).  The inputs of a call are drawn from the step's own seeded generator
(rays(), points(), normals(), pixel_list(), the lattice, slice stack or measure grid in the step; a labelling's own lattice is
components_util.synthetic of the step's kind, dims and seed)."""
import math
import random

import handle_sequences as hs

FAMILIES = ("render", "aa", "post", "points", "rays", "pick", "surfaces", "occlusion", "lighting", "mesh", "atlas", "survey", "slices", "spans", "measure",
            "components", "failed")
# sdfr_postprocess takes device tensors only; sdfr_mesh_survey and sdfr_mesh_fit answer into one host record and have no on_host
HOST_AND_DEVICE = tuple(f for f in FAMILIES if f not in ("post", "survey", "failed"))
DEVICE_ONLY = ("post", "survey")
# (failed, failed) cannot be: a failed call always sits between two valid calls
PAIRS = tuple((a, b) for a in FAMILIES for b in FAMILIES if (a, b) != ("failed", "failed"))

ITEMS = (1, 63, 64, 65, 255, 1000, 4096)
FRAME_SIZES = tuple(s for s in hs.SMALL_SIZES if s[0] <= 320 and s[1] <= 180)
AA_SIZES = tuple(s for s in FRAME_SIZES if s[0] <= 160 and s[1] <= 90)
AA_FACTORS = (2, 4)
MAX_LATTICE = 24
CELLS = (0.09, 0.13, 0.17)
TILES = (4, 8, 16)
MAX_ATLAS_WIDTH = 256
LAYER_SETS = (("albedo",), ("normal",), ("lit",), ("albedo", "normal"), ("albedo", "lit"), ("normal", "lit"), ("albedo", "normal", "lit"))
MESH_FORMS = (None, None, "surfaces", "occlusion", "lighting", "atlas_occlusion", "sharp", "sharp_surfaces")
SHARP_FORMS = ("sharp", "sharp_surfaces")         # sdfr_mesh_extract_sharp; the second feeds its vertices to meshSurfaces
AXES = ("x", "y", "z")
BANDS = (0.0, 0.5, 2.0)                           # surveyMesh: the band in cells
FIT_LEVELS, FIT_MARGINS, MAX_FIT = (0, 2, 3), (0, 1), 40  # fitMesh: a search grid of at most MAX_FIT (<= 64) cells per axis
MAX_SLICE_LAYERS = 8
MAX_SPANS = (0, 1, 3, 64)
SPAN_CALLS = ("querySpans", "pickSpans", "pickSpansFrame", "meshSpans")
# (min_step, t_max, max_steps) of the span calls.  "finish": every ray reaches t_max (t_max / min_step + 1 <= max_steps); "short": a small
# min_step and 32 steps, so that rays near a surface run out of steps.  Rays and pixels march a quarter of limits.range, a mesh's rays
# (unit normals, from 0.2 outside the vertex) two units
SPAN_PARAMS = {"finish": dict(rays=(100.0 / 256.0, 25.0, 256), mesh=(0.05, 2.0, 256)), "short": dict(rays=(0.02, 25.0, 32), mesh=(0.01, 2.0, 32))}
MEASURE_COLUMNS = (1, 7, 8, 9, 24)
MEASURE_BIG = 72                                  # 72 x 72 columns are 81 tiles: more than a run of 64, so that k_measure_reduce runs a pass
# (min_step, max_steps) of a measure; dw spans the box, so t_max = 1.  "short": columns near a surface run out of steps.  iso is 0 but for
# the measure of the workspace_cuts block
MEASURE_PARAMS = {"finish": (1.0 / 64.0, 128), "short": (1.0 / 512.0, 48)}
COMPONENT_CALLS = ("labelComponents", "labelLattice")  # the scene's own distances on the step's lattice; the caller's lattice
# labelLattice: components_util.synthetic(kind, dims, seed) -- every point a component, one long path, an enclosed void, -0.0 and tiny values
SYNTHETIC_KINDS = ("noise", "checkerboard", "serpentine", "hollow_box", "zeros")
# the capacity of a labelling by name, the count C being known only on the GPU: "none" capacity 0 and no records (the counting call),
# "exact" C, "roomy" C + 3, "short" C - 1 (SDFR_OK with the counts, the records untouched, the labels written; C = 1: as "exact")
CAPACITY_RULES = ("none", "exact", "roomy", "short")
GROW_DIMS = (47, 47, 31)                          # 48 x 48 x 32 points: as a checkerboard more components than COMPONENTS_TABLE_FIRST
SPLITS = hs.SPLITS
DEBUG_VARS = {"debug_nx": 0.3, "debug_ny": 1.0}  # + the point debug_vars() puts the plane through: the driver's debug plane
KEEP = 64 << 20                                   # k_query_stage_keep (sdfr_api.cpp): what a handle keeps of `query` and of `mesh`
STAGE_ALIGN = 256                                 # SDFR_STAGE_ALIGN (sdfr_stage.h)
MESH_BLOCK = 256                                  # SDFR_MESH_BLOCK (sdfr_mesh.h)
HIT_BYTES, SURFACE_BYTES, OCCLUSION_BYTES, LIGHTING_BYTES, LIGHTS_BYTES = 48, 128, 16, 64, 8 * 80
SPAN_SUMMARY_BYTES, SPAN_BYTES, MEASURE_COLUMN_BYTES = 32, 8, 40
MESH_SURVEY_WORK_BYTES = 4096 * (1 + 10 + 12)     # sdfr_mesh_survey.h
MEASURE_TALLY_BYTES = 128 * (2 + 13 * 16)         # sdfr_query_args.h
COMPONENT_BYTES, COMPONENT_RESULT_BYTES, COMPONENTS_TABLE_FIRST = 40, 256 * 8, 1 << 16  # sdfr_components.h, sdfr_components_plan.h

# argument errors refused on the host before anything is launched: (kind, sdfr_last_error); all SDFR_ERR_INVALID_ARGUMENT but the capacities
# smaller than the counts, which is SDFR_OK with the counts and nothing written
FAILURES = (("negative_n", "bad item count"), ("null_pointer", "null pointer"), ("bad_on_host", "on_host must be 0 or 1"),
            ("mesh_negative_capacity", "negative capacity"), ("mesh_small_capacity", None), ("aa_factor_3", "factor must be 1, 2, 4 or 8"),
            ("aa_bad_format", "bad format"), ("atlas_bad_layout", "bad atlas"), ("slice_negative_capacity", "negative capacity"),
            ("slice_small_capacity", None), ("span_max_spans_65", "bad span parameters"), ("measure_nu_0", "bad measure grid"),
            ("survey_bad_band", "band must be finite and >= 0"), ("fit_bad_margin", "margin must be 0..8"),
            ("components_negative_capacity", "negative capacity"), ("components_small_capacity", None), ("components_null_lattice", "null pointer"))
FAILURE_KINDS = tuple(k for k, _ in FAILURES)
SHARED_KINDS = FAILURE_KINDS[:3]  # the argument errors every query entry has
SPAN_ENTRIES = ("ray_spans", "pick_spans", "mesh_spans")
FAILURE_ENTRIES = ("points", "rays", "pick", "surfaces", "occlusion", "lighting") + SPAN_ENTRIES  # whose entry a shared kind goes through

BLOCKS = ("staging", "lanes", "large_mesh", "aa_in_flight", "scene_change", "workspace_cuts", "large_new", "components_grow")
STRETCH = 10  # free steps on the run-time scene, inside the scene_change block: one entry per seed (every entry compiles the scene again)
BLOCK_STEPS = {"staging": 4, "lanes": 4, "large_mesh": 2, "aa_in_flight": 6, "scene_change": 4 + STRETCH, "workspace_cuts": 6, "large_new": 5,
               "components_grow": 6}
BIG_FRAME = (384, 240)  # pickLighting(None, hits, lights) of it on the host: past the keep (staging_bytes)
BIG_SPAN_FRAME = (448, 280)  # pickSpans(None, max_spans=64) of it on the host: past the keep; 440 x 280 is not

SEEDS = (143, 136, 319, 54, 2, 8, 226, 285)  # the committed seeds (what they cover: tests/test_handle_mixed_cpu.py)
STEPS = 80

# the scene variables the sequences move (hs.SCENE_VARS, but the lense stays off the camera orbit's centre: at zpos 0 nothing of the scene
# is left around it, and the lattices there would be empty)
SCENE_VARS = dict(hs.SCENE_VARS, lense=dict(hs.SCENE_VARS["lense"], zpos=(5.0, 25.0)))

# where a scene's surface is: the centre of its point boxes and lattices
CENTRES = {"labyrinth": (-2.0, 3.9, 4.37), "cube_sea": (0.0, 0.1, 0.0), "fractal": (0.5, 1.2, 0.0), "lense": (0.0, 0.0, 0.0), "gems": (1.0, 0.1, -2.2),
           "light_shadows": (0.0, 1.2, -0.5), hs.RUNTIME_SCENE: (0.0, 1.2, -1.0)}


def _aligned(b):
    return (b + STAGE_ALIGN - 1) // STAGE_ALIGN * STAGE_ALIGN


def stage_total(pieces):
    """stage_offsets (sdfr_stage.h): the pieces one after the other, each on a multiple of 256 bytes"""
    return sum(_aligned(b) for b in pieces)


def staging_bytes(step):
    """bytes of `query` a HOST call stages, by the formulas of the plans (sdfr_query_plan.h, sdfr_atlas_plan.h, sdfr_mesh_plan.h); a mesh
    extraction's are known only with its counts: None"""
    p = step
    n = p.get("n", 0)
    hits = HIT_BYTES if p.get("hits") else 0
    call = p["call"]
    if call == "queryDistance":
        return stage_total([n * 12, 0, n * 4, n * 12 if p["normals"] else 0, 0, 0])
    if call in ("queryRays", "pick"):
        return stage_total([n * (8 if call == "pick" else 12), 0 if call == "pick" else n * 12, n * HIT_BYTES, 0, 0, 0])
    if call in ("queryRaySurfaces", "meshSurfaces", "pickSurfaces"):
        ins = [0, 0] if p.get("frame") else ([n * 8, 0] if call == "pickSurfaces" else [n * 12, n * 12])
        return stage_total(ins + [n * hits, n * SURFACE_BYTES, 0, 0])
    if call in ("queryRayLighting", "meshLighting", "pickLighting"):
        ins = [0, 0] if p.get("frame") else ([n * 8, 0] if call == "pickLighting" else [n * 12, n * 12])
        return stage_total(ins + [n * hits, 0, n * LIGHTING_BYTES, n * LIGHTS_BYTES if p["lights"] else 0])
    if call == "queryOcclusion":
        return stage_total([n * 12, n * 12, n * OCCLUSION_BYTES, 0, 0, 0])
    if call == "hitOcclusion":
        return stage_total([n * HIT_BYTES, 0, n * OCCLUSION_BYTES, 0, 0, 0])
    if call in ("querySpans", "pickSpans", "meshSpans"):  # plan_spans (sdfr_span_plan.h): the two inputs, the summaries, the spans
        ins = [0, 0] if p.get("frame") else ([n * 8, 0] if call == "pickSpans" else [n * 12, n * 12])
        return stage_total(ins + [n * SPAN_SUMMARY_BYTES, n * p["max_spans"] * SPAN_BYTES])
    if call == "measure":  # plan_measure (sdfr_measure_plan.h): the columns alone
        g = p["grid"]
        return stage_total([g["nu"] * g["nv"] * MEASURE_COLUMN_BYTES if p["columns"] else 0])
    if call in COMPONENT_CALLS:  # components_impl (sdfr_api.cpp): the caller's lattice and the labels; the records come straight from the table
        pts = lattice_points(component_dims(p))
        return stage_total([pts * 4 if call == "labelLattice" else 0, pts * 4 if p["labels"] else 0])
    return None


def lattice_points(dims):
    return (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1)


def component_dims(step):
    """the cells of a labelling's lattice: the step's lattice around the scene, or the dims of the caller's"""
    return step["lattice"]["dims"] if step["call"] == "labelComponents" else step["dims"]


def _scan_sum_words(n):
    """mesh_scan_sum_words (sdfr_mesh.h)"""
    words = 0
    while n > MESH_BLOCK:
        n = (n + MESH_BLOCK - 1) // MESH_BLOCK
        words += n
    return words


def workspace_bytes(dims):
    """bytes of `mesh` an extraction over `dims` cells needs, plain or sharp: the four pieces of plan_mesh (sdfr_mesh_plan.h)"""
    points = (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1)
    cells = dims[0] * dims[1] * dims[2]
    return stage_total([points * 4, (cells + 1) * 4, (points + 1) * 4, (_scan_sum_words(cells + 1) + _scan_sum_words(points + 1)) * 4])


def survey_workspace_bytes(dims):
    """... a survey of `dims` cells needs: the two pieces of plan_mesh_survey (sdfr_mesh_plan.h)"""
    return stage_total([(dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1) * 4, MESH_SURVEY_WORK_BYTES])


def slice_workspace_bytes(dims, layers):
    """... a slice extraction of `layers` lattices of `dims` cells needs: the five pieces of plan_slice (sdfr_slice_plan.h)"""
    points = (dims[0] + 1) * (dims[1] + 1) * layers
    return stage_total([points * 4, (points + 1) * 4, (points + 1) * 4, 2 * _scan_sum_words(points + 1) * 4, 2 * (layers + 1) * 4])


def measure_workspace_bytes(nu, nv):
    """... a measure of nu x nv columns needs: the three pieces of plan_measure (sdfr_measure_plan.h)"""
    tiles = ((nu + 7) // 8) * ((nv + 7) // 8)
    return stage_total([tiles * 80, (tiles + 63) // 64 * 80, MEASURE_TALLY_BYTES])


def components_workspace_bytes(dims, own_lattice, components):
    """... a labelling over `dims` cells needs once `components` are counted: the six pieces of plan_components and of
    plan_components_fill (sdfr_components_plan.h) -- the table has room for COMPONENTS_TABLE_FIRST components (or every point's, if
    fewer) and never less.  The cut before they are counted: components = 1"""
    points = lattice_points(dims)
    table = max(min(points, COMPONENTS_TABLE_FIRST), components) * COMPONENT_BYTES
    return stage_total([0 if own_lattice else points * 4, points * 4, (points + 1) * 4, _scan_sum_words(points + 1) * 4, COMPONENT_RESULT_BYTES, table])


def _smallest(past):
    n = 1
    while not past(n):
        n += 1
    return n


BIG_LATTICE = (_smallest(lambda n: workspace_bytes((n, n, n)) > KEEP),) * 3          # the smallest cube of cells whose workspace is past the keep
BIG_SURVEY = (_smallest(lambda n: survey_workspace_bytes((n, n, n)) > KEEP),) * 3    # ... whose survey's workspace is
BIG_COMPONENTS = (_smallest(lambda n: components_workspace_bytes((n, n, n), False, 1) > KEEP),) * 3  # ... whose labelling's workspace is
BIG_SLICE_LAYERS = 8
BIG_SLICE = (_smallest(lambda n: slice_workspace_bytes((n, n), BIG_SLICE_LAYERS) > KEEP),) * 2  # the smallest square stack of 8 layers likewise


def slice_grid(lat, axis, layers, angle=0.0):
    """the slice stack of a lattice's box: `layers` planes across `axis`, each in the middle of its slab of the box, cells of the
    lattice's size along the two other axes (u, v, w: the cyclic order that ends in the axis); angle: du and dv turned about dw, the
    layer's middle staying where it is"""
    w = AXES.index(axis)
    u, v = (w + 1) % 3, (w + 2) % 3
    cell, dims = lat["cell"], lat["dims"]
    depth = dims[w] * cell / layers
    c, s = math.cos(angle), math.sin(angle)
    du, dv, dw = [0.0] * 3, [0.0] * 3, [0.0] * 3
    du[u], du[v], dv[u], dv[v], dw[w] = cell * c, cell * s, -cell * s, cell * c, depth
    mid = list(lat["origin"])
    mid[u], mid[v], mid[w] = mid[u] + 0.5 * dims[u] * cell, mid[v] + 0.5 * dims[v] * cell, mid[w] + 0.5 * depth
    origin = [mid[a] - 0.5 * dims[u] * du[a] - 0.5 * dims[v] * dv[a] for a in range(3)]
    r = lambda x: tuple(round(t, 5) for t in x)  # noqa: E731
    return dict(origin=r(origin), du=r(du), dv=r(dv), dw=r(dw), dims=(dims[u], dims[v]), layers=layers)


def measure_grid(lat, axis, nu, nv, tilt=0.0):
    """nu x nv columns over a lattice's box, through the middles of their cells of its lower face across `axis`; dw spans the box's
    depth (t_max = 1); tilt: dw leans towards u by that share of the depth"""
    w = AXES.index(axis)
    u, v = (w + 1) % 3, (w + 2) % 3
    cell, dims = lat["cell"], lat["dims"]
    du, dv, dw = [0.0] * 3, [0.0] * 3, [0.0] * 3
    du[u], dv[v], dw[w] = dims[u] * cell / nu, dims[v] * cell / nv, dims[w] * cell
    dw[u] = tilt * dw[w]
    origin = list(lat["origin"])
    origin[u], origin[v] = origin[u] + 0.5 * du[u] - 0.5 * dw[u], origin[v] + 0.5 * dv[v]
    r = lambda x: tuple(round(t, 5) for t in x)  # noqa: E731
    return dict(origin=r(origin), du=r(du), dv=r(dv), dw=r(dw), nu=nu, nv=nv)


def span_params(step):
    """(min_step, t_max, max_steps) of a span step"""
    return SPAN_PARAMS[step["march"]]["mesh" if step["call"] == "meshSpans" else "rays"]


def eye_and_front(scene, t):
    kind, eye, target = hs.camera(scene, t)
    d = target if kind == "dir" else tuple(a - b for a, b in zip(target, eye))
    n = math.sqrt(sum(x * x for x in d))
    return eye, tuple(x / n for x in d)


def rays(step):
    """(origins, dirs), n rows each: from the step's camera eye into a cone around its view direction, lengths 0.25 .. 4 as given"""
    rng = random.Random(step["seed"])
    eye, front = eye_and_front(step["state"]["scene"], step["state"]["t"])
    dirs = []
    for _ in range(step["n"]):
        length = math.exp(rng.uniform(math.log(0.25), math.log(4.0)))
        dirs.append(tuple((f + rng.uniform(-0.6, 0.6)) * length for f in front))
    return [eye] * step["n"], dirs


def points(step):
    """n points of a box around the scene's centre"""
    rng = random.Random(step["seed"] + 1)
    c = CENTRES[step["state"]["scene"]]
    return [tuple(c[a] + rng.uniform(-2.5, 2.5) for a in range(3)) for _ in range(step["n"])]


def normals(step):
    """n unit vectors"""
    rng = random.Random(step["seed"] + 2)
    out = []
    while len(out) < step["n"]:
        v = [rng.gauss(0, 1) for _ in range(3)]
        n = math.sqrt(sum(x * x for x in v))
        if n > 1e-3:
            out.append(tuple(x / n for x in v))
    return out


def pixel_list(step):
    """n pixels (x, y) of the step's w x h frame and of a rim around it: the first is always outside"""
    rng = random.Random(step["seed"] + 3)
    w, h = step["w"], step["h"]
    out = [(-1, 0), (w, h - 1), (0, h), (w - 1, h - 1), (0, 0)][:step["n"]]
    while len(out) < step["n"]:
        out.append((rng.randrange(-2, w + 2), rng.randrange(-2, h + 2)))
    return out


def lattice(scene, rng, most=MAX_LATTICE, least=5, dims=None, cell=None):
    """(origin, cell, dims) of a lattice around the scene's centre, a little off it so that no lattice plane is a plane of the scene"""
    cell = cell or rng.choice(CELLS)
    dims = dims or tuple(rng.randrange(least, most + 1) for _ in range(3))
    c = CENTRES[scene]
    origin = tuple(round(c[a] - 0.5 * dims[a] * cell + rng.uniform(0.01, 0.05), 4) for a in range(3))
    return dict(origin=origin, cell=cell, dims=dims)


def debug_vars(scene):
    """the driver's debug plane through a point a little under the scene's centre, tilted"""
    c = CENTRES[scene]
    return dict(DEBUG_VARS, debug_x=c[0], debug_y=round(c[1] - 0.1, 3), debug_z=c[2])


def oracle_frame(oracle, st, w, h):
    """the oracle's frame (oracle: the pyoracle module) of a step's state `st` for a w x h image: the orbit's camera, the limits, the
    scene variables and the debug plane"""
    import numpy as np

    fovy = np.float32(60.0) * np.float32(3.14159265358979) / np.float32(180.0)
    kind, eye, target = hs.camera(st["scene"], st["t"])
    basis = (oracle.camera_lookat if kind == "lookat" else oracle.camera_direction)(eye, target, fovy, np.float32(w) / np.float32(h))
    f = oracle.default_frame(st["scene"], w, h, basis=basis, stime=st["stime"])
    for name, v in dict(hs.DEFAULT_LIMITS, **hs.LIMITS[st["limits"]]).items():
        setattr(f, name, v)
    slots = {row[0]: row[6] for row in oracle.var_table(st["scene"])}
    for name, v in list(st["vars"].items()) + (list(debug_vars(st["scene"]).items()) if st["debug"] else []):
        if slots[name] >= 0:
            f.scene_var[slots[name]] = v
        else:
            setattr(f, name, v)
    return f


def share_of(pair):
    """which of the committed seeds works towards a pair of families first: a diagonal, so that no seed has all the pairs of one family"""
    return (FAMILIES.index(pair[0]) + FAMILIES.index(pair[1])) % len(SEEDS)


def slot_of(seed):
    return SEEDS.index(seed) if seed in SEEDS else seed % len(SEEDS)


class _Gen:
    def __init__(self, seed, n, slot=None):
        self.rng = rng = random.Random(seed)
        self.n = n
        self.slot = slot_of(seed) if slot is None else slot
        self.state = dict(scene=None, limits="default", vars={}, t=0.0, stime=0.0, schedule="pixel", launch="auto", shortcuts=False, fif=1,
                          debug=False, split=(0, 1))
        self.steps = []
        self.runtime_entries = 0
        self.failed = 0
        # this seed's share of the coverage the committed seeds have together
        self.want_pairs = {p for p in PAIRS if share_of(p) == self.slot}
        self.want_runtime = {f for k, f in enumerate(FAMILIES) if k % len(SEEDS) == self.slot}
        self.want_forms = {(f, host, fif) for f in HOST_AND_DEVICE for host in (False, True) for fif in (1, 2)}
        self.want_forms |= {(f, False, fif) for f in DEVICE_ONLY for fif in (1, 2)}
        self.want_debug = set(FAMILIES)
        self.used = {}
        self.last_frame = None   # index of the last render / aa step: what post processes
        self.last_hits = None    # index of the last step that answered hit records
        self.last_mesh = None    # index of the last extraction
        # the scripted blocks in a seeded order, with seeded gaps of free steps between them
        order = list(BLOCKS)
        rng.shuffle(order)
        free = n - sum(BLOCK_STEPS.values())
        cuts = sorted(rng.sample(range(3, free - 3), len(order)))
        self.block_at, at = {}, 0
        for k, name in enumerate(order):
            at = cuts[k] + sum(BLOCK_STEPS[b] for b in order[:k])
            self.block_at[at] = name
        self.scripted = set()  # the steps that are scripted: all of a block's but the free steps of the stretch
        for at, name in self.block_at.items():
            self.scripted.update(k for k in range(at, at + BLOCK_STEPS[name]) if name != "scene_change" or not 2 <= k - at < 2 + STRETCH)

    # ---- state -----------------------------------------------------------------------------------------------------------------
    def change(self, key, value, changes):
        if self.state[key] != value:
            self.state[key] = value
            changes[key] = value

    def load(self, scene, changes):
        st = self.state
        if scene == st["scene"]:
            return
        if scene == hs.RUNTIME_SCENE:
            self.runtime_entries += 1
        st["vars"] = {}  # loading a scene resets its variables, the debug plane's too
        st["debug"] = False
        st["scene"] = changes["scene"] = scene
        st["t"] = changes["t"] = round(self.rng.uniform(0, 2 * math.pi), 4)

    def builtin(self, changes):
        self.load(self.rng.choice([s for s in hs.BUILTIN_SCENES if s != self.state["scene"]]), changes)

    def place(self, changes):
        """the scene of a free step: now and then another built-in one, once a stretch on the run-time scene"""
        rng, st = self.rng, self.state
        if st["scene"] is None:
            self.builtin(changes)
        elif rng.random() < 0.12:
            self.builtin(changes)

    def settings(self, family, changes):
        rng, st = self.rng, self.state
        if st["scene"] is None:
            self.builtin(changes)
        scene = st["scene"]
        if rng.random() < 0.15:
            self.change("schedule", rng.choice(hs.SCHEDULES), changes)
        if rng.random() < 0.2:
            self.change("launch", rng.choice(hs.LAUNCH_MODES), changes)
        if rng.random() < 0.15:
            self.change("shortcuts", not st["shortcuts"], changes)
        if rng.random() < 0.12:
            self.change("limits", rng.choice(sorted(hs.LIMITS)), changes)
        if scene in SCENE_VARS and rng.random() < 0.25:
            name = rng.choice(sorted(SCENE_VARS[scene]))
            lo, hi = SCENE_VARS[scene][name]
            v = round(rng.uniform(lo, hi), 3)
            st["vars"] = dict(st["vars"], **{name: v})
            changes["var"] = (name, v)
        debug = st["debug"]
        if family in self.want_debug:
            debug = debug or rng.random() < 0.5
        elif rng.random() < 0.25:
            debug = not debug
        self.change("debug", debug, changes)
        if rng.random() < 0.5:
            self.change("t", round(rng.uniform(0, 2 * math.pi), 4), changes)
        if rng.random() < 0.25:
            self.change("stime", round(rng.uniform(0, 3), 3), changes)

    # ---- what comes next -------------------------------------------------------------------------------------------------------
    def allowed(self, i):
        prev = self.steps[-1]["family"] if self.steps else None
        out = [f for f in FAMILIES if f != "failed"]
        if self.last_frame is None:
            out.remove("post")
        edge = i == 0 or i == self.n - 1 or i + 1 in self.scripted or i - 1 in self.scripted
        if prev not in (None, "failed") and not edge:
            out.append("failed")
        return out

    def pick_family(self, i):
        rng = self.rng
        if i == 0:
            return "render"
        prev = self.steps[-1]["family"]
        allowed = self.allowed(i)
        if prev == "failed" and self.steps[-1]["fail"].startswith("mesh_") and self.steps[-2]["family"] in FAILURE_ENTRIES[:6] and "render" in allowed:
            return "render"  # a failed mesh call between a query and a render: one of the interleavings the sequences are there for
        if self.state["scene"] == hs.RUNTIME_SCENE:
            duty = [f for f in allowed if f in self.want_runtime]
            if duty:
                return rng.choice(duty)
        fresh = [f for f in allowed if (prev, f) in self.want_pairs]
        if fresh:
            return rng.choice(fresh)
        # nothing new from here: go where the most is left to start from (a failed call cannot be followed by one)
        left = {f: sum(1 for (a, b) in self.want_pairs if a == f and (f != "failed" or b != "failed")) for f in allowed}
        best = max(left.values())
        if best == 0:
            return rng.choice([f for f in allowed if f != "failed"])
        return rng.choice([f for f in allowed if left[f] == best])

    def pick_form(self, family, changes):
        """host or device, and one or two frames in flight: what is left to cover first"""
        rng, st = self.rng, self.state
        left = sorted((h, fif) for (f, h, fif) in self.want_forms if f == family)  # (sorted: a set's order is not the seed's)
        if family in DEVICE_ONLY:
            host = False
            if left and st["fif"] not in [fif for _h, fif in left]:
                self.change("fif", left[0][1], changes)
            elif not left and rng.random() < 0.15:
                self.change("fif", 3 - st["fif"], changes)
        elif left:
            here = [h for h, fif in left if fif == st["fif"]]
            if here:
                host = rng.choice(here)
            else:
                host, fif = rng.choice(left)
                self.change("fif", fif, changes)
        else:
            host = rng.random() < 0.5
            if rng.random() < 0.1:
                self.change("fif", 3 - st["fif"], changes)
        return host

    def vary(self, key, options):
        """one of `options`, those not yet taken for `key` first: a seed goes through the variants of a call instead of drawing some twice"""
        used = self.used.setdefault(key, [])
        left = [o for o in options if o not in used]
        if not left:
            del used[:]
            left = list(options)
        o = self.rng.choice(left)
        used.append(o)
        return o

    # ---- the calls -------------------------------------------------------------------------------------------------------------
    def new(self, i, family, call, changes, host, block=None, **params):
        s = dict(i=i, family=family, call=call, host=host, set=changes, block=block, seed=self.rng.randrange(1 << 30), **params)
        s["state"] = dict(self.state, vars=dict(self.state["vars"]))
        self.steps.append(s)
        st = self.state
        if len(self.steps) > 1:
            self.want_pairs.discard((self.steps[-2]["family"], family))
        if has_form(s):
            self.want_forms.discard((family, host, st["fif"]))
        if st["debug"]:
            self.want_debug.discard(family)
        if st["scene"] == hs.RUNTIME_SCENE:
            self.want_runtime.discard(family)
        if family in ("render", "aa") and call != "renderPrivateStrips":
            self.last_frame = i
        if (call in ("queryRays", "pick") or params.get("hits")) and block is None:
            self.last_hits = i
        if family == "mesh" and call == "extractMesh" and block != "large_mesh":
            self.last_mesh = i
        return s

    def free_step(self, i, family, changes):
        rng, st, vary = self.rng, self.state, self.vary
        host = self.pick_form(family, changes)
        scene = st["scene"]
        yes_no = (False, True)
        n = vary("n " + family, ITEMS)
        w, h = vary("size", FRAME_SIZES)
        if family == "render":
            return self.new(i, family, "render", changes, host, w=w, h=h, fmt=vary("render fmt", (hs.RGBA32F, hs.RGBA16F)), stats=vary("render stats", yes_no))
        if family == "aa":
            w, h = vary("aa size", AA_SIZES)
            return self.new(i, family, "renderAA", changes, host, w=w, h=h, factor=vary("factor", AA_FACTORS), fmt=vary("aa fmt", (hs.RGBA32F, hs.RGBA16F)),
                            stats=vary("aa stats", yes_no))
        if family == "post":
            return self.new(i, family, "postprocess", changes, False, src=self.last_frame)
        if family == "points":
            return self.new(i, family, "queryDistance", changes, host, n=n, normals=vary("points normals", yes_no))
        if family == "rays":
            return self.new(i, family, "queryRays", changes, host, n=n)
        if family == "pick":
            return self.new(i, family, "pick", changes, host, n=n, w=w, h=h)
        if family == "surfaces":
            call = vary("surfaces", ("queryRaySurfaces", "pickSurfaces", "pickSurfacesFrame", "meshSurfaces"))
            hits = vary(call + " hits", yes_no)
            if call == "pickSurfacesFrame":
                return self.new(i, family, "pickSurfaces", changes, host, n=w * h, w=w, h=h, frame=True, hits=hits)
            if call == "meshSurfaces":
                return self.new(i, family, call, changes, host, n=n, hits=hits, lattice=lattice(scene, rng), reach=0.2)
            return self.new(i, family, call, changes, host, n=n, w=w, h=h, frame=False, hits=hits)
        if family == "occlusion":
            call = vary("occlusion", ("hitOcclusion of a step", "hitOcclusion", "queryOcclusion"))
            if call == "hitOcclusion of a step" and self.last_hits is not None:
                return self.new(i, family, "hitOcclusion", changes, host, n=self.steps[self.last_hits]["n"], src=self.last_hits, bias=0.01, radius=1.0)
            if call == "hitOcclusion":
                return self.new(i, family, "hitOcclusion", changes, host, n=n, src=None, bias=0.01, radius=1.0)
            return self.new(i, family, "queryOcclusion", changes, host, n=n, bias=0.05, radius=1.0)
        if family == "lighting":
            call = vary("lighting", ("queryRayLighting", "pickLighting", "pickLightingFrame", "meshLighting"))
            hits, lights = vary(call + " hits", yes_no), vary(call + " lights", yes_no)
            if call == "pickLightingFrame":
                return self.new(i, family, "pickLighting", changes, host, n=w * h, w=w, h=h, frame=True, hits=hits, lights=lights)
            if call == "meshLighting":
                return self.new(i, family, call, changes, host, n=n, hits=hits, lights=lights, lattice=lattice(scene, rng), reach=0.2)
            return self.new(i, family, call, changes, host, n=n, w=w, h=h, frame=False, hits=hits, lights=lights)
        if family == "mesh":
            form = vary("mesh form", MESH_FORMS)
            lat = lattice(scene, rng, 14 if form == "atlas_occlusion" else MAX_LATTICE)
            more = dict(tile=vary("tile", TILES), width=vary("width", (64, 128, MAX_ATLAS_WIDTH)), layers=vary("layers", LAYER_SETS)) if form == "atlas_occlusion" else {}
            return self.new(i, family, "extractMesh", changes, host, lattice=lat, normals=form not in (None, "sharp") or vary("mesh normals", yes_no), form=form, **more)
        if family == "atlas":
            src = self.last_mesh if self.last_mesh is not None and vary("atlas src", yes_no) else None
            lat = self.steps[src]["lattice"] if src is not None else lattice(scene, rng, 12)
            call = vary("atlas", ("atlasTexels", "bakeAtlas", "bakeAtlas"))
            return self.new(i, family, call, changes, host, src=src, lattice=lat, tile=vary("tile", TILES), width=vary("width", (64, 128, MAX_ATLAS_WIDTH)),
                            layers=vary("layers", LAYER_SETS) if call == "bakeAtlas" else (), reach=0.2)
        if family == "survey":
            if vary("survey", ("surveyMesh", "surveyMesh", "fitMesh")) == "fitMesh":
                return self.new(i, family, "fitMesh", changes, False, lattice=lattice(scene, rng, MAX_FIT, 24), levels=vary("levels", FIT_LEVELS),
                                margin=vary("margin", FIT_MARGINS))
            lat = lattice(scene, rng)
            return self.new(i, family, "surveyMesh", changes, False, lattice=lat, band=round(vary("band", BANDS) * lat["cell"], 4))
        if family == "slices":
            lat = lattice(scene, rng)
            axis = vary("slice axis", AXES + ("oblique",))
            stack = slice_grid(lat, rng.choice(AXES), vary("slice layers", tuple(range(1, MAX_SLICE_LAYERS + 1))), round(rng.uniform(0.2, 1.3), 3)) \
                if axis == "oblique" else slice_grid(lat, axis, vary("slice layers", tuple(range(1, MAX_SLICE_LAYERS + 1))))
            call = vary("slices", ("extractSlices", "extractSlices", "extractSlices", "countSlices"))
            return self.new(i, family, call, changes, host, slices=stack, axis=axis, coords=vary("coords", yes_no), layer_vertices=vary("layer_vertices", yes_no),
                            layer_segments=vary("layer_segments", yes_no))
        if family == "spans":
            call = vary("spans", SPAN_CALLS)
            more = dict(max_spans=vary("max_spans", MAX_SPANS), march=vary("march", tuple(SPAN_PARAMS)))
            if call == "pickSpansFrame":
                w, h = vary("spans size", AA_SIZES)
                return self.new(i, family, "pickSpans", changes, host, n=w * h, w=w, h=h, frame=True, **more)
            if call == "meshSpans":
                return self.new(i, family, call, changes, host, n=n, lattice=lattice(scene, rng), reach=0.2, **more)
            return self.new(i, family, call, changes, host, n=n, w=w, h=h, frame=False, **more)
        if family == "measure":
            big = vary("measure big", (False, False, False, True))
            nu, nv = (MEASURE_BIG, MEASURE_BIG) if big else (vary("nu", MEASURE_COLUMNS), vary("nv", MEASURE_COLUMNS))
            axis = vary("measure axis", AXES + ("tilted",))
            grid = measure_grid(lattice(scene, rng), rng.choice(AXES), nu, nv, 0.3) if axis == "tilted" else measure_grid(lattice(scene, rng), axis, nu, nv)
            return self.new(i, family, "measure", changes, host, grid=grid, axis=axis, columns=vary("columns", yes_no), march=vary("measure march", tuple(MEASURE_PARAMS)))
        if family == "components":
            call = vary("components", COMPONENT_CALLS)
            more = dict(labels=vary(call + " labels", yes_no), capacity=vary(call + " capacity", CAPACITY_RULES))
            if call == "labelLattice":
                return self.new(i, family, call, changes, host, dims=lattice(scene, rng)["dims"], kind=vary("synthetic", SYNTHETIC_KINDS), **more)
            return self.new(i, family, call, changes, host, lattice=lattice(scene, rng), **more)
        assert family == "failed"
        # the failed calls of all seeds are numbered slot, slot + seeds, ...: the kinds in turn, and a shared kind through the entries in turn,
        # the span entries first
        g = self.slot + self.failed * len(SEEDS)
        kind = FAILURE_KINDS[g % len(FAILURE_KINDS)]
        turn = SPAN_ENTRIES + FAILURE_ENTRIES[:-len(SPAN_ENTRIES)]
        entry = turn[(g // len(FAILURE_KINDS) * len(SHARED_KINDS) + g % len(FAILURE_KINDS)) % len(turn)]
        self.failed += 1
        lat = lattice(scene, rng, 8)
        return self.new(i, family, "failed", changes, rng.random() < 0.5, fail=kind, entry=entry, n=rng.choice(ITEMS[:5]), w=w, h=h, lattice=lat,
                        slices=slice_grid(lat, "y", 4))

    # ---- the scripted blocks ---------------------------------------------------------------------------------------------------
    def block(self, i, name):
        rng, st = self.rng, self.state
        k = i - [at for at, b in self.block_at.items() if b == name][0]
        changes = {}
        if k == 0 and name != "scene_change":
            self.settings("render", changes)
            if st["scene"] == hs.RUNTIME_SCENE:
                self.builtin(changes)
        scene = st["scene"]
        if name == "staging":
            # a host query past the keep (`query` is released at its end), then the three ways `query` is cut, small
            if k == 0:
                w, h = BIG_FRAME
                return self.new(i, "lighting", "pickLighting", changes, True, name, n=w * h, w=w, h=h, frame=True, hits=True, lights=True)
            if k == 1:
                return self.new(i, "atlas", "bakeAtlas", changes, True, name, src=None, lattice=lattice(scene, rng, 8), tile=4, width=64,
                                layers=("albedo", "normal", "lit"), reach=0.2)
            if k == 2:
                return self.new(i, "mesh", "extractMesh", changes, True, name, lattice=lattice(scene, rng, 9), normals=True, form=None)
            return self.new(i, "rays", "queryRays", changes, True, name, n=65)
        if name == "lanes":
            # two frames in flight: an extraction on one lane, a frame (the lanes swap), a larger extraction on the other lane (waits
            # for the first one's emit work, grows `mesh`), a smaller one (reuses it); read after one sync
            self.change("fif", 2, changes)
            if k == 1:
                w, h = rng.choice(FRAME_SIZES[3:])
                return self.new(i, "render", "render", changes, False, name, w=w, h=h, fmt=hs.RGBA32F, stats=True, defer=True)
            lat = lattice(scene, rng, dims={0: (11, 9, 10), 2: (24, 23, 22), 3: (7, 8, 6)}[k])
            return self.new(i, "mesh", "extractMesh", changes, False, name, lattice=lat, normals=True, form=None, defer=k != 3)
        if name == "large_mesh":
            lat = lattice(scene, rng, 10)
            if k == 0:
                lat = lattice(scene, rng, dims=BIG_LATTICE, cell=0.02)
                return self.new(i, "mesh", "countMesh", changes, rng.random() < 0.5, name, lattice=lat, normals=False, form=None)
            return self.new(i, "mesh", "extractMesh", changes, rng.random() < 0.5, name, lattice=lat, normals=True, form=None)
        if name == "aa_in_flight":
            # a strip split left set across an anti-aliased frame between two plain frames in flight; A, B: two images of one size
            self.change("fif", 2, changes)
            if k == 0:
                self.size = rng.choice(AA_SIZES[3:])
                self.change("schedule", "pixel", changes)
                split = rng.choice(SPLITS)
                if st["split"] != split:
                    st["split"] = changes["split"] = split
            w, h = self.size
            if k in (0, 5):
                return self.new(i, "render", "renderPrivateStrips", changes, False, name, w=w, h=h, fmt=hs.RGBA32F, stats=False)
            self.change("t", round(rng.uniform(0, 2 * math.pi), 4), changes)
            if k == 2:
                return self.new(i, "aa", "renderAA", changes, False, name, w=w, h=h, factor=2, fmt=hs.RGBA32F, stats=True, image="B", defer=True)
            return self.new(i, "render", "render", changes, False, name, w=w, h=h, fmt=hs.RGBA32F, stats=True, image="AB"[k == 3], defer=k != 4)
        if name == "workspace_cuts":
            # `mesh` cut 5, 3, 2, 4 and 5 ways in one run, two frames in flight, every output in device form: a slice extraction at the
            # largest free size (its emit enqueued), a frame (the lanes swap), a measure smaller than that workspace (it lands inside what
            # the emit still reads) and a survey, both synchronous and read at once, a sharp extraction larger than all before (`mesh`
            # grows behind the event), a smaller slice extraction (reuses it); the deferred answers are read after that one's sync
            self.change("fif", 2, changes)
            if k == 0:
                stack = slice_grid(lattice(scene, rng, dims=(MAX_LATTICE,) * 3), rng.choice(AXES), MAX_SLICE_LAYERS)
                return self.new(i, "slices", "extractSlices", changes, False, name, slices=stack, axis=None, coords=True, layer_vertices=True, layer_segments=True, defer=True)
            if k == 1:
                w, h = rng.choice(FRAME_SIZES[3:])
                return self.new(i, "render", "render", changes, False, name, w=w, h=h, fmt=hs.RGBA32F, stats=True, defer=True)
            if k == 2:
                grid = measure_grid(lattice(scene, rng, dims=(12, 12, 12), cell=0.13), rng.choice(AXES), MEASURE_COLUMNS[-1], MEASURE_COLUMNS[-1])
                return self.new(i, "measure", "measure", changes, False, name, grid=grid, axis=None, columns=True, march="finish", iso=0.01, alone=True)
            if k == 3:
                lat = lattice(scene, rng, dims=(9, 10, 11))
                return self.new(i, "survey", "surveyMesh", changes, False, name, lattice=lat, band=round(0.5 * lat["cell"], 4), alone=True)
            if k == 4:
                return self.new(i, "mesh", "extractMesh", changes, False, name, lattice=lattice(scene, rng, dims=(24, 23, 22)), normals=True, form="sharp", defer=True)
            stack = slice_grid(lattice(scene, rng, dims=(9, 7, 8)), "y", 3)
            return self.new(i, "slices", "extractSlices", changes, False, name, slices=stack, axis=None, coords=True, layer_vertices=True, layer_segments=True)
        if name == "large_new":
            # the large calls of the survey, the slices and the spans, each followed by a small call that cuts the buffer again: a survey
            # past the keep; a counting call of a stack past the keep, then a small measure; a host pickSpans of a whole frame whose staging
            # is past the keep, then a small host measure with `columns`, which is staged in `query`
            if k == 0:
                lat = lattice(scene, rng, dims=BIG_SURVEY, cell=0.02)
                return self.new(i, "survey", "surveyMesh", changes, False, name, lattice=lat, band=0.0)
            if k == 1:
                n = BIG_SLICE[0]
                stack = slice_grid(dict(origin=tuple(round(c - 0.5 * n * 0.005 + 0.003, 4) for c in CENTRES[scene]), cell=0.005, dims=(n, n, n)), "y", BIG_SLICE_LAYERS)
                return self.new(i, "slices", "countSlices", changes, rng.random() < 0.5, name, slices=stack, axis=None, coords=False, layer_vertices=True, layer_segments=True)
            if k in (2, 4):
                grid = measure_grid(lattice(scene, rng, dims=(12, 12, 12), cell=0.13), rng.choice(AXES), 9, 8)
                return self.new(i, "measure", "measure", changes, k == 4 or rng.random() < 0.5, name, grid=grid, axis=None, columns=True, march="finish")
            w, h = BIG_SPAN_FRAME
            return self.new(i, "spans", "pickSpans", changes, True, name, n=w * h, w=w, h=h, frame=True, max_spans=MAX_SPANS[-1], march="short")
        if name == "components_grow":
            # the labelling's growth of `mesh` in the middle of its call, on a handle that has lived, two frames in flight, every array in
            # device form: a counting call past the keep (`mesh` is released at its end); a labelling of one component (`mesh` is now
            # exactly the first cut at GROW_DIMS); a small extraction (its emit enqueued, reading `mesh`); a frame (the lanes swap); a
            # checkerboard at GROW_DIMS, every point a component: the first cut fits what is there, so the host does not wait for the
            # emit's event, then the call grows `mesh`, copies and frees the old buffer; a smaller extraction (reuses the grown one)
            self.change("fif", 2, changes)
            if k == 0:
                lat = lattice(scene, rng, dims=BIG_COMPONENTS, cell=0.02)
                return self.new(i, "components", "labelComponents", changes, False, name, lattice=lat, labels=False, capacity="none")
            if k == 1:
                return self.new(i, "components", "labelLattice", changes, False, name, dims=GROW_DIMS, kind="all_outside", labels=True, capacity="exact")
            if k == 3:
                w, h = rng.choice(FRAME_SIZES[3:])
                return self.new(i, "render", "render", changes, False, name, w=w, h=h, fmt=hs.RGBA32F, stats=True, defer=True)
            if k == 4:
                return self.new(i, "components", "labelLattice", changes, False, name, dims=GROW_DIMS, kind="checkerboard", labels=True, capacity="exact", alone=True)
            lat = lattice(scene, rng, dims={2: (11, 9, 10), 5: (7, 8, 6)}[k])
            return self.new(i, "mesh", "extractMesh", changes, False, name, lattice=lat, normals=True, form=None, defer=k == 2)
        assert name == "scene_change"
        # device work enqueued, then a scene change with no sync of the test's own: the answers are those of the scene of the call.  To
        # the run-time scene, STRETCH free steps on it, and from it again
        if k == 0:
            self.settings("rays", changes)
            if st["scene"] == hs.RUNTIME_SCENE:
                self.builtin(changes)
            return self.new(i, "rays", "queryRays", changes, False, name, n=1000, defer=True)
        if k == 1:
            self.load(hs.RUNTIME_SCENE, changes)
            return self.new(i, "mesh", "extractMesh", changes, False, name, lattice=lattice(hs.RUNTIME_SCENE, rng), normals=True, form=None, defer=True)
        if k < 2 + STRETCH:
            family = self.pick_family(i)
            self.settings(family, changes)
            return self.free_step(i, family, changes)
        if k == 2 + STRETCH:
            if self.slot % 2:  # every other seed: a span kernel of the run-time scene's module is in flight when the scene goes
                return self.new(i, "spans", "querySpans", changes, False, name, n=255, w=1, h=1, frame=False, max_spans=3, march="finish", defer=True)
            return self.new(i, "surfaces", "queryRaySurfaces", changes, False, name, n=255, w=1, h=1, frame=False, hits=True, defer=True)
        self.builtin(changes)
        return self.new(i, "points", "queryDistance", changes, True, name, n=64, normals=True)

    def step(self, i):
        for at, name in self.block_at.items():
            if at <= i < at + BLOCK_STEPS[name]:
                return self.block(i, name)
        changes = {}
        self.place(changes)
        family = self.pick_family(i)
        self.settings(family, changes)
        if family == "post" and self.last_frame is None:
            family = "render"
        return self.free_step(i, family, changes)


def sequence(seed, n=None, slot=None):
    """The steps of `seed`: a list of dicts (see the module's doc string).  Deterministic per seed.  slot: which share of the coverage
    the seed works towards first (default: its place among the committed seeds)."""
    n = STEPS if n is None else n
    g = _Gen(seed, n, slot)
    for i in range(n):
        g.step(i)
    return g.steps


# ---- what a sequence covers (tests/test_handle_mixed_cpu.py) ----------------------------------------------------------------------
def transitions(steps):
    return {(a["family"], b["family"]) for a, b in zip(steps, steps[1:])}


def has_form(s):
    """whether on_host decides where an array of the step lives: a measure's `columns` (without them it answers into its host record
    alone), a labelling's lattice, records or labels (the counting call of the scene's own distances without labels has none)"""
    if s["family"] == "measure":
        return bool(s.get("columns"))
    if s["family"] == "components":
        return s["call"] == "labelLattice" or s["labels"] or s["capacity"] != "none"
    return True


def forms(steps):
    """{(family, host, frames in flight)} of the steps with an array whose place on_host decides (has_form)"""
    return {(s["family"], s["host"], s["state"]["fif"]) for s in steps if s["family"] != "failed" and has_form(s)}


def on_runtime_scene(steps):
    return {s["family"] for s in steps if s["state"]["scene"] == hs.RUNTIME_SCENE}


def with_debug(steps):
    return {s["family"] for s in steps if s["state"]["debug"]}


def blocks(steps):
    """{name: [steps]} of the scripted blocks"""
    out = {}
    for s in steps:
        if s["block"]:
            out.setdefault(s["block"], []).append(s)
    return out


def failure_kinds(steps):
    return {s["fail"] for s in steps if s["family"] == "failed"}


def oracle_checkable(s):
    """whether the GPU tier can hold a step's reference answer against the CPU oracle: a built-in scene (the oracle has no run-time
    scene; a labelling of the caller's lattice needs none), and no counting call over a lattice of millions of points, which numpy
    would take too long for; and a step whose answers are read at once (the GPU tier checks a step when it reads it, and reads the
    deferred ones of a block together)"""
    large = s["call"] == "countMesh" or (s["block"] == "large_new" and s["call"] in ("surveyMesh", "countSlices")) or \
        (s["block"] == "components_grow" and s["call"] == "labelComponents")
    return s["family"] != "failed" and (s["state"]["scene"] != hs.RUNTIME_SCENE or s["call"] == "labelLattice") and not large and not s.get("defer")


def runtime_entries(steps):
    return sum(1 for s in steps if s["set"].get("scene") == hs.RUNTIME_SCENE)

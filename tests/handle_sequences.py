"""Seeded sequences of calls on ONE renderer handle, for the tests of what a handle carries from frame to frame: its
workspace (grown on demand, per lane with two frames in flight), the tile cursors and the row order a persistent launch
learned, the two lanes of sdfr_set_frames_in_flight(2), the host staging buffers, the strip split, the schedule, the launch
mode, step shortcuts, limits, variables and a scene compiled at run time.

No torch, no GPU: the CPU tier (tests/test_handle_sequences_cpu.py) checks what the committed seeds cover, the GPU tier
(tests/test_gpu_handle_state.py) runs them.  A step is one call on the handle, with the settings changed just before it
(`set`) and the whole state it is rendered in (`state`), which is what a fresh handle needs to render its reference."""
import math
import random

# what a step is, for the coverage of transitions: a failed call, then a frame of the scene compiled at run time, then one of
# the wavefront schedule, then the call itself
CATEGORIES = ("device", "host", "strips", "private", "wavefront", "runtime", "failed")

BUILTIN_SCENES = ("labyrinth", "cube_sea", "fractal", "lense", "gems", "light_shadows")
RUNTIME_SCENE = "noise_lod"  # sdf_playground_amd/scenes/noise_lod.hlsl, through initShaderHlsl
MAX_RUNTIME_ENTRIES = 2      # each switch to the run-time scene compiles it again: a few seconds

SMALL_SIZES = ((1, 1), (7, 5), (65, 9), (96, 64), (160, 90), (240, 160), (333, 77), (320, 180), (640, 360))
LARGE_SIZES = ((1280, 720), (1920, 1080))
MAX_LARGE_STEPS = 4

# sdfr_limits of a new handle (frame_defaults, the reference's pshader_sdf.hlsl values); a limits setting is applied in full
DEFAULT_LIMITS = dict(iter_count=100, bounce_count=16, ray_count=8, light_count=8, range=100.0, max_cost_default=7, extension_lights=0,
                      extension_marble_reflection=0.0, dist_eps=0.0001, grad_eps=0.0001, reflect_eps=0.001, refract_eps=0.001, shadow_eps=0.0003)
# the limits of the BASELINE configurations (bench.CONFIGS; tests/test_handle_sequences_cpu.py keeps the two equal) and more lights
LIMITS = {
    "default": {},
    "2": dict(iter_count=128, max_cost_default=6),
    "3": dict(iter_count=256),
    "3r": dict(iter_count=256, extension_marble_reflection=0.25),
    "4": dict(iter_count=512),
    "5": dict(iter_count=100, max_cost_default=9, extension_lights=7),
    "lights3": dict(extension_lights=3),
}

# scene variables (VAR_ tags) and their ranges; the other built-in scenes have none
SCENE_VARS = {
    "lense": {"mixing": (0.0, 1.0), "xpos": (-4.0, 4.0), "ypos": (-4.0, 4.0), "zpos": (0.0, 25.0)},
    "noise_lod": {"lod": (0.0, 40.0), "freq": (0.5, 8.0), "bump": (0.0, 0.05)},
}

SCHEDULES = ("pixel", "wavefront")
LAUNCH_MODES = ("auto", "per_tile", "persistent")
SCHEDULE = {"wavefront": 0, "pixel": 1}                  # the library's values of the names above
LAUNCH = {"auto": 0, "per_tile": 1, "persistent": 2}
NAN32 = 0x7FC0DEAD  # what a GPU test fills its buffers with: a quiet NaN with a payload no render produces
NAN16 = 0x7E5A
WORLDS = (2, 3, 8)
SPLITS = ((1, 2), (1, 3), (2, 5), (3, 4), (1, 8))
RGBA32F, RGBA16F, STRIP_RGB32F_A8, STRIP_RGB16F_A8 = 0, 1, 2, 3
FAILURES = ("format", "huge")  # a bad format; a frame of more than 2^30 pixels (through the raw sdfr_render)
HUGE_SIZE = (32768, 32769)
MAX_FAILED = 5

SEEDS = (1, 45, 60)  # the committed seeds (what they cover: tests/test_handle_sequences_cpu.py)
STEPS = 56


def limits(name):
    """the full limits of the setting `name`"""
    return dict(DEFAULT_LIMITS, **LIMITS[name])


def camera(scene, t):
    """(kind, eye, target) of the orbit of `scene` at angle t: 'dir' = eye + direction, 'lookat' = eye + point."""
    c, s = math.cos(t), math.sin(t)
    if scene == "labyrinth":
        return ("dir", (1.5 * c, 5.0, 1.5 * s), (c, -0.35, s))
    if scene == "cube_sea":
        return ("dir", (3 * c, 4.5, 3 * s), (math.cos(t + 0.6), -0.45, math.sin(t + 0.6)))
    if scene == "fractal":
        return ("lookat", (2.2 * c, 1.6, 2.2 * s), (0.0, 1.0, 0.0))
    if scene == "lense":
        return ("lookat", (7 * s, 0.5, 7 * c), (0.0, 0.0, 0.0))
    if scene == "gems":
        return ("lookat", (2.5 * c, 2.0, 2.5 * s), (0.0, 1.0, 0.0))
    if scene == "light_shadows":
        return ("lookat", (9 * s, 5.0, -9 * c), (0.0, 1.0, 0.0))
    if scene == RUNTIME_SCENE:
        return ("lookat", (5 * s, 2.0, -5 * c), (0.0, 1.0, 0.0))
    raise KeyError(scene)


def category(step):
    if step["call"] == "failed":
        return "failed"
    if step["state"]["scene"] == RUNTIME_SCENE:
        return "runtime"
    if step["state"]["schedule"] == "wavefront":
        return "wavefront"
    return step["call"]


def pixels(step):
    return step["w"] * step["h"]


class _Gen:
    def __init__(self, seed, n):
        self.rng = random.Random(seed)
        self.n = n
        self.state = dict(scene=None, limits="default", vars={}, t=0.0, stime=0.0, schedule="pixel", launch="auto", shortcuts=False, fif=1,
                          split=(0, 1))
        self.steps = []
        self.covered = set()
        self.runtime_entries = 0
        self.failed = 0
        self.doubled = False
        self.large = 0
        self.size = (160, 90)
        rng = self.rng
        # the scripted block, in the middle: [a workspace growth with two frames in flight, a frame into the same pixel_stats
        # buffer, a failed call, a shrink back]; before it every frame is small, so that the growth is one
        self.block = rng.randrange(int(n * 0.35), int(n * 0.55))

    def change(self, key, value, changes):
        if self.state[key] != value:
            self.state[key] = value
            changes[key] = value

    def pick_category(self, i):
        rng = self.rng
        prev = category(self.steps[-1]) if self.steps else None
        allowed = ["device", "host", "strips", "private", "wavefront"]
        if self.state["scene"] == RUNTIME_SCENE or self.runtime_entries < MAX_RUNTIME_ENTRIES:
            allowed.append("runtime")
        fail_ok = 0 < i < self.n - 1 and self.failed < MAX_FAILED and i not in (self.block - 1, self.block + 1)
        if prev == "failed":
            fail_ok = fail_ok and not self.doubled and (len(self.steps) < 2 or category(self.steps[-2]) != "failed")
        elif any(category(s) == "failed" for s in self.steps[-3:]):
            fail_ok = False
        if fail_ok:
            allowed.append("failed")
        fresh = [c for c in allowed if (prev, c) not in self.covered]
        if "failed" in fresh and rng.random() < 0.35:
            return "failed"
        fresh = [c for c in fresh if c != "failed"]
        if fresh and rng.random() < 0.8:
            return rng.choice(fresh)
        return rng.choice([c for c in allowed if c != "failed"])

    def settings(self, cat, changes):
        """the settings a step of category `cat` needs, and the others drawn at random"""
        rng, st = self.rng, self.state
        scene = st["scene"]
        if cat == "runtime":
            scene = RUNTIME_SCENE
        elif cat != "failed" and (scene is None or scene == RUNTIME_SCENE or rng.random() < 0.15):
            scene = rng.choice([s for s in BUILTIN_SCENES if s != scene])
        if scene != st["scene"]:
            if scene == RUNTIME_SCENE:
                self.runtime_entries += 1
            st["vars"] = {}  # loading a scene resets its variables
            changes["scene"] = scene
            st["scene"] = scene
            changes["t"] = st["t"] = round(rng.uniform(0, 2 * math.pi), 4)  # every scene has its own orbit
        if cat == "wavefront":
            self.change("schedule", "wavefront", changes)
        elif cat in ("device", "host", "strips", "private"):
            self.change("schedule", "pixel", changes)
        elif rng.random() < 0.2:
            self.change("schedule", rng.choice(SCHEDULES), changes)
        if rng.random() < 0.25:
            self.change("launch", rng.choice(LAUNCH_MODES), changes)
        if rng.random() < 0.2:
            self.change("shortcuts", not st["shortcuts"], changes)
        if rng.random() < 0.15:
            self.change("limits", rng.choice(sorted(LIMITS)), changes)
        if scene in SCENE_VARS and rng.random() < 0.3:
            name = rng.choice(sorted(SCENE_VARS[scene]))
            lo, hi = SCENE_VARS[scene][name]
            v = round(rng.uniform(lo, hi), 3)
            st["vars"] = dict(st["vars"], **{name: v})
            changes["var"] = (name, v)
        if rng.random() < 0.6:
            self.change("t", round(rng.uniform(0, 2 * math.pi), 4), changes)
        if rng.random() < 0.3:
            self.change("stime", round(rng.uniform(0, 3), 3), changes)

    def draw_size(self, i):
        rng = self.rng
        if i < self.block or self.large >= MAX_LARGE_STEPS or rng.random() < 0.9:
            return rng.choice(SMALL_SIZES) if rng.random() < 0.6 else self.size
        self.large += 1
        return rng.choice(LARGE_SIZES)

    def step(self, i):
        rng, st = self.rng, self.state
        changes = {}
        scripted = self.block <= i < self.block + 4
        if i == self.block:
            cat = "device"
        elif i == self.block + 1:
            cat = category(self.steps[-1])
        elif i == self.block + 2:
            cat = "failed"
        else:
            cat = self.pick_category(i)
        if i == self.block + 1:
            pass  # the same state as the growth: only the camera moves
        else:
            self.settings(cat, changes)
        if scripted:
            self.change("fif", 2, changes)
        elif i > self.block + 3 and rng.random() < 0.12 or i < self.block and rng.random() < 0.08:
            self.change("fif", 3 - st["fif"], changes)
        if i == self.block + 1:
            self.change("t", round(rng.uniform(0, 2 * math.pi), 4), changes)

        call = {"device": "device", "host": "host", "strips": "strips", "private": "private", "failed": "failed"}.get(cat)
        if call is None:  # wavefront, runtime: any call
            call = rng.choice(("device", "device", "host", "strips", "private"))
        prev = self.steps[-1] if self.steps else None
        s = dict(i=i, call=call, set=changes, fmt=RGBA32F, stats=False, reuse_image=False, reuse_stats=False)
        if call == "failed":
            s["fail"] = rng.choice(FAILURES)
            s["w"], s["h"] = self.size
            self.failed += 1
            if prev is not None and prev["call"] == "failed":
                self.doubled = True
        else:
            if i == self.block:
                w, h = rng.choice(LARGE_SIZES)
                self.large += 1
            elif i == self.block + 1:
                w, h = prev["w"], prev["h"]
            elif i == self.block + 3:
                w, h = rng.choice(SMALL_SIZES[2:])
            else:
                w, h = self.draw_size(i)
            s["w"], s["h"] = w, h
            self.size = (w, h)
            if call == "strips":
                s["world"] = rng.choice(WORLDS)
                s["fmt"] = rng.choice((RGBA32F, RGBA16F, STRIP_RGB32F_A8, STRIP_RGB16F_A8))
            elif call == "private":
                split = rng.choice(SPLITS)
                if st["split"] != split:
                    changes["split"] = st["split"] = split
                s["fmt"] = rng.choice((RGBA32F, RGBA16F))
            else:
                s["fmt"] = rng.choice((RGBA32F, RGBA16F))
                s["stats"] = i in (self.block, self.block + 1) or rng.random() < 0.6
                if call == "device" and prev is not None and prev["call"] == "device" and (prev["w"], prev["h"]) == (w, h):
                    s["reuse_image"] = prev["fmt"] == s["fmt"] and i != self.block + 1 and rng.random() < 0.5
                    s["reuse_stats"] = prev["stats"] and s["stats"] and (i == self.block + 1 or rng.random() < 0.6)
        s["state"] = dict(st, vars=dict(st["vars"]))
        self.steps.append(s)
        if len(self.steps) > 1:
            self.covered.add((category(self.steps[-2]), category(s)))


def sequence(seed, n=STEPS):
    """The steps of `seed`: a list of dicts (see the module's doc string).  Deterministic per seed."""
    g = _Gen(seed, n)
    for i in range(n):
        g.step(i)
    return g.steps


def transitions(steps):
    return {(category(a), category(b)) for a, b in zip(steps, steps[1:])}


def workspace_growths(steps):
    """indices of the frames larger than twice every frame before them on the handle"""
    out, most = [], 0
    for s in steps:
        if s["call"] == "failed":
            continue
        if most and pixels(s) > 2 * most:
            out.append(s["i"])
        most = max(most, pixels(s))
    return out

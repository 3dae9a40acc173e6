"""CPU tier: the GPU tier's scaffold (tests/gpu_util.py) on a stub that records its method calls.  The call sequences written out
below are the ones the families' own copies of _setup made before there was a scaffold: a change to them changes what every GPU
test sends to the library."""
import os
import types

import numpy as np
import pytest

import gpu_util as gu
import query_util as qu

LIMITS = dict(iter_count=100, bounce_count=16, ray_count=8, light_count=8, range=100.0, max_cost_default=7, extension_lights=0,
              extension_marble_reflection=0.0, dist_eps=0.0001, grad_eps=0.0001, reflect_eps=0.001, refract_eps=0.001, shadow_eps=0.0003)
OF = types.SimpleNamespace(stime=0.75, eye=(1.0, 2.0, 3.0), front=(0.0, 0.0, 1.0), right=(1.0, 0.0, 0.0), top=(0.0, 1.0, 0.0), width=64, height=48)


class Recorder:
    """every method call is recorded as (name, args, kwargs); setValue answers `accepts`"""

    def __init__(self, accepts=True):
        self.calls, self.accepts = [], accepts

    def __getattr__(self, name):
        def method(*args, **kwargs):
            self.calls.append((name, args, kwargs))
            return self.accepts if name == "setValue" else None
        return method


def _frame_calls(shortcuts=False, **limits):
    return [("setParameters", (0.75,), {}), ("setCameraBasis", ((1.0, 2.0, 3.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)), {}),
            ("setLimits", (), dict(LIMITS, **limits)), ("setStepShortcuts", (shortcuts,), {})]


def test_the_default_limits_are_the_one_literal():
    import handle_sequences as hs

    assert gu.DEFAULT_LIMITS is hs.DEFAULT_LIMITS and gu.DEFAULT_LIMITS == LIMITS and list(gu.DEFAULT_LIMITS) == list(LIMITS)


def test_setup_of_a_builtin_scene():
    r = Recorder()
    gu.setup(r, "labyrinth", OF)
    assert r.calls == [("initShader", ("labyrinth",), {})] + _frame_calls()


def test_setup_of_a_runtime_scene():
    r = Recorder()
    gu.setup(r, "noise_lod", OF)
    path = os.path.join(qu.ROOT, "sdf_playground_amd", "scenes", "noise_lod.hlsl")
    assert os.path.isfile(path)
    assert r.calls == [("initShaderHlsl", ("noise_lod", path), {})] + _frame_calls()


def test_setup_with_limits_variables_and_shortcuts():
    r = Recorder()
    gu.setup(r, "lense", OF, variables={"xpos": 0.7, "mixing": 0.35}, limits=dict(light_count=1, extension_marble_reflection=0.25), shortcuts=True)
    assert r.calls == [("initShader", ("lense",), {})] + _frame_calls(True, light_count=1, extension_marble_reflection=0.25) + [
        ("setValue", ("xpos", 0.7), {}), ("setValue", ("mixing", 0.35), {})]
    assert gu.DEFAULT_LIMITS == LIMITS  # (the caller's limits did not leak into the defaults)


def test_setup_without_loading():
    r = Recorder()
    gu.setup(r, None, OF, load=False)
    assert r.calls == _frame_calls()


def test_setup_raises_when_a_variable_is_refused():
    r = Recorder(accepts=False)
    with pytest.raises(AssertionError):
        gu.setup(r, "lense", OF, variables={"no_such_variable": 1.0})
    assert r.calls[-1] == ("setValue", ("no_such_variable", 1.0), {})


def test_load_takes_the_scene_kind_from_its_name():
    r = Recorder()
    gu.load(r, "dialect_tour")
    gu.load(r, "cube_sea")
    assert [c[0] for c in r.calls] == ["initShaderHlsl", "initShader"] and r.calls[1] == ("initShader", ("cube_sea",), {})


class Frames:
    """a handle whose renders, stats and timings repeat -- but for what `fault` names"""

    def __init__(self, fault=None):
        self.fault, self.renders, self.inside = fault, 0, False
        self.queries = 0

    def render(self, cam, w, h, pixel_stats=False):
        assert cam is None and pixel_stats is True
        self.renders += 1
        img = np.linspace(0.0, 1.0, w * h * 4, dtype=np.float32).reshape(h, w, 4)
        st = np.arange(w * h * 3, dtype=np.int32).reshape(h, w, 3)
        if self.renders == 2 and self.fault == "image":
            img.view(np.uint32)[h - 1, w - 1, 3] ^= 1  # one bit
        if self.renders == 2 and self.fault == "pixel_stats":
            st[0, 0, 1] += 1
        return img, st

    def query(self):
        self.queries += 1

    def getStats(self):
        moved = self.fault == "stats" and self.queries > 0
        return types.SimpleNamespace(pixels=12, rays=30, march_evals=400 + moved, hits=7, march_launches=1, shade_launches=2)

    def getTimings(self):
        return (0.25, 0.5 + (self.fault == "timings" and self.queries > 0))


def test_rendering_untouched_passes_when_everything_repeats():
    r = Frames()
    with gu.rendering_untouched(r, 6, 4) as (img0, s0):
        r.query()
        assert img0.shape == (4, 6, 4) and s0 == (12, 30, 400, 7, 1, 2) and r.renders == 1
    assert r.renders == 2


@pytest.mark.parametrize("fault", ["stats", "timings", "image", "pixel_stats"])
def test_rendering_untouched_raises(fault):
    r = Frames(fault)
    with pytest.raises(AssertionError):
        with gu.rendering_untouched(r, 6, 4):
            r.query()
    assert r.renders == (1 if fault in ("stats", "timings") else 2)


def test_with_size_restores_the_size_when_the_body_raises():
    of = types.SimpleNamespace(width=64, height=48)
    with gu.with_size(of, 9, 7) as f:
        assert f is of and (of.width, of.height) == (9, 7)
    assert (of.width, of.height) == (64, 48)
    with pytest.raises(KeyError):
        with gu.with_size(of, 9, 7):
            raise KeyError("body")
    assert (of.width, of.height) == (64, 48)


def test_stats_and_to_host_on_numpy():
    assert gu.stats(Frames()) == (12, 30, 400, 7, 1, 2)
    a = np.arange(3)
    assert gu.to_host(a, sync=False) is a and gu.to_host((a, a), sync=False) == (a, a)

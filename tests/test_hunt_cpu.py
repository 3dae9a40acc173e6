"""CPU tier: the shortcut-heavy parity hunt of the GPU tier (tests/test_gpu_fuzz.py), case for case, on the host build of the product's
per-pixel pipeline (tests/hostsim) against the oracle: step shortcuts on, eight lights in half of the cases, any ray budget and queue
length, dist_eps at its largest in 40 % of the cases, cameras between, above and below the lense's blob fields, the light ball anywhere.
Pixels, rays and hits bit for bit; the step counters never above the oracle's.  1 500 lense cases, so that an escape rule that is wrong
for one ray in a few hundred cases (the direction towards a directional light is |L| / (|L| + dist_eps) long, not 1) fails here on every
run without a GPU."""
import os
import sys

import numpy as np
import pytest

from shortcut_scenes import HUNT_OPTIONS, HUNT_SIZE, LENSE_HUNT_CASES, LENSE_HUNT_SEEDS, RULE_HUNT_CASES, RULE_HUNT_SCENES, RULE_HUNT_SEED

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def _hunt(oracle, cases, seed, scenes):
    import fuzz_parity
    import hostsim

    n, bad, saved = 0, [], 0
    for scene, c, case in fuzz_parity.draw_cases(cases, seed, HUNT_SIZE, scenes, **HUNT_OPTIONS):
        assert case["shortcuts"]
        ref, rst, _ = oracle.render(scene, case["f"], stats=True)
        hf = hostsim.frame_from_oracle(case["f"])
        hf.step_shortcuts = 1
        img, st = hostsim.render(scene, hf)
        n += 1
        if not fuzz_parity.same_as_oracle(img, st, ref, rst, True):
            bad.append((scene, c, case["eye"], case["tgt"], case["stime"], case["limits"], case["values"],
                        int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=2).sum())))
        saved += int(rst[..., 1].sum(dtype=np.int64) - st[..., 1].sum(dtype=np.int64)) > 0
    return n, bad, saved


@pytest.mark.parametrize("seed", LENSE_HUNT_SEEDS)
def test_lense_hunt_on_the_host(oracle, seed):
    n, bad, saved = _hunt(oracle, LENSE_HUNT_CASES, seed, ["lense"])
    assert n == LENSE_HUNT_CASES
    assert not bad, (len(bad), bad[:3])
    assert saved > n // 2  # escapes_from spoke in most cases: the hunt puts the rule to work


def test_rule_scenes_hunt_on_the_host(oracle):
    n, bad, saved = _hunt(oracle, RULE_HUNT_CASES, RULE_HUNT_SEED, list(RULE_HUNT_SCENES))
    assert n == RULE_HUNT_CASES * len(RULE_HUNT_SCENES)
    assert not bad, (len(bad), bad[:3])
    assert saved > n // 3

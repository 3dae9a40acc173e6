"""GPU tier: a short, seeded run of the randomised parity hunt (tools/fuzz_parity.py): random
cameras (also far away, grazing the floor), times, variable values, limits and schedules for all
22 scenes against the oracle, bit for bit.  The long runs (190 000 cases in round 1, no mismatch) are
recorded in profiles/README.md."""
import os
import sys

import pytest

from shortcut_scenes import HUNT_OPTIONS, HUNT_SIZE, LENSE_HUNT_CASES, LENSE_HUNT_SEEDS, RULE_HUNT_CASES, RULE_HUNT_SCENES, RULE_HUNT_SEED

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_randomised_parity_all_scenes():
    import fuzz_parity

    n, bad = fuzz_parity.run(cases=8, seed=7, size=(64, 48))
    assert n == 8 * 22
    assert not bad, bad[:3]


def test_randomised_parity_with_step_shortcuts_and_any_ray_budget():
    """the same hunt on the pixel schedule with step shortcuts on, eight lights in half of the cases and any ray budget (1-16) and
    queue length (1-8): what the escape rules and the shadow rays delivered from the light loop have to respect"""
    import fuzz_parity

    scenes = ["gems", "lense", "fast_sphere", "fractal", "neon", "basic_transparency", "terrain", "light_shadows"]
    n, bad = fuzz_parity.run(cases=40, seed=11, size=(64, 48), scenes=scenes, shortcut_heavy=True)
    assert n == 40 * len(scenes)
    assert not bad, bad[:3]


@pytest.mark.parametrize("seed", LENSE_HUNT_SEEDS)
def test_lense_hunt_with_step_shortcuts(seed):
    """lense's escapes_from against the oracle, sized to the hunt that found its last bug: 1 500 cases over three seeds, dist_eps at its
    largest in 40 % of them, cameras between, above and below the blob fields, the light ball anywhere (the CPU tier runs the same
    cases on the host build: tests/test_hunt_cpu.py)"""
    import fuzz_parity

    n, bad = fuzz_parity.run(cases=LENSE_HUNT_CASES, seed=seed, size=HUNT_SIZE, scenes=["lense"], **HUNT_OPTIONS)
    assert n == LENSE_HUNT_CASES
    assert not bad, (len(bad), bad[:3])


def test_rule_scenes_hunt_with_step_shortcuts():
    """the same hunt for the bench's other scenes with an escape rule, 300 cases each"""
    import fuzz_parity

    n, bad = fuzz_parity.run(cases=RULE_HUNT_CASES, seed=RULE_HUNT_SEED, size=HUNT_SIZE, scenes=list(RULE_HUNT_SCENES), **HUNT_OPTIONS)
    assert n == RULE_HUNT_CASES * len(RULE_HUNT_SCENES)
    assert not bad, (len(bad), bad[:3])

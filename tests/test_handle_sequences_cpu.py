"""CPU tier: the seeded call sequences of tests/handle_sequences.py, which tests/test_gpu_handle_state.py runs on one handle,
are reproducible and cover what they are there to cover -- checked here, not left to the luck of the seeds."""
import itertools

import handle_sequences as hs


def test_sequences_are_deterministic_per_seed():
    for seed in hs.SEEDS:
        assert hs.sequence(seed) == hs.sequence(seed)
    assert hs.sequence(hs.SEEDS[0]) != hs.sequence(hs.SEEDS[1])


def test_committed_seeds_cover_every_transition():
    """every ordered pair of {full device, full host, strips, private, wavefront, run-time scene, failed call}"""
    seen = set()
    for seed in hs.SEEDS:
        seen |= hs.transitions(hs.sequence(seed))
    missing = sorted(set(itertools.product(hs.CATEGORIES, repeat=2)) - seen)
    assert not missing, missing


def test_each_seed_carries_the_hazards_with_two_frames_in_flight():
    for seed in hs.SEEDS:
        steps = hs.sequence(seed)
        fif2 = [s for s in steps if s["state"]["fif"] == 2]
        assert [i for i in hs.workspace_growths(steps) if steps[i]["state"]["fif"] == 2], seed
        assert any(s["call"] == "failed" for s in fif2), seed
        assert any(s["reuse_stats"] for s in fif2), seed
        # and one shrink back after a growth
        growth = hs.workspace_growths(steps)[0]
        assert any(s["call"] != "failed" and hs.pixels(s) < hs.pixels(steps[growth]) for s in steps[growth + 1:]), seed


def test_sequences_keep_their_rules():
    for seed in hs.SEEDS:
        steps = hs.sequence(seed)
        assert len(steps) == hs.STEPS
        # a failed call (or two) always sits between two valid frames
        assert steps[0]["call"] != "failed" and steps[-1]["call"] != "failed"
        for a, b, c in zip(steps, steps[1:], steps[2:]):
            assert not (a["call"] == b["call"] == c["call"] == "failed"), seed
        # switching to the run-time scene compiles it: a bounded number of times
        entries = sum(1 for a, b in zip([None] + steps, steps) if b["state"]["scene"] == hs.RUNTIME_SCENE and
                      (a is None or a["state"]["scene"] != hs.RUNTIME_SCENE))
        assert entries <= hs.MAX_RUNTIME_ENTRIES, seed
        for s in steps:
            st = s["state"]
            assert st["scene"] in hs.BUILTIN_SCENES + (hs.RUNTIME_SCENE,)
            assert set(st["vars"]) <= set(hs.SCENE_VARS.get(st["scene"], {}))
            if s["call"] == "failed":
                continue
            assert (s["w"], s["h"]) in hs.SMALL_SIZES + hs.LARGE_SIZES
            assert s["fmt"] in ((0, 1, 2, 3) if s["call"] == "strips" else (0, 1))
            if s["call"] == "private":
                assert st["split"][0] > 0
        assert sum(1 for s in steps if s["call"] != "failed" and (s["w"], s["h"]) in hs.LARGE_SIZES) <= hs.MAX_LARGE_STEPS + 1


def test_limits_are_the_benchmark_s():
    import bench

    for key in ("2", "3", "3r", "4", "5"):
        assert hs.LIMITS[key] == bench.CONFIGS[key]["limits"], key
    assert bench.CONFIGS["5g"]["limits"] == hs.LIMITS["5"]

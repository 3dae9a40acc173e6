"""CPU tier of the mixed handle sequences (tests/handle_mixed_sequences.py): the committed seeds cover what they are there to cover.
The GPU tier (tests/test_gpu_handle_mixed.py) runs them."""
import handle_mixed_sequences as hm
import handle_sequences as hs

SEQUENCES = {seed: hm.sequence(seed) for seed in hm.SEEDS}
ALL = [s for steps in SEQUENCES.values() for s in steps]
SEQUENCES_OF = {id(s): steps for steps in SEQUENCES.values() for s in steps}


def _plain(x):
    """a step as comparable data"""
    return repr(x)


def test_deterministic_per_seed_and_seeds_differ():
    for seed, steps in SEQUENCES.items():
        assert len(steps) == hm.STEPS and [s["i"] for s in steps] == list(range(hm.STEPS))
        assert _plain(steps) == _plain(hm.sequence(seed)), seed
        for s in steps[:8]:
            assert hm.rays(dict(s, n=5)) == hm.rays(dict(s, n=5)) and hm.points(dict(s, n=5)) == hm.points(dict(s, n=5))
    texts = [_plain(steps) for steps in SEQUENCES.values()]
    assert len(set(texts)) == len(texts)
    assert len({tuple(s["family"] for s in steps) for steps in SEQUENCES.values()}) == len(texts)


def test_every_ordered_pair_of_families_is_a_pair_of_consecutive_steps():
    """all 12 x 12 but (failed, failed): a failed call always sits between two valid calls"""
    assert len(hm.FAMILIES) == 12 and len(hm.PAIRS) == 143
    seen = set().union(*(hm.transitions(steps) for steps in SEQUENCES.values()))
    assert not set(hm.PAIRS) - seen, sorted(set(hm.PAIRS) - seen)


def test_every_family_in_host_and_device_form_with_one_and_two_frames_in_flight():
    """(postprocess takes device tensors only: it has no host form)"""
    seen = set().union(*(hm.forms(steps) for steps in SEQUENCES.values()))
    want = {(f, host, fif) for f in hm.HOST_AND_DEVICE for host in (False, True) for fif in (1, 2)} | {("post", False, 1), ("post", False, 2)}
    assert not want - seen, sorted(want - seen)
    assert all(s["family"] in hm.FAMILIES for s in ALL)


def test_every_call_and_variant_of_the_families_occurs():
    calls = {s["call"] for s in ALL}
    assert calls >= {"render", "renderAA", "postprocess", "queryDistance", "queryRays", "pick", "queryRaySurfaces", "pickSurfaces", "meshSurfaces",
                     "queryOcclusion", "hitOcclusion", "queryRayLighting", "pickLighting", "meshLighting", "extractMesh", "countMesh", "atlasTexels",
                     "bakeAtlas", "renderPrivateStrips", "failed"}
    for call in ("pickSurfaces", "pickLighting"):
        assert {bool(s.get("frame")) for s in ALL if s["call"] == call} == {False, True}, call  # a pixel list, and None = the whole frame
    for call, key in (("render", "stats"), ("renderAA", "stats"), ("queryDistance", "normals"), ("queryRaySurfaces", "hits"), ("pickLighting", "hits"),
                      ("pickLighting", "lights"), ("extractMesh", "normals")):
        assert {bool(s[key]) for s in ALL if s["call"] == call} == {False, True}, (call, key)
    assert {s["fmt"] for s in ALL if s["call"] == "render"} == {hs.RGBA32F, hs.RGBA16F}
    assert {s["factor"] for s in ALL if s["call"] == "renderAA"} == set(hm.AA_FACTORS)
    assert {s["form"] for s in ALL if s["call"] == "extractMesh"} == set(hm.MESH_FORMS)
    assert {s["src"] is None for s in ALL if s["call"] == "hitOcclusion"} == {False, True}
    assert {s["src"] is None for s in ALL if s["family"] == "atlas"} == {False, True}
    assert len({s["layers"] for s in ALL if s["call"] == "bakeAtlas"}) >= 5
    assert {s["tile"] for s in ALL if s["family"] == "atlas"} == set(hm.TILES)
    assert {s["n"] for s in ALL if s["block"] is None and s["call"] in ("queryDistance", "queryRays", "pick")} == set(hm.ITEMS)


def test_every_family_on_the_run_time_scene_and_with_the_debug_plane():
    assert set().union(*(hm.on_runtime_scene(steps) for steps in SEQUENCES.values())) == set(hm.FAMILIES)
    assert set().union(*(hm.with_debug(steps) for steps in SEQUENCES.values())) == set(hm.FAMILIES)
    for steps in SEQUENCES.values():
        assert hm.runtime_entries(steps) <= hs.MAX_RUNTIME_ENTRIES
        # one handle alternates between the DBG and the non-DBG kernels
        flips = sum(1 for a, b in zip(steps, steps[1:]) if a["state"]["debug"] != b["state"]["debug"])
        assert flips >= 4


def test_each_seed_has_the_five_scripted_blocks():
    for seed, steps in SEQUENCES.items():
        b = hm.blocks(steps)
        assert sorted(b) == ["aa_in_flight", "lanes", "large_mesh", "scene_change", "staging"] == sorted(hm.BLOCKS), seed
        for name, part in b.items():
            if name == "scene_change":  # its scripted steps are the first two and the last two, free steps on the run-time scene between them
                first, end = part[0]["i"], part[0]["i"] + hm.BLOCK_STEPS[name]
                assert [s["i"] for s in part] == [first, first + 1, end - 2, end - 1], (seed, name)
                assert all(s["state"]["scene"] == hs.RUNTIME_SCENE and s["block"] is None for s in steps[first + 2:end - 2]), seed
            else:
                assert [s["i"] for s in part] == list(range(part[0]["i"], part[0]["i"] + hm.BLOCK_STEPS[name])), (seed, name)

        # 1: a host query past the keep, then the three ways `query` is cut, each small and on the host
        big, bake, mesh, rays = b["staging"]
        assert (big["call"], big["frame"], big["hits"], big["lights"], big["host"]) == ("pickLighting", True, True, True, True)
        assert hm.staging_bytes(big) > hm.KEEP
        w, h = hm.BIG_FRAME
        assert hm.staging_bytes(big) == w * h * (48 + 64 + 640) == 69304320  # (every piece a multiple of 256 bytes already)
        assert hm.staging_bytes(dict(big, n=(w - 8) * h)) <= hm.KEEP or hm.staging_bytes(dict(big, n=w * (h - 8))) <= hm.KEEP  # no smaller frame of whole tiles
        assert [s["call"] for s in (bake, mesh, rays)] == ["bakeAtlas", "extractMesh", "queryRays"] and all(s["host"] for s in (bake, mesh, rays))
        assert hm.staging_bytes(rays) < 1 << 20

        # 2: two frames in flight; the second extraction grows the workspace, the third reuses it
        m1, frame, m2, m3 = b["lanes"]
        assert [s["call"] for s in (m1, frame, m2, m3)] == ["extractMesh", "render", "extractMesh", "extractMesh"]
        assert all(s["state"]["fif"] == 2 and not s["host"] for s in (m1, frame, m2, m3))
        w1, w2, w3 = (hm.workspace_bytes(s["lattice"]["dims"]) for s in (m1, m2, m3))
        assert w1 < w2 and w3 < w2 and w2 <= hm.KEEP
        assert m1["lattice"]["dims"] != m2["lattice"]["dims"] != m3["lattice"]["dims"]
        assert [bool(s.get("defer")) for s in (m1, frame, m2, m3)] == [True, True, True, False]  # read after one sync

        # 3: a workspace past the keep (the counting call reserves and releases it), then a small extraction
        count, small = b["large_mesh"]
        assert count["call"] == "countMesh" and hm.workspace_bytes(count["lattice"]["dims"]) > hm.KEEP
        n = count["lattice"]["dims"][0]
        assert hm.workspace_bytes((n - 1,) * 3) <= hm.KEEP
        assert small["call"] == "extractMesh" and hm.workspace_bytes(small["lattice"]["dims"]) < 1 << 20

        # 4: a strip split left set across an anti-aliased frame between plain frames in flight
        p0, a1, aa, b2, a3, p1 = b["aa_in_flight"]
        assert [s["call"] for s in (p0, a1, aa, b2, a3, p1)] == ["renderPrivateStrips", "render", "renderAA", "render", "render", "renderPrivateStrips"]
        assert [s.get("image") for s in (a1, aa, b2, a3)] == ["A", "B", "B", "A"]
        assert all(s["state"]["fif"] == 2 and not s["host"] for s in (p0, a1, aa, b2, a3, p1))
        split = p0["state"]["split"]
        assert split[0] > 0 and all(s["state"]["split"] == split for s in (a1, aa, b2, a3, p1)) and "split" not in p1["set"]
        assert len({(s["w"], s["h"]) for s in (p0, a1, aa, b2, a3, p1)}) == 1 and len(hs_private_rows(p0["h"], split)) > 0
        assert [bool(s.get("defer")) for s in (a1, aa, b2, a3)] == [True, True, True, False]

        # 5: scene changes under enqueued device work, one to and one from the run-time scene
        q, m, s2, last = b["scene_change"]
        assert all(s.get("defer") and not s["host"] for s in (q, m, s2)) and not last.get("defer")
        assert q["state"]["scene"] in hs.BUILTIN_SCENES and m["state"]["scene"] == s2["state"]["scene"] == hs.RUNTIME_SCENE and last["state"]["scene"] in hs.BUILTIN_SCENES
        assert "scene" in m["set"] and "scene" in last["set"] and not steps[m["i"] + 1].get("defer")
        assert m["call"] == "extractMesh" and q["family"] != "mesh" and s2["family"] not in ("mesh", "render")
        assert hm.runtime_entries(steps) == 1  # every entry compiles the scene and its query kernels again: seconds

        assert any(part[0]["state"]["fif"] == 2 for part in b.values())


def hs_private_rows(height, split):
    m, M = split
    return [r for r in range(height) if (r // 8) % M < m]


def test_every_failure_kind_and_each_between_two_valid_calls():
    assert set().union(*(hm.failure_kinds(steps) for steps in SEQUENCES.values())) == set(hm.FAILURE_KINDS)
    assert len(hm.FAILURE_KINDS) == 8
    for steps in SEQUENCES.values():
        for s in steps:
            if s["family"] == "failed":
                i = s["i"]
                assert 0 < i < len(steps) - 1 and steps[i - 1]["family"] != "failed" and steps[i + 1]["family"] != "failed"
                assert not steps[i - 1].get("defer")


def test_sizes_outside_the_scripted_blocks_are_the_smallest_that_cross_the_edges():
    for s in ALL:
        if s["block"]:
            continue
        if "n" in s and not s.get("frame"):
            assert s["n"] in hm.ITEMS or s["call"] == "hitOcclusion", s
        if "w" in s:
            assert (s["w"], s["h"]) in hm.FRAME_SIZES and s["w"] <= 320 and s["h"] <= 180
        if s["call"] == "renderAA":
            assert s["w"] <= 160 and s["h"] <= 90
        if "lattice" in s:
            assert max(s["lattice"]["dims"]) <= hm.MAX_LATTICE
        if "tile" in s:
            assert s["tile"] in (4, 8, 16) and s["width"] <= 256 and s["width"] % max(8, s["tile"]) == 0
    # the edges themselves: a lattice that is no cube, item counts around the 64 items of a block, pixels outside the frame
    assert any(len(set(s["lattice"]["dims"])) == 3 for s in ALL if "lattice" in s)
    for s in ALL:
        if s["call"] in ("pick", "pickSurfaces", "pickLighting") and not s.get("frame"):
            px = hm.pixel_list(s)
            assert len(px) == s["n"] and not (0 <= px[0][0] < s["w"] and 0 <= px[0][1] < s["h"])


def test_every_lattice_meets_the_surface():
    """a lattice feeds an extraction, the vertices of the mesh queries or an atlas: by the oracle's distances every one of the committed
    seeds has vertices and quads, in the state of its step (scene variables and the debug plane included)"""
    import mesh_util as mu
    import query_util as qu

    for s in ALL:
        if "lattice" not in s or s["state"]["scene"] == hs.RUNTIME_SCENE or s["call"] == "countMesh":
            continue
        src = SEQUENCES_OF[id(s)][s["src"]] if s["family"] == "atlas" and s["src"] is not None else s  # an atlas of an earlier step's mesh
        st, lat = src["state"], src["lattice"]
        if st["scene"] == hs.RUNTIME_SCENE:
            continue
        of = qu.frame(st["scene"], st["stime"], 16, 9, dict(st["vars"], **(hm.debug_vars(st["scene"]) if st["debug"] else {})))
        D = qu.oracle_points(st["scene"], of, mu.lattice_points(lat["origin"], lat["cell"], lat["dims"]), normals=False)[0]
        pos, idx = mu.surface_nets(D, lat["origin"], lat["cell"], lat["dims"], 0.0)
        assert len(pos) >= 8 and len(idx) >= 4, (s["i"], s["call"], st["scene"], st["vars"], lat, len(pos), len(idx))


def test_the_interleavings_the_suite_never_ran_before():
    """the four named in the tests' reason for being, each somewhere in the committed seeds"""
    queries = ("points", "rays", "pick", "surfaces", "occlusion", "lighting")
    # a host atlas bake right after the host lighting query that pushed `query` past its keep: the staging block, every seed
    # a device extraction, a frame (the lanes swap), an extraction that reuses `mesh` on the other lane: the lanes block, every seed
    # an anti-aliased frame between two plain frames in flight: the aa_in_flight block, every seed
    # a failed mesh call between a query and a render
    assert any(s["family"] == "failed" and s["fail"].startswith("mesh_") and steps[s["i"] - 1]["family"] in queries and steps[s["i"] + 1]["family"] == "render"
               for steps in SEQUENCES.values() for s in steps)

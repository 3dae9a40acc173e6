"""CPU tier of the mixed handle sequences (tests/handle_mixed_sequences.py): the committed seeds cover what they are there to cover,
the component labelling included -- both calls, every capacity rule and synthetic lattice, and the block in which the labelling grows
the workspace in the middle of its call, whose bytes are followed here by the plan's formulas, themselves held against the library's
plan.  The GPU tier (tests/test_gpu_handle_mixed.py) runs them."""
import numpy as np

import handle_mixed_oracle as ho
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
    """all 17 x 17 but (failed, failed): a failed call always sits between two valid calls"""
    assert len(hm.FAMILIES) == 17 and len(hm.PAIRS) == 288 and len(set(hm.FAMILIES)) == 17
    assert set(hm.FAMILIES) >= {"survey", "slices", "spans", "measure", "components"}
    seen = set().union(*(hm.transitions(steps) for steps in SEQUENCES.values()))
    assert not set(hm.PAIRS) - seen, sorted(set(hm.PAIRS) - seen)


def test_every_family_in_host_and_device_form_with_one_and_two_frames_in_flight():
    """(postprocess takes device tensors only, a survey and a fit answer into a host record: no host form and no device form; a
    measure counts with `columns` alone, a labelling with a lattice of the caller's, records or labels)"""
    seen = set().union(*(hm.forms(steps) for steps in SEQUENCES.values()))
    assert set(hm.HOST_AND_DEVICE) == set(hm.FAMILIES) - {"post", "survey", "failed"}
    want = {(f, host, fif) for f in hm.HOST_AND_DEVICE for host in (False, True) for fif in (1, 2)}
    want |= {(f, False, fif) for f in ("post", "survey") for fif in (1, 2)}
    assert not want - seen, sorted(want - seen)
    assert all(s["columns"] for s in ALL if s["family"] == "measure" and (s["family"], s["host"], s["state"]["fif"]) in hm.forms([s]))
    assert {(s["host"], s["state"]["fif"]) for s in ALL if s["call"] == "measure" and s["columns"]} == {(h, f) for h in (False, True) for f in (1, 2)}
    assert all(s["family"] in hm.FAMILIES for s in ALL)
    assert "components" in hm.HOST_AND_DEVICE
    for s in ALL:
        if s["family"] == "components":
            assert hm.has_form(s) == (s["call"] == "labelLattice" or s["labels"] or s["capacity"] != "none"), s
    for call in hm.COMPONENT_CALLS:  # each of the two entries by itself, wherever its arrays live
        assert {(s["host"], s["state"]["fif"]) for s in ALL if s["call"] == call and hm.has_form(s)} == {(h, f) for h in (False, True) for f in (1, 2)}, call


def test_every_call_and_variant_of_the_families_occurs():
    calls = {s["call"] for s in ALL}
    assert calls >= {"render", "renderAA", "postprocess", "queryDistance", "queryRays", "pick", "queryRaySurfaces", "pickSurfaces", "meshSurfaces",
                     "queryOcclusion", "hitOcclusion", "queryRayLighting", "pickLighting", "meshLighting", "extractMesh", "countMesh", "atlasTexels",
                     "bakeAtlas", "renderPrivateStrips", "failed", "surveyMesh", "fitMesh", "extractSlices", "countSlices", "querySpans", "pickSpans",
                     "meshSpans", "measure", "labelComponents", "labelLattice"}
    for call in ("pickSurfaces", "pickLighting", "pickSpans"):
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
    # the families that came with the survey, the slices, the spans, the measure and the sharp mesh
    free = [s for s in ALL if s["block"] is None]
    assert set(hm.SHARP_FORMS) <= set(hm.MESH_FORMS) and {s["normals"] for s in ALL if s.get("form") == "sharp"} == {False, True}
    assert {round(s["band"] / s["lattice"]["cell"], 1) for s in free if s["call"] == "surveyMesh"} == set(hm.BANDS) == {0.0, 0.5, 2.0}
    assert {s["levels"] for s in ALL if s["call"] == "fitMesh"} == {0, 2, 3} and {s["margin"] for s in ALL if s["call"] == "fitMesh"} == {0, 1}
    assert {s["axis"] for s in free if s["family"] == "slices"} == {"x", "y", "z", "oblique"}
    for s in free:
        if s["family"] == "slices":  # an axis-aligned stack has du and dv along two axes and dw along the third; an oblique one has them turned about dw
            g = s["slices"]
            zeros = [sum(1 for x in g[k] if x == 0.0) for k in ("du", "dv", "dw")]
            assert zeros == ([1, 1, 2] if s["axis"] == "oblique" else [2, 2, 2]), s
            assert abs(sum(a * b for a, b in zip(g["du"], g["dv"]))) < 1e-5 and all(sum(a * b for a, b in zip(g[k], g["dw"])) == 0 for k in ("du", "dv"))
    assert {s["slices"]["layers"] for s in free if s["family"] == "slices"} >= {1, hm.MAX_SLICE_LAYERS}
    for key in ("coords", "layer_vertices", "layer_segments"):
        assert {s[key] for s in ALL if s["call"] == "extractSlices"} == {False, True}, key
    spans = [s for s in free if s["family"] == "spans"]
    assert {(s["call"], bool(s.get("frame"))) for s in spans} == {("querySpans", False), ("pickSpans", False), ("pickSpans", True), ("meshSpans", False)}
    assert {s["max_spans"] for s in spans} == {0, 1, 3, 64} and {s["march"] for s in spans} == {"finish", "short"}
    for march, sets in hm.SPAN_PARAMS.items():
        for min_step, t_max, max_steps in sets.values():  # "finish": every ray reaches t_max within its steps, whatever the distances
            assert (t_max / min_step + 2 <= max_steps) == (march == "finish") and (march == "finish" or max_steps == 32)
    measures = [s for s in free if s["family"] == "measure"]
    assert {s["grid"]["nu"] for s in measures} | {s["grid"]["nv"] for s in measures} == set(hm.MEASURE_COLUMNS) | {hm.MEASURE_BIG} == {1, 7, 8, 9, 24, 72}
    assert any(-(-s["grid"]["nu"] // 8) * -(-s["grid"]["nv"] // 8) > 64 for s in measures)  # more than one run of 64 tiles: the reduction runs a pass
    assert {s["axis"] for s in measures} == {"x", "y", "z", "tilted"} and {s["columns"] for s in measures} == {False, True}
    assert {s["march"] for s in measures} == {"finish", "short"} and all(ms <= 128 for _m, ms in hm.MEASURE_PARAMS.values())
    for s in measures:
        assert sum(1 for x in s["grid"]["dw"] if x != 0.0) == (2 if s["axis"] == "tilted" else 1), s
    # the labelling: both calls, each with and without labels and under all four capacity rules; every synthetic kind
    labellings = [s for s in free if s["family"] == "components"]
    assert set(hm.CAPACITY_RULES) == {"none", "exact", "roomy", "short"} and set(hm.COMPONENT_CALLS) == {"labelComponents", "labelLattice"}
    assert {(s["call"], s["labels"]) for s in labellings} == {(c, l) for c in hm.COMPONENT_CALLS for l in (False, True)}
    assert {(s["call"], s["capacity"]) for s in labellings} == {(c, r) for c in hm.COMPONENT_CALLS for r in hm.CAPACITY_RULES}
    assert {(s["labels"], s["capacity"]) for s in labellings} == {(l, r) for l in (False, True) for r in hm.CAPACITY_RULES}
    assert {s["kind"] for s in labellings if s["call"] == "labelLattice"} == set(hm.SYNTHETIC_KINDS) >= {"noise", "checkerboard", "serpentine", "hollow_box", "zeros"}
    for s in labellings:
        assert ("lattice" in s) == (s["call"] == "labelComponents") and ("dims" in s) == (s["call"] == "labelLattice"), s
        if s["call"] == "labelLattice":
            D, iso = ho.synthetic_lattice(s)
            assert D.shape == tuple(n + 1 for n in reversed(s["dims"])) and D.dtype == np.float32 and iso == 0.0, s


def test_every_seed_has_every_family_where_the_oracle_can_check_it():
    """the GPU tier holds every family's reference answer against the CPU oracle at least once per seed: every seed has a step of
    every family on a built-in scene that is no counting call over millions of points"""
    for seed, steps in SEQUENCES.items():
        seen = {s["family"] for s in steps if hm.oracle_checkable(s)}
        assert seen == set(hm.FAMILIES) - {"failed"}, (seed, sorted(set(hm.FAMILIES) - {"failed"} - seen))


def test_every_family_on_the_run_time_scene_and_with_the_debug_plane():
    assert set().union(*(hm.on_runtime_scene(steps) for steps in SEQUENCES.values())) == set(hm.FAMILIES)
    assert set().union(*(hm.with_debug(steps) for steps in SEQUENCES.values())) == set(hm.FAMILIES)
    for steps in SEQUENCES.values():
        assert hm.runtime_entries(steps) <= hs.MAX_RUNTIME_ENTRIES
        # one handle alternates between the DBG and the non-DBG kernels
        flips = sum(1 for a, b in zip(steps, steps[1:]) if a["state"]["debug"] != b["state"]["debug"])
        assert flips >= 4


def test_each_seed_has_the_eight_scripted_blocks():
    for seed, steps in SEQUENCES.items():
        b = hm.blocks(steps)
        assert sorted(b) == ["aa_in_flight", "components_grow", "lanes", "large_mesh", "large_new", "scene_change", "staging", "workspace_cuts"] == sorted(hm.BLOCKS), seed
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
        assert s2["call"] in ("queryRaySurfaces", "querySpans")
        assert hm.runtime_entries(steps) == 1  # every entry compiles the scene and its query kernels again: seconds

        # 6: `mesh` cut 5, 3, 2, 4 and 5 ways in one run, behind the other lane's enqueued emit work
        sl, frame, me, su, sh, sl2 = b["workspace_cuts"]
        assert [s["call"] for s in (sl, frame, me, su, sh, sl2)] == ["extractSlices", "render", "measure", "surveyMesh", "extractMesh", "extractSlices"]
        assert all(s["state"]["fif"] == 2 and not s["host"] for s in (sl, frame, me, su, sh, sl2))
        assert [bool(s.get("defer")) for s in (sl, frame, me, su, sh, sl2)] == [True, True, False, False, True, False]
        assert me.get("alone") and su.get("alone") and not sl2.get("alone")  # read at once, the deferred answers after the last call's sync
        assert sh["form"] == "sharp" and me["columns"] and me["iso"] == 0.01  # (an iso-surface of its own: the one measure off the scene's surface)
        g = sl["slices"]
        assert g["dims"] == (hm.MAX_LATTICE, hm.MAX_LATTICE) and g["layers"] == hm.MAX_SLICE_LAYERS  # the largest free size
        cuts = [hm.slice_workspace_bytes(g["dims"], g["layers"]), hm.measure_workspace_bytes(me["grid"]["nu"], me["grid"]["nv"]),
                hm.survey_workspace_bytes(su["lattice"]["dims"]), hm.workspace_bytes(sh["lattice"]["dims"]),
                hm.slice_workspace_bytes(sl2["slices"]["dims"], sl2["slices"]["layers"])]
        assert cuts[1] < cuts[0] and cuts[3] > max(cuts[:3]) and cuts[4] < cuts[3] and max(cuts) <= hm.KEEP, cuts
        assert cuts[0] == 256 * (3 * 79 + 2) and cuts[1] == 768 + 256 + 128 * 210  # 25 * 25 * 8 points in 5 pieces; 9 tiles, one run, the tally

        # 7: the large calls of the new families, each followed by a small call that cuts the buffer again
        big, count, m1, px, m2 = b["large_new"]
        assert [s["call"] for s in (big, count, m1, px, m2)] == ["surveyMesh", "countSlices", "measure", "pickSpans", "measure"]
        n = big["lattice"]["dims"][0]
        assert big["lattice"]["dims"] == (n, n, n) and hm.survey_workspace_bytes((n, n, n)) > hm.KEEP >= hm.survey_workspace_bytes((n - 1,) * 3)
        assert hm.survey_workspace_bytes((n, n, n)) == (n + 1) ** 3 * 4 + 4096 * 23 and n == 255
        g = count["slices"]
        n = g["dims"][0]
        assert g["dims"] == (n, n) and hm.slice_workspace_bytes((n, n), g["layers"]) > hm.KEEP >= hm.slice_workspace_bytes((n - 1, n - 1), g["layers"])
        assert hm.measure_workspace_bytes(m1["grid"]["nu"], m1["grid"]["nv"]) < 1 << 20
        w, h = hm.BIG_SPAN_FRAME
        assert (px["host"], px["frame"], px["max_spans"], px["n"], px["w"], px["h"]) == (True, True, 64, w * h, w, h) and w % 8 == 0 and h % 8 == 0
        assert hm.staging_bytes(px) == w * h * (32 + 64 * 8) == 68239360 > hm.KEEP  # (every piece a multiple of 256 bytes already)
        assert hm.staging_bytes(dict(px, n=(w - 8) * h)) <= hm.KEEP or hm.staging_bytes(dict(px, n=w * (h - 8))) <= hm.KEEP  # no smaller frame of whole tiles
        assert m2["host"] and m2["columns"] and 0 < hm.staging_bytes(m2) < 1 << 20

        # 8: the labelling grows `mesh` in the middle of its call, behind the other lane's enqueued emit work.  `mesh.bytes` through the
        # block: sdfr_device_buffer::reserve allocates exactly what is asked for and never shrinks, release_large frees past the keep
        count, one, m1, frame, many, m2 = b["components_grow"]
        assert [s["call"] for s in (count, one, m1, frame, many, m2)] == ["labelComponents", "labelLattice", "extractMesh", "render", "labelLattice", "extractMesh"]
        assert all(s["state"]["fif"] == 2 and not s["host"] for s in (count, one, m1, frame, many, m2))
        assert [bool(s.get("defer")) for s in (count, one, m1, frame, many, m2)] == [False, False, True, True, False, False]
        assert many.get("alone") and not m2.get("alone")  # the labelling is synchronous and read at once, the deferred answers after the last call's sync
        assert (count["capacity"], count["labels"]) == ("none", False) and (many["capacity"], many["labels"]) == ("exact", True) and one["labels"]
        n = count["lattice"]["dims"][0]
        assert count["lattice"]["dims"] == (n, n, n) == hm.BIG_COMPONENTS and 170 <= n <= 180 and count["lattice"]["cell"] == 0.02
        assert hm.components_workspace_bytes((n, n, n), False, 1) > hm.KEEP >= hm.components_workspace_bytes((n - 1,) * 3, False, 1)
        assert one["dims"] == many["dims"] == hm.GROW_DIMS == (47, 47, 31) and (one["kind"], many["kind"]) == ("all_outside", "checkerboard")
        points = 48 * 48 * 32
        assert ho.components(one)[0]["components"] == 1 and ho.components(many)[0]["components"] == points == 73728 > hm.COMPONENTS_TABLE_FIRST == 65536
        mesh_bytes = 0                                                            # after the counting call: past the keep, released
        first = hm.components_workspace_bytes(one["dims"], True, 1)
        mesh_bytes = max(mesh_bytes, first)                                       # after the labelling of one component ...
        assert mesh_bytes == first == hm.components_workspace_bytes(many["dims"], True, 1) == 3214848  # ... exactly the first cut of the checkerboard's
        assert first == 2 * 294912 + 256 + 1280 + 2048 + 65536 * 40               # parent, scan (one word more: one piece more of 256 bytes), sums, result, table
        assert hm.workspace_bytes(m1["lattice"]["dims"]) < mesh_bytes             # the extraction whose emit is enqueued: `mesh` stays
        grown = hm.components_workspace_bytes(many["dims"], True, points)
        assert mesh_bytes < grown == first + (points - 65536) * 40 == 3542528 <= hm.KEEP  # the second cut: larger, the growth in the middle of the call
        mesh_bytes = max(mesh_bytes, grown)
        assert hm.workspace_bytes(m2["lattice"]["dims"]) < mesh_bytes and m1["lattice"]["dims"] != m2["lattice"]["dims"]

        assert any(part[0]["state"]["fif"] == 2 for part in b.values())
    kinds = {hm.blocks(steps)["scene_change"][2]["call"] for steps in SEQUENCES.values()}
    assert kinds == {"queryRaySurfaces", "querySpans"}  # the call in flight on the run-time scene when it goes: both kinds


def test_the_restated_components_plan_is_the_librarys():
    """components_workspace_bytes and the labelling's staging_bytes against sdfr_components_plan.h itself, built for the CPU
    (tests/cpp/components_plan_host.cpp): the free sizes' extremes, a lattice that is no cube, the block's dims before and after the
    growth and around the 65536 components the table first has room for, and the cube past the keep with its neighbour below"""
    import components_util as cu

    n = hm.BIG_COMPONENTS[0]
    cases = [(dims, own, C) for dims in ((5, 5, 5), (24, 24, 24), (7, 23, 14), hm.GROW_DIMS, (n, n, n), (n - 1,) * 3) for own in (0, 1)
             for C in (1, 2, 65535, 65536, 65537, 73728) if C <= hm.lattice_points(dims)]
    line = "1 0.0 0.0 0.0 1.0 %d %d %d 0.0 %d %d %d %d %d 1 1 %d"  # (the format: tests/cpp/components_plan_host.cpp)
    answers = cu.run_plan([line % (dims + (own, own, C, 1, labels, C)) for dims, own, C in cases for labels in (0, 1)])
    assert len(answers) == 2 * len(cases)
    for k, (dims, own, C) in enumerate(cases):
        for labels in (0, 1):
            fields = answers[2 * k + labels].split(";")
            assert fields[0] == "0" and int(fields[-1]) == hm.components_workspace_bytes(dims, bool(own), C), (dims, own, C)
            first = int(fields[-1]) if C <= hm.COMPONENTS_TABLE_FIRST else hm.components_workspace_bytes(dims, bool(own), 1)
            assert sum(-(-int(w) // 256) * 256 for w in fields[5].split()) == first == hm.components_workspace_bytes(dims, bool(own), 1)  # the cut before they are counted
            step = dict(call="labelLattice" if own else "labelComponents", lattice=dict(dims=dims), dims=dims, labels=bool(labels))
            assert hm.staging_bytes(step) == sum(-(-int(b) // 256) * 256 for b in fields[6].split()), (dims, own, labels)


def hs_private_rows(height, split):
    m, M = split
    return [r for r in range(height) if (r // 8) % M < m]


def test_every_failure_kind_and_each_between_two_valid_calls():
    assert set().union(*(hm.failure_kinds(steps) for steps in SEQUENCES.values())) == set(hm.FAILURE_KINDS)
    assert len(hm.FAILURE_KINDS) == 17
    assert [dict(hm.FAILURES)[k] for k in ("components_negative_capacity", "components_small_capacity", "components_null_lattice")] == ["negative capacity", None, "null pointer"]
    assert dict(hm.FAILURES)["slice_negative_capacity"] == "negative capacity" and dict(hm.FAILURES)["slice_small_capacity"] is None
    assert [dict(hm.FAILURES)[k] for k in ("span_max_spans_65", "measure_nu_0", "survey_bad_band", "fit_bad_margin")] == [
        "bad span parameters", "bad measure grid", "band must be finite and >= 0", "margin must be 0..8"]
    # the kinds every query entry has go through the three span entries too
    assert {s["entry"] for s in ALL if s["family"] == "failed" and s["fail"] in hm.SHARED_KINDS} >= set(hm.SPAN_ENTRIES)
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
            assert max(s["lattice"]["dims"]) <= (hm.MAX_FIT if s["call"] == "fitMesh" else hm.MAX_LATTICE) and hm.MAX_FIT <= 64
        if "dims" in s:
            assert s["call"] == "labelLattice" and 5 <= min(s["dims"]) and max(s["dims"]) <= hm.MAX_LATTICE <= 24  # at most 25^3 points
        if "slices" in s:
            assert max(s["slices"]["dims"]) <= 24 and 1 <= s["slices"]["layers"] <= 8
        if s["family"] == "spans" and s.get("frame"):
            assert (s["w"], s["h"]) in hm.AA_SIZES and s["n"] == s["w"] * s["h"]
        if s["family"] == "measure":
            assert {s["grid"]["nu"], s["grid"]["nv"]} <= set(hm.MEASURE_COLUMNS) | {hm.MEASURE_BIG}
        if "tile" in s:
            assert s["tile"] in (4, 8, 16) and s["width"] <= 256 and s["width"] % max(8, s["tile"]) == 0
    # the edges themselves: a lattice that is no cube, item counts around the 64 items of a block, pixels outside the frame
    assert any(len(set(s["lattice"]["dims"])) == 3 for s in ALL if "lattice" in s)
    for s in ALL:
        if s["call"] in ("pick", "pickSurfaces", "pickLighting", "pickSpans") and not s.get("frame"):
            px = hm.pixel_list(s)
            assert len(px) == s["n"] and not (0 <= px[0][0] < s["w"] and 0 <= px[0][1] < s["h"])


def test_every_lattice_meets_the_surface():
    """a lattice feeds an extraction, the vertices of the mesh queries or an atlas: by the oracle's distances every one of the committed
    seeds has vertices and quads, in the state of its step (scene variables and the debug plane included)"""
    import mesh_util as mu
    import query_util as qu

    for s in ALL:
        if "lattice" not in s or s["state"]["scene"] == hs.RUNTIME_SCENE or s["call"] == "countMesh" or s["block"] == "large_new":
            continue
        if s["block"] == "components_grow" and s["call"] == "labelComponents":  # millions of points: surface_condition() looks at their signs
            continue
        src = SEQUENCES_OF[id(s)][s["src"]] if s["family"] == "atlas" and s["src"] is not None else s  # an atlas of an earlier step's mesh
        st, lat = src["state"], src["lattice"]
        if st["scene"] == hs.RUNTIME_SCENE:
            continue
        of = qu.frame(st["scene"], st["stime"], 16, 9, dict(st["vars"], **(hm.debug_vars(st["scene"]) if st["debug"] else {})))
        D = qu.oracle_points(st["scene"], of, mu.lattice_points(lat["origin"], lat["cell"], lat["dims"]), normals=False)[0]
        pos, idx = mu.surface_nets(D, lat["origin"], lat["cell"], lat["dims"], 0.0)
        assert len(pos) >= 8 and len(idx) >= 4, (s["i"], s["call"], st["scene"], st["vars"], lat, len(pos), len(idx))


def surface_condition(s):
    """What a step of the survey, the slices, the spans, the measure or the labelling on a built-in scene meets of the surface, by the
    oracle's distances in the step's state: (None, {}) if the step has nothing to meet, else (the condition it misses or None, what
    was seen)"""
    if s["state"]["scene"] == hs.RUNTIME_SCENE:
        return None, {}
    of = ho.frame(s, s.get("w") or 16, s.get("h") or 9)
    call = s["call"]
    if call in ("extractSlices", "countSlices") or (call == "failed" and s["fail"].startswith("slice_")):
        pos, _uv, seg, _lv, _ls = ho.slices(s, of)
        return (None if len(pos) >= 8 and len(seg) >= 4 else "a slice stack has at least 8 vertices and 4 segments"), dict(vertices=len(pos), segments=len(seg))
    if call in ("querySpans", "pickSpans", "meshSpans"):
        S, _spans = ho.spans(s, of, ho.span_rays(s, of, ho.mesh_vertices(s, of) if call == "meshSpans" else None), max_spans=0)
        seen = dict(crossing=float((S["crossings"] > 0).mean()), over=bool((S["spans"] > s["max_spans"]).any()), out_of_steps=bool((S["flags"] & 4).any()),
                    invalid=bool((S["valid"] == -1).any()))
        return (None if s["n"] < 64 or seen["crossing"] >= 0.125 else "of 64 or more items one in eight has a crossing"), seen
    if call == "measure":
        res, _col = ho.measure(s, of)
        seen = dict(columns_hit=res["columns_hit"])
        return (None if s["grid"]["nu"] * s["grid"]["nv"] < 64 or res["columns_hit"] >= 8 else "of 64 or more columns 8 are hit"), seen
    if call == "surveyMesh" and s["block"] == "large_new":  # vertices > 0: some lattice point is inside and some is not
        with np.errstate(invalid="ignore"):
            inside = ho.lattice_distances(s, of) < 0
        return (None if inside.any() and not inside.all() else "a survey has vertices"), {}
    if call == "surveyMesh":
        got = ho.survey(s, of)
        return (None if got["active_cells"] > 0 else "a survey has vertices"), dict(vertices=got["active_cells"])
    if call == "fitMesh":
        got = ho.fit(s, of)
        return (None if got["state"] == 1 else "a fit returns SDFR_FIT_FOUND"), dict(state=got["state"], dims=got["dims"])
    if call == "labelComponents" and s["block"] == "components_grow":  # millions of points: a solid and a void = some point is inside and some is not
        with np.errstate(invalid="ignore"):
            inside = ho.lattice_distances(s, of) < 0
        return (None if inside.any() and not inside.all() else "a labelling of the scene has a solid and a void"), {}
    if call == "labelComponents":
        counts = ho.components(s, of)[0]
        missed = None if counts["solids"] >= 1 and counts["voids"] >= 1 else "a labelling of the scene has a solid and a void"
        return missed, dict(components=counts["components"], short=counts["components"] if s["capacity"] == "short" else 0)
    return None, {}


def components_seen(s):
    """what a labelling step of the caller's lattice has, by the definition: needs no scene, so on the run-time scene too"""
    counts = ho.components(s)[0]
    return dict(components=counts["components"], short=counts["components"] if s["capacity"] == "short" else 0)


def test_every_input_of_the_new_families_meets_the_surface():
    """conditions, not measurements: slices with contours, rays with crossings, columns that are hit, surveys with vertices, fits that
    find, labellings of the scene with a solid and a void -- every step of the committed seeds on a built-in scene, in its state (scene
    variables and the debug plane included); and over all seeds some ray has more spans than are stored, some runs out of steps, some
    pixel is outside its frame, some labelling has three or more components and some with the capacity rule "short" has two or more
    (with one it would fall back to "exact")"""
    seen_all = dict(over=False, out_of_steps=False, invalid=False, three_components=False, short_of_two=False)
    for s in ALL:
        missed, seen = surface_condition(s)
        assert missed is None, (missed, s["i"], s["call"], s["state"]["scene"], s["state"]["vars"], s["state"]["debug"], seen)
        if s["call"] == "labelLattice" and s["block"] is None:
            seen = components_seen(s)
        seen = dict(seen, three_components=seen.get("components", 0) >= 3, short_of_two=seen.get("short", 0) >= 2)
        for k in seen_all:
            seen_all[k] = seen_all[k] or bool(seen.get(k))
    assert all(seen_all.values()), seen_all
    assert hm.BANDS[0] == 0.0  # (a survey's vertices do not depend on the band)


def test_the_interleavings_the_suite_never_ran_before():
    """the four named in the tests' reason for being, each somewhere in the committed seeds"""
    queries = ("points", "rays", "pick", "surfaces", "occlusion", "lighting")
    # a host atlas bake right after the host lighting query that pushed `query` past its keep: the staging block, every seed
    # a device extraction, a frame (the lanes swap), an extraction that reuses `mesh` on the other lane: the lanes block, every seed
    # an anti-aliased frame between two plain frames in flight: the aa_in_flight block, every seed
    # a failed mesh call between a query and a render
    assert any(s["family"] == "failed" and s["fail"].startswith("mesh_") and steps[s["i"] - 1]["family"] in queries and steps[s["i"] + 1]["family"] == "render"
               for steps in SEQUENCES.values() for s in steps)

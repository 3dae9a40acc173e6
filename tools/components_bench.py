"""Time of sdfr_components_label on the GPU, stage by stage, against the only way to a piece count without it -- the lattice's distances
copied to the host and labelled there by the library's own union on one CPU thread -- in the same session.

    python tools/components_bench.py run --yardstick --out run.json                                              # the host's clock
    rocprofv3 --kernel-trace -d <dir> --output-format csv -- python tools/components_bench.py run --out trace_run.json   # a run of its own
    python tools/components_bench.py report <dir> trace_run.json run.json [direct_dir direct_trace_run.json]  >  profiles/components_bench.json

run: per scene (time 0.5, the default limits; the box of mesh_bench.py, --cells^3 cells) one counting call, then `warmup` + `reps` calls of
sdfr_components_label with device arrays for the records and the labels; the host clock around each (the calls are synchronous).  With
--yardstick also, `yardstick-reps` times: queryDistance over the lattice's points on the device and the copy of the distances to the host,
then tests/cpp/components_host.cpp (the library's union with a plain min, -O2, one thread) over them; its counts must be the GPU's.
SDFR_LIBRARY in the environment selects another build of the library, e.g. one made with -DSDFR_COMPONENTS_BRICK=0 (no brick stage, every
edge united in global memory).  report: the kernel times of a traced run, per scene the median over the `reps` timed calls of each stage --
sample, bricks, seams, flatten, number (root flags, scan, labels), tally + pack -- and of their sum.  Prints one JSON object."""
import argparse
import csv
import ctypes
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STAGES = (("sample", ("query_lattice",)), ("bricks", ("k_components_bricks", "k_components_identity")), ("seams", ("k_components_seams",)),
          ("flatten", ("k_components_flatten",)), ("number", ("k_components_roots", "k_mesh_scan", "k_components_number")),
          ("tally_pack", ("k_components_init", "k_components_tally", "k_components_pack", "k_components_finish")))
HOST_LIB = os.path.join(ROOT, "tools", "libsdfr_components_host.so")


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def host_library():
    """the CPU stand-in, built with -O2"""
    source = os.path.join(ROOT, "tests", "cpp", "components_host.cpp")
    csrc = os.path.join(ROOT, "sdf_playground_amd", "csrc")
    if not os.path.exists(HOST_LIB) or os.path.getmtime(HOST_LIB) < max(os.path.getmtime(source), os.path.getmtime(os.path.join(csrc, "sdfr_components.h"))):
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + csrc, source, "-o", HOST_LIB], check=True)
    L = ctypes.CDLL(HOST_LIB)
    L.cmp_label.restype = ctypes.c_int64
    L.cmp_label.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int64] + [ctypes.c_void_p] * 3
    return L


def run(args):
    import numpy as np
    import torch
    import sdf_playground_amd as sp
    from mesh_bench import BOXES

    L = sp.load_library()
    r = sp.SDFRenderer(0)
    n = args.cells
    out = {"cells": n, "lattice_points": (n + 1) ** 3, "reps": args.reps, "warmup": args.warmup, "library": os.environ.get("SDFR_LIBRARY", "the package's"), "scenes": {}}
    for scene in args.scenes.split(","):
        r.initShader(scene)
        r.setParameters(0.5)
        r.setCamera(sp.Camera())
        origin, edge = BOXES.get(scene, ((-4.0, -0.5, -4.0), 8.0))
        cell = edge / n
        grid = sp.MeshGrid((ctypes.c_float * 3)(*origin), cell, n, n, n, 0.0)
        counts = sp.ComponentCounts()
        r._check(L.sdfr_components_label(r._h, ctypes.byref(grid), 0, None, None, ctypes.byref(counts), 0))
        C = int(counts.components)
        records = torch.empty((C, 10), dtype=torch.int32, device="cuda")
        labels = torch.empty((n + 1) ** 3, dtype=torch.int32, device="cuda")
        ms = []
        for _ in range(args.warmup + args.reps):
            again = sp.ComponentCounts()
            t0 = time.perf_counter()
            r._check(L.sdfr_components_label(r._h, ctypes.byref(grid), C, ctypes.c_void_p(records.data_ptr()), ctypes.c_void_p(labels.data_ptr()), ctypes.byref(again), 0))
            ms.append((time.perf_counter() - t0) * 1e3)
            assert bytes(again) == bytes(counts)
        rec = {"origin": origin, "cell": cell, "counts": counts.as_dict(), "host_ms": {"label": median(ms[args.warmup:]), "min": min(ms[args.warmup:]), "max": max(ms[args.warmup:])}}
        if args.yardstick:
            H = host_library()
            c32 = float(np.float32(cell))
            k, j, i = torch.meshgrid(*[torch.arange(n + 1, dtype=torch.float32, device="cuda")] * 3, indexing="ij")
            points = torch.stack([origin[0] + i * c32, origin[1] + j * c32, origin[2] + k * c32], dim=-1).reshape(-1, 3).contiguous()
            del i, j, k
            host_records, host_labels = np.zeros((n + 1) ** 3, sp.COMPONENT_DTYPE), np.zeros((n + 1) ** 3, np.uint32)
            lattice_ms, label_ms = [], []
            for _ in range(args.yardstick_reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                D = r.queryDistance(points)
                r.sync()
                D = D.cpu().numpy()
                t1 = time.perf_counter()
                host_counts = sp.ComponentCounts()
                found = H.cmp_label(ctypes.addressof(grid), D.ctypes.data, None, 0, host_records.ctypes.data, host_labels.ctypes.data, ctypes.addressof(host_counts))
                t2 = time.perf_counter()
                lattice_ms.append((t1 - t0) * 1e3)
                label_ms.append((t2 - t1) * 1e3)
                agree = found == C and bytes(host_counts) == bytes(counts)
            # (the point query computes origin + i * cell as the lattice kernel does: the same distances, so the same counts)
            rec["yardstick_ms"] = {"lattice_to_host": median(lattice_ms), "host_label": median(label_ms), "sum": median(lattice_ms) + median(label_ms), "reps": args.yardstick_reps,
                                   "counts_agree": bool(agree), "labels_agree": bool(np.array_equal(host_labels, labels.cpu().numpy().view(np.uint32)))}
            del points
        out["scenes"][scene] = rec
        del records, labels
    r.close()
    text = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


def stage_times(where, run_json):
    """{scene: {stage: median us over the timed calls, "sum": ...}} of the traced run"""
    meta = json.load(open(run_json))
    rows = []
    for path in glob.glob(os.path.join(where, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda d: int(d["Dispatch_Id"]))
    # a call starts at its lattice launch; per scene: the counting call, then warmup + reps calls
    calls = []
    for d in rows:
        name = d["Kernel_Name"]
        stage = next((s for s, keys in STAGES if any(k in name for k in keys)), None)
        if stage is None:
            continue
        if stage == "sample":
            calls.append({s: 0.0 for s, _k in STAGES})
        if calls:
            calls[-1][stage] += (int(d["End_Timestamp"]) - int(d["Start_Timestamp"])) * 1e-3
    per_scene = 1 + meta["warmup"] + meta["reps"]
    assert len(calls) == per_scene * len(meta["scenes"]), (len(calls), per_scene, len(meta["scenes"]))
    out = {}
    for at, scene in enumerate(meta["scenes"]):
        timed = calls[at * per_scene + 1 + meta["warmup"]:(at + 1) * per_scene]
        out[scene] = {s: round(median([c[s] for c in timed]), 2) for s, _k in STAGES}
        out[scene]["sum"] = round(median([sum(c.values()) for c in timed]), 2)
    return out, meta


def report(paths):
    stages, meta = stage_times(paths[0], paths[1])
    out = json.load(open(paths[2]))
    out["kernel_time_source"] = "rocprofv3 --kernel-trace, a run of its own; medians over the timed calls, microseconds"
    for scene, rec in out["scenes"].items():
        rec["kernel_us"] = stages[scene]
        assert rec["counts"] == meta["scenes"][scene]["counts"], scene
    if len(paths) == 5:
        direct, direct_meta = stage_times(paths[3], paths[4])
        for scene, rec in out["scenes"].items():
            rec["kernel_us_without_bricks"] = direct[scene]
            rec["same_counts_without_bricks"] = direct_meta["scenes"][scene]["counts"] == rec["counts"]
            rec["host_ms_without_bricks"] = direct_meta["scenes"][scene]["host_ms"]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("run", "report"))
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--scenes", default="labyrinth,tree,gyroid")
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--yardstick", action="store_true")
    ap.add_argument("--yardstick-reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mode == "run":
        run(a)
    elif len(a.paths) in (3, 5):
        report(a.paths)
    else:
        sys.exit(__doc__)

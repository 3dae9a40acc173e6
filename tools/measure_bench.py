"""Time of sdfr_measure on the GPU against the way to the same volume without it -- sdfr_query_ray_spans with max_spans = 0 over the same
rays into device arrays, the summaries copied back and summed on the host -- in the same session.

    rocprofv3 --kernel-trace -d <dir> --output-format csv -- python tools/measure_bench.py run --out run.json
    python tools/measure_bench.py report <dir> run.json  >  profiles/measure_bench.json

run: per scene (time 0.5, the default limits) the box of the surface is fitted inside a search box (fitMesh), 1024 x 1024 columns are laid
over it along y, and with min_step = depth / 512 `warmup` + `reps` calls of measure are made, then as many of querySpans(max_spans=0,
device=True) over the columns' rays, each followed by the copy of the summaries to the host and the host's sum of inside_length.  It
measures nothing itself but the host clock around the synchronised calls.  report: the kernel times of that run from the trace -- per
scene the median duration of k_query_measure, of the k_measure_reduce passes of a call together, and of k_query_spans over the `reps`
timed calls --, the share of the measure kernel's time that the butterflies, the atomics and the fp64 sums take (its difference to
k_query_spans on the same rays), and the bytes each way moves to the host.  Prints one JSON object."""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 1024
STEP_FRACTION = 512  # min_step = depth / 512
MAX_STEPS = 4096
SEARCH = ((-8.0, -1.0, -8.0), 0.0625, (256, 128, 256))  # the search box of the fit: origin, cell, dims
SCENE_STRUCTS = {"fast_sphere": "SceneFastSphere", "labyrinth": "SceneLabyrinth", "tree": "SceneTree"}


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def run(args):
    import ctypes

    import numpy as np
    import torch
    import sdf_playground_amd as sp

    r = sp.SDFRenderer(0)
    out = {"columns": [N, N], "reps": args.reps, "warmup": args.warmup, "max_steps": MAX_STEPS, "scenes": {}}
    f3 = lambda a: (ctypes.c_float * 3)(*[float(x) for x in a])  # noqa: E731
    for scene in args.scenes.split(","):
        r.initShader(scene)
        r.setParameters(0.5)
        fit = r.fitMesh(*SEARCH)
        fitted = fit["state"] == sp.FIT_FOUND  # (else: the search box itself)
        lo = np.array(fit["origin"] if fitted else SEARCH[0])
        hi = lo + SEARCH[1] * np.array(fit["dims"] if fitted else SEARCH[2])
        cu, cv, depth = (hi[0] - lo[0]) / N, (hi[2] - lo[2]) / N, float(hi[1] - lo[1])
        grid = sp.MeasureGrid(f3((lo[0] + 0.5 * cu, lo[1], lo[2] + 0.5 * cv)), f3((cu, 0, 0)), f3((0, 0, cv)), f3((0, 1, 0)), N, N)
        min_step = depth / STEP_FRACTION
        # the same rays for the span query: the columns' origins as the kernel computes them
        j, i = np.mgrid[0:N, 0:N]
        o32 = lambda k: np.float32(grid.origin[k]) + i.ravel().astype(np.float32) * np.float32(grid.du[k]) + j.ravel().astype(np.float32) * np.float32(grid.dv[k])  # noqa: E731
        origins = torch.as_tensor(np.stack([o32(0), o32(1), o32(2)], 1).astype(np.float32)).cuda()
        dirs = torch.as_tensor(np.tile(np.array([0, 1, 0], np.float32), (N * N, 1))).cuda()

        def timed(call):
            ms = []
            for _ in range(args.warmup + args.reps):
                r.sync()
                t0 = time.perf_counter()
                res = call()
                r.sync()
                ms.append((time.perf_counter() - t0) * 1e3)
            return res, median(ms[args.warmup:])

        def by_spans():
            summaries, _none = r.querySpans(origins, dirs, min_step, t_max=depth, max_steps=MAX_STEPS, max_spans=0)
            r.sync()
            s = summaries.cpu().numpy().view(sp.SPAN_SUMMARY_DTYPE).reshape(-1)
            return s, float(s["inside_length"].astype(np.float64).sum())

        res, measure_ms = timed(lambda: r.measure(grid, min_step, t_max=depth, max_steps=MAX_STEPS))
        (s, length), spans_ms = timed(by_spans)
        props = sp.measureProperties(grid, res, 1.0)
        out["scenes"][scene] = {
            "fitted": bool(fitted), "box_lo": [float(x) for x in lo], "box_hi": [float(x) for x in hi], "min_step": min_step, "depth": depth,
            "measure": {k: v for k, v in res.as_dict().items()}, "properties": props,
            "steps_sum": int(res.steps), "spans_steps_sum": int(s["steps"].astype(np.int64).sum()),
            "volume_by_spans": length * cu * cv, "volume_by_measure": props["volume"],
            "bytes_to_host": {"measure": 160, "spans": int(s.nbytes)},
            "host_ms": {"measure": measure_ms, "spans_copy_sum": spans_ms}}
    r.close()
    text = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


def report(where, run_json):
    out = json.load(open(run_json))
    rows = []
    for path in glob.glob(os.path.join(where, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda d: int(d["Dispatch_Id"]))
    calls = out["warmup"] + out["reps"]
    reduce_us = [(int(d["End_Timestamp"]) - int(d["Start_Timestamp"])) * 1e-3 for d in rows if "k_measure_reduce" in d["Kernel_Name"]]
    passes_per_call = len(reduce_us) // (calls * len(out["scenes"])) if out["scenes"] else 0
    at = 0
    for scene, rec in out["scenes"].items():
        struct = SCENE_STRUCTS.get(scene, scene)
        rec["kernel_us"] = {}
        for kernel in ("k_query_measure", "k_query_spans"):
            us = [(int(d["End_Timestamp"]) - int(d["Start_Timestamp"])) * 1e-3 for d in rows if kernel in d["Kernel_Name"] and struct + "," in d["Kernel_Name"]]
            assert len(us) == calls, (scene, kernel, len(us))
            rec["kernel_us"][kernel] = {"median": median(us[out["warmup"]:]), "min": min(us[out["warmup"]:]), "max": max(us[out["warmup"]:])}
        per_call = [sum(reduce_us[at + c * passes_per_call: at + (c + 1) * passes_per_call]) for c in range(calls)]
        at += calls * passes_per_call
        rec["kernel_us"]["k_measure_reduce"] = {"passes": passes_per_call, "median": median(per_call[out["warmup"]:])}
        m, s = rec["kernel_us"]["k_query_measure"]["median"], rec["kernel_us"]["k_query_spans"]["median"]
        rec["reduction_share_of_measure_kernel"] = (m - s) / m
        rec["measure_over_spans_kernel_time"] = m / s
    out["kernel_time_source"] = "rocprofv3 --kernel-trace, a run of its own; medians over the timed repetitions"
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("run", "report"))
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scenes", default="fast_sphere,labyrinth,tree")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mode == "run":
        run(a)
    elif len(a.paths) == 2:
        report(a.paths[0], a.paths[1])
    else:
        sys.exit(__doc__)

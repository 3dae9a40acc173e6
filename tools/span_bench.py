"""Throughput of the whole-frame span query (sdfr_pick_spans without a pixel list) on the GPU, device arrays, against the first-hit query
of the same frame (sdfr_pick over every pixel: the k_query_rays kernel) in the same session.

    rocprofv3 --kernel-trace -d <dir> --output-format csv -- python tools/span_bench.py run --out run.json
    python tools/span_bench.py report <dir> run.json  >  profiles/span_bench.json

run: per scene (the start-up camera, time 0.5, a 1920 x 1080 frame, the default limits) `warmup` + `reps` calls of pickSpans(None, ...)
with min_step = limits.range / 512, t_max = limits.range, max_steps = 4096 and max_spans = 4, then as many of pick over the list of all
pixels; the sum of `steps` and the flags of the last span call are kept.  It measures nothing itself but the host clock around the
synchronised calls.  report: the kernel times of that run from the trace -- per scene the median duration of k_query_spans and of
k_query_rays over the `reps` timed calls -- and from them samples per second (the sum of `steps` over the kernel time), the mean
`steps` per ray and the ratio to the first-hit kernel.  Prints one JSON object."""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
RANGE_FRACTION = 512  # min_step = limits.range / 512
MAX_STEPS, MAX_SPANS = 4096, 4
SCENE_STRUCTS = {"fast_sphere": "SceneFastSphere", "labyrinth": "SceneLabyrinth", "tree": "SceneTree"}


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def run(args):
    import numpy as np
    import torch
    import sdf_playground_amd as sp

    r = sp.SDFRenderer(0)
    out = {"width": W, "height": H, "reps": args.reps, "warmup": args.warmup, "max_steps": MAX_STEPS, "max_spans": MAX_SPANS, "scenes": {}}
    ys, xs = np.mgrid[0:H, 0:W]
    pixels = torch.as_tensor(np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)).cuda()
    hits = torch.empty((W * H, 12), dtype=torch.float32, device="cuda")
    for scene in args.scenes.split(","):
        r.initShader(scene)
        r.setParameters(0.5)
        r.setCamera(sp.Camera())
        limits = r.getLimits()
        min_step = float(limits.range) / RANGE_FRACTION

        def timed(call):
            ms = []
            for _ in range(args.warmup + args.reps):
                r.sync()
                t0 = time.perf_counter()
                res = call()
                r.sync()
                ms.append((time.perf_counter() - t0) * 1e3)
            return res, median(ms[args.warmup:])

        (summaries, _spans), span_ms = timed(lambda: r.pickSpans(None, W, H, min_step, max_steps=MAX_STEPS, max_spans=MAX_SPANS, device=True))
        _hits, pick_ms = timed(lambda: r.pick(pixels, W, H, out=hits))
        s = summaries.cpu().numpy().view(sp.SPAN_SUMMARY_DTYPE).reshape(-1)
        h = hits.cpu().numpy().view(sp.HIT_DTYPE).reshape(-1)
        steps = s["steps"].astype(np.int64)
        tiles = steps.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)  # (1920 and 1080 are multiples of 8)
        out["scenes"][scene] = {
            "min_step": min_step, "range": float(limits.range), "rays": int(len(s)), "steps_sum": int(steps.sum()), "steps_mean": float(steps.mean()),
            "steps_max": int(steps.max()), "out_of_steps": int(((s["flags"] & sp.SPAN_OUT_OF_STEPS) != 0).sum()),
            "rays_with_spans": int((s["spans"] > 0).sum()), "spans_mean": float(s["spans"].mean()), "spans_over_capacity": int((s["spans"] > MAX_SPANS).sum()),
            # a wave is as long as its longest ray: the steps a tile's lanes make over 64 times its longest lane's
            "lane_utilisation": float(steps.sum() / (64.0 * tiles.max(1).astype(np.int64).sum())),
            "pick_iterations_sum": int(h["iterations"].astype(np.int64).sum()), "pick_iterations_mean": float(h["iterations"].mean()),
            "host_ms": {"pick_spans": span_ms, "pick": pick_ms}}
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
    for scene, rec in out["scenes"].items():
        struct = SCENE_STRUCTS.get(scene, scene)
        rec["kernel_us"] = {}
        for kernel in ("k_query_spans", "k_query_rays"):
            us = [(int(d["End_Timestamp"]) - int(d["Start_Timestamp"])) * 1e-3 for d in rows if kernel in d["Kernel_Name"] and struct + "," in d["Kernel_Name"]]
            assert len(us) == out["warmup"] + out["reps"], (scene, kernel, len(us))
            rec["kernel_us"][kernel] = {"median": median(us[out["warmup"]:]), "min": min(us[out["warmup"]:]), "max": max(us[out["warmup"]:])}
        span_s, pick_s = rec["kernel_us"]["k_query_spans"]["median"] * 1e-6, rec["kernel_us"]["k_query_rays"]["median"] * 1e-6
        rec["span_samples_per_s"] = rec["steps_sum"] / span_s
        rec["pick_iterations_per_s"] = rec["pick_iterations_sum"] / pick_s
        rec["span_over_pick_time"] = span_s / pick_s
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

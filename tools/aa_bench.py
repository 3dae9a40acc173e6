"""Cost of an anti-aliased frame (sdfr_render_aa) on the GPU, device memory out.

    python tools/aa_bench.py [--cases labyrinth:3840x2160x4,lense:3840x2160x2] [--reps 20] [--warmup 3] [--baseline]

Per case scene:WxHxK (the start-up camera, time 0.5, the reference's limits): ms per anti-aliased frame (sdfr_get_stats: first pass's
start to the last resolve's end), the time inside the resolve launches (the library's events around them while profiling is on, a
run of its own), the passes, the bytes the resolve reads and its read rate as a fraction of a device-to-device hipMemcpyAsync of as
many bytes in the same process, and the peak device memory the process held (hipMemGetInfo before and after).  Each figure: after
`warmup` calls, median of `reps`.  SDFR_AA_BUDGET_BYTES in the environment sets the pass budget (the A/B of DESIGN.md 4.7).

--baseline: the first yardstick instead -- sdfr_render of S (K * W x K * H) in one piece into device memory, where it fits.  It
needs nothing but sdfr_render, so it also runs on a build that has no sdfr_render_aa.  Prints one JSON object."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def spread(values):
    values = sorted(values)
    return [values[0], values[len(values) // 2], values[-1]]


def used_bytes(torch):
    free, total = torch.cuda.mem_get_info()
    return total - free


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="labyrinth:3840x2160x2,labyrinth:3840x2160x4,labyrinth:1920x1080x8,lense:3840x2160x2,lense:3840x2160x4")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline", action="store_true")
    args = ap.parse_args()

    import torch
    import sdf_playground_amd as sp

    out = {"reps": args.reps, "warmup": args.warmup, "baseline": args.baseline, "budget": os.environ.get("SDFR_AA_BUDGET_BYTES", "default"), "cases": {}}
    for case in args.cases.split(","):
        scene, size = case.split(":")
        w, h, k = (int(v) for v in size.lower().split("x"))
        torch.cuda.empty_cache()
        idle = used_bytes(torch)
        r = sp.SDFRenderer(0)
        r.initShader(scene)
        r.setParameters(0.5)
        cam = sp.Camera()
        cam.SetAspect(w / h)
        r.setCamera(cam)
        res = {"width": w, "height": h, "factor": k}
        if args.baseline:
            s_bytes = 16 * k * k * w * h
            if s_bytes > 6 << 30:
                res["skipped"] = "S is %.1f GB" % (s_bytes / 1e9)
                out["cases"][case] = res
                r.close()
                continue
            img = torch.empty((k * h, k * w, 4), dtype=torch.float32, device="cuda")
            times = []
            for i in range(args.warmup + args.reps):
                r.render(None, k * w, k * h, out=img)
                if i >= args.warmup:
                    times.append(r.getStats().ms_gpu)
            r.sync()
            res.update(ms_render_s=median(times), ms_render_s_spread=spread(times), peak_device_bytes=used_bytes(torch) - idle)
            del img
        else:
            img = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
            times, resolve = [], []
            for i in range(args.warmup + args.reps):
                r.renderAA(None, w, h, k, out=img)
                if i >= args.warmup:
                    times.append(r.getStats().ms_gpu)
            peak = used_bytes(torch) - idle
            r.setProfiling(True)  # events around every resolve: a run of its own, they serialise nothing but cost a little
            for i in range(args.warmup + args.reps):
                r.renderAA(None, w, h, k, out=img)
                if i >= args.warmup:
                    resolve.append(r.getTimings()["draw: resolve"])
            r.setProfiling(False)
            r.sync()
            read_bytes = 16 * k * k * w * h
            # the second yardstick: a device-to-device copy of as many bytes as the resolve reads, in pieces no larger than a pass
            piece = min(read_bytes, 256 << 20)
            src = torch.empty(piece, dtype=torch.uint8, device="cuda")
            dst = torch.empty(piece, dtype=torch.uint8, device="cuda")
            copies = []
            for i in range(args.warmup + args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                done = 0
                while done < read_bytes:
                    n = min(piece, read_bytes - done)
                    dst[:n].copy_(src[:n], non_blocking=True)
                    done += n
                b.record()
                b.synchronize()
                if i >= args.warmup:
                    copies.append(a.elapsed_time(b))
            ms_resolve, ms_copy = median(resolve), median(copies)
            res.update(ms_aa=median(times), ms_aa_spread=spread(times), ms_resolve=ms_resolve, ms_resolve_spread=spread(resolve),
                       resolve_read_bytes=read_bytes, resolve_read_GBps=read_bytes / (ms_resolve * 1e-3) / 1e9, ms_copy_same_bytes=ms_copy,
                       copy_read_GBps=read_bytes / (ms_copy * 1e-3) / 1e9, resolve_rate_over_copy=ms_copy / ms_resolve, peak_device_bytes=peak)
            del img, src, dst
        out["cases"][case] = res
        r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

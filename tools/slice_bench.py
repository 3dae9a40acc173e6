"""Throughput of the slice extraction (sdfr_slice_extract) on the GPU, device memory out.

    python tools/slice_bench.py [--reps 20] [--warmup 3] [--scenes fast_sphere,labyrinth,tree]

Per scene (the start-up camera, time 0.5), on the box tools/mesh_bench.py uses, two stacks of horizontal planes with about the lattice
points of that benchmark's 256^3 cells: one layer of 4096 x 4096 cells at y = 1, the height the start-up camera looks at, and 256 layers
of 256 x 256 cells through the whole box.
A slice records no stage timings (it leaves the handle's timings alone), so two host-clock figures per stack, each the median of `reps`
calls after `warmup`: the counting call -- sample the lattice, classify, both prefix sums, the layer offsets, the read-back --, and the
filling call into device arrays of exactly the counted size, which runs all of that again and then emits, timed up to the end of the
emit work.  The yardstick is mesh_bench.py's "sample" and "classify_scan" stages on its lattice of 257^3 points.
SDFR_SLICE_ROWS=1 in the environment maps a wave to 64 consecutive points of the linear index instead of an 8 x 8 tile of one layer
(the A/B of DESIGN.md 4.14).  Prints one JSON object."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.mesh_bench import BOXES, median  # noqa: E402

STACKS = {"one layer 4096x4096": (4096, 4096, 1), "256 layers 256x256": (256, 256, 256)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="fast_sphere,labyrinth,tree")
    args = ap.parse_args()

    import torch
    import sdf_playground_amd as sp

    L = sp.load_library()
    r = sp.SDFRenderer(0)
    out = {"reps": args.reps, "warmup": args.warmup, "slice_rows": os.environ.get("SDFR_SLICE_ROWS", "0"), "scenes": {}}
    f3 = lambda v: (ctypes.c_float * 3)(*[float(x) for x in v])  # noqa: E731
    for scene in args.scenes.split(","):
        (x0, y0, z0), edge = BOXES.get(scene, ((-4.0, -0.5, -4.0), 8.0))
        r.initShader(scene)
        r.setParameters(0.5)
        r.setCamera(sp.Camera())
        out["scenes"][scene] = {}
        for name, (nu, nv, layers) in STACKS.items():
            step = edge / layers
            grid = sp.SliceGrid(f3((x0, y0 + 0.5 * step if layers > 1 else 1.0, z0)), f3((edge / nu, 0, 0)), f3((0, 0, edge / nv)), f3((0, step, 0)), nu, nv, layers, 0.0)
            points = (nu + 1) * (nv + 1) * layers
            counts = sp.SliceCounts()

            def call(vcap, scap, pos, uv, seg):
                t0 = time.perf_counter()
                rc = L.sdfr_slice_extract(r._h, ctypes.byref(grid), vcap, scap, pos, uv, seg, None, None, ctypes.byref(counts), 0)
                r.sync()
                assert rc == 0, rc
                return (time.perf_counter() - t0) * 1e3

            count_ms = [call(0, 0, None, None, None) for _ in range(args.warmup + args.reps)][args.warmup:]
            v, s = int(counts.vertices), int(counts.segments)
            pos = torch.empty((max(v, 1), 3), dtype=torch.float32, device="cuda")
            uv = torch.empty((max(v, 1), 2), dtype=torch.float32, device="cuda")
            seg = torch.empty((max(s, 1), 2), dtype=torch.int32, device="cuda")
            ptr = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
            fill_ms = [call(v, s, ptr(pos), ptr(uv), ptr(seg)) for _ in range(args.warmup + args.reps)][args.warmup:]
            c, f = median(count_ms), median(fill_ms)
            out["scenes"][scene][name] = {"lattice_points": points, "vertices": v, "segments": s, "ms": {"counting_call": c, "filling_call": f},
                                          "counting_points_per_s": points / (c * 1e-3), "filling_points_per_s": points / (f * 1e-3)}
            del pos, uv, seg
            torch.cuda.empty_cache()
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

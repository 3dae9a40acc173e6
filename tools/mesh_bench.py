"""Throughput of the mesh extraction (sdfr_mesh_extract) on the GPU, device memory out.

    python tools/mesh_bench.py [--cells 256] [--reps 20] [--warmup 3] [--scenes fast_sphere,labyrinth,tree]

Per scene (the start-up camera, time 0.5), on a box of cells^3 cells around the start-up view's content: lattice points/s of the
lattice kernel (the "sample" stage of an extraction), points/s of sdfr_query_distance on the same lattice points in device memory
(what the library offered before the lattice kernel), the split of one extraction with normals into sample / classify + prefix
sums / emit / normals (GPU time between events the library records while profiling is on), and the vertices and triangles
produced.  Each figure: after `warmup` calls, median of `reps`.  SDFR_MESH_LATTICE_ROWS=1 in the environment maps a wave to 64
consecutive points of a lattice row instead of a 4 x 4 x 4 brick (the A/B of DESIGN.md 4.6).  Prints one JSON object."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the box's low corner and edge length per scene: the content the start-up camera (eye (0, 2, -3), looking at (0, 1, 0)) sees
BOXES = {"fast_sphere": ((-2.0, -0.5, -2.0), 4.0), "labyrinth": ((-8.0, -0.5, -6.0), 16.0), "tree": ((-4.0, -0.5, -4.0), 8.0)}


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="fast_sphere,labyrinth,tree")
    args = ap.parse_args()

    import torch
    import sdf_playground_amd as sp

    r = sp.SDFRenderer(0)
    n = args.cells
    out = {"cells": n, "reps": args.reps, "warmup": args.warmup, "lattice_rows": os.environ.get("SDFR_MESH_LATTICE_ROWS", "0"), "scenes": {}}
    for scene in args.scenes.split(","):
        origin, edge = BOXES.get(scene, ((-4.0, -0.5, -4.0), 8.0))
        cell = edge / n
        r.initShader(scene)
        r.setParameters(0.5)
        r.setCamera(sp.Camera())
        r.setProfiling(True)
        stages = []
        for k in range(args.warmup + args.reps):
            pos, _nrm, idx = r.extractMesh(origin, cell, (n, n, n), device=True)
            if k >= args.warmup:
                stages.append(r.getMeshTimings())
        r.setProfiling(False)
        ms = {key: median([s[key] for s in stages]) for key in stages[0]}
        points = (n + 1) ** 3
        # the same lattice points through the point query, device memory in and out
        ax = [torch.tensor(origin[a], dtype=torch.float32, device="cuda") + torch.arange(n + 1, dtype=torch.float32, device="cuda") * torch.tensor(cell, dtype=torch.float32, device="cuda")
              for a in range(3)]
        z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        pts = torch.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1).contiguous()
        del x, y, z
        dist = torch.empty(points, dtype=torch.float32, device="cuda")
        times = []
        for k in range(args.warmup + args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r.queryDistance(pts, out=dist)
            b.record()
            b.synchronize()
            if k >= args.warmup:
                times.append(a.elapsed_time(b))
        ms_query = median(times)
        out["scenes"][scene] = {
            "origin": origin, "cell": cell, "lattice_points": points, "vertices": int(pos.shape[0]), "triangles": int(idx.shape[0]),
            "lattice_points_per_s": points / (ms["sample"] * 1e-3), "query_points_per_s": points / (ms_query * 1e-3),
            "ms": dict(ms, query_distance=ms_query, extraction=sum(ms.values())),
        }
        del pts, dist, pos, idx, _nrm
        torch.cuda.empty_cache()
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

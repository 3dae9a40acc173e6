"""Stage times of sdfr_mesh_extract and sdfr_mesh_extract_sharp on the GPU, device memory out.

    python tools/mesh_sharp_bench.py [--reps 10] [--warmup 2]

The labyrinth (time 0.5) on the box of the CLI's example: origin (-6, 0, -3), cell 0.02, 300 x 100 x 300 cells.  Per entry the split of one
extraction with normals into sample / classify + prefix sums / emit / normals (GPU time between events the library records while
profiling is on; the sharp vertices are part of "emit"), after `warmup` calls the median of `reps`, and the vertices and triangles.
SDFR_LIBRARY in the environment selects another build of the library, e.g. one made with -DSDFR_MESH_SHARP_LANES=1 (a lane per vertex
instead of a lane per edge: the A/B of DESIGN.md 4.12).  Prints one JSON object."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ORIGIN, CELL, DIMS = (-6.0, 0.0, -3.0), 0.02, (300, 100, 300)


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import sdf_playground_amd as sp

    r = sp.SDFRenderer(0)
    r.initShader("labyrinth")
    r.setParameters(0.5)
    r.setCamera(sp.Camera())
    r.setProfiling(True)
    out = {"library": os.environ.get("SDFR_LIBRARY", "libsdfr.so"), "scene": "labyrinth", "origin": ORIGIN, "cell": CELL, "dims": DIMS,
           "lattice_points": (DIMS[0] + 1) * (DIMS[1] + 1) * (DIMS[2] + 1), "reps": args.reps, "warmup": args.warmup}
    for name, sharp in (("sdfr_mesh_extract", False), ("sdfr_mesh_extract_sharp", True)):
        stages = []
        for k in range(args.warmup + args.reps):
            pos, _nrm, idx = r.extractMesh(ORIGIN, CELL, DIMS, device=True, sharp=sharp)
            if k >= args.warmup:
                stages.append(r.getMeshTimings())
        ms = {key: median([s[key] for s in stages]) for key in stages[0]}
        out[name] = {"vertices": int(pos.shape[0]), "triangles": int(idx.shape[0]), "ms": dict(ms, extraction=sum(ms.values()))}
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

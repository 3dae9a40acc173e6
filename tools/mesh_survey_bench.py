"""Cost of sdfr_mesh_survey and sdfr_mesh_fit beside the counting call of sdfr_mesh_extract (capacities 0), one handle, one process.

    python tools/mesh_survey_bench.py [--scene labyrinth] [--cells 160,256] [--fit-cells 512] [--levels 3] [--reps 10] [--warmup 3]

The scene's box of mesh_bench.py (the labyrinth: origin (-8, -0.5, -6), edge 16), time 0.5, the reference's limits.  All three calls are
synchronous -- each reads its result back --, so the figure is the host's clock around the call: the lattice, the kernels, the copy
back, and for a workspace of more than 64 MiB its allocation and release, which such a call pays every time.
  per --cells n: the counting call and the survey (band 0, and band 1.75 cells) over the same n^3 grid, alternated call by call;
  per --fit-cells n: the counting call over the whole n^3 grid and sdfr_mesh_fit with --levels over it as the search grid, alternated.
After `warmup` rounds, `reps` rounds; per figure [min, median, max] in ms.  Also what each call found, and that the survey's counts are the
counting call's.  Prints one JSON object."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def spread(values):
    values = sorted(values)
    return [round(v, 4) for v in (values[0], values[len(values) // 2], values[-1])]


def alternate(calls, warmup, reps):
    """{name: call} -> {name: [min, median, max] ms}, the calls taken in turn round after round"""
    times = {name: [] for name in calls}
    for k in range(warmup + reps):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            if k >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: spread(v) for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="labyrinth")
    ap.add_argument("--cells", default="160,256")
    ap.add_argument("--fit-cells", default="512")
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import ctypes

    import sdf_playground_amd as sp
    from mesh_bench import BOXES

    L = sp.load_library()
    r = sp.SDFRenderer(0)
    r.initShader(args.scene)
    r.setParameters(0.5)
    r.setCamera(sp.Camera())
    origin, edge = BOXES.get(args.scene, ((-4.0, -0.5, -4.0), 8.0))

    def counting(cell, n):
        grid = sp.MeshGrid((ctypes.c_float * 3)(*origin), cell, n, n, n, 0.0)
        counts = sp.MeshCounts()
        r._check(L.sdfr_mesh_extract(r._h, ctypes.byref(grid), 0, 0, None, None, None, ctypes.byref(counts), 0))
        return int(counts.vertices), int(counts.triangles)

    out = {"scene": args.scene, "origin": origin, "edge": edge, "reps": args.reps, "warmup": args.warmup, "survey": {}, "fit": {}}
    for n in [int(x) for x in args.cells.split(",") if x]:
        cell = edge / n
        res = alternate({"counting_call_ms": lambda: counting(cell, n), "survey_band0_ms": lambda: r.surveyMesh(origin, cell, (n,) * 3),
                         "survey_band175_ms": lambda: r.surveyMesh(origin, cell, (n,) * 3, band=1.75 * cell)}, args.warmup, args.reps)
        s, (v, t) = r.surveyMesh(origin, cell, (n,) * 3, band=1.75 * cell), counting(cell, n)
        res.update(lattice_points=(n + 1) ** 3, workspace_mib={"counting_call": round(12 * (n + 1) ** 3 / 2 ** 20, 1), "survey": round(4 * (n + 1) ** 3 / 2 ** 20, 1)},
                   survey=s, counts_agree=(s["active_cells"], 2 * s["quads"]) == (v, t),
                   survey_over_counting={k: round(res[k][1] / res["counting_call_ms"][1], 3) for k in ("survey_band0_ms", "survey_band175_ms")})
        out["survey"][str(n)] = res
    for n in [int(x) for x in args.fit_cells.split(",") if x]:
        cell = edge / n
        res = alternate({"counting_call_ms": lambda: counting(cell, n), "fit_ms": lambda: r.fitMesh(origin, cell, (n,) * 3, levels=args.levels)}, args.warmup, args.reps)
        f = r.fitMesh(origin, cell, (n,) * 3, levels=args.levels)
        res.update(lattice_points=(n + 1) ** 3, levels=args.levels, fit={k: f[k] for k in ("state", "level", "surveys", "lo", "hi", "dims")},
                   fit_over_counting=round(res["fit_ms"][1] / res["counting_call_ms"][1], 3))
        if f["state"] == sp.FIT_FOUND:
            res["fitted_counts"] = counting_fitted(r, L, sp, f, cell)
            res["search_counts"] = counting(cell, n)
        out["fit"][str(n)] = res
    r.close()
    print(json.dumps(out))


def counting_fitted(r, L, sp, f, cell):
    import ctypes

    grid = sp.MeshGrid((ctypes.c_float * 3)(*f["origin"]), cell, f["dims"][0], f["dims"][1], f["dims"][2], 0.0)
    counts = sp.MeshCounts()
    r._check(L.sdfr_mesh_extract(r._h, ctypes.byref(grid), 0, 0, None, None, None, ctypes.byref(counts), 0))
    return int(counts.vertices), int(counts.triangles)


if __name__ == "__main__":
    main()

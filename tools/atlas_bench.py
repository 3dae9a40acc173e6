"""Cost of baking a mesh's texture atlas on the GPU (sdfr_atlas_bake) beside the composition it replaces, device memory, one handle.

    python tools/atlas_bench.py [--configs labyrinth:7,gems:7] [--quads 100000] [--tile 8] [--reps 20] [--warmup 3]

Per configuration -- a scene, or scene:extension_lights -- with the start-up camera's content (mesh_bench.py's box), time 0.5, the
reference's limits and the library's default step shortcuts: the scene is meshed at a cell that gives about --quads quads (a counting
extraction at 128^3 cells, then the cell scaled by the square root of the ratio), the atlas is --tile texels per tile edge and
square-ish (atlasDefaultWidth), and GPU time between two events on the handle's stream is taken of
  (a) sdfr_atlas_bake, albedo layer: 16 + 4 bytes written per texel;
  (b) sdfr_atlas_bake, lit layer: 16 + 4 bytes;
  (c) sdfr_atlas_bake, albedo and lit: 32 + 4 bytes;
  (d) sdfr_atlas_texels: 24 + 4 bytes written per texel;
  (e) sdfr_mesh_surfaces over (d)'s texels, device records: 24 bytes read, 128 written;
  (f) sdfr_mesh_lighting over (d)'s texels, device records: 24 bytes read, 64 written.
(d) + (e) is the composition (a) replaces, (d) + (f) the one (b) replaces; they also need the 24 + 128 or 24 + 64 bytes of workspace per
texel that the fused call does not.  Each figure: after `warmup` calls, the median of `reps`, with [min, median, max].  Also: texels
per second of the fused calls and of the compositions (the medians added), and whether the lit plane equals the composition's records
bit for bit.  One process; run it under a time limit.  Prints one JSON object."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def spread(values):
    values = sorted(values)
    return [values[0], values[len(values) // 2], values[-1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="labyrinth:7,gems:7")
    ap.add_argument("--quads", type=int, default=100000)
    ap.add_argument("--tile", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    import sdf_playground_amd as sp
    from mesh_bench import BOXES

    L = sp.load_library()
    vp = ctypes.c_void_p

    def events(call):
        times = []
        for k in range(args.warmup + args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            if k >= args.warmup:
                times.append(a.elapsed_time(b))
        return spread(times)

    out = {"tile": args.tile, "reps": args.reps, "warmup": args.warmup, "configs": {}}
    for config in [c for c in args.configs.split(",") if c]:
        scene, _, ext = config.partition(":")
        r = sp.SDFRenderer(0)
        r.initShader(scene)
        r.setParameters(0.5)
        r.setLimits(extension_lights=int(ext or 0))
        r.setCamera(sp.Camera())
        origin, edge = BOXES.get(scene, ((-4.0, -0.5, -4.0), 8.0))
        cells = 128
        _p, _n, idx = r.extractMesh(origin, edge / cells, (cells,) * 3, device=True)
        first = idx.shape[0] // 2
        cells = max(8, min(1024, int(round(cells * (args.quads / max(first, 1)) ** 0.5))))
        cell = edge / cells
        pos, nrm, idx = r.extractMesh(origin, cell, (cells,) * 3, device=True)
        v, t = pos.shape[0], idx.shape[0]
        atlas = sp.atlasLayout(t, args.tile)
        w, h = atlas.width, atlas.height
        n = w * h
        reach = 2.0 * cell
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")  # noqa: E731
        albedo, lit, valid = f32(n, 4), f32(n, 4), torch.empty(n, dtype=torch.int32, device="cuda")
        tp, tn, tv = f32(n, 3), f32(n, 3), torch.empty(n, dtype=torch.int32, device="cuda")
        surfaces, lighting = f32(n, 32), f32(n, 16)
        A = ctypes.byref(atlas)
        mesh = (vp(pos.data_ptr()), vp(nrm.data_ptr()), vp(idx.data_ptr()))
        p = lambda a: vp(a.data_ptr())  # noqa: E731

        def bake(layers, pa, pl):
            return lambda: r._check(L.sdfr_atlas_bake(r._h, A, v, *mesh, reach, layers, pa, None, pl, p(valid), 0))

        res = {
            "bake_albedo_ms": events(bake(1, p(albedo), None)),
            "bake_lit_ms": events(bake(4, None, p(lit))),
            "bake_albedo_lit_ms": events(bake(5, p(albedo), p(lit))),
            "texels_ms": events(lambda: r._check(L.sdfr_atlas_texels(r._h, A, v, *mesh, p(tp), p(tn), p(tv), 0))),
            "mesh_surfaces_ms": events(lambda: r._check(L.sdfr_mesh_surfaces(r._h, n, p(tp), p(tn), reach, None, p(surfaces), 0))),
            "mesh_lighting_ms": events(lambda: r._check(L.sdfr_mesh_lighting(r._h, n, p(tp), p(tn), reach, None, p(lighting), None, 0))),
        }
        torch.cuda.synchronize()
        live = tv == 1
        hit = valid == 1
        same = (lit[:, :3].view(torch.int32) == lighting[:, 12:15].view(torch.int32)).all(1)
        med = lambda k: res[k][1]  # noqa: E731
        res.update({
            "cells": cells, "cell": cell, "vertices": v, "quads": t // 2, "width": w, "height": h, "texels": n, "tile_texels": int((tv != -1).sum()),
            "valid_texels": int(live.sum()), "hit_texels": int(hit.sum()),
            "lit_equals_the_composition": bool(same[hit].all()) and bool((lighting.view(torch.int32)[:, 0][live] == valid[live]).all()),
            "bytes_written_per_texel": {"bake_albedo": 20, "bake_lit": 20, "bake_albedo_lit": 36, "texels_then_surfaces": 28 + 128, "texels_then_lighting": 28 + 64},
            "bytes_read_per_texel_by_the_second_call": 24,
            "composition_albedo_ms": med("texels_ms") + med("mesh_surfaces_ms"), "composition_lit_ms": med("texels_ms") + med("mesh_lighting_ms"),
        })
        res["texels_per_second"] = {"bake_albedo": n / med("bake_albedo_ms") * 1e3, "bake_lit": n / med("bake_lit_ms") * 1e3,
                                    "bake_albedo_lit": n / med("bake_albedo_lit_ms") * 1e3, "composition_albedo": n / res["composition_albedo_ms"] * 1e3,
                                    "composition_lit": n / res["composition_lit_ms"] * 1e3}
        res["fused_over_composition"] = {"albedo": med("bake_albedo_ms") / res["composition_albedo_ms"], "lit": med("bake_lit_ms") / res["composition_lit_ms"]}
        out["configs"][config] = res
        del albedo, lit, valid, tp, tn, tv, surfaces, lighting, pos, nrm, idx
        r.close()
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

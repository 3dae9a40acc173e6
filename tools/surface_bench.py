"""Cost of the surface queries (sdfr_pick_surfaces, sdfr_mesh_surfaces) on the GPU, device memory out.

    python tools/surface_bench.py [--scenes labyrinth,lense] [--size 3840x2160] [--reps 20] [--warmup 3]
                                  [--mesh-scenes fast_sphere,labyrinth,tree] [--cells 256]

Per scene (the start-up camera, time 0.5, the reference's limits), GPU time between two events on the handle's stream:
  (a) sdfr_pick_surfaces of the whole frame (no pixel list: a wave per 8 x 8 tile), with and without hit records;
  (b) the yardstick: sdfr_pick of the same pixels given as a device list in row-major order -- the same marches, 48 bytes a pixel;
  (c) a device-to-device copy of as many bytes as (a) writes, 128 or 176 bytes a pixel;
  and sdfr_pick_surfaces of the same pixel list, which separates the tile mapping from the surface evaluation.
The expectation under test is (a) <= (b) + (c).  Per mesh scene, on mesh_bench.py's box of cells^3 cells: an extraction with normals
into device arrays with and without the surfaces at its vertices (host clock around the call and a sync: an extraction reads its
counts back), and sdfr_mesh_surfaces alone on the mesh left on the device (events).  With each, the march iterations of the items
(sdfr_hit.iterations): their mean, and the mean over waves of the slowest lane's, which is what a wave waits for.  Each figure:
after `warmup` calls, the median of `reps`, with [min, median, max].  Prints one JSON object."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def spread(values):
    values = sorted(values)
    return [values[0], values[len(values) // 2], values[-1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="labyrinth,lense")
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mesh-scenes", default="fast_sphere,labyrinth,tree")
    ap.add_argument("--cells", type=int, default=256)
    args = ap.parse_args()

    import torch
    import sdf_playground_amd as sp
    from mesh_bench import BOXES

    L = sp.load_library()
    w, h = (int(v) for v in args.size.lower().split("x"))
    n = w * h
    vp = ctypes.c_void_p

    def events(call):
        """ms between events around `call`, [min, median, max] over the timed repetitions"""
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

    out = {"width": w, "height": h, "reps": args.reps, "warmup": args.warmup, "frames": {}, "meshes": {}}
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.int32, device="cuda"), torch.arange(w, dtype=torch.int32, device="cuda"), indexing="ij")
    pixels = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1).contiguous()
    del xs, ys
    hits = torch.empty((n, 12), dtype=torch.float32, device="cuda")
    srf = torch.empty((n, 32), dtype=torch.float32, device="cuda")
    copy_src = torch.empty(176 * n, dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty(176 * n, dtype=torch.uint8, device="cuda")
    p_px, p_hits, p_srf = vp(pixels.data_ptr()), vp(hits.data_ptr()), vp(srf.data_ptr())
    for scene in [s for s in args.scenes.split(",") if s]:
        r = sp.SDFRenderer(0)
        r.initShader(scene)
        r.setParameters(0.5)
        cam = sp.Camera()
        cam.SetAspect(w / h)
        r.setCamera(cam)

        def ok(rc):
            r._check(rc)

        res = {
            "frame_surfaces_ms": events(lambda: ok(L.sdfr_pick_surfaces(r._h, w, h, n, None, None, p_srf, 0))),
            "frame_surfaces_hits_ms": events(lambda: ok(L.sdfr_pick_surfaces(r._h, w, h, n, None, p_hits, p_srf, 0))),
            "pick_list_ms": events(lambda: ok(L.sdfr_pick(r._h, w, h, n, p_px, p_hits, 0))),
            "list_surfaces_ms": events(lambda: ok(L.sdfr_pick_surfaces(r._h, w, h, n, p_px, None, p_srf, 0))),
            "list_surfaces_hits_ms": events(lambda: ok(L.sdfr_pick_surfaces(r._h, w, h, n, p_px, p_hits, p_srf, 0))),
            "copy_128_ms": events(lambda: copy_dst[:128 * n].copy_(copy_src[:128 * n], non_blocking=True)),
            "copy_176_ms": events(lambda: copy_dst[:176 * n].copy_(copy_src[:176 * n], non_blocking=True)),
        }
        torch.cuda.synchronize()
        valid = srf.view(torch.int32)[:, 3]
        res["hit_fraction"] = float((valid == 1).float().mean())
        # what a wave waits for: the march iterations of its slowest lane, for waves of 64 pixels of a row and of 8 x 8 tiles
        # (the frame cropped to whole waves of either shape)
        it = hits.view(torch.int32)[:, 8].reshape(h, w)[:h // 8 * 8, :w // 64 * 64].float()
        res["iterations"] = {"mean": float(it.mean()), "mean_of_wave_max_rows": float(it.reshape(-1, 64).max(1).values.mean()),
                             "mean_of_wave_max_tiles": float(it.reshape(it.shape[0] // 8, 8, it.shape[1] // 8, 8).permute(0, 2, 1, 3).reshape(-1, 64).max(1).values.mean())}
        a, b, c128, c176 = (res[k][1] for k in ("frame_surfaces_ms", "pick_list_ms", "copy_128_ms", "copy_176_ms"))
        res["expectation_a_le_b_plus_c"] = {"without_hits": [a, b + c128, a <= b + c128],
                                            "with_hits": [res["frame_surfaces_hits_ms"][1], b + c176, res["frame_surfaces_hits_ms"][1] <= b + c176]}
        out["frames"][scene] = res
        r.close()
    del pixels, hits, srf, copy_src, copy_dst
    torch.cuda.empty_cache()

    cells = args.cells
    for scene in [s for s in args.mesh_scenes.split(",") if s]:
        origin, edge = BOXES.get(scene, ((-4.0, -0.5, -4.0), 8.0))
        cell = edge / cells
        r = sp.SDFRenderer(0)
        r.initShader(scene)
        r.setParameters(0.5)
        r.setCamera(sp.Camera())

        def wall(surfaces):
            times = []
            for k in range(args.warmup + args.reps):
                r.sync()
                t0 = time.perf_counter()
                mesh = r.extractMesh(origin, cell, (cells, cells, cells), device=True, surfaces=surfaces)
                r.sync()
                if k >= args.warmup:
                    times.append((time.perf_counter() - t0) * 1e3)
            return spread(times), mesh

        plain_ms, _mesh = wall(False)
        with_ms, (pos, nrm, _idx, msrf) = wall(True)
        v = int(pos.shape[0])
        alone = events(lambda: r._check(L.sdfr_mesh_surfaces(r._h, v, vp(pos.data_ptr()), vp(nrm.data_ptr()), 2.0 * cell, None, vp(msrf.data_ptr()), 0)))
        mhits = torch.empty((v, 12), dtype=torch.float32, device="cuda")
        r._check(L.sdfr_mesh_surfaces(r._h, v, vp(pos.data_ptr()), vp(nrm.data_ptr()), 2.0 * cell, vp(mhits.data_ptr()), vp(msrf.data_ptr()), 0))
        torch.cuda.synchronize()
        it = mhits.view(torch.int32)[:v // 64 * 64, 8].float()
        out["meshes"][scene] = {"origin": origin, "cell": cell, "vertices": v, "extract_ms": plain_ms, "extract_with_surfaces_ms": with_ms,
                                "mesh_surfaces_alone_ms": alone, "valid_fraction": float((msrf.view(torch.int32)[:, 3] == 1).float().mean()),
                                "iterations": {"mean": float(it.mean()), "max": float(it.max()), "mean_of_wave_max": float(it.reshape(-1, 64).max(1).values.mean())}}
        del pos, nrm, _idx, msrf, _mesh, mhits
        r.close()
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

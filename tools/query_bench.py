"""Throughput of the scene queries (sdfr_query_distance, sdfr_query_rays, sdfr_pick) on the GPU, device memory in and out.

    python tools/query_bench.py [--n 8388608] [--reps 20] [--warmup 3]

Per scene (fast_sphere, labyrinth, lense, tree; the start-up camera, time 0.5): points/s of distance queries without and with
normals at n points spread over a box around the scene, rays/s of ray queries from the camera into its view cone in random order
(no screen coherence), picks/s of every pixel of a 3840 x 2160 frame in raster order, and for comparison the rays/s of a 4K
render of the same view (every ray of its pixels: primary, shadow and secondary).  Each figure: device events around one call,
after `warmup` calls, median of `reps`.  Prints one JSON object."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps, warmup):
    import torch

    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="fast_sphere,labyrinth,lense,tree")
    args = ap.parse_args()

    import torch
    import sdf_playground_amd as sp

    r = sp.SDFRenderer(0)  # queries run on the handle's stream: the default stream, which the events above are recorded on
    n = args.n
    g = torch.Generator(device="cuda").manual_seed(1)
    W, H = 3840, 2160
    ys, xs = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.int32), torch.arange(W, device="cuda", dtype=torch.int32), indexing="ij")
    pixels = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1).contiguous()
    out = {"n": n, "reps": args.reps, "warmup": args.warmup, "pick_frame": [W, H], "scenes": {}}
    for scene in args.scenes.split(","):
        r.initShader(scene)
        r.setParameters(0.5)
        cam = sp.Camera()
        cam.SetAspect(W / H)
        r.setCamera(cam)
        eye = torch.tensor(r.getCameraBasis()[0], device="cuda")
        basis = torch.tensor(r.getCameraBasis(), device="cuda")
        pts = (torch.rand((n, 3), generator=g, device="cuda") * torch.tensor([8.0, 4.0, 8.0], device="cuda") - torch.tensor([4.0, 0.0, 2.0], device="cuda")).contiguous()
        dist = torch.empty(n, device="cuda")
        nrm = torch.empty((n, 3), device="cuda")
        s = torch.rand((n, 2), generator=g, device="cuda") * 2 - 1
        dirs = basis[1][None] + s[:, :1] * basis[2][None] + s[:, 1:] * basis[3][None]
        dirs = (dirs / dirs.norm(dim=1, keepdim=True)).contiguous()
        origins = eye[None].expand(n, 3).contiguous()
        hits = torch.empty((n, 12), device="cuda")
        phits = torch.empty((W * H, 12), device="cuda")
        ms_pts = median_ms(lambda: r.queryDistance(pts, out=dist), args.reps, args.warmup)
        ms_nrm = median_ms(lambda: r.queryDistance(pts, normals=True, out=dist, out_normals=nrm), args.reps, args.warmup)
        ms_rays = median_ms(lambda: r.queryRays(origins, dirs, out=hits), args.reps, args.warmup)
        ms_pick = median_ms(lambda: r.pick(pixels, W, H, out=phits), args.reps, args.warmup)
        img = torch.empty((H, W, 4), device="cuda")
        ms_render = median_ms(lambda: r.render(None, W, H, out=img), args.reps, args.warmup)
        rays_rendered = int(r.getStats().rays)
        hit_frac = float((hits[:, 10].view(torch.int32) == 1).float().mean())
        out["scenes"][scene] = {
            "points_per_s": n / (ms_pts * 1e-3), "points_with_normals_per_s": n / (ms_nrm * 1e-3),
            "rays_per_s": n / (ms_rays * 1e-3), "ray_hit_fraction": hit_frac, "picks_per_s": W * H / (ms_pick * 1e-3),
            "render_4k_ms": ms_render, "render_rays_per_s": rays_rendered / (ms_render * 1e-3),
            "ms": {"points": ms_pts, "points_normals": ms_nrm, "rays": ms_rays, "pick_4k": ms_pick},
        }
        assert math.isfinite(ms_pts)
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

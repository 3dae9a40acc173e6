"""The kernels one handle launches for a fixed tour of the entry points, as (kernel name, grid, workgroup size) in launch order: what a
host-side change of the launch path must leave as it was.

    rocprofv3 --kernel-trace -d <dir> --output-format csv -- python tools/kernel_sequence.py run        (or: queries)
    python tools/kernel_sequence.py list <dir>  >  sequence.txt        (then diff two of them)

run: for the labyrinth and then for a run-time scene (scenes/noise_lod.hlsl) -- a 64 x 64 render, one query of each kind over 1000
items, one extraction of a 16^3-cell mesh with normals, one factor-2 sdfr_render_aa of 64 x 64; host arrays throughout.
queries: for the same two scenes -- a 64 x 64 render, one call of each query entry point (the G-buffer of a 9 x 7 frame among them)
over 1000 items with host arrays and then with device tensors, one extraction of a 16^3-cell mesh.
list: the kernel trace(s) under <dir>, one dispatch per line."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run():
    import numpy as np
    import sdf_playground_amd as sp

    rng = np.random.default_rng(3)
    pts = rng.uniform(-3, 3, (1000, 3)).astype(np.float32)
    dirs = rng.normal(size=(1000, 3)).astype(np.float32)
    px = np.stack([rng.integers(0, 64, 1000), rng.integers(0, 64, 1000)], 1).astype(np.int32)
    r = sp.SDFRenderer(0)
    for scene in ("labyrinth", "noise_lod"):
        if scene == "labyrinth":
            r.initShader(scene)
        else:
            r.initShaderHlsl(scene, os.path.join(ROOT, "sdf_playground_amd", "scenes", scene + ".hlsl"))
        r.setParameters(0.5)
        r.render(None, 64, 64)
        r.queryDistance(pts, normals=True)
        r.queryRays(pts, dirs)
        r.pick(px, 64, 64)
        pos, _nrm, idx = r.extractMesh((-2.0, -0.5, -2.0), 0.25, (16, 16, 16))
        r.renderAA(None, 64, 64, factor=2)
        print("%s: %d vertices, %d triangles" % (scene, len(pos), len(idx)))
    r.close()


def queries():
    import numpy as np
    import torch
    import sdf_playground_amd as sp

    rng = np.random.default_rng(3)
    pts = rng.uniform(-3, 3, (1000, 3)).astype(np.float32)
    dirs = rng.normal(size=(1000, 3)).astype(np.float32)
    px = np.stack([rng.integers(0, 64, 1000), rng.integers(0, 64, 1000)], 1).astype(np.int32)
    r = sp.SDFRenderer(0)
    for scene in ("labyrinth", "noise_lod"):
        if scene == "labyrinth":
            r.initShader(scene)
        else:
            r.initShaderHlsl(scene, os.path.join(ROOT, "sdf_playground_amd", "scenes", scene + ".hlsl"))
        r.setParameters(0.5)
        r.render(None, 64, 64)
        for device in (False, True):
            p, d, x = (torch.from_numpy(a).cuda() for a in (pts, dirs, px)) if device else (pts, dirs, px)
            r.queryDistance(p, normals=True)
            hits = r.queryRays(p, d)
            r.pick(x, 64, 64)
            r.queryRaySurfaces(p, d, hits=True)
            r.pickSurfaces(x, 64, 64)
            r.pickSurfaces(None, 9, 7, hits=True, device=device)
            r.meshSurfaces(p, d, 0.25)
            r.queryOcclusion(p, d, 0.01, 1.0)
            r.hitOcclusion(hits, 0.01, 1.0)
            r.sync()
        pos, _nrm, idx = r.extractMesh((-2.0, -0.5, -2.0), 0.25, (16, 16, 16))
        print("%s: %d vertices, %d triangles" % (scene, len(pos), len(idx)))
    r.close()


def listing(where):
    rows = []
    for path in glob.glob(os.path.join(where, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda d: int(d["Dispatch_Id"]))
    for d in rows:
        print("%s grid %s %s %s workgroup %s %s %s" % ((d["Kernel_Name"],) + tuple(d[k + a] for k in ("Grid_Size_", "Workgroup_Size_") for a in "XYZ")))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 2 and sys.argv[1] == "queries":
        queries()
    elif len(sys.argv) == 3 and sys.argv[1] == "list":
        listing(sys.argv[2])
    else:
        sys.exit(__doc__)

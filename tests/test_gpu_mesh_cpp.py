"""GPU tier: one sdfr_mesh_extract through the C++ mirror (include/sdfr.hpp) from a plain g++ program (tests/cpp/host_mesh.cpp),
equal to what the Python class returns for the same grid."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_extracts_the_same_mesh(tmp_path):
    import sdf_playground_amd as sp

    exe, out = str(tmp_path / "host_mesh"), str(tmp_path / "mesh.raw")
    libdir = os.path.dirname(sp.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "host_mesh.cpp"),
                    "-L" + libdir, "-lsdfr", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    scene, stime, origin, cell, dims, iso = "sierpinski", 0.5, (-1.85, -0.3, -1.05), 0.1, (37, 29, 21), 0.02
    args = [exe, scene, repr(stime)] + [repr(v) for v in origin] + [repr(cell)] + [str(d) for d in dims] + [repr(iso), out]
    env = dict(os.environ, LD_LIBRARY_PATH=libdir + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    run = subprocess.run(args, capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    raw = np.fromfile(out, np.uint8)
    v, t = (int(x) for x in raw[:16].view(np.int64))
    assert v > 500 and t > 500 and raw.size == 16 + 24 * v + 12 * t
    pos = raw[16:16 + 12 * v].view(np.uint32).reshape(v, 3)
    nrm = raw[16 + 12 * v:16 + 24 * v].view(np.uint32).reshape(v, 3)
    idx = raw[16 + 24 * v:].view(np.uint32).reshape(t, 3)
    r = sp.SDFRenderer(0)
    try:
        r.initShader(scene)
        r.setParameters(stime)
        p_ref, n_ref, i_ref = r.extractMesh(origin, cell, dims, iso=iso)
    finally:
        r.close()
    assert np.array_equal(pos, p_ref.view(np.uint32)) and np.array_equal(nrm, n_ref.view(np.uint32)) and np.array_equal(idx, i_ref)

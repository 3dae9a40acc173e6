"""Generates the committed fixtures that stand in for the reference tree in tests/ (data only, never its sources).

The tests run where the reference checkout is absent (a clean checkout, the GPU box), so what they compare against is
frozen here, once, from the reference tree:
  tests/golden/reference/camera.npz       the reference's own Camera.cpp / Math3D.cpp (oracle/_ref, compiled from that checkout) on 200
                                          seeded cameras, look-at and direction: inputs and the 12 basis floats
  tests/golden/reference/var_tags.json    the VAR_ tags of the driver and of every scene file (Engine/shader): name -> min, max,
                                          start, step, as the reference's parser reads them (the oracle's restatement of it)
  tests/golden/reference/screenshots/    a fixed sample of each screenshot the fits of reference_images.json were made on, one
                                          file per screenshot: every 16th row (tools/fit_reference_images.py: sample_rows), RGB
                                          and edge flag; the statistics of the oracle on it go into reference_images.json
                                          ("sample_stats")
  tests/golden/reference/scene_renders.json  every scene file of the reference (Engine/shader/scenes), translated from its own
                                          dialect and rendered on the CPU around the product's per-pixel pipeline (tests/hostsim)
                                          at a default and a moved camera with moved variables -- checked here against the oracle,
                                          bit for bit -- frozen as the frame, the slot order of the generated class and SHA-256
                                          digests of the pixels and of the ray / step / hit counters

  python tools/make_reference_fixtures.py --reference DIR
"""
import argparse
import glob
import hashlib
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import pyoracle as po  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CAMERA_SEED, CAMERA_CASES = 7, 200
SCENE_SEED = 2026
FOVY = np.float32(60.0) * np.float32(3.14159265358979) / np.float32(180.0)


def camera_cases():
    """The seeded inputs of the camera comparison: (eye, target, fovy, aspect, roll) x CAMERA_CASES."""
    rng = np.random.default_rng(CAMERA_SEED)
    eye, tgt, fovy, aspect, roll = [], [], [], [], []
    for k in range(CAMERA_CASES):
        eye.append(rng.uniform(-8, 8, 3).astype(np.float32))
        tgt.append(rng.uniform(-8, 8, 3).astype(np.float32))
        fovy.append(np.float32(rng.uniform(0.3, 2.0)))
        aspect.append(np.float32(rng.uniform(0.5, 2.5)))
        roll.append(np.float32(0.0 if k % 2 == 0 else rng.uniform(-1, 1)))
    return np.array(eye), np.array(tgt), np.array(fovy, np.float32), np.array(aspect, np.float32), np.array(roll, np.float32)


def make_camera():
    ref = po.ref_camera_lib()
    assert ref is not None, "oracle/_ref not built"
    eye, tgt, fovy, aspect, roll = camera_cases()
    basis = np.zeros((CAMERA_CASES, 2, 12), np.float32)  # [case, look-at / direction, eye front right top]
    for k in range(CAMERA_CASES):
        for is_dir in (0, 1):
            ref.ref_camera_basis(eye[k].ctypes.data, tgt[k].ctypes.data, is_dir, fovy[k], aspect[k], roll[k], basis[k, is_dir].ctypes.data)
    np.savez_compressed(os.path.join(GOLDEN, "reference", "camera.npz"), eye=eye, target=tgt, fovy=fovy, aspect=aspect, roll=roll, basis=basis)


def make_var_tags(reference):
    from sdf_playground_amd.cli import parse_var_tags

    def tags(path):
        text = open(path).read()
        mine, ref = parse_var_tags(text), po.parse_vars(text)
        assert list(mine) == list(ref), path
        out = {}
        for k, v in ref.items():
            assert tuple(np.float32(x) for x in mine[k]) == tuple(np.float32(x) for x in v[:4]), (path, k)
            out[k] = [float(x) for x in v[:4]]
        return out

    shader = os.path.join(reference, "Engine", "shader")
    scenes = {}
    for path in sorted(glob.glob(os.path.join(shader, "scenes", "sdf_scene_*.hlsl"))):
        scenes[os.path.basename(path)[len("sdf_scene_"):-len(".hlsl")]] = tags(path)
    doc = {"_comment": "VAR_ tags (name: min, max, start, step) of the reference's Engine/shader/pshader_sdf.hlsl (driver) and of every "
                       "Engine/shader/scenes/sdf_scene_<stem>.hlsl, as its ShaderVariableManager::parseFile reads them; made by "
                       "tools/make_reference_fixtures.py",
           "driver": tags(os.path.join(shader, "pshader_sdf.hlsl")), "scenes": scenes}
    with open(os.path.join(GOLDEN, "reference", "var_tags.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def make_screenshots(reference):
    import fit_reference_images as fr

    fr.IMAGES = os.path.join(reference, "Images")
    path = os.path.join(GOLDEN, "reference_images.json")
    with open(path) as f:
        doc = json.load(f)
    samples = os.path.join(GOLDEN, "reference", "screenshots")
    os.makedirs(samples, exist_ok=True)
    for name, (file, _scene, _g, _v) in sorted(fr.TARGETS.items()):
        r0 = fr.ROWS_FROM.get(name, 0)
        ref8 = fr.load_reference(name)[r0:]
        rows = fr.sample_rows(fr.H - r0)
        rgb, edge = ref8[rows], fr.edges(ref8.astype(np.int32))[rows]
        np.savez_compressed(os.path.join(samples, fr.sample_name(file)), **fr.encode_sample(rgb, edge))  # (multi-lights.png: two targets, one file)
        back, back_edge = fr.load_sample(samples, file)
        assert np.array_equal(back, rgb) and np.array_equal(back_edge, edge), file
    for name, e in doc["images"].items():
        p = list(e["eye"]) + [e["yaw"], e["pitch"], e["stime"]]
        e["sample_stats"], _d = fr.compare_sample(name, p, samples, variables=e.get("variables", {}))
        print(name, json.dumps(e["sample_stats"]))
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def frame_to_dict(f):
    return {name: (list(getattr(f, name)) if hasattr(getattr(f, name), "__len__") else getattr(f, name)) for name, _t in po.OrcFrame._fields_}


def frame_from_dict(d):
    f = po.OrcFrame()
    for name, v in d.items():
        if isinstance(v, list):
            for i, x in enumerate(v):
                getattr(f, name)[i] = x
        else:
            setattr(f, name, v)
    return f


def render_digests(img, st):
    """SHA-256 of a frame's pixels (every NaN as one bit pattern) and of its per-pixel ray / step / hit counters."""
    img = np.where(np.isnan(img), np.float32(np.nan), img).astype(np.float32)
    return {"rgba_sha256": hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest(),
            "stats_sha256": hashlib.sha256(np.ascontiguousarray(st, dtype=np.uint32).tobytes()).hexdigest()}


def make_scene_renders(reference):
    import hostsim

    paths = sorted(glob.glob(os.path.join(reference, "Engine", "shader", "scenes", "sdf_scene_*.hlsl")))
    names = [os.path.basename(p)[len("sdf_scene_"):-len(".hlsl")] for p in paths]
    texts = [open(p).read() for p in paths]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        libs = list(ex.map(lambda nt: hostsim.build_hlsl("ref_" + nt[0], nt[1]), zip(names, texts)))
    rng = np.random.default_rng(SCENE_SEED)
    scenes = {}
    for name, (L, slots) in zip(names, libs):
        table = po.var_table(name)
        assert slots == [r[0] for r in sorted(table, key=lambda r: r[6]) if r[6] >= 0], name
        heavy = name in ("tree", "terrain", "distortion", "tiling")
        w, h = (40, 28) if heavy else (72, 48)
        cases = []
        for k in range(2):
            if k == 0:
                f = po.default_frame(name, w, h, stime=0.5)
            else:
                eye = (float(rng.uniform(-5, 5)), float(rng.uniform(0.4, 5)), float(rng.uniform(-6, -2)))
                f = po.default_frame(name, w, h, basis=po.camera_lookat(eye, (0.0, 1.0, 0.0), FOVY, np.float32(w) / np.float32(h)), stime=1.7)
                for _vname, mn, mx, _start, _step, _v, slot in table:
                    if slot >= 0:
                        f.scene_var[slot] = float(np.float32(rng.uniform(mn, mx)))
                f.max_cost_default = 9
                f.debug_ny, f.debug_y = (1.0, 0.6) if name == "cube" else (0.0, 0.0)  # once through the debug-plane build
            img, st = hostsim.render_hlsl(L, hostsim.frame_from_oracle(f))
            ref, rst, _ = po.render(name, f, stats=True)
            assert render_digests(img, st) == render_digests(ref, rst), (name, k)  # the reference's text renders the oracle's bits
            cases.append(dict(frame=frame_to_dict(f), **render_digests(img, st)))
        scenes[name] = {"slots": slots, "cases": cases}
    doc = {"_comment": "Every Engine/shader/scenes/sdf_scene_<stem>.hlsl of the reference, translated from its dialect (sdfr_hlsl.h) and "
                       "rendered on the CPU around the product's per-pixel pipeline (tests/hostsim): slots = the variables the generated "
                       "class reads, in order; per case the frame (oracle/pyoracle.py OrcFrame) and SHA-256 of the RGBA float32 pixels "
                       "(NaN as one bit pattern) and of the uint32 ray / step / hit counters.  Made by tools/make_reference_fixtures.py",
           "scenes": scenes}
    with open(os.path.join(GOLDEN, "reference", "scene_renders.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout (Engine/, Images/)")
    a = ap.parse_args()
    # the oracle, and oracle/_ref: the reference's Camera.cpp / Math3D.cpp compiled from the checkout given
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "liboracle.so", "ref", "REF=" + os.path.abspath(a.reference)], check=True)
    import sdf_playground_amd as sp

    sp.build()  # libsdfr.so: the dialect's translator (sdfr_translate_scene_hlsl) for the scene renders
    os.makedirs(os.path.join(GOLDEN, "reference"), exist_ok=True)
    make_camera()
    make_var_tags(a.reference)
    make_screenshots(a.reference)
    make_scene_renders(a.reference)


if __name__ == "__main__":
    main()

"""Cameras, cases and oracle frames that a CPU test file and GPU test files share: the diagnostic scenes "normal_test" and
"debug_materials" (tests/test_normal_cpu.py, test_debug_materials_cpu.py and their GPU tiers) and the two dialect scenes with oracle
twins (tests/test_hlsl_cpu.py, test_gpu_hlsl.py).  `oracle` is the oracle fixture's module.  Test infrastructure: the product never
imports this."""
import numpy as np

FOVY = np.float32(60.0) * np.float32(3.14159265358979) / np.float32(180.0)


def lookat_frame(oracle, scene, cam, w, h, stime, **kw):
    """the scene's default frame from cam = (eye, look-at); kw: scene variables by name, else fields of the frame"""
    f = oracle.default_frame(scene, w, h, basis=oracle.camera_lookat(cam[0], cam[1], FOVY, np.float32(w) / np.float32(h)), stime=stime)
    slots = {r[0]: r[6] for r in oracle.var_table(scene)}
    for k, v in kw.items():
        if k in slots and slots[k] >= 0:
            f.scene_var[slots[k]] = v
        else:
            setattr(f, k, v)
    return f


# ---- normal_test ----------------------------------------------------------------------------------------------------------------------
NORMAL_W, NORMAL_H = 120, 80
NORMAL_CAMS = [((0.2, 2.2, -4.6), (0.0, 0.5, -0.2)), ((3.2, 1.1, -2.4), (1.2, 0.5, -0.3)), ((-3.4, 1.5, -1.6), (-1.2, 0.6, 0.1)), ((0.8, 5.0, -0.9), (0.6, 0.0, -0.5))]
EPS_DEFAULT = dict(dist_eps=0.0001, grad_eps=0.0001, reflect_eps=0.001, refract_eps=0.001, shadow_eps=0.0003)
EPS_OTHER = dict(dist_eps=0.0005, grad_eps=0.002, reflect_eps=0.004, refract_eps=0.0025, shadow_eps=0.0011)


def normal_frame(oracle, scene, cam, stime=0.4, w=NORMAL_W, h=NORMAL_H, **kw):
    return lookat_frame(oracle, scene, cam, w, h, stime, **kw)


# ---- debug_materials ------------------------------------------------------------------------------------------------------------------
MATERIALS_W, MATERIALS_H = 96, 64
MATERIALS_CAMS = [((0.0, 1.6, -4.2), (0.0, 0.6, 0.0)), ((-3.5, 0.9, -2.0), (-0.6, 0.5, 0.0)), ((0.3, 4.0, -0.8), (0.3, 0.5, 0.0))]


def materials_frame(oracle, cam, iter_count, stime=0.4, **kw):
    f = oracle.default_frame("debug_materials", MATERIALS_W, MATERIALS_H, stime=stime,
                             basis=oracle.camera_lookat(cam[0], cam[1], FOVY, np.float32(MATERIALS_W) / np.float32(MATERIALS_H)))
    f.iter_count = iter_count
    for k, v in kw.items():
        setattr(f, k, v)
    return f


# ---- the dialect scenes with oracle twins ---------------------------------------------------------------------------------------------
# cameras: (eye, lookat)
TWIN_CAMS = [((0.0, 2.0, -5.0), (0.0, 1.0, 0.0)), ((4.5, 1.2, -3.5), (0.5, 0.8, 0.5)), ((-3.0, 4.0, 4.5), (0.0, 0.6, 1.0)), ((0.3, 0.4, -14.0), (0.0, 1.0, 0.0))]
TWIN_CASES = {
    # 2-D / 4-D simplex noise, grad4; camera_distance and the ray offsets read in the geometry step (pshader_sdf.hlsl:187-218)
    "noise_lod": [dict(), dict(lod=3.0, freq=6.5, bump=0.04), dict(lod=40.0, stime=3.9, max_cost_default=9), dict(debug_ny=1.0, debug_y=0.8)],
    # swizzled l-values, inout swizzles, float3x3 + mul, static const initialisers, saturating (int), a voronoi overload, VAR_ quirks
    "dialect_tour": [dict(), dict(spin=-1.3, reach=2.7, blend=0.25, shine=0.8), dict(stime=5.2, extension_lights=5, max_cost_default=9), dict(debug_nx=1.0, debug_x=0.3)],
}


def twin_frame(oracle, scene, cam, w=96, h=64, stime=0.7, **extra):
    return lookat_frame(oracle, scene, cam, w, h, stime, **extra)

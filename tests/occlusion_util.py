"""Shared by the occlusion tests (test_occlusion_cpu.py, test_gpu_occlusion.py): the oracle's definition of the occlusion record
(tests/cpp/occlusion_oracle.h), the library's occlusion functions built for the CPU (tests/cpp/occlusion_host.cpp), the items the
tests ask about and a scene whose answer is known without either.  Frames, ray samples and the bit comparison are query_util's.
Test infrastructure: the product never imports this."""
import ctypes

import numpy as np

import query_util as qu

OCCLUSION_WORDS = 4
BIAS, RADIUS = 0.01, 1.0

# A floor (y = 0) with a wall (x = 0) on its -x side, in the run-time dialect: the answer at a point of the floor is known from
# the direction table alone (wall_expectation)
FLOOR_AND_WALL = """#include "sdf_primitives.hlsl"
#include "sdf_common.hlsl"

void map(GeometryInput geometry, MarchingInput march, MaterialInput material_input, inout MaterialOutput material_output, bool geometry_step, inout float output_scene_distance)
{
	float d = min(geometry.pos.y, geometry.pos.x);
	if (geometry_step)
	{
		OBJECT(d);
	}
	else if (MATERIAL(d))
	{
		material_output.diffuse_color = float4(0.5f, 0.5f, 0.5f, 1.f);
	}
}

void map_normal(GeometryInput geometry, inout NormalOutput output)
{
}

void map_light(GeometryInput input, inout LightOutput output[LIGHT_COUNT], inout float ambient_lighting_factor)
{
	output[0].used = true;
	output[0].pos = float4(-1.f, -1.f, 2.f, 1.f);
	output[0].color = float3(1.f, 1.f, 1.f);
}

float3 map_background(float3 dir, uint iter_count)
{
	return float3(0.f, 0.f, 0.f);
}
"""

def oracle_lib():
    L = qu.build_oracle_lib()
    vp, cf = ctypes.c_void_p, ctypes.c_float
    L.oo_points.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, vp, vp, cf, cf, vp]
    L.oo_hits.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, vp, cf, cf, vp]
    L.oo_directions.argtypes = [vp]
    return L


def host_lib(scene, text=None):
    """The library's occlusion functions for the CPU; `text`: the dialect text of a run-time scene that is no file"""
    L = qu.build_host_lib("occlusion_host", "occlusion_host.cpp", scene, text)
    vp, cf = ctypes.c_void_p, ctypes.c_float
    L.oh_occlusion.argtypes = [ctypes.c_char_p, vp, ctypes.c_int, vp, vp, vp, cf, cf, vp]
    L.oh_directions.argtypes = [vp]
    return L


def _f3(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def oracle_points(scene, of, points, normals, bias=BIAS, radius=RADIUS):
    """[n, 4] uint32 words of sdfr_occlusion"""
    p, nr = _f3(points), _f3(normals)
    out = np.empty((len(p), OCCLUSION_WORDS), np.uint32)
    assert oracle_lib().oo_points(scene.encode(), ctypes.byref(of), len(p), qu._p(p), qu._p(nr), bias, radius, qu._p(out)) == 0
    return out


def oracle_hits(scene, of, hits, bias=BIAS, radius=RADIUS):
    h = qu.hits_array(hits)
    out = np.empty((len(h), OCCLUSION_WORDS), np.uint32)
    assert oracle_lib().oo_hits(scene.encode(), ctypes.byref(of), len(h), qu._p(h), bias, radius, qu._p(out)) == 0
    return out


def host_points(scene, U, points, normals, bias=BIAS, radius=RADIUS, text=None):
    p, nr = _f3(points), _f3(normals)
    out = np.empty((len(p), OCCLUSION_WORDS), np.uint32)
    assert host_lib(scene, text).oh_occlusion(scene.encode(), ctypes.byref(U), len(p), qu._p(p), qu._p(nr), None, bias, radius, qu._p(out)) == 0
    return out


def host_hits(scene, U, hits, bias=BIAS, radius=RADIUS):
    h = qu.hits_array(hits)
    out = np.empty((len(h), OCCLUSION_WORDS), np.uint32)
    assert host_lib(scene).oh_occlusion(scene.encode(), ctypes.byref(U), len(h), None, None, qu._p(h), bias, radius, qu._p(out)) == 0
    return out


def host_directions():
    d = np.empty((64, 3), np.float32)
    host_lib("fast_sphere").oh_directions(qu._p(d))
    return d


def occlusion_array(o):
    """OCCLUSION_DTYPE records, a device tensor's copy or [n, 4] 32-bit words -> [n, 4] uint32"""
    return np.ascontiguousarray(o).view(np.uint32).reshape(-1, OCCLUSION_WORDS)


def hit_items(scene, of, seed, n):
    """the oracle's hit records [n, 12] of n of query_util's rays: hits and misses both"""
    o, d = qu.ray_samples(of, seed, n)
    return qu.oracle_rays(scene, of, o, d)


def points_of_hits(hits):
    """the same items as plain arrays: (points, normals), and which of them are items at all (hit == 1)"""
    h = qu.hits_array(hits)
    return h[:, 2:5].copy().view(np.float32), h[:, 5:8].copy().view(np.float32), h[:, 10] == 1


def well_formed(rec):
    """what the record promises whatever the scene"""
    rec = occlusion_array(rec)
    mask = rec[:, 0].astype(np.uint64) | (rec[:, 1].astype(np.uint64) << np.uint64(32))
    pop = np.array([bin(int(m)).count("1") for m in mask], np.uint32)
    assert np.array_equal(pop, rec[:, 2])
    valid = rec[:, 3].view(np.int32)
    assert np.isin(valid, (1, 0, -1)).all() and not rec[valid != 1][:, :3].any()


def partial_share(rec):
    """of the valid items, the share with 0 < occluded < 64"""
    rec = occlusion_array(rec)
    v = rec[rec[:, 3] == 1]
    return float(((v[:, 2] > 0) & (v[:, 2] < 64)).mean()) if len(v) else 0.0


WALL_ITEM = (np.array([[0.5, 0.0, 0.0]], np.float32), np.array([[0.0, 1.0, 0.0]], np.float32))


def wall_expectation(table):
    """FLOOR_AND_WALL at WALL_ITEM with bias 0.01, radius 1: the normal (0, 1, 0) gives world direction (D[k][0], D[k][2], -D[k][1]), which
    rises off the floor and meets the wall x = 0 at t = 0.5 / -D[k][0]: bit k is set iff that is <= 1.  Returns (expected bits [64]
    bool, compared [64] bool): directions within 2 % of the radius are left out, the march ending within dist_eps of the wall."""
    d0 = table[:, 0].astype(np.float64)
    with np.errstate(divide="ignore"):
        t = np.where(d0 < 0, 0.5 / -d0, np.inf)
    return t <= 1.0, ~(np.abs(t - 1.0) < 0.02)


def mask_bits(rec):
    """[n, 64] bool of [n, 4] words"""
    rec = occlusion_array(rec)
    mask = rec[:, 0].astype(np.uint64) | (rec[:, 1].astype(np.uint64) << np.uint64(32))
    return ((mask[:, None] >> np.arange(64, dtype=np.uint64)[None]) & np.uint64(1)).astype(bool)

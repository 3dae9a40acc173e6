"""Builds libsdfr.so (C ABI + gfx950 kernels) in-tree with hipcc.

Every source is compiled to an object of its own, in parallel; the per-scene kernels (SCENE_SOURCES) are compiled
once per scene of the registry (-DSDFR_SCENE=<scene index>, scene_command), so that the build takes ~20 s on 8 cores
instead of a minute and a scene can have code-generation options of its own (SCENE_FLAGS below).

Flags that matter for correctness:
  -ffp-contract=off   only the explicit fma() calls fuse (arithmetic contract)
  -fno-slp-vectorize  no v_pk_*_f32: on gfx950 a packed fp32 op costs more issue time than the two
                      scalar ops it replaces (tools/ubench: pk_add 6.1 vs 2 x 2.5 cycles); measured at
                      4K: labyrinth -4 %, cube_sea -15 %, lense +5 %
  default hipcc fp32 divide/sqrt are correctly rounded and denormals are kept; do not add
  -ffast-math / -fgpu-flush-denormals-to-zero / -fno-hip-fp32-correctly-rounded-divide-sqrt.
"""
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libsdfr.so")
OBJDIR = os.path.join(HERE, "build")
SOURCES = ["sdfr_api.cpp", "sdfr_comm.cpp", "sdfr_components.hip", "sdfr_hlsl.cpp", "sdfr_jit.cpp", "sdfr_kernels.hip", "sdfr_mesh.hip", "sdfr_post.hip", "sdfr_resolve.hip", "sdfr_slice.hip"]
# the render kernels, and the query kernels in a unit of their own: both per scene, with the scene's options
SCENE_SOURCES = ["sdfr_kernels_scene.hip", "sdfr_query_scene.hip"]
ARCH = "gfx950"
# Per scene: options that change the register ASSIGNMENT or the instruction ORDER of its kernels, never the arithmetic.  A three-source
# instruction (v_fma_f32, v_fmac_f32) whose sources all lie in one VGPR bank (register number mod 4) issues at half rate on gfx950
# (tools/ubench/bank_ubench.hip, profiles/r03_bank_ubench.txt), the allocator does not know, and how many of a march loop's fma land
# that way is luck: tools/isa_loops.py counts them, and a scene whose default draw is a bad one gets another (each scene is a compile
# unit of its own).  Chosen by that count, kept where the GPU confirmed it (profiles/r03_launch_experiments.txt):
#   fractal 15 -> 4 of its march loop's 104 fma, coordinate_material, terrain (-2.0 / -1.1 / -1.9 % at 4K), tiling (-4 %): local live ranges
#   assigned shortest first; cube_sea 4 -> 2 of 33 (BASELINE configuration 2 -2.1 %), shell (-2 %): scheduler strategy max-memory-clause;
#   lense 12 -> 0 of 79 (configuration 5 -0.9 %): top-down pre-RA scheduling (which costs distortion 12 %, hence per scene).
_REV = ["-mllvm", "-greedy-reverse-local-assignment"]
_MAXMEM = ["-mllvm", "-amdgpu-sched-strategy=max-memory-clause"]
_TOPDOWN = ["-mllvm", "-misched-prera-direction=topdown"]
_MAXILP = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]
# round 4 (tools/flag_search.py, gpurun_out/r04/s14): the fractal's 104-fma march loop draws 1 one-bank fma under max-ilp (4 under the reversed
# local assignment it had, 15 by default): BASELINE configuration 4 1.044 / 1.048 -> 1.031 / 1.025 ms (-1.7 %), 20 bytes more scratch
# outside the loop.  The same search left the labyrinth (default draw: rev +0.8 %, top-down +3 %), gems (+-0) and cube_sea where they were.
SCENE_FLAGS = {"SceneFractal": _MAXILP, "SceneCoordinateMaterial": _REV, "SceneTerrain": _REV, "SceneTiling": _REV,
               "SceneCubeSea": _MAXMEM, "SceneShell": _MAXMEM, "SceneLense": _TOPDOWN}


def scene_registry():
    """[(index, struct name)] of the scenes compiled ahead of time (csrc/sdfr_perpixel.h)."""
    text = open(os.path.join(CSRC, "sdfr_perpixel.h")).read()
    return [(int(i), n) for i, n in re.findall(r"X\((\d+), (Scene\w+)\)", text)]


FLAGS = ["--offload-arch=" + ARCH, "-std=c++17", "-O3", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "-x", "hip", "-Wno-unused-result",
         "-Wno-unknown-pragmas", "-I" + CSRC]


def _hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def scene_command(scene, source, out, extra=(), own=None):
    """The hipcc command of one scene unit: `source` (one of SCENE_SOURCES) for `scene` (struct name) with the shipped options,
    then `extra`, then the scene's own options -- SCENE_FLAGS, or `own` instead where given -- writing `out`."""
    index = {name: i for i, name in scene_registry()}[scene]
    own = SCENE_FLAGS.get(scene, []) if own is None else own
    return ([_hipcc()] + FLAGS + list(extra) + ["-DSDFR_SCENE=%d" % index] + list(own)
            + [os.path.join(CSRC, source), "-o", out])


def _deps():
    # this file too: a change of the recipe (flags, units) is a change of the library
    return [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(os.path.dirname(HERE), "include", "sdfr.h"), os.path.abspath(__file__)]


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in _deps())


def build(force=False, verbose=False, extra=(), out=None, jobs=None, scene_flags=None):
    """Compile every HIP source for gfx950 into sdf_playground_amd/libsdfr.so (or `out`).
    scene_flags: {scene struct name: [flags]} instead of SCENE_FLAGS for those scenes (only their units differ from the default build)."""
    if out is None and not force and not _stale():
        return LIB
    hipcc = _hipcc()
    extra = list(extra)
    objdir = os.path.join(OBJDIR, hashlib.sha1(" ".join(extra).encode()).hexdigest()[:10] if extra else "default")
    os.makedirs(objdir, exist_ok=True)
    source_units, scene_units = [], []  # (object, command)
    for s in SOURCES:
        obj = os.path.join(objdir, s + ".o")
        source_units.append((obj, [hipcc] + FLAGS + extra + ["-c", os.path.join(CSRC, s), "-o", obj]))
    for i, name in scene_registry():
        own = (scene_flags or {}).get(name, SCENE_FLAGS.get(name, []))
        # other options than the scene's own: objects of their own, which a default build never reuses
        tag = "" if own == SCENE_FLAGS.get(name, []) else "." + hashlib.sha1(" ".join(own).encode()).hexdigest()[:8]
        for src in SCENE_SOURCES:
            obj = os.path.join(objdir, "%s.%d%s.o" % (src, i, tag))
            scene_units.append((obj, scene_command(name, src, obj, extra + ["-c"], own)))
    newest_dep = max(os.path.getmtime(d) for d in _deps())

    def compile_unit(u):
        obj, cmd = u
        if not force and os.path.exists(obj) and os.path.getmtime(obj) > newest_dep:
            return
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)

    # the scene units first: they are the long ones
    with ThreadPoolExecutor(max_workers=jobs or min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(compile_unit, scene_units + source_units))
    cmd = [hipcc, "--offload-arch=" + ARCH, "-fPIC", "-shared"] + [obj for obj, _cmd in source_units + scene_units] + ["-o", out or LIB]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    return out or LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose="-v" in sys.argv)
    print(LIB)

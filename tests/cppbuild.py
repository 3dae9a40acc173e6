"""The one way a test compiles C++: the flags that make a host build compute the kernels' bits, a compile step that rebuilds what
is stale and never leaves a half-written output, the dependency lists, and the include file of a run-time scene.  Test
infrastructure: the product never imports this."""
import glob
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "sdf_playground_amd", "csrc")
ORACLE = os.path.join(ROOT, "oracle")
BUILD = os.path.join(HERE, "cpp", "_build")

# The arithmetic contract of every host build that is compared with the kernels or the oracle bit for bit: no contraction of a
# multiply and an add the source keeps apart (the kernels are built with -ffp-contract=off too), the fmaf the source does write as
# the one instruction (-mfma; -mavx2 with it), and sqrtf and its kin as instructions, not calls that set errno.
EXACT_FLAGS = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-fno-math-errno", "-Wno-unknown-pragmas"]
# the plan programs: host arithmetic in integers, no HIP header on the include path, and no warning let through
PLAIN_FLAGS = ["-std=c++17", "-O2", "-Wall", "-Werror"]


def compile(out, sources, deps, flags, shared=True):
    """g++ `sources` into the library (or, shared=False, the program) `out`, if it is missing or older than a source or one of `deps`.
    The compiler writes out + ".tmp", which replaces `out` only when it is whole: a compile that fails or is interrupted leaves
    the previous `out` as it was, and raises.  -> out"""
    sources = list(sources)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in sources + list(deps)):
        tmp = out + ".tmp"
        try:
            subprocess.run(["g++"] + list(flags) + (["-shared"] if shared else []) + ["-o", tmp] + sources, check=True)
            os.replace(tmp, out)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    return out


def csrc_lib(name, source):
    """tests/cpp/_build/lib<name>.so: `source` over the product's headers, with EXACT_FLAGS alone"""
    return compile(os.path.join(BUILD, "lib%s.so" % name), [source], csrc_headers(), EXACT_FLAGS + ["-I" + CSRC])


def plan_program(source, name=None, flags=()):
    """tests/cpp/_build/<name>: the stand-alone program tests/cpp/<source>.cpp over the product's host headers, with PLAIN_FLAGS and `flags`"""
    return compile(os.path.join(BUILD, name or source), [os.path.join(HERE, "cpp", source + ".cpp")], csrc_headers(),
                   PLAIN_FLAGS + list(flags) + ["-I" + CSRC], shared=False)


def csrc_headers():
    """what anything that includes the product's headers depends on: every header of csrc"""
    return sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.inl")))


def oracle_headers():
    """likewise for the oracle's definitions"""
    return sorted(glob.glob(os.path.join(ORACLE, "*.h")))


def write_if_changed(path, text):
    """a generated source keeps its time stamp, and what was built from it stays fresh, while its text stays the same"""
    if not os.path.exists(path) or open(path).read() != text:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    return path


def scene_include(path, text, translate=None):
    """Writes the file a host build includes as its run-time scene (-DSDFR_HLSL_SCENE_FILE): the VAR_ macros, then translate(text), or
    `text` itself for a scene in the library's C++ form.  The macros are the ones the run-time compiler generates (sdfr_jit.cpp):
    VAR_<name>(...) reads U.scene_var[k], k = the order in which the names first appear in `text`.  -> the names, by slot"""
    slots = []
    for m in re.finditer(r"VAR_(\w+)\s*\(", text):
        if m.group(1) not in slots:
            slots.append(m.group(1))
    prelude = "".join("#define VAR_%s(...) (U.scene_var[%d])\n" % (n, k) for k, n in enumerate(slots))
    write_if_changed(path, prelude + (translate(text) if translate else text))
    return slots


def default_threads():
    """threads of a host render: the machine's CPUs, 16 at the most -- what a command gets on a shared machine, and the C++ stand-ins' cap"""
    return min(16, os.cpu_count() or 1)

"""How far sin1, cos1, sincos1, atan21, exp21, log21 and pow1 are from the functions they stand for: the sweep of
tests/cpp/math_accuracy_host.cpp (the host build of sdfr_math.h against libm in double), the table it is recorded in
(tests/golden/math_accuracy.json), and the arguments the scenes really feed to these functions (the oracle's census build).

    python tests/math_accuracy_util.py --write      sweeps, runs the census, and rewrites the table

Shared by tests/test_math_accuracy_cpu.py, tests/test_golden_cpu.py and tests/test_gpu_math_accuracy.py.  Test infrastructure: the
product never imports this."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np

import cppbuild

TABLE = os.path.join(cppbuild.HERE, "golden", "math_accuracy.json")
SOURCE = os.path.join(cppbuild.HERE, "cpp", "math_accuracy_host.cpp")

# the stated domain of sin1 / cos1 / sincos1: on it |result| <= 1 and the absolute error stays below ABS_BOUND
SINCOS_DOMAIN = 65536.0
ABS_BOUND = 3e-7
STRIDE, FAR_STRIDE = 1, 17  # every float of the swept ranges; every 17th of sin and cos between 2^16 and 2^26
# libm's own error: truth is exact to about 2^-29 of an fp32 ulp, so a later run may exceed a recorded figure by that much
ULP_SLACK = 2.0 ** -28

ROW_FUNCTIONS = ("sin1", "cos1", "atan21", "atan21_pairs", "exp21", "log21", "pow1")
ARGUMENTS = {
    "sin1": "x >= 0 (sin1(-x) = -sin1(x) bit for bit, asserted by the sweep): every float of [2^-14, 2^16); below, each binade's edges +-3 floats and 4096 "
            "hashed mantissas; from 2^16 to 2^26 every 17th float and the edges.  Rows are binades of x.",
    "cos1": "as sin1 (cos1(-x) = cos1(x) bit for bit)",
    "atan21": "atan21(y, 1): every float y of [2^-30, 2^30] (atan21(-y, 1) = -atan21(y, 1) and atan1(y) = atan21(y, 1) bit for bit).  Rows are binades of y.",
    "atan21_pairs": "2^24 hashed pairs of finite bit patterns (y, x), all four quadrants.  Rows are binades of |y / x|.",
    "exp21": "every float of 2^-24 <= |x| <= 150, both signs; the thresholds 128 and -126 lie inside.  Rows are sign and binade of x.",
    "log21": "every positive float, denormals included.  Rows are binades of x.",
    "pow1": "2^24 hashed pairs (x, y): x in (0, 4] uniform and log-uniform with y in [-128, 128); x in [0.5, 1 - 2^-23] with y in [1, 8192] (Blinn); "
            "x in (0, 1] with y in [0, 128).  Rows are binades of |y * log2 x|, the product the inner exp21 receives.",
}
# mah_eval / mah_truth
WHAT = {"sin1": 0, "cos1": 1, "atan21": 2, "exp21": 3, "log21": 4, "pow1": 5, "sincos1.x": 6, "sincos1.y": 7, "sincos1_small.x": 8, "sincos1_small.y": 9}


class _Row(ctypes.Structure):
    _fields_ = ([(k, ctypes.c_int32) for k in ("fn", "sign", "binade", "pad")] + [(k, ctypes.c_uint64) for k in ("n", "nonfinite", "tiny", "broken", "compared", "differ")] +
                [(k, ctypes.c_double) for k in ("ulp", "abs", "maxres")] + [(k, ctypes.c_uint64) for k in ("ulp_at", "abs_at", "maxres_at")])


_lib = None


def lib():
    global _lib
    if _lib is None:
        so = cppbuild.compile(os.path.join(cppbuild.BUILD, "libmath_accuracy_host.so"), [SOURCE], cppbuild.csrc_headers() + cppbuild.oracle_headers(),
                              cppbuild.EXACT_FLAGS + ["-pthread", "-Wall", "-I" + cppbuild.CSRC, "-I" + cppbuild.ORACLE])
        _lib = ctypes.CDLL(so)
    return _lib


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def evaluate(what, x, y=None):
    """the host build's float32 results of function `what` (a name of WHAT, or its number; + 100: oracle/detmath.h's)"""
    x = np.ascontiguousarray(x, np.float32)
    y = None if y is None else np.ascontiguousarray(y, np.float32)
    out = np.empty(len(x), np.float32)
    assert lib().mah_eval(WHAT.get(what, what), ctypes.c_longlong(len(x)), _vp(x), _vp(y), _vp(out)) == 0
    return out


def truth(what, x, y=None):
    """libm's double results"""
    x = np.ascontiguousarray(x, np.float32)
    y = None if y is None else np.ascontiguousarray(y, np.float32)
    out = np.empty(len(x), np.float64)
    assert lib().mah_truth(WHAT.get(what, what), ctypes.c_longlong(len(x)), _vp(x), _vp(y), _vp(out)) == 0
    return out


def sample(which, first, n):
    """items [first, first + n) of the sweep's hashed samples: "atan21_pairs" -> (y, x), "pow1" -> (x, y)"""
    a, b = np.empty(n, np.float32), np.empty(n, np.float32)
    assert lib().mah_sample({"atan21_pairs": 0, "pow1": 1}[which], ctypes.c_longlong(first), ctypes.c_longlong(n), _vp(a), _vp(b)) == 0
    return a, b


def row_key(sign, binade, of_float=True):
    """of_float: the binade is a float argument's (zero and the denormals have rows of their own), not that of a double quantity"""
    return ("-" if sign else "+") + ("zero" if of_float and binade == -128 else "denormal" if of_float and binade == -127 else "2^%d" % binade)


def _args(key, two):
    return ["0x%08x" % (key >> 32)] + (["0x%08x" % (key & 0xFFFFFFFF)] if two else [])


def sweep(threads=None, stride=STRIDE, far_stride=FAR_STRIDE):
    """-> {function: {row key: {n, ulp, ulp_at, abs, abs_at, max_abs_result, max_abs_result_at, tiny, nonfinite, broken, compared, differ}}}"""
    rows = (_Row * 4096)()
    n = lib().mah_run(threads or cppbuild.default_threads(), stride, far_stride, rows, len(rows))
    assert n > 0
    out = {f: {} for f in ROW_FUNCTIONS}
    for r in rows[:n]:
        two = ROW_FUNCTIONS[r.fn] in ("atan21", "atan21_pairs", "pow1")
        out[ROW_FUNCTIONS[r.fn]][row_key(r.sign, r.binade, ROW_FUNCTIONS[r.fn] not in ("atan21_pairs", "pow1"))] = {
            "n": r.n, "ulp": r.ulp, "ulp_at": _args(r.ulp_at, two), "abs": r.abs, "abs_at": _args(r.abs_at, two),
            "max_abs_result": r.maxres, "max_abs_result_at": _args(r.maxres_at, two),
            "tiny": r.tiny, "nonfinite": r.nonfinite, "broken": r.broken, "compared": r.compared, "differ": r.differ}
    return out


def load():
    with open(TABLE) as fh:
        return json.load(fh)


def bits(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


def same(got, want):
    """bit for bit: zero keeps its sign; NaN matches any NaN (x86 and gfx950 differ in the default payload)"""
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def from_hex(args):
    return [np.array([int(a, 16)], np.uint32).view(np.float32)[0] for a in args]


def binade_of_float(x):
    """as the sweep's binade_of: unbiased exponent, -127 for denormals, -128 for zero"""
    m = bits(x) & np.uint32(0x7FFFFFFF)
    e = (m >> np.uint32(23)).astype(np.int64)
    return np.where(m == 0, -128, np.where(e == 0, -127, e - 127))


def binade_of_double(t):
    """as the sweep's binade_of_double (rows of atan21_pairs and pow1)"""
    t = np.abs(np.asarray(t, np.float64))
    with np.errstate(all="ignore"):
        e = np.frexp(np.where(np.isfinite(t) & (t > 0), t, 1.0))[1].astype(np.int64) - 1
    e = np.where(t > 0, np.where(np.isinf(t), 130, e), -150)
    return np.clip(e, -150, 130)


def row_keys(function, x, y=None):
    """the table row of every point (x: the function's first argument, y: its second)"""
    if function == "atan21_pairs":
        with np.errstate(all="ignore"):
            b = binade_of_double(np.where(y == 0, np.inf, np.abs(x.astype(np.float64) / y.astype(np.float64))))  # atan21(first, second): |first / second|
        sign = np.zeros(len(x), bool)
    elif function == "pow1":
        with np.errstate(all="ignore"):
            b, sign = binade_of_double(y.astype(np.float64) * truth("log21", x)), np.zeros(len(x), bool)
    else:
        b, sign = binade_of_float(x), (np.signbit(x) if function == "exp21" else np.zeros(len(x), bool))
    return [row_key(s, k, function not in ("atan21_pairs", "pow1")) for s, k in zip(sign, b)]


def errors(values, t):
    """of float32 results against double truth, as the sweep scores them -> (ulps of the true value, absolute error, scored): a point is
    scored where result and truth are finite and the truth does not round to infinity; ulps are NaN where |truth| < 2^-126"""
    v = np.asarray(values, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        scored = np.isfinite(v) & np.isfinite(t) & (np.abs(t) < float.fromhex("0x1.ffffffp+127"))
        d = np.abs(v - t)
        e = np.frexp(np.where(scored & (t != 0), np.abs(t), 1.0))[1] - 1
        ulps = d / np.ldexp(1.0, e - 23)
        ulps = np.where(t == 0, np.where(d == 0, 0.0, np.inf), ulps)
        ulps = np.where((np.abs(t) < 2.0 ** -126) & (t != 0), np.nan, ulps)
    return ulps, d, scored


def exceeding(function, table_rows, values, t, x, y=None):
    """the points whose error exceeds the recorded figure of their row (ulps, or absolutely) -> (bool array, report lines)"""
    ulps, d, scored = errors(values, t)
    keys = row_keys(function, x, y)
    rec_ulp = np.array([table_rows[k]["ulp"] if k in table_rows else -1.0 for k in keys])
    rec_abs = np.array([table_rows[k]["abs"] if k in table_rows else -1.0 for k in keys])
    rec_max = np.array([table_rows[k]["max_abs_result"] if k in table_rows else 0.0 for k in keys])
    with np.errstate(all="ignore"):
        bad = scored & ((np.nan_to_num(ulps, nan=0.0) > rec_ulp + ULP_SLACK) | (d > rec_abs + 2.0 ** -52 * np.maximum(rec_max, np.abs(t))))
    lines = ["%s(%s) = %r: %.6g ulp, abs %.6g; row %s records %.6g ulp, abs %.6g" %
             (function, ", ".join(float(a[i]).hex() for a in ((x,) if y is None else (x, y))), float(values[i]), ulps[i], d[i], keys[i], rec_ulp[i], rec_abs[i])
             for i in np.flatnonzero(bad)[:8]]
    return bad, lines


# ---- which arguments the scenes feed --------------------------------------------------------------------------------------------
CENSUS_SIZE = {"golden": (40, 40), "reference_cameras": (60, 40), "bench": (64, 36)}
# scenes that may hand sin or cos a non-finite argument, each with its explanation (none does today)
NONFINITE_SINCOS_ALLOWED = {}


def census_frames(oracle):
    """(set, label, scene, frame) of every frame of the census: the golden fixtures, the cameras and times fitted to the reference's
    screenshots, and the frames bench.py sweeps, each at a small size"""
    import bench
    import golden_util as gu

    for path in gu.golden_files():
        f = gu.oracle_frame(oracle, np.load(path))
        f.width, f.height = CENSUS_SIZE["golden"]
        yield "golden", os.path.basename(path)[:-4], gu.scene_of(path), f
    with open(os.path.join(cppbuild.HERE, "golden", "reference_images.json")) as fh:
        fits = json.load(fh)["images"]
    w, h = CENSUS_SIZE["reference_cameras"]
    fovy = np.float32(60.0) * np.float32(3.14159265358979) / np.float32(180.0)
    for name in sorted(fits):
        e = fits[name]
        scene = "light_shadows" if e["scene"] == "light_shadows_backwards" else e["scene"]
        direction = (math.cos(e["pitch"]) * math.sin(e["yaw"]), math.sin(e["pitch"]), math.cos(e["pitch"]) * math.cos(e["yaw"]))
        f = oracle.default_frame(scene, w, h, basis=oracle.camera_direction(e["eye"], direction, fovy, np.float32(w) / np.float32(h)), stime=e["stime"])
        slots = {row[0]: row[6] for row in oracle.var_table(scene)}
        for k, v in e.get("variables", {}).items():
            f.scene_var[slots[k]] = v
        yield "reference_cameras", name, scene, f
    w, h = CENSUS_SIZE["bench"]
    for config in bench.CONFIGS:
        for k in range(bench.SWEEP):
            yield "bench", "%s/%d" % (config, k), bench.CONFIGS[config]["scene"], bench.oracle_frame(oracle, k, w, h, config=config)


def census(oracle):
    """-> {set: {scene: {"sincos_max": largest finite |argument| of sin or cos, "sincos_nonfinite": count, "pow_product": [lo, hi] of y * log2 x,
    "exp2": [lo, hi] or None, "log2": [lo, hi] or None}}}, the extremes over the set's frames of that scene"""
    oracle.build(census=True, ref=False)
    out = {}
    for group, _label, scene, f in sorted(census_frames(oracle), key=lambda c: (c[0] != "golden", c[0] != "reference_cameras", c[2])):
        oracle.census(scene, f)
        m = oracle.census.last_math
        e = out.setdefault(group, {}).setdefault(scene, {"sincos_max": 0.0, "sincos_nonfinite": 0, "pow_product": None, "exp2": None, "log2": None})
        if m["sincos"][1] is not None:
            e["sincos_max"] = max(e["sincos_max"], m["sincos"][1])
        e["sincos_nonfinite"] += m["sincos"][3]
        for key, name in (("pow_product", "pow"), ("exp2", "exp2"), ("log2", "log2")):
            if m[name][0] is not None:
                e[key] = [min(m[name][0], e[key][0]), max(m[name][1], e[key][1])] if e[key] else [m[name][0], m[name][1]]
    return out


def _dump(doc):
    """one table row per line"""
    def rows(d):
        return "{\n" + ",\n".join("        %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in d.items()) + "\n      }"

    head = {k: v for k, v in doc.items() if k not in ("functions", "census")}
    text = json.dumps(head, indent=2)[:-2] + ',\n  "functions": {\n'
    text += ",\n".join('    %s: {\n      "arguments": %s,\n      "rows": %s\n    }' % (json.dumps(f), json.dumps(doc["functions"][f]["arguments"]), rows(doc["functions"][f]["rows"]))
                       for f in doc["functions"])
    text += '\n  },\n  "census": {\n' + ",\n".join("    %s: %s" % (json.dumps(g), rows(doc["census"][g]).replace("\n      }", "\n    }").replace("\n        ", "\n      ")) for g in doc["census"])
    return text + "\n  }\n}\n"


def write_table():
    import sys

    sys.path.insert(0, cppbuild.ROOT)
    sys.path.insert(0, cppbuild.ORACLE)
    import pyoracle

    swept = sweep()
    doc = {
        "about": "Error of the deterministic elementary functions (sdf_playground_amd/csrc/sdfr_math.h, host build; oracle/detmath.h is bit-equal on every "
                 "251st argument of the sweep) against libm in double, per binade, as measured by tests/cpp/math_accuracy_host.cpp. "
                 "ulp: largest error in ulps of the true value; abs: largest absolute error; *_at: the arguments' bits; tiny: truths below 2^-126, which "
                 "enter abs only; nonfinite: results that are not finite where the truth's fp32 rounding is (or the reverse). "
                 "Rewritten by `python tests/math_accuracy_util.py --write`.",
        "yardstick": {"truth": "libm in double (sin, cos, atan2, exp2, log2, pow), exact to about 2^-29 of an fp32 ulp; worst cases confirmed with mpmath at 60 digits",
                      "compiler": subprocess.run(["g++", "--version"], capture_output=True, text=True, check=True).stdout.splitlines()[0],
                      "libc": " ".join(os.confstr("CS_GNU_LIBC_VERSION").split()) if hasattr(os, "confstr") else ""},
        "sweep": {"stride": STRIDE, "far_stride": FAR_STRIDE, "threads_do_not_matter": True},
        "domain": {"sin1, cos1, sincos1": "|x| <= 2^16: |result| <= 1 and absolute error < %g" % ABS_BOUND},
        "summary": summary(swept),
        "functions": {f: {"arguments": ARGUMENTS[f], "rows": swept[f]} for f in ROW_FUNCTIONS},
        "census": census(pyoracle),
    }
    doc["census"] = {"about": {"what": "largest finite |argument| the scenes hand to sin or cos, count of non-finite ones, and the extremes of pow's y * log2 x, "
                                       "exp2's and log2's arguments (oracle census build), per set of frames and scene; frame sizes " + json.dumps(CENSUS_SIZE)},
                     **doc["census"]}
    with open(TABLE, "w") as fh:
        fh.write(_dump(doc))


def in_domain(key):
    """whether a row of sin1 / cos1 lies inside the stated domain (binades below 2^16)"""
    return key in ("+zero", "+denormal") or int(key[3:]) < 16


def summary(swept):
    """the largest figures per function (of sin1 and cos1: on the stated domain and beyond it)"""
    def top(rows):
        rows = list(rows)
        return {"ulp": max(r["ulp"] for r in rows), "abs": max(r["abs"] for r in rows), "max_abs_result": max(r["max_abs_result"] for r in rows)}

    out = {}
    for f in ("sin1", "cos1"):
        out[f + ", |x| < 2^16"] = top(r for k, r in swept[f].items() if in_domain(k))
        out[f + ", 2^16 <= |x| <= 2^26"] = top(r for k, r in swept[f].items() if not in_domain(k))
    for f in ("atan21", "atan21_pairs", "log21"):
        out[f] = top(swept[f].values())
    out["exp21"] = {"ulp": max(r["ulp"] for r in swept["exp21"].values())}
    out["pow1, |y log2 x| < 1"] = {"ulp": max(r["ulp"] for k, r in swept["pow1"].items() if int(k[3:]) < 0)}
    out["pow1"] = {"ulp": max(r["ulp"] for r in swept["pow1"].values())}
    return out


if __name__ == "__main__":
    import sys

    if sys.argv[1:] == ["--write"]:
        write_table()
    else:
        print(__doc__)


# ---- the device build, directly: one run-time scene whose distance is one function of (p.x, p.y), chosen by (int)stime ---------------
TOKEN = "SDFR_FAST_EXACT_MATH"
MAX_POINTS = 32768
# (case name, expression of x = p.x and y = p.y, the table's function, mah_eval's function)
CASES = [
    ("sin1", "sin1(x)", "sin1", "sin1"), ("cos1", "cos1(x)", "cos1", "cos1"),
    ("sincos1.x", "sincos1(x).x", "sin1", "sincos1.x"), ("sincos1.y", "sincos1(x).y", "cos1", "sincos1.y"),
    ("sincos1_small.x", "sincos1_small(x).x", "sin1", "sincos1_small.x"), ("sincos1_small.y", "sincos1_small(x).y", "cos1", "sincos1_small.y"),
    ("atan21", "atan21(x, y)", "atan21", "atan21"), ("atan21_pairs", "atan21(x, y)", "atan21_pairs", "atan21"),
    ("exp21", "exp21(x)", "exp21", "exp21"), ("log21", "log21(x)", "log21", "log21"), ("pow1", "pow1(x, y)", "pow1", "pow1"),
    # the negative control, here and never in product code: sin1 whose reduction drops the third Cody-Waite term
    ("control_sin", "control_sin(x)", "sin1", "sin1"),
]
CASE_NAMES = [c[0] for c in CASES]


def scene_text(fast_math):
    cases = "".join("\t\tcase %d: return %s; // %s\n" % (k, c[1], c[0]) for k, c in enumerate(CASES))
    return ("// accuracy scene: dist = one elementary function of (p.x, p.y), chosen by (int)stime (tests/math_accuracy_util.py)\n" +
            ("// %s: the fast exact forms, in situ\n" % TOKEN if fast_math else "") +
            "#if defined(__HIPCC_RTC__) || defined(__HIPCC__)\n#define PROBE_FN __host__ __device__ __attribute__((noinline))\n#else\n#define PROBE_FN\n#endif\n"
            "// sin1 with a reduction that is subtly wrong: two Cody-Waite terms instead of three\n"
            "SDF_HD float control_sin(float x)\n{\n"
            "\tconst float k = rne1(x * 0.636619772367581343f);\n"
            "\tfloat r = fma1(-k, 1.5703125f, x);\n"
            "\tr = fma1(-k, 4.837512969970703125e-4f, r);\n"
            "\tconst float q = k - 4.f * floor1(k * 0.25f);\n"
            "\tconst float s = sin_kernel(r), c = cos_kernel(r);\n"
            "\tconst float v = (q == 1.f || q == 3.f) ? c : s;\n"
            "\treturn (q >= 2.f) ? -v : v;\n}\n"
            "struct Scene\n{\n"
            "\tstatic SDF_HD void prepare(FrameU &) {}\n"
            "\tstruct RayInv { float unused; };\n"
            "\tstatic SDF_HD RayInv ray_setup(const FrameU &, vec3, const RayFlags &) { RayInv r; r.unused = 0.f; return r; }\n"
            "\t// one copy per module, not one per evaluation of every kernel that evaluates the scene: the module compiles in seconds\n"
            "\tstatic PROBE_FN float probe(int which, float x, float y)\n\t{\n\t\tswitch (which)\n\t\t{\n" + cases + "\t\t}\n\t\treturn 0.f;\n\t}\n"
            "\tstatic SDF_HD float dist(const FrameU &U, const RayInv &, vec3 p, vec3, bool) { return probe((int)U.stime, p.x, p.y); }\n"
            "\tstatic SDF_HD void material(const FrameU &, const SurfacePoint &, Material &) {}\n"
            "\tstatic SDF_HD bool light(const FrameU &, int, Light &) { return false; }\n"
            "\tstatic SDF_HD float ambient() { return 0.075f; }\n"
            "\tstatic SDF_HD vec3 background(const FrameU &, vec3, uint32_t) { return V3s(0.f); }\n"
            "};\n")


def _u(b):
    return np.asarray(b, np.uint32).view(np.float32)


def _edges(lo, hi, first=None, last=None):
    """the floats 2^e - 3 .. 2^e + 3 ulps for lo <= e <= hi, kept inside [first, last]"""
    b = np.array([((e + 127) << 23) + d for e in range(lo, hi + 1) for d in range(-3, 4)], np.int64)
    v = _u(b.astype(np.uint32))
    return v[(v >= (first if first is not None else 0)) & (v <= (last if last is not None else np.inf))]


def _worst(table, function, keep=lambda key: True):
    rows = [r for k, r in table["functions"][function]["rows"].items() if keep(k)]
    a = np.array([from_hex(r[at + "_at"]) for r in rows for at in ("ulp", "abs", "max_abs_result") if r[at] != 0], np.float32)  # (a figure of 0 has no argument)
    return a[:, 0], (a[:, 1] if a.shape[1] > 1 else None)


def _both(v):
    return np.concatenate([v, -v]).astype(np.float32)


def device_points(case, table, fast_math):
    """(x, y) of a case, MAX_POINTS at the most: the table's worst cases, every binade edge of the function's swept range +-3 floats, for
    sin and cos the two floats nearest k pi / 2 (k = 1..4096 and the powers of two up to the domain's edge), and a seeded sample.
    Every point lies where the sweep took every float (or is one of its samples), so the recorded figure of its row holds for it."""
    rng = np.random.default_rng(CASE_NAMES.index(case) + 0x5DF0)
    function = CASES[CASE_NAMES.index(case)][2]
    if function in ("sin1", "cos1"):
        wx = np.concatenate([_worst(table, f, in_domain)[0] for f in ("sin1", "cos1")])
        k = np.concatenate([np.arange(1, 4097), 2 ** np.arange(13, 16)]).astype(np.float64)
        near = (k * (np.pi / 2)).astype(np.float32)
        near = np.concatenate([near, np.nextafter(near, np.where(near.astype(np.float64) > k * (np.pi / 2), np.float32(0), np.float32(np.inf)).astype(np.float32))])
        x = np.concatenate([wx, [0.0], _u([1, 2, 3, 0x7FFFFD, 0x7FFFFE, 0x7FFFFF]), _edges(-126, 16, last=SINCOS_DOMAIN), near])
        x = _both(x)
        n = MAX_POINTS - len(x)
        s = np.concatenate([np.exp2(rng.uniform(-14, 16, n // 2)), rng.uniform(2.0 ** -14, SINCOS_DOMAIN, n - n // 2)]) * rng.choice([-1.0, 1.0], n)
        x = np.concatenate([x, s.astype(np.float32)])
        if case.startswith("sincos1_small"):
            x = np.concatenate([x[np.abs(x) <= 0.75], _both(np.array([0.75, np.nextafter(np.float32(0.75), np.float32(0))], np.float32)),
                                _both(rng.uniform(2.0 ** -14, 0.75, 4096).astype(np.float32))])
        return x, np.zeros(len(x), np.float32)
    if case == "atan21":
        wx, wy = _worst(table, "atan21")
        x = _both(np.concatenate([wx, _edges(-30, 30, first=2.0 ** -30, last=2.0 ** 30), np.exp2(rng.uniform(-30, 30, 8192)).astype(np.float32)]))
        return x, np.ones(len(x), np.float32)
    if case == "atan21_pairs":
        wx, wy = _worst(table, "atan21_pairs")
        sx, sy = sample("atan21_pairs", 0, 16384)
        x, y = np.concatenate([wx, sx]), np.concatenate([wy, sy])
        if fast_math:  # the one reciprocal inside, of the ratio, stays in rcp1's documented domain, as in the probes
            with np.errstate(all="ignore"):
                ratio = np.abs(x.astype(np.float64) / y.astype(np.float64))
            keep = (y == 0) | (ratio == 0) | ((ratio >= 2.0 ** -100) & (ratio <= 2.0 ** 100))
            x, y = x[keep], y[keep]
        return x, y
    if case == "exp21":
        f32 = np.float32
        x = np.concatenate([_worst(table, "exp21")[0], _both(_edges(-24, 7, first=2.0 ** -24, last=150.0)),
                            np.array([128.0, np.nextafter(f32(128), f32(0)), -126.0, np.nextafter(f32(-126), f32(-200)), -149.0, -150.0, 150.0], f32),
                            rng.uniform(-150, 150, 8192).astype(f32), _both(np.exp2(rng.uniform(-24, 7, 4096)).astype(f32))])
        return x, np.zeros(len(x), f32)
    if case == "log21":
        x = np.concatenate([_worst(table, "log21")[0], _u([1, 2, 3, 0x7FFFFD, 0x7FFFFE, 0x7FFFFF, 0x7F7FFFFF]), _edges(-126, 127),
                            _u(rng.integers(1, 0x7F800000, 16384, dtype=np.int64).astype(np.uint32))])
        return x, np.zeros(len(x), np.float32)
    assert case == "pow1"
    wx, wy = _worst(table, "pow1")
    sx, sy = sample("pow1", 0, 30000)
    return np.concatenate([wx, sx]), np.concatenate([wy, sy])


def check_case(case, table, values, x, y):
    """what the device build's `values` at (x, y) must satisfy -> failure lines: (a) the host build's bits; (b) the error against
    libm in double within the recorded figure of each point's row; (c) |sin|, |cos| <= 1 on the domain"""
    _, _, function, what = CASES[CASE_NAMES.index(case)]
    two = function in ("atan21", "atan21_pairs", "pow1")
    failures = []
    if case != "control_sin":
        want = evaluate(what, x, y if two else None)
        differ = np.flatnonzero(~same(values, want))
        failures += ["%s(%s): device %08x, host %08x" % (case, float(x[i]).hex() + (", " + float(y[i]).hex() if two else ""), bits(values)[i], bits(want)[i]) for i in differ[:8]]
    t = truth(function.replace("_pairs", ""), x, y if two else None)
    bad, lines = exceeding(function, table["functions"][function]["rows"], values, t, x, y if two else None)
    failures += lines
    if function in ("sin1", "cos1"):
        failures += ["|%s(%s)| = %r > 1" % (case, float(x[i]).hex(), float(values[i])) for i in np.flatnonzero(~(np.abs(values) <= 1))[:8]]
    return failures


CONTROL_FROM = 4096.0  # from here on the dropped term, 7.5e-8 per quarter turn, is 2e-4 and more: two thousand times the recorded figure


def control_caught(table, values, x):
    """the fraction of the control's points with |x| >= CONTROL_FROM whose error exceeds the recorded figure of their row.  The dropped term
    shifts the reduced argument by d >= 2e-4 and the sine by d |cos x|, so only points where |cos x| > 0.01 are counted: at the
    crests of the sine, which the points nearest an odd k pi / 2 visit on purpose, a shifted argument changes nothing"""
    far = (np.abs(x) >= CONTROL_FROM) & (np.abs(truth("cos1", x)) > 0.01)
    bad, _ = exceeding("sin1", table["functions"]["sin1"]["rows"], values[far], truth("sin1", x[far]), x[far])
    assert far.sum() > 1000
    return float(bad.mean())

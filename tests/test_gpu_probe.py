"""GPU tier of the probe scenes (tests/probe_scenes.py): the device build of sdfr_math.h, sdfr_noise.h and sdfr_lib.h, function by function,
against the oracle.  One test per (group of probes, math mode): the group's text is compiled by hiprtc once, then every probe is one
selector value and one to thirty-two small distance queries whose raw fp32 answers must be the oracle's kat_batch bit for bit -- zero
keeps its sign, NaN matches any NaN.  With the token SDFR_FAST_EXACT_MATH the same text runs the fast forms of sqrt1 / rcp1 / div_c in
situ; the inputs the oracle's census flags as outside their documented domains are dropped there, nothing else, and there is no
tolerance anywhere.  The CPU tier (tests/test_probe_cpu.py) holds the host build of the same table to the same values."""
import numpy as np
import pytest

import probe_scenes as ps

pytestmark = pytest.mark.gpu

HOST_SAMPLE = 64  # points of each probe's first call that are also queried from a host array


@pytest.fixture(scope="module")
def census_oracle(oracle):
    oracle.build(census=True, ref=False)
    return oracle


def device_values(renderer, probe):
    """the probe's N_POINTS values: queryDistance on device tensors, call by call; the first HOST_SAMPLE points also from a host array"""
    import torch

    renderer.setParameters(float(probe.case))
    pts = ps.points(probe)
    out = np.empty(ps.N_POINTS, np.float32)
    for k, (rows, variables) in enumerate(ps.calls(probe)):
        for name, v in variables.items():
            assert renderer.setValue(name, v), name
        p = np.ascontiguousarray(pts[rows])
        d = renderer.queryDistance(torch.from_numpy(p).to("cuda"))
        assert d.shape == (len(p),) and d.dtype == torch.float32
        out[rows] = d.cpu().numpy()
        if k == 0:
            h = renderer.queryDistance(p[:HOST_SAMPLE])
            assert np.array_equal(h.view(np.uint32), out[rows][:HOST_SAMPLE].view(np.uint32)), "%s: host array and device tensor disagree" % probe.name
    return out


@pytest.mark.parametrize("fast_math", [False, True], ids=["ieee", "fast"])
@pytest.mark.parametrize("group", ps.GROUPS)
def test_device_functions_equal_the_oracle(census_oracle, group, fast_math):
    import sdf_playground_amd as sp

    r = sp.SDFRenderer(0)
    try:
        r.initShaderSource("probe_%s_%s" % (group, "fast" if fast_math else "ieee"), ps.scene_text(group, fast_math))
        assert [v for v in r.getVariableMap() if not v.startswith(("debug_", "show_"))] == sorted(ps.VAR_NAMES)
        failed, controls = [], {}
        for probe in ps.probes(group, controls=True):
            got, want = device_values(r, probe), ps.expected(census_oracle, probe)
            keep = ps.kept(census_oracle, probe, fast_math)
            differ = int((~ps.same(got, want) & keep).sum())
            if probe.control:
                controls[probe.name] = differ
            elif differ:
                failed.append(ps.mismatch_report(probe, got, want, keep))
        if failed:
            print("\n".join(failed))
        assert not failed, "%d of %d probes differ from the oracle: %s" % (len(failed), len(ps.probes(group)), [f.split(" ")[0] for f in failed])
        # the negative controls: a comparison this loose would pass them
        if "control:min" in controls:
            assert controls["control:min"] > 0, "(a < b ? a : b) passed for min1 on NaN and signed zeros"
            if fast_math:
                assert controls["control:sqrt"] > 0, "with the token sqrt1 equals sqrt on -0, denormals and +inf: the fast build is not the fast build"
            else:
                assert controls["control:sqrt"] == 0, "without the token sqrt1 is not the IEEE square root"
    finally:
        r.close()

"""GPU tier: the device build of sin1, cos1, sincos1, sincos1_small, atan21, exp21, log21 and pow1 against true values, directly.  One
run-time scene per math mode (plain, and with SDFR_FAST_EXACT_MATH) whose distance is one function of (p.x, p.y), chosen by
(int)stime, as in tests/probe_scenes.py; one distance query of at most 32 768 points per function (tests/math_accuracy_util.py
device_points: the recorded worst cases, every binade edge +-3 floats, the floats nearest k pi / 2, a seeded sample).  The device's
values must (a) be the host build's bits, (b) lie within the figure tests/golden/math_accuracy.json records for their binade, against
libm in double computed here, and (c) for sin and cos stay within [-1, 1].  A negative control in the scene's text, sin1 without the
third Cody-Waite term, must fail (b) at the large arguments of the domain: a reduction that is subtly wrong in oracle and kernel alike
would be caught.  The CPU tier (tests/test_math_accuracy_cpu.py) runs the same text, points and checks through a host build."""
import numpy as np
import pytest

import math_accuracy_util as mau

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table():
    return mau.load()


@pytest.mark.parametrize("fast_math", [False, True], ids=["ieee", "fast"])
def test_device_functions_against_true_values(table, fast_math):
    import torch

    import sdf_playground_amd as sp

    r = sp.SDFRenderer(0)
    try:
        r.initShaderSource("math_accuracy_%s" % ("fast" if fast_math else "ieee"), mau.scene_text(fast_math))
        failures, caught = [], None
        for k, case in enumerate(mau.CASE_NAMES):
            x, y = mau.device_points(case, table, fast_math)
            assert len(x) <= mau.MAX_POINTS
            r.setParameters(float(k))
            p = np.ascontiguousarray(np.stack([x, y, np.zeros_like(x)], 1), np.float32)
            d = r.queryDistance(torch.from_numpy(p).to("cuda"))
            assert d.shape == (len(p),) and d.dtype == torch.float32
            v = d.cpu().numpy()
            if case == "control_sin":
                caught = mau.control_caught(table, v, x)
            else:
                failures += mau.check_case(case, table, v, x, y)
        assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures[:40]))
        assert caught is not None and caught > 0.99, "sin1 without its third reduction term passes the recorded bound at |x| >= %g (caught %r)" % (mau.CONTROL_FROM, caught)
    finally:
        r.close()

"""The fp64 K = 5 / 10 wavefront control kernel computes the bits recorded in tests/golden/wave_parent_bits.npz: c_k of the
last step, the warm-start matrix ut and u0 of every step after three receding-horizon steps in one launch from non-zero
controls (B = 5), at (cart, K 10, T 200), (omni, K 10, T 200), (cart, K 5, T 130) and (omni, K 5, T 70), each with the c_k
output requested and without it (the call form bench.py times).  The fixture was recorded from the commit before D moved
into registers in the gradient (csrc/control_wave_regd.inc): c_k is formed before the gradient runs, and a change behind it
must not move it -- clamped controls amplify one unit in the last place of c_k to sign flips within 50 steps.

The inputs are regenerated from the seeds in tools/record_wave_bits.py.  After a toolchain change that moves the bits,
re-record ON THE GPU with a build of the commit whose results are the reference:

    python tools/record_wave_bits.py

A re-record is a statement that the bits moved: say in the commit that does it what moved them.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import record_wave_bits as rec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(rec.FIXTURE) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("with_ck", [True, False], ids=["ck", "timed_form"])
@pytest.mark.parametrize("model,K,horizon", rec.CASES)
def test_three_steps_are_the_recorded_bits(golden, model, K, horizon, with_ck):
    k = rec.case_key(model, K, horizon)
    got = rec.run_case(model, K, horizon, with_ck)
    names = ("ck", "ut", "u0") if with_ck else ("ut", "u0")
    for name in names:
        want = golden["%s_%s" % (k, name)]
        if not with_ck:
            want = (rec.bits(want) ^ golden["%s_%s_nock_xor" % (k, name)]).view(np.float64)
        diff = got[name] != want
        print(k, name, "ck" if with_ck else "timed form", "entries that differ: %d of %d" % (int(diff.sum()), diff.size),
              "max |difference| %.3g" % float(np.abs(got[name] - want).max()))
        assert np.array_equal(got[name], want), (k, name, int(diff.sum()), diff.size)

"""The fp64 K = 5 / 10 wavefront control kernel computes the bits recorded in tests/golden/wave_trim_parent_bits.npz: c_k of
the last step, ut and u0 of every step after three receding-horizon steps in one launch from non-zero controls (B = 5), with
the c_k output requested and without it, at the horizon shapes tests/test_gpu_wave_parent_bits.py does not reach: T = 193 (a
last slot of one point), T = 100 and T = 150 (partly valid upper halves of the contraction's tiles), T = 64 (one slot, no
tail), T = 20 (a partly valid lower half), and one case per model whose limits are so tight that most controls sit on umin /
umax.  The fixture was recorded from the commit before the staging entry of the contraction and the control update shed their
selects, copies and address arithmetic: nothing of that may move a bit.

The inputs are regenerated from the seeds in tools/record_wave_trim_bits.py; re-record ON THE GPU with a build of the commit
whose results are the reference (python tools/record_wave_trim_bits.py), and say in the commit that does it what moved the bits.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import record_wave_trim_bits as rec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(rec.FIXTURE) as f:
        return {k: f[k] for k in f.files}


def test_horizons_reach_the_shapes():
    rec.check_shapes()


@pytest.mark.parametrize("with_ck", [True, False], ids=["ck", "timed_form"])
@pytest.mark.parametrize("model,K,T,scale", rec.CASES, ids=[rec.case_key(*c) for c in rec.CASES])
def test_three_steps_are_the_recorded_bits(golden, model, K, T, scale, with_ck):
    k = rec.case_key(model, K, T, scale)
    got = rec.run_case(model, K, T, scale, with_ck)
    names = ("ck", "ut", "u0") if with_ck else ("ut", "u0")
    for name in names:
        want = golden["%s_%s" % (k, name)]
        if not with_ck:
            want = (rec.bits(want) ^ golden["%s_%s_nock_xor" % (k, name)]).view(np.float64)
        diff = got[name] != want
        print(k, name, "ck" if with_ck else "timed form", "entries that differ: %d of %d" % (int(diff.sum()), diff.size),
              "max |difference| %.3g" % float(np.abs(got[name] - want).max()))
        assert np.array_equal(got[name], want), (k, name, int(diff.sum()), diff.size)
    if scale != 1.0:  # the clamp's two limits, exactly their bits (the recorded arrays hold them: asserted when recorded)
        share, at_min, at_max = rec.on_limits(model, scale, got["ut"])
        print(k, "on a limit: %.3f of the clamped controls" % share)
        assert share > 0.5 and at_min and at_max


@pytest.mark.parametrize("model,K,T,scale", rec.TIGHT_CASES, ids=[rec.case_key(*c) for c in rec.TIGHT_CASES])
def test_one_launch_is_three_calls(model, K, T, scale):
    one = rec.run_case(model, K, T, scale, False, one_launch=True)
    three = rec.run_case(model, K, T, scale, False, one_launch=False)
    for name in ("ut", "u0"):
        assert np.array_equal(one[name], three[name]), (rec.case_key(model, K, T, scale), name)

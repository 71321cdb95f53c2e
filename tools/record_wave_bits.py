#!/usr/bin/env python3
"""Records tests/golden/wave_parent_bits.npz: what the fp64 K = 5 / 10 wavefront control kernel leaves after three
receding-horizon steps in one launch from non-zero controls (c_k of the last step, the warm-start matrix ut, u0 of every
step), B = 5.  tests/test_gpu_wave_parent_bits.py regenerates the inputs from the seeds below and asserts array_equal.

Run it on the GPU with a build of the commit whose bits are the reference:

    python tools/record_wave_bits.py [OUT.npz]

Every case runs twice: with the c_k output requested and without it (what bench.py times: ut and u0 only).  The second
run's arrays are stored as the XOR of their bit patterns with the first run's -- all zero while the two agree, so the file
stays small without assuming that they do.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "wave_parent_bits.npz")
CASES = [("simple_cart", 10, 20.0), ("omni", 10, 20.0), ("simple_cart", 5, 13.0), ("omni", 5, 7.0)]
B, N_STEPS = 5, 3


def case_key(model, K, horizon):
    return "%s_K%d_T%d" % (model, K, int(round(horizon * 10)))


def inputs(model, K, horizon):
    """(pose per step [N_STEPS, B, 3], controls [B, T, 3]) of a case, from its seed"""
    from tests.gpu_util import random_poses
    T = int(round(horizon * 10))
    rng = np.random.default_rng(1009 * K + T + (7 if model == "omni" else 0))
    pose0 = random_poses(rng, B)
    seq = pose0[None] + np.cumsum(rng.normal(scale=0.02, size=(N_STEPS, B, 3)), axis=0)
    ut0 = rng.uniform(-0.4, 0.4, (B, T, 3))
    if model == "simple_cart":
        ut0[:, :, 1] = 0.0
    return seq, ut0


def run_case(model, K, horizon, with_ck):
    """three steps in one launch; {"ck": [B, K^2] (with_ck only), "ut": [B, T, 3], "u0": [N_STEPS, B, 3]}"""
    import torch
    from tests.gpu_util import make_pair

    def dev(a):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()

    eng, _ = make_pair(model, K, horizon, n_oracles=0)
    assert eng.T == int(round(horizon * 10))
    seq, ut0 = inputs(model, K, horizon)
    d_ut = dev(ut0)
    d_u0 = torch.full((N_STEPS, B, 3), float("nan"), dtype=torch.float64, device="cuda")
    d_ck = torch.full((B, eng.K2), float("nan"), dtype=torch.float64, device="cuda") if with_ck else None
    eng.control_batch(B, dev(seq), d_ut, d_u0, ck=d_ck, n_steps=N_STEPS, pose_step_stride=B, u0_step_stride=B)
    torch.cuda.synchronize()
    eng.close()
    out = {"ut": d_ut.cpu().numpy(), "u0": d_u0.cpu().numpy()}
    if with_ck:
        out["ck"] = d_ck.cpu().numpy()
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    arrays = {}
    for model, K, horizon in CASES:
        k = case_key(model, K, horizon)
        a, b = run_case(model, K, horizon, True), run_case(model, K, horizon, False)
        for name in ("ck", "ut", "u0"):
            assert np.isfinite(a[name]).all(), (k, name)
            arrays["%s_%s" % (k, name)] = a[name]
        for name in ("ut", "u0"):
            arrays["%s_%s_nock_xor" % (k, name)] = bits(a[name]) ^ bits(b[name])
    np.savez_compressed(path, **arrays)
    print("%s: %d arrays, %d bytes" % (path, len(arrays), os.path.getsize(path)))


if __name__ == "__main__":
    main()

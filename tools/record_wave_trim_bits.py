#!/usr/bin/env python3
"""Records tests/golden/wave_trim_parent_bits.npz: the scheme of tools/record_wave_bits.py (B = 5, three receding-horizon
steps in one launch from non-zero seeded controls, c_k requested and not, the second run stored as the XOR of its bit
patterns with the first's) at the horizon shapes that fixture does not reach and the staging entry / control update of the
fp64 K = 5 / 10 wavefront control kernel do:

  T = 193   four slots, the last one with ONE point (cooperative tail, no upper half-pass in the last slot)
  T = 100   two slots of 52 / 48 lanes: upper halves with 20 / 16 valid rows
  T = 150   three slots of 54 / 48 / 48 lanes: upper halves with 22 / 16 / 16 valid rows
  T = 64    one full slot, no tail
  T = 20    one slot of 20 lanes: a LOWER half with zero rows, no upper half-pass
  tight     limits so narrow that most controls sit on umin / umax (both of them, the limits' own bits)

tests/test_gpu_wave_trim_bits.py regenerates the inputs from the seeds below and asserts array_equal.  Run it on the GPU with
a build of the commit whose bits are the reference:

    python tools/record_wave_trim_bits.py [OUT.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from record_wave_bits import B, N_STEPS, bits  # noqa: E402  (the scheme's constants and helper)

FIXTURE = os.path.join(ROOT, "tests", "golden", "wave_trim_parent_bits.npz")
DT = 0.1
TIGHT = 0.02  # the tight cases' limits: this fraction of the models' (1, 1 | 0, 2)
# (model, K, T, limit scale)
CASES = [("simple_cart", 10, 193, 1.0), ("omni", 5, 193, 1.0),
         ("omni", 10, 100, 1.0), ("simple_cart", 5, 100, 1.0),
         ("simple_cart", 10, 150, 1.0), ("omni", 5, 150, 1.0),
         ("omni", 10, 64, 1.0), ("simple_cart", 5, 64, 1.0),
         ("omni", 10, 20, 1.0), ("simple_cart", 5, 20, 1.0),
         ("simple_cart", 10, 200, TIGHT), ("omni", 5, 150, TIGHT)]
TIGHT_CASES = [c for c in CASES if c[3] != 1.0]


def case_key(model, K, T, scale):
    return "%s_K%d_T%d%s" % (model, K, T, "" if scale == 1.0 else "_tight")


def lanes_in_slot(T):
    """lanes of the wavefront that own a step in slot j, for every slot (the kernel's lane -> step map,
    csrc/control_wave_impl.hpp)"""
    S = (T + 63) // 64
    r_top = T - 64 * (S - 1)
    top_heavy = S > 1 and r_top <= 8
    q16 = r_top if top_heavy else ((T // S) & ~15)
    rem = T - S * q16
    sc = S - 1 if top_heavy else (rem + 15) >> 4
    return [q16 + ((rem - j + sc - 1) // sc if j < sc else 0) for j in range(S)]


def limits(model, scale):
    from tests.gpu_util import MODELS
    return np.array(MODELS[model][3]) * scale


def make_engine(model, K, T, scale):
    from ergodic_exploration_amd import capi
    from tests.gpu_util import MAP_BOUNDS, MEANS, MODELS, SIGMAS
    _, em, rdiag, _ = MODELS[model]
    lim = limits(model, scale)
    # the engine takes T = trunc(horizon / dt): half a step of slack keeps the quotient off the integer
    eng = capi.Engine(capi.make_config(em, DT, (T + 0.5) * DT, 0.1, 1.0, K, np.diag(rdiag), -lim, lim))
    eng.set_target_gaussians(MEANS, SIGMAS)
    eng.config_domain(MAP_BOUNDS)
    assert eng.T == T, (eng.T, T)
    return eng


def inputs(model, K, T, scale):
    """(pose per step [N_STEPS, B, 3], controls [B, T, 3]) of a case, from its seed"""
    from tests.gpu_util import random_poses
    rng = np.random.default_rng(2003 * K + T + (7 if model == "omni" else 0) + (100000 if scale != 1.0 else 0))
    pose0 = random_poses(rng, B)
    seq = pose0[None] + np.cumsum(rng.normal(scale=0.02, size=(N_STEPS, B, 3)), axis=0)
    ut0 = rng.uniform(-0.4, 0.4, (B, T, 3))
    if model == "simple_cart":
        ut0[:, :, 1] = 0.0
    return seq, ut0


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def run_case(model, K, T, scale, with_ck, one_launch=True):
    """three steps, in one launch or in three calls of one step; {"ck": [B, K^2] (with_ck only; the last step's),
    "ut": [B, T, 3], "u0": [N_STEPS, B, 3]}"""
    import torch
    eng = make_engine(model, K, T, scale)
    seq, ut0 = inputs(model, K, T, scale)
    d_seq, d_ut = _dev(seq), _dev(ut0)
    d_u0 = torch.full((N_STEPS, B, 3), float("nan"), dtype=torch.float64, device="cuda")
    d_ck = torch.full((B, eng.K2), float("nan"), dtype=torch.float64, device="cuda") if with_ck else None
    if one_launch:
        eng.control_batch(B, d_seq, d_ut, d_u0, ck=d_ck, n_steps=N_STEPS, pose_step_stride=B, u0_step_stride=B)
    else:
        for n in range(N_STEPS):
            eng.control_batch(B, d_seq[n], d_ut, d_u0[n], ck=d_ck)
    torch.cuda.synchronize()
    eng.close()
    out = {"ut": d_ut.cpu().numpy(), "u0": d_u0.cpu().numpy()}
    if with_ck:
        out["ck"] = d_ck.cpu().numpy()
    return out


def on_limits(model, scale, ut):
    """(share of the clamped components of ut that sit on a limit, some sit on umin, some sit on umax)"""
    lim = limits(model, scale)
    comp = [r for r in range(3) if lim[r] > 0.0]
    v = ut[..., comp]
    at_max, at_min = v == lim[comp], v == -lim[comp]
    return float((at_max | at_min).mean()), bool(at_min.any()), bool(at_max.any())


def check_shapes():
    """the horizons reach what they are here for"""
    up = lambda T: [n - 32 for n in lanes_in_slot(T)]  # noqa: E731  valid rows of the upper halves
    assert lanes_in_slot(193) == [64, 64, 64, 1]
    assert all(0 < n < 32 for n in up(100)) and len(up(100)) == 2, up(100)
    assert all(0 < n < 32 for n in up(150)) and len(up(150)) == 3, up(150)
    assert all(32 < n < 64 for T in (100, 150) for n in lanes_in_slot(T))
    assert lanes_in_slot(64) == [64]
    assert len(lanes_in_slot(20)) == 1 and 0 < lanes_in_slot(20)[0] < 32
    assert lanes_in_slot(200) == [64, 64, 64, 8]


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    check_shapes()
    arrays = {}
    for case in CASES:
        k = case_key(*case)
        a, b = run_case(*case, True), run_case(*case, False)
        for name in ("ck", "ut", "u0"):
            assert np.isfinite(a[name]).all(), (k, name)
            arrays["%s_%s" % (k, name)] = a[name]
        for name in ("ut", "u0"):
            arrays["%s_%s_nock_xor" % (k, name)] = bits(a[name]) ^ bits(b[name])
        share, lo, hi = on_limits(case[0], case[3], a["ut"])
        print("%-28s on a limit: %.3f of the clamped controls (umin %s, umax %s)" % (k, share, lo, hi))
        if case in TIGHT_CASES:
            assert share > 0.5 and lo and hi, (k, share, lo, hi)
    np.savez_compressed(path, **arrays)
    print("%s: %d arrays, %d bytes" % (path, len(arrays), os.path.getsize(path)))


if __name__ == "__main__":
    main()

"""A last slot that holds no point in lanes 32..63 (slot 3 of T = 193 .. 200) runs no upper half-pass in the block
contraction of the fp64 K = 5 / 10 wavefront kernel, and its all-zero tile is not staged (csrc/control_wave_impl.hpp, the
software-pipelined kBlock4 loop).  The LDS tiles are handed from slot to slot and from step to step, so what is checked here
is that nothing of a step depends on what the skipped stores would have left: three receding-horizon steps in one launch
equal three separate calls bitwise, at T = 200 (the short last slot) and T = 130 (every slot has an upper half), K = 5 and
10, both models, B = 5 (a partial workgroup and wavefronts 0 .. 3 of a full one).  Parity with the oracle at these horizons
is tests/test_gpu_control_parity.py::test_top_heavy_horizons_and_cooperative_last_slot.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.gpu_util import make_pair, random_poses
from tests.test_gpu_control_parity import dev

pytestmark = pytest.mark.gpu

B = 5


# tests/test_gpu_multi_step.py::test_steps_in_one_launch_equal_separate_calls already runs (simple_cart, K = 10, T = 200); its
# other wavefront-kernel fp64 cases are (omni, 10, T = 195) and (omni, 5, T = 5), none of the shapes below
@pytest.mark.parametrize("model,K,horizon", [
    ("omni", 10, 20.0), ("simple_cart", 5, 20.0), ("omni", 5, 20.0),
    ("simple_cart", 10, 13.0), ("omni", 10, 13.0), ("simple_cart", 5, 13.0), ("omni", 5, 13.0),
])
def test_three_steps_in_one_launch_equal_three_calls_bitwise(model, K, horizon):
    n_steps = 3
    eng, _ = make_pair(model, K, horizon, n_oracles=0)
    T = eng.T
    assert T == int(round(horizon * 10))
    rng = np.random.default_rng(31 * K + T)
    pose0 = random_poses(rng, B)
    seq = pose0[None] + np.cumsum(rng.normal(scale=0.02, size=(n_steps, B, 3)), axis=0)
    ut0 = rng.uniform(-0.4, 0.4, (B, T, 3))
    if model == "simple_cart":
        ut0[:, :, 1] = 0.0
    d_seq = dev(seq)
    ut_a, u0_a = dev(ut0), torch.empty((n_steps, B, 3), dtype=torch.float64, device="cuda")
    for n in range(n_steps):
        eng.control_batch(B, d_seq[n], ut_a, u0_a[n])
    ut_b = dev(ut0)
    u0_b = torch.full((n_steps, B, 3), float("nan"), dtype=torch.float64, device="cuda")
    eng.control_batch(B, d_seq, ut_b, u0_b, n_steps=n_steps, pose_step_stride=B, u0_step_stride=B)
    torch.cuda.synchronize()
    eng.close()
    assert not torch.equal(ut_b, dev(ut0))   # (something was computed)
    assert torch.equal(ut_a, ut_b) and torch.equal(u0_a, u0_b)

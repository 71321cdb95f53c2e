"""Every element of D = lambda (c - phi) reaches the right multiply-add of the gradient when D is held in registers (fp64
K = 5 / 10 wavefront kernel, csrc/control_wave_regd.inc: element e = k2 K + k1 in lane e % 16, register e / 16, taken by
DPP row broadcast).  The shared c_k is phi + 0.5 e_m (d_ck_shared), so D is one-hot: a broadcast from the wrong lane or
register, or one that feeds the wrong accumulator, changes edx by the whole of that element's term.

  * every m at K = 10 with T = 72 (two slots, no cooperative last slot) and at K = 5 with T = 70, B = 3, both models;
  * at T = 200 the elements on the register boundaries -- slots 0 .. 2 read registers, the cooperative last slot reads LDS;
  * every case once with edx requested (the instances with stage outputs) and once with ut / u0 only (the timed instances).

Against the oracle with eo_control_set_shared_ck, on the bars of the parity tests: 1e-9 max(1, |stage|).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.gpu_util import MAP_BOUNDS, make_pair, random_poses
from tests.test_gpu_control_parity import TOL, dev

pytestmark = pytest.mark.gpu

B = 3
EDGES = {10: [0, 15, 16, 31, 32, 47, 48, 63, 64, 79, 80, 95, 96, 99], 5: [0, 15, 16, 24]}


def scaled(got, want):
    """difference on the parity tests' scale: max |got - want| / max(1, |stage|)"""
    return float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))


@pytest.mark.parametrize("model", ["simple_cart", "omni"])
@pytest.mark.parametrize("K,horizon,elements", [
    (10, 7.2, list(range(100))), (5, 7.0, list(range(25))), (10, 20.0, EDGES[10]), (5, 20.0, EDGES[5]),
])
def test_one_hot_D_against_oracle(model, K, horizon, elements):
    eng, ors = make_pair(model, K, horizon, n_oracles=B)
    T, K2 = eng.T, eng.K2
    assert T == int(round(horizon * 10)) and K2 == K * K
    rng = np.random.default_rng(977 * K + T)
    poses = random_poses(rng, B)
    ut0 = rng.uniform(-0.4, 0.4, (B, T, 3))
    if model == "simple_cart":
        ut0[:, :, 1] = 0.0
    phik = np.array(ors[0].phik, dtype=np.float64).reshape(-1)
    assert phik.shape == (K2,)
    d_pose = dev(poses)
    d_u0 = torch.empty((B, 3), dtype=torch.float64, device="cuda")
    d_edx = torch.empty((B, T, 3), dtype=torch.float64, device="cuda")
    worst = {"edx": 0.0, "ut": 0.0, "u0": 0.0, "ut_timed": 0.0, "u0_timed": 0.0}
    for m in elements:
        shared = phik.copy()
        shared[m] += 0.5
        d_shared = dev(shared)
        want = []
        for b in range(B):
            ors[b].ut = ut0[b].T.copy()
            ors[b].set_shared_ck(shared)
            u, st = ors[b].control(MAP_BOUNDS, poses[b], None, stages=True)
            want.append((np.array(u), np.array(st["edx"]), np.array(st["ut"])))
            # the element's term is there to be misplaced (m = 0: k1 sin(0) = k2 sin(0) = 0, no term)
            assert m == 0 or np.abs(want[-1][1]).max() > 0.0
        for timed in (False, True):
            d_ut = dev(ut0)
            d_edx.fill_(float("nan"))
            eng.control_batch(B, d_pose, d_ut, d_u0, ck_shared=d_shared, **({} if timed else {"edx": d_edx}))
            torch.cuda.synchronize()
            ut, u0 = d_ut.cpu().numpy(), d_u0.cpu().numpy()
            edx = d_edx.cpu().numpy()
            sfx = "_timed" if timed else ""
            for b in range(B):
                u, e, w = want[b]
                errs = {"ut" + sfx: scaled(ut[b].T, w), "u0" + sfx: scaled(u0[b], u)}
                if not timed:
                    errs["edx"] = scaled(edx[b].T, e)
                for k, v in errs.items():
                    worst[k] = max(worst[k], v)
                    assert v <= TOL, (model, K, T, m, b, k, v)
    eng.close()
    print("one-hot D", model, K, T, "%d elements" % len(elements), {k: "%.2e" % v for k, v in worst.items()})

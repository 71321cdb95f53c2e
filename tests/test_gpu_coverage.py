"""Coverage of a fleet's history on the device (include/ergodic_amd.h: eea_replay_history_records, eea_records_metric;
csrc/coverage_kernel.hip): the sum record of every robot's whole stored history and the ergodic metric
eps = sum_k lamda_k (c_k - phi_k)^2 of sum records.

Checker: the oracle, not the engine -- c_k from pyoracle.traj_coeff (Basis::trajCoeff) on the shifted poses, phi_k and lamda_k
from an oracle control object after the same set_target / config_target.  Two-Gaussian target, a domain with xmin, ymin != 0,
poses from a box that overhangs the domain on every side.

Bounds: c_k 1e-11 (fp64, the project's TOL_CK) and 1e-5 (fp32 at <= 300 points, the project's fp32 c_k bound); eps
8 K^2 1e-11: |c|, |phi| <= 1 and lamda <= 1, so |d eps| <= sum 2 |c - phi| (|dc| + |dphi|) <= K^2 2 2 (1e-11 + 1e-11)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pyoracle as po
from ergodic_exploration_amd import capi
from tests.gpu_util import MAP_BOUNDS, make_pair

pytestmark = pytest.mark.gpu

TOL_CK, TOL_CK_F32 = 1e-11, 1e-5
CAPACITY = 1024
# the edges of the lane loop (64 poses per pass), of the 4-pose matrix-instruction step and of a full store
COUNTS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 300, 1000, CAPACITY]
BIGGER = (-2.0, 13.0, -1.5, 7.0)   # the map after it has grown: another lx, ly and map_pos
SENTINEL = -7.0


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _poses(counts, dtype=np.float64, seed=3):
    """[ticks][B][3]: x, y from a box that overhangs MAP_BOUNDS by 2 m on every side"""
    rng = np.random.default_rng(seed)
    ticks, B = max(max(counts), 1), len(counts)
    p = np.stack([rng.uniform(MAP_BOUNDS[0] - 2.0, MAP_BOUNDS[1] + 2.0, (ticks, B)),
                  rng.uniform(MAP_BOUNDS[2] - 2.0, MAP_BOUNDS[3] + 2.0, (ticks, B)), rng.uniform(-np.pi, np.pi, (ticks, B))], 2)
    return p.astype(dtype)


def _fill(poses, counts, capacity=CAPACITY):
    """a device memory filled to ragged per-robot counts through masks (as _ragged of tests/test_gpu_replay_memory.py)"""
    ticks, B = max(max(counts), 1), len(counts)
    masks = (np.arange(ticks)[:, None] < np.asarray(counts)[None, :]).astype(np.int32)
    mem = capi.ReplayMemory(B, capacity, 16, seed=1, real_size=poses.dtype.itemsize)
    d_poses, d_masks = _dev(poses), _dev(masks)
    for t in range(max(counts)):
        mem.append(d_poses[t], d_masks[t])
    return mem


def _oracle_ck(poses, counts, K, bounds):
    """per robot: Basis::trajCoeff of its stored poses shifted by map_pos (None for a robot without poses)"""
    lx, ly = bounds[1] - bounds[0], bounds[3] - bounds[2]
    out = []
    for b, n in enumerate(counts):
        xy = poses[:n, b, :2].astype(np.float64) - np.array([bounds[0], bounds[2]])
        out.append(po.traj_coeff(lx, ly, K, xy.T.copy()) if n else None)
    return out


def _records(mem, eng, dtype=torch.float64):
    rec = torch.full((mem.B, eng.ck_record_len), SENTINEL, dtype=dtype, device="cuda")
    mem.history_records(eng, rec)
    torch.cuda.synchronize()
    return rec


def _check_records(rec, counts, want, K, tol):
    rec = rec.cpu().numpy().astype(np.float64)
    worst = 0.0
    for b, n in enumerate(counts):
        assert rec[b, K * K] == n, (b, rec[b, K * K], n)
        assert (rec[b, K * K + 1:] == 0.0).all(), b
        if n == 0:
            assert (rec[b] == 0.0).all()
        else:
            err = np.abs(rec[b, :K * K] / n - want[b]).max()
            worst = max(worst, err)
            assert err <= tol, (b, n, err)
    print("K = %d: max |rec / n - c_k(oracle)| = %.3e (bound %.0e)" % (K, worst, tol))


@pytest.fixture(scope="module")
def fleet():
    """the ragged fleet of test 1: fp64, K = 10, one memory, its records and the oracle's c_k, phi_k, lamda_k"""
    K = 10
    eng, (orc,) = make_pair("omni", K, 1.0)
    poses = _poses(COUNTS)
    mem = _fill(poses, COUNTS)
    ck = _oracle_ck(poses, COUNTS, K, MAP_BOUNDS)
    rec = _records(mem, eng)
    f = dict(K=K, eng=eng, orc=orc, poses=poses, mem=mem, ck=ck, rec=rec, phik=np.array(orc.phik), lamdak=np.array(orc.lamdak))
    yield f
    mem.close()
    eng.close()


def _eps(ck, phik, lamdak):
    return float((lamdak * (ck - phik) ** 2).sum())


def test_ragged_fleet_against_the_oracle(fleet):
    """1. counts 0 .. capacity, fp64, K = 10: count exact, padding exactly 0, the empty robot all zeros, c_k to 1e-11"""
    assert fleet["mem"].counts()[0].tolist() == COUNTS
    _check_records(fleet["rec"], COUNTS, fleet["ck"], fleet["K"], TOL_CK)


@pytest.mark.parametrize("K", [5, 20])
def test_basis_sizes(K):
    """2. K = 5 (a tile three quarters empty) and K = 20 (2 x 2 tiles) at counts 1, 65, 300"""
    counts = [1, 65, 300]
    eng, _ = make_pair("omni", K, 1.0)
    poses = _poses(counts, seed=K)
    mem = _fill(poses, counts, capacity=512)
    _check_records(_records(mem, eng), counts, _oracle_ck(poses, counts, K, MAP_BOUNDS), K, TOL_CK)
    mem.close()
    eng.close()


def test_fp32_engine_with_an_fp32_store():
    """3. counts <= 300 (where the project's fp32 c_k bound 1e-5 is held by its own tests)"""
    K, counts = 10, [0, 1, 3, 64, 65, 130, 300]
    eng, _ = make_pair("omni", K, 1.0, precision=capi.PREC_F32)
    poses = _poses(counts, dtype=np.float32, seed=32)
    mem = _fill(poses, counts, capacity=300)
    rec = _records(mem, eng, torch.float32)
    _check_records(rec, counts, _oracle_ck(poses, counts, K, MAP_BOUNDS), K, TOL_CK_F32)
    mem.close()
    eng.close()


def test_metric_against_numpy_on_the_oracles_coefficients(fleet):
    """4. eps per record against numpy fp64 on the oracle's c_k, phi_k, lamda_k; the empty robot gives sum lamda phi^2; d_ck
    is rec / n to 1 ulp"""
    K, eng, rec, B = fleet["K"], fleet["eng"], fleet["rec"], len(COUNTS)
    eps = torch.full((B,), SENTINEL, dtype=torch.float64, device="cuda")
    ck = torch.full((B, K * K), SENTINEL, dtype=torch.float64, device="cuda")
    capi.records_metric(eng, rec, eps, ck=ck)
    eps_only = torch.full((B,), SENTINEL, dtype=torch.float64, device="cuda")
    capi.records_metric(eng, rec, eps_only)
    torch.cuda.synchronize()
    eps, ck, h_rec = eps.cpu().numpy(), ck.cpu().numpy(), rec.cpu().numpy()
    assert np.array_equal(eps, eps_only.cpu().numpy())
    bound = 8 * K * K * 1e-11
    for b, n in enumerate(COUNTS):
        want_ck = fleet["ck"][b] if n else np.zeros(K * K)
        want = _eps(want_ck, fleet["phik"], fleet["lamdak"])
        print("robot %d (n = %d): eps = %.15g, oracle %.15g, diff %.3e (bound %.1e)" % (b, n, eps[b], want, abs(eps[b] - want), bound))
        assert abs(eps[b] - want) <= bound
        quot = h_rec[b, :K * K] / n if n else np.zeros(K * K)
        assert (np.abs(ck[b] - quot) <= np.spacing(np.abs(quot))).all(), b
    assert (ck[0] == 0.0).all() and abs(eps[0] - float((fleet["lamdak"] * fleet["phik"] ** 2).sum())) <= bound


def test_fleet_metric_through_the_record_sum(fleet):
    """5. coverage(): the fleet's eps against the oracle's trajCoeff of all robots' poses concatenated; element K^2 of the
    fleet record is sum n_b; the per-robot eps are those of records_metric"""
    K, eng, mem = fleet["K"], fleet["eng"], fleet["mem"]
    eps, eps_fleet = mem.coverage(eng)
    torch.cuda.synchronize()
    ws = mem._coverage_ws
    again = mem.coverage(eng)
    torch.cuda.synchronize()
    assert mem._coverage_ws is ws and again[0] is eps and again[1] is eps_fleet    # workspaces: once per object, not per call
    rec, fleet_rec = (t.cpu().numpy() for t in mem.coverage_records)
    assert np.array_equal(rec, fleet["rec"].cpu().numpy())
    assert fleet_rec[K * K] == sum(COUNTS) and (fleet_rec[K * K + 1:] == 0.0).all()
    everything = np.concatenate([fleet["poses"][:n, b, :2] for b, n in enumerate(COUNTS)]) - np.array([MAP_BOUNDS[0], MAP_BOUNDS[2]])
    want_ck = po.traj_coeff(MAP_BOUNDS[1] - MAP_BOUNDS[0], MAP_BOUNDS[3] - MAP_BOUNDS[2], K, everything.T.copy())
    assert np.abs(fleet_rec[:K * K] / sum(COUNTS) - want_ck).max() <= TOL_CK
    want = _eps(want_ck, fleet["phik"], fleet["lamdak"])
    got = float(eps_fleet.cpu().numpy()[0])
    print("fleet eps = %.15g, oracle %.15g, diff %.3e" % (got, want, abs(got - want)))
    assert abs(got - want) <= 8 * K * K * 1e-11
    per_robot = torch.empty(len(COUNTS), dtype=torch.float64, device="cuda")
    capi.records_metric(eng, fleet["rec"], per_robot)
    torch.cuda.synchronize()
    assert torch.equal(per_robot, eps)


def test_bitwise_reproducible_and_independent_of_the_sharding(fleet):
    """6. the call twice: equal bits; memories holding robots [0, 5) and [5, 13): bitwise the rows of the one memory"""
    eng, rec = fleet["eng"], fleet["rec"]
    assert torch.equal(_records(fleet["mem"], eng), rec)
    parts = []
    for lo, hi in ((0, 5), (5, len(COUNTS))):
        counts = COUNTS[lo:hi]
        mem = _fill(np.ascontiguousarray(fleet["poses"][:max(counts), lo:hi]), counts)
        parts.append(_records(mem, eng))
        mem.close()
    assert torch.equal(torch.cat(parts), rec)


def test_records_follow_a_domain_change(fleet):
    """7. after the map has grown (eea_config_domain to a larger extent) the SAME store gives the records of the new lx, ly
    and map_pos -- what a running sum kept at append time would get wrong"""
    K, mem = fleet["K"], fleet["mem"]
    eng, (orc,) = make_pair("omni", K, 1.0)
    before = _records(mem, eng)
    assert torch.equal(before, fleet["rec"])          # (another engine, the same domain: the same bits)
    assert eng.config_domain(BIGGER)                  # rebuilt
    orc.config_target(BIGGER)
    after = _records(mem, eng)
    _check_records(after, COUNTS, _oracle_ck(fleet["poses"], COUNTS, K, BIGGER), K, TOL_CK)
    h_before, h_after = before.cpu().numpy(), after.cpu().numpy()
    for b, n in enumerate(COUNTS):
        if n:
            assert np.abs(h_after[b, :K * K] - h_before[b, :K * K]).max() > 1e-3 * n, b
    eps = torch.empty(len(COUNTS), dtype=torch.float64, device="cuda")
    capi.records_metric(eng, after, eps)              # ... and the metric uses the rebuilt phi_k
    torch.cuda.synchronize()
    phik, lamdak = np.array(orc.phik), np.array(orc.lamdak)
    want = _eps(h_after[-1, :K * K] / COUNTS[-1], phik, lamdak)
    assert abs(float(eps[-1]) - want) <= 8 * K * K * 1e-11
    eng.close()


def test_coverage_inside_the_fleet_loop_without_a_host_round_trip():
    """8. append_sample -> tick_batch -> integrate_twist_batch for 20 ticks of 64 robots on ONE stream with coverage() every 5th
    tick and no synchronising call before the final one (every call here only enqueues; the eps tensors are copied on the
    stream) -- against the same loop with a device-wide synchronisation after every call: the eps values read at the end
    are equal (as test_fleet_loop_without_a_host_round_trip asserts its own claim)"""
    from tests.test_gpu_fleet_tick import _engine
    from tests.test_gpu_replay_memory import _scenario
    from tests.test_host_mirror import COLL, DWA
    B, batch, ticks, cap, dt, model = 64, 8, 20, 32, 0.1, "omni"
    grid_a, _, bounds, poses0 = _scenario(B, np.random.default_rng(6))
    ccfg = capi.make_collision_cfg(bounds[0], bounds[2], 0.05, grid_a.xsize, grid_a.ysize, *COLL)
    dcfg = capi.DwaCfg(*DWA[model])
    eng = _engine(model)
    eng.config_domain(bounds)
    T = eng.T
    d_grid = _dev(grid_a.data, torch.int8)
    stream = torch.cuda.Stream()

    def run(sync_every_call):
        wait = torch.cuda.synchronize if sync_every_call else (lambda: None)
        z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device="cuda")
        d_pose, d_vb = _dev(poses0), z(B, 3)
        d_ut, d_follow, d_count, d_u, d_traj = z(B, T, 3), z(B, dt=torch.int32), z(B, dt=torch.int32), z(B, 3), z(B, T, 3)
        d_valid, d_skip, d_source = z(B, dt=torch.int32), z(B, dt=torch.int32), z(B, dt=torch.int32)
        d_cols, d_n = z(B, batch, 3), z(B, dt=torch.int32)
        mem = capi.ReplayMemory(B, cap, batch, seed=99)
        seen = []
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for t in range(ticks):
                mem.append_sample(d_pose, t, d_cols, d_n, stream=stream.cuda_stream)
                wait()
                eng.tick_batch(B, d_pose, d_ut, d_follow, d_count, d_u, d_vb, d_grid, d_traj, d_valid, d_skip, ccfg, dcfg, 0.1, 0.5,
                               source=d_source, mem_cols=d_cols, n_mem=d_n, mem_stride=batch, stream=stream.cuda_stream, grid_epoch=1)
                wait()
                capi.integrate_twist_batch(d_pose, d_u, dt, stream=stream.cuda_stream)
                d_vb.copy_(d_u)
                wait()
                if t % 5 == 4:
                    eps, eps_fleet = mem.coverage(eng, stream=stream.cuda_stream)
                    seen.append((eps.clone(), eps_fleet.clone()))
                    wait()
        stream.synchronize()
        out = [(a.cpu().numpy(), float(b.cpu().numpy()[0])) for a, b in seen]
        counts = mem.counts()[0].tolist()
        mem.close()
        return out, counts

    free, free_counts = run(False)
    synced, synced_counts = run(True)
    assert free_counts == synced_counts == [ticks] * B and len(free) == len(synced) == ticks // 5
    for (a, fa), (b, fb) in zip(free, synced):
        assert np.array_equal(a, b) and fa == fb
    assert all(np.isfinite(a).all() and (a > 0).all() and fa > 0 for a, fa in free)
    assert not np.array_equal(free[0][0], free[-1][0])    # (the fleet moved: its coverage changed)
    eng.close()


def test_argument_errors_with_live_handles(fleet):
    """9. a real_size mismatch between the engine and the store: EEA_ERR_INVALID_ARGUMENT, nothing written"""
    eng = fleet["eng"]
    mem32 = capi.ReplayMemory(3, 8, 4, real_size=4)
    rec = torch.full((3, eng.ck_record_len), SENTINEL, dtype=torch.float64, device="cuda")
    with pytest.raises(capi.EngineError) as ei:
        mem32.history_records(eng, rec)
    assert ei.value.status == capi.ERR_INVALID_ARGUMENT and "real_size" in str(ei.value)
    with pytest.raises(capi.EngineError) as ei:
        fleet["mem"].history_records(eng, None)
    assert ei.value.status == capi.ERR_INVALID_ARGUMENT
    with pytest.raises(capi.EngineError) as ei:
        capi.records_metric(eng, rec[:0], rec)
    assert ei.value.status == capi.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert (rec.cpu().numpy() == SENTINEL).all()
    mem32.close()

"""The pooled replay memory on the device (include/ergodic_amd.h, eea_replay_pool_sample; csrc/replay_kernel.hip): every robot's
columns drawn from the stored poses of ALL robots of the memory object, optionally without its own, into the mem_cols / n_mem
buffers of eea_control_batch.

Checker: the numpy restatement tests/pool_restatement.py (tests/test_replay_pool.py holds it to a brute-force pool) -- columns
and n_mem BITWISE: the kernels move poses, they compute nothing in floating point.  Every column buffer starts as SENTINEL, so
"equal to the restated buffer" includes "nothing written past n_mem"."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ergodic_exploration_amd import capi
from tests import pool_restatement as pr
from tests import replay_restatement as rr
from tests.gpu_util import MAP_BOUNDS, make_pair, random_poses

pytestmark = pytest.mark.gpu

SENTINEL = -7.0   # what the column buffers hold where nothing may be written
TOL_CK, TOL = 1e-11, 1e-9   # c_k; controls -- times max(1, |stage|)


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _filled(counts, capacity, batch=4, dtype=np.float64, seed=0x5eed0000beef, robot0=0):
    """a device memory and its restatement filled to the per-robot counts through masked appends"""
    B, ticks = len(counts), int(max(counts))
    rng = np.random.default_rng(3)
    poses = rng.uniform(-3.0, 9.0, (ticks, B, 3)).astype(dtype)
    masks = (np.arange(ticks)[:, None] < np.asarray(counts)[None, :]).astype(np.int32)
    mem = capi.ReplayMemory(B, capacity, batch, seed=seed, robot0=robot0, real_size=np.dtype(dtype).itemsize)
    ref = rr.ReplayMemory(B, capacity, batch, seed=seed, robot0=robot0, dtype=dtype)
    d_poses, d_masks = _dev(poses), _dev(masks)
    for t in range(ticks):
        mem.append(d_poses[t], d_masks[t])
        ref.append(poses[t], masks[t])
    return mem, ref


def _buffers(B, stride, dtype, n0=-1):
    d_cols = torch.full((B, stride, 3), SENTINEL, dtype=_tdt(dtype), device="cuda")
    d_n = torch.full((B,), n0, dtype=torch.int32, device="cuda")
    return d_cols, d_n, np.full((B, stride, 3), SENTINEL, dtype=dtype), np.full(B, n0, dtype=np.int32)


def _pool_both(mem, ref, draw, n_cols, stride, dtype, exclude_self, accumulate=False, n0=-1):
    d_cols, d_n, cols, n = _buffers(ref.B, stride, dtype, n0)
    mem.sample_pool(draw, n_cols, d_cols, d_n, exclude_self=exclude_self, accumulate=accumulate)
    torch.cuda.synchronize()
    pr.sample_pool(ref, draw, n_cols, cols, n, exclude_self=exclude_self, accumulate=accumulate)
    return d_cols.cpu().numpy(), d_n.cpu().numpy(), cols, n


@pytest.mark.parametrize("exclude_self", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_smallest_shape(dtype, exclude_self):
    """1. five robots with an empty first one, a full store and the last robot (27 poses): 4 columns are draws, 64 columns
    take every pose of the pool in order; a second draw gives other columns"""
    counts = [0, 3, 16, 1, 7]
    mem, ref = _filled(counts, capacity=16, dtype=dtype)
    assert mem.counts()[0].tolist() == counts
    for n_cols in (4, 64):
        got, got_n, want, want_n = _pool_both(mem, ref, 5, n_cols, n_cols + 2, dtype, exclude_self)
        assert got_n.tolist() == want_n.tolist() == [min(27 - (c if exclude_self else 0), n_cols) for c in counts]
        assert np.array_equal(got, want), n_cols
        other, _, want2, _ = _pool_both(mem, ref, 6 + 2**32, n_cols, n_cols + 2, dtype, exclude_self)
        assert np.array_equal(other, want2) and np.array_equal(other, got) == (n_cols == 64)
    mem.close()


@pytest.mark.parametrize("exclude_self", [False, True])
@pytest.mark.parametrize("B", [1025, 4099])
def test_owner_search_at_its_boundaries(B, exclude_self):
    """2. more robots than the coarse table has entries (every 2nd / 8th offset is staged), counts 0 .. 4 with runs of >= 70
    robots without poses: in front, in the middle, ACROSS robot 1024 and over the last robots -- equal consecutive offsets,
    where an upper bound and a lower bound differ and a coarse / fine search can step into an empty robot"""
    rng = np.random.default_rng(B)
    counts = rng.integers(0, 5, B)
    for lo, hi in ((0, 3), (100, 180), (985, 1060), (B - 75, B)) + (((2000, 2100),) if B > 2100 else ()):
        counts[lo:min(hi, B)] = 0
    assert counts[1023] == 0 and counts[1024] == 0 and counts[B - 1] == 0 and counts[0] == 0
    mem, ref = _filled(counts.tolist(), capacity=4)
    got, got_n, want, want_n = _pool_both(mem, ref, 9, 8, 8, np.float64, exclude_self)
    assert got_n.tolist() == want_n.tolist() == [8] * B
    assert np.array_equal(got, want)
    owner, _, _ = pr.pool_indices(ref.count, ref.seed, 0, 9, 8, exclude_self)
    assert len(np.unique(owner)) > B // 2 and (ref.count[owner] > 0).all()   # the draws reach all over the fleet
    mem.close()


def test_degenerate_pools():
    """3. one robot that leaves itself out: nothing to draw from; a fleet whose only non-empty robot is robot 2: robot 2 gets
    nothing without itself, the others its poses -- all five in order at 8 columns, draws at 3"""
    mem, ref = _filled([6], capacity=8)
    got, got_n, _, _ = _pool_both(mem, ref, 1, 4, 4, np.float64, True)
    assert got_n.tolist() == [0] and (got == SENTINEL).all()
    got, got_n, want, want_n = _pool_both(mem, ref, 1, 4, 4, np.float64, False)   # ... with itself: its own memory, pooled
    assert got_n.tolist() == [4] and np.array_equal(got, want)
    mem.close()
    mem, ref = _filled([0, 0, 5, 0, 0, 0], capacity=8)
    for exclude_self in (False, True):
        for n_cols in (8, 3):
            got, got_n, want, want_n = _pool_both(mem, ref, 2, n_cols, 8, np.float64, exclude_self)
            assert got_n.tolist() == want_n.tolist() == [0 if exclude_self and b == 2 else min(5, n_cols) for b in range(6)]
            assert np.array_equal(got, want)
        assert (got[2] == SENTINEL).all() == exclude_self
    mem.close()
    mem, ref = _filled([0, 0, 0], capacity=2, seed=1)    # (never appended to: max count 0)
    got, got_n, _, _ = _pool_both(mem, ref, 2, 4, 4, np.float64, False)
    assert got_n.tolist() == [0, 0, 0] and (got == SENTINEL).all()
    mem.close()


def test_accumulate_puts_the_pool_behind_the_own_columns():
    """4. append_sample at batch size 4, then the pooled call with accumulate on the same buffers: the own columns stay bit for
    bit, the pooled columns are those of the plain call, n_mem is the sum; a stride one short drops the last column only; a
    row that is full already (or claims more) gets nothing; a negative count is an empty row"""
    counts, batch, n_cols, B = [0, 3, 16, 1, 7], 4, 6, 5
    mem, ref = _filled(counts, capacity=16, batch=batch)
    pose = np.random.default_rng(8).uniform(-3.0, 9.0, (B, 3))
    d_own, d_n_own, cols, n = _buffers(B, batch + n_cols, np.float64)
    mem.append_sample(_dev(pose), 12, d_own, d_n_own)
    ref.append_sample(pose, 12, cols, n)
    d_both, d_n_both = d_own.clone(), d_n_own.clone()
    mem.sample_pool(12, n_cols, d_both, d_n_both, exclude_self=True, accumulate=True)
    plain, plain_n, _, _ = _pool_both(mem, ref, 12, n_cols, n_cols, np.float64, True)
    pr.sample_pool(ref, 12, n_cols, cols, n, exclude_self=True, accumulate=True)
    own, n_own, both, n_both = d_own.cpu().numpy(), d_n_own.cpu().numpy(), d_both.cpu().numpy(), d_n_both.cpu().numpy()
    assert n_own.tolist() == [1, 4, 4, 2, 4] and plain_n.tolist() == [n_cols] * B
    assert n_both.tolist() == (n_own + plain_n).tolist() == n.tolist()
    for b in range(B):
        assert np.array_equal(both[b, :n_own[b]], own[b, :n_own[b]])
        assert np.array_equal(both[b, n_own[b]:n_both[b]], plain[b]) and (both[b, n_both[b]:] == SENTINEL).all()
    assert np.array_equal(both, cols)
    # one column short: the robots with four own columns lose their last pooled column, nothing else changes
    d_short, d_n_short = d_own[:, :batch + n_cols - 1].contiguous(), d_n_own.clone()
    mem.sample_pool(12, n_cols, d_short, d_n_short, exclude_self=True, accumulate=True)
    short, n_short = d_short.cpu().numpy(), d_n_short.cpu().numpy()
    assert n_short.tolist() == [7, 9, 9, 8, 9]
    for b in range(B):
        assert np.array_equal(short[b, :n_short[b]], both[b, :n_short[b]]) and (short[b, n_short[b]:] == SENTINEL).all()
    # rows that are full, claim more than the stride, or claim less than nothing
    for n0, want_n in ((n_cols, n_cols), (n_cols + 3, n_cols + 3), (-2, n_cols)):
        got, got_n, want, want_n_ref = _pool_both(mem, ref, 12, n_cols, n_cols, np.float64, True, accumulate=True, n0=n0)
        assert got_n.tolist() == want_n_ref.tolist() == [want_n] * B and np.array_equal(got, want)
        assert (got == SENTINEL).all() == (n0 > 0) and (n0 > 0 or np.array_equal(got, plain))
    mem.close()


def test_draws_are_those_of_the_global_robot_id():
    """5. robot0 = 7: robot b draws what the restatement draws for the global id 7 + b -- the columns robots 7 .. 11 of a
    memory that starts at robot 0 would draw from this pool, and not those of robots 0 .. 4"""
    counts = [9, 3, 16, 1, 7]
    mem, ref = _filled(counts, capacity=16, robot0=7)
    got, got_n, want, _ = _pool_both(mem, ref, 5, 4, 4, np.float64, False)
    assert np.array_equal(got, want) and got_n.tolist() == [4] * 5
    r64 = pr.pool_r64(ref.seed, 5, 7 + np.arange(5), 4)
    owner, slot = pr.owner_slot(pr.offsets(counts), [[(int(r) * 36) >> 64 for r in row] for row in r64])
    assert np.array_equal(got, ref.store[owner, slot])
    ref.robot0 = 0
    cols0, n0 = np.full((5, 4, 3), SENTINEL), np.zeros(5, dtype=np.int32)
    pr.sample_pool(ref, 5, 4, cols0, n0)
    assert all(not np.array_equal(cols0[b], got[b]) for b in range(5))
    mem.close()


def test_counts_are_those_the_stream_holds():
    """6. append, pooled sample, append, pooled sample on ONE stream with no synchronisation in between: every sample sees
    the counts (and poses) of the appends in front of it, and only those"""
    B, cap = 7, 8
    mem = capi.ReplayMemory(B, cap, 4, seed=21)
    ref = rr.ReplayMemory(B, cap, 4, seed=21)
    rng = np.random.default_rng(2)
    poses, masks = rng.uniform(-3.0, 9.0, (4, B, 3)), np.array([[1, 0, 1, 1, 0, 0, 1], [1, 1, 0, 1, 0, 1, 1]] * 2, dtype=np.int32)
    d_poses, d_masks = _dev(poses), _dev(masks)
    dev_out, ref_out = [_buffers(B, 5, np.float64)[:2] for _ in range(4)], [_buffers(B, 5, np.float64)[2:] for _ in range(4)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for t in range(4):
            mem.append(d_poses[t], d_masks[t], stream=stream.cuda_stream)
            mem.sample_pool(t, 5, *dev_out[t], exclude_self=bool(t % 2), stream=stream.cuda_stream)
    stream.synchronize()
    for t in range(4):
        ref.append(poses[t], masks[t])
        pr.sample_pool(ref, t, 5, *ref_out[t], exclude_self=bool(t % 2))
        assert np.array_equal(dev_out[t][0].cpu().numpy(), ref_out[t][0]), t
        assert dev_out[t][1].cpu().numpy().tolist() == ref_out[t][1].tolist(), t
    assert ref_out[0][1].tolist() == [4] * B and ref_out[3][1].tolist() == [5] * B   # the pool grew from 4 poses past 5
    mem.close()


def test_the_control_call_takes_own_and_pooled_columns():
    """7. BASELINE configs[0] (Omni, K = 5, T = 5), 8 robots: the own columns (batch 4) with the pooled ones behind them go into
    eea_control_batch; the oracle is fed the restated columns.  fp64 bars of DESIGN.md section 0: c_k <= 1e-11, controls
    <= 1e-9, times max(1, |stage|)"""
    B, batch, n_cols = 8, 4, 6
    counts = [0, 3, 16, 1, 7, 5, 2, 9]
    rng = np.random.default_rng(17)
    eng, ors = make_pair("omni", 5, 0.5, n_oracles=B)
    T = eng.T
    assert T == 5
    mem = capi.ReplayMemory(B, 16, batch, seed=99)
    ref = rr.ReplayMemory(B, 16, batch, seed=99)
    for t in range(max(counts)):
        p, mask = random_poses(rng, B), (t < np.asarray(counts)).astype(np.int32)
        mem.append(_dev(p), _dev(mask))
        ref.append(p, mask)
    poses, ut0 = random_poses(rng, B), rng.uniform(-0.5, 0.5, (B, T, 3))
    d_cols, d_n, cols, n = _buffers(B, batch + n_cols, np.float64)
    mem.sample(3, d_cols, d_n)
    mem.sample_pool(3, n_cols, d_cols, d_n, exclude_self=True, accumulate=True)
    ref.sample(3, cols, n)
    pr.sample_pool(ref, 3, n_cols, cols, n, exclude_self=True, accumulate=True)
    d_ut, d_u0 = _dev(ut0), torch.empty((B, 3), dtype=torch.float64, device="cuda")
    d_ck, d_status = torch.empty((B, eng.K2), dtype=torch.float64, device="cuda"), torch.full((B,), -1, dtype=torch.int32, device="cuda")
    eng.control_batch(B, _dev(poses), d_ut, d_u0, mem_cols=d_cols, n_mem=d_n, mem_stride=batch + n_cols, ck=d_ck, status=d_status)
    torch.cuda.synchronize()
    assert np.array_equal(d_cols.cpu().numpy(), cols) and d_n.cpu().numpy().tolist() == n.tolist() == [min(c, batch) + n_cols for c in counts]
    assert (d_status.cpu().numpy() == 0).all()
    ck, ut, u0 = d_ck.cpu().numpy(), d_ut.cpu().numpy(), d_u0.cpu().numpy()
    for b in range(B):
        ors[b].ut = ut0[b].T
        u, st = ors[b].control(MAP_BOUNDS, poses[b], cols[b, :n[b]].T.copy(), stages=True)
        for name, got, want, tol in (("ck", ck[b], st["ck"], TOL_CK), ("ut", ut[b].T, st["ut"], TOL), ("u0", u0[b], u, TOL)):
            err, bar = np.abs(got - want).max(), tol * max(1.0, np.abs(want).max())
            print("robot %d %s: |delta| %.3g, bar %.3g" % (b, name, err, bar))
            assert err <= bar, (b, name, err, bar)
    mem.close()
    eng.close()


def test_closed_loop_without_a_host_round_trip():
    """8. 64 robots x 20 ticks of append_sample -> pooled sample (without the robot's own poses, accumulated) -> control_batch
    -> integrate_twist_batch on ONE stream with NO synchronisation inside the loop, against the same loop with a
    synchronisation, the columns restated on the host and uploaded every tick: poses, warm starts, twists, columns, n_mem and
    counts bitwise.  Batch 4: the own columns are draws from tick 5 on; the pool (63 (t + 1) poses) is always drawn from"""
    B, batch, n_cols, ticks, cap, dt, seed = 64, 4, 6, 20, 32, 0.1, 4242
    stride = batch + n_cols
    eng, _ = make_pair("omni", 5, 0.5, n_oracles=0)
    T = eng.T
    poses0 = random_poses(np.random.default_rng(6), B)
    stream = torch.cuda.Stream()

    def run(on_device):
        d_pose = _dev(poses0)
        d_ut, d_u0 = torch.zeros((B, T, 3), dtype=torch.float64, device="cuda"), torch.zeros((B, 3), dtype=torch.float64, device="cuda")
        d_cols, d_n, cols, n = _buffers(B, stride, np.float64, n0=0)
        mem = capi.ReplayMemory(B, cap, batch, seed=seed) if on_device else None
        ref = None if on_device else rr.ReplayMemory(B, cap, batch, seed=seed)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for t in range(ticks):
                if on_device:
                    mem.append_sample(d_pose, t, d_cols, d_n, stream=stream.cuda_stream)
                    mem.sample_pool(t, n_cols, d_cols, d_n, exclude_self=True, accumulate=True, stream=stream.cuda_stream)
                else:
                    stream.synchronize()
                    ref.append_sample(d_pose.cpu().numpy(), t, cols, n)
                    pr.sample_pool(ref, t, n_cols, cols, n, exclude_self=True, accumulate=True)
                    d_cols.copy_(torch.from_numpy(cols))
                    d_n.copy_(torch.from_numpy(n))
                eng.control_batch(B, d_pose, d_ut, d_u0, mem_cols=d_cols, n_mem=d_n, mem_stride=stride, stream=stream.cuda_stream)
                capi.integrate_twist_batch(d_pose, d_u0, dt, stream=stream.cuda_stream)
        stream.synchronize()
        counts = mem.counts()[0] if on_device else ref.count
        if on_device:
            mem.close()
        return [x.cpu().numpy() for x in (d_pose, d_ut, d_u0, d_cols, d_n)] + [np.asarray(counts, dtype=np.int64)]

    dev_state, host_state = run(True), run(False)
    for name, a, b in zip(("pose", "ut", "u0", "columns", "n_mem", "counts"), dev_state, host_state):
        assert np.array_equal(a, b), name
    assert dev_state[4].tolist() == [stride] * B and dev_state[5].tolist() == [ticks] * B
    assert not np.array_equal(dev_state[0], poses0)   # (the fleet moved)
    eng.close()


def test_errors_leave_the_buffers_alone():
    """9. every argument error of the header: EEA_ERR_INVALID_ARGUMENT, eea_last_error names it, nothing is written"""
    mem, _ = _filled([3, 2, 5], capacity=8)
    d_cols, d_n, _, _ = _buffers(3, 4, np.float64)
    L, h, s0 = capi.lib(), mem.h, None
    pc, pn = capi._ptr(d_cols), capi._ptr(d_n)
    for args, word in (((None, 0, 4, 0, 0, pc, pn, 4, s0), b"null"), ((h, 0, 4, 0, 0, None, pn, 4, s0), b"null"),
                       ((h, 0, 4, 0, 0, pc, None, 4, s0), b"null"), ((h, 0, 0, 0, 0, pc, pn, 4, s0), b"n_cols"),
                       ((h, 0, 0, 1, 1, pc, pn, 4, s0), b"n_cols"), ((h, 0, 5, 0, 0, pc, pn, 4, s0), b"mem_stride"),
                       ((h, 0, 4, 0, 0, pc, pn, 0, s0), b"mem_stride"), ((h, 0, 4, 0, 1, pc, pn, 0, s0), b"mem_stride")):
        assert L.eea_replay_pool_sample(*args) == capi.ERR_INVALID_ARGUMENT, args
        assert word in L.eea_last_error(), (args, L.eea_last_error())
    with pytest.raises(capi.EngineError) as ei:
        mem.sample_pool(0, 5, d_cols, d_n)                # through the wrapper: the stride of the tensor is one short
    assert ei.value.status == capi.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert (d_cols.cpu().numpy() == SENTINEL).all() and (d_n.cpu().numpy() == -1).all()
    assert mem.counts()[0].tolist() == [3, 2, 5]
    mem.sample_pool(0, 5, d_cols, d_n, accumulate=True)   # accumulate takes a stride below n_cols: it clips
    torch.cuda.synchronize()
    assert d_n.cpu().numpy().tolist() == [4, 4, 4]
    mem.close()

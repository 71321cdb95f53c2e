"""The fleet replay memory on the device (include/ergodic_amd.h, eea_replay_*; csrc/replay_kernel.hip): ReplayBuffer::append /
sampleMemory (reference buffer.cpp:54-62, 64-111) for B robots as kernels that fill the mem_cols / n_mem buffers of
eea_control_batch / eea_tick_batch.

Checker: the numpy restatement tests/replay_restatement.py (its random stream is pinned to the published Philox known answers
in tests/test_replay_memory.py) -- columns, counts and stores BITWISE: the kernels move poses, they compute nothing in floating
point.  The closed loops run on the scenario of tests/test_gpu_fleet_tick.py (its helpers, its assertions and tolerances): the
sampled regime of sampleMemory meets the fleet tick here for the first time."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pyoracle as po
from ergodic_exploration_amd import capi
from tests import replay_restatement as rr
from tests.test_gpu_fleet_tick import SOURCES, _engine
from tests.test_host_mirror import COLL, DWA, OracleExploration, _grid_with

pytestmark = pytest.mark.gpu

SENTINEL = -7.0   # what the column buffers hold where nothing may be written


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _ragged(dtype, batch, targets, capacity, seed, robot0=0):
    """a device memory and its restatement filled to ragged per-robot counts through masks"""
    B, ticks = len(targets), max(targets)
    rng = np.random.default_rng(3)
    poses = rng.uniform(-3.0, 9.0, (ticks, B, 3)).astype(dtype)
    masks = (np.arange(ticks)[:, None] < np.asarray(targets)[None, :]).astype(np.int32)
    mem = capi.ReplayMemory(B, capacity, batch, seed=seed, robot0=robot0, real_size=np.dtype(dtype).itemsize)
    ref = rr.ReplayMemory(B, capacity, batch, seed=seed, robot0=robot0, dtype=dtype)
    d_poses, d_masks = _dev(poses), _dev(masks)
    for t in range(ticks):
        mem.append(d_poses[t], d_masks[t])
        ref.append(poses[t], masks[t])
    return mem, ref


def _sample_both(mem, ref, draw, stride, dtype):
    B = ref.B
    d_cols = torch.full((B, stride, 3), SENTINEL, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
    d_n = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    mem.sample(draw, d_cols, d_n)
    torch.cuda.synchronize()
    cols, n = np.full((B, stride, 3), SENTINEL, dtype=dtype), np.full(B, -1, dtype=np.int32)
    ref.sample(draw, cols, n)
    return d_cols.cpu().numpy(), d_n.cpu().numpy(), cols, n


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_columns_equal_the_restatement_bitwise(dtype):
    """1. ragged counts (0, below the batch size, equal to it, one more, thousands; robots on both sides of a wavefront /
    workgroup boundary of the kernel), fp64 and fp32: columns and n_mem bitwise, nothing written past n_mem; the same draw
    gives the same columns, another draw others"""
    batch = 100
    targets = [0, 37, 100, 101, 2500, 4000, 1, 99, 3000, 100, 101]
    mem, ref = _ragged(dtype, batch, targets, capacity=4096, seed=0x5eed0000beef, robot0=11)
    counts, dropped = mem.counts()
    assert counts.tolist() == targets == ref.count.tolist() and dropped == 0
    for b in (1, 3, 5):
        assert np.array_equal(mem.read(b), ref.store[b, :targets[b]])
    assert np.array_equal(mem.read(5, 3990, 10), ref.store[5, 3990:4000])
    got, got_n, want, want_n = _sample_both(mem, ref, 5, batch + 4, dtype)
    assert got_n.tolist() == want_n.tolist() == [min(t, batch) for t in targets]
    assert np.array_equal(got, want)                      # (the sentinels past n_mem included)
    again, _, _, _ = _sample_both(mem, ref, 5, batch + 4, dtype)
    assert np.array_equal(again, got)
    other, other_n, want2, _ = _sample_both(mem, ref, 6 + 2**32, batch + 4, dtype)
    assert np.array_equal(other, want2) and other_n.tolist() == want_n.tolist()
    sampled = [b for b, t in enumerate(targets) if t > batch]
    assert all(not np.array_equal(other[b], got[b]) for b in sampled)
    assert all(np.array_equal(other[b], got[b]) for b in range(len(targets)) if b not in sampled)
    # argument checks with a live handle
    with pytest.raises(capi.EngineError) as ei:
        mem.sample(0, torch.empty((len(targets), batch - 1, 3), device="cuda"), torch.empty(len(targets), dtype=torch.int32, device="cuda"))
    assert ei.value.status == capi.ERR_INVALID_ARGUMENT
    with pytest.raises(capi.EngineError):
        mem.read(1, 30, 8)                                # past robot 1's 37 poses
    with pytest.raises(capi.EngineError):
        mem.read(len(targets), 0, 0)
    mem.reset()
    assert mem.counts()[0].tolist() == [0] * len(targets)
    mem.close()


def test_a_full_store_drops_and_counts():
    """2. buffer.cpp:61, "Buffer is full": further appends change nothing in the store, the counter counts them -- through
    append and through the fused append_sample"""
    B, cap, batch = 5, 6, 4
    mem = capi.ReplayMemory(B, cap, batch, seed=9)
    ref = rr.ReplayMemory(B, cap, batch, seed=9)
    rng = np.random.default_rng(1)
    for t in range(9):
        pose, mask = rng.uniform(-1.0, 1.0, (B, 3)), np.array([1, 1, t % 2, 1, 0], dtype=np.int32)
        mem.append(_dev(pose), _dev(mask))
        ref.append(pose, mask)
    counts, dropped = mem.counts()
    assert counts.tolist() == ref.count.tolist() == [6, 6, 4, 6, 0] and dropped == ref.dropped == 9
    before = [mem.read(b) for b in range(B)]
    d_cols = torch.full((B, batch, 3), SENTINEL, dtype=torch.float64, device="cuda")
    d_n = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    cols, n = np.full((B, batch, 3), SENTINEL), np.full(B, -1, dtype=np.int32)
    pose = rng.uniform(-1.0, 1.0, (B, 3))
    mem.append_sample(_dev(pose), 3, d_cols, d_n)
    ref.append_sample(pose, 3, cols, n)
    counts, dropped = mem.counts()
    assert counts.tolist() == ref.count.tolist() == [6, 6, 5, 6, 1] and dropped == ref.dropped == 12
    for b in (0, 1, 3):
        assert np.array_equal(mem.read(b), before[b]) and np.array_equal(before[b], ref.store[b])
    assert np.array_equal(d_cols.cpu().numpy(), cols) and d_n.cpu().numpy().tolist() == n.tolist() == [4, 4, 4, 4, 1]
    mem.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_append_sample_is_append_then_sample(dtype):
    """3. the fused launch against the two separate ones, bitwise, where the slot appended IN the launch is drawn: most robots
    go from 100 to n = batch size + 1 = 101 poses (70 robots x 100 draws from 101 slots: the newest one is drawn -- asserted
    on the restatement), the first ten hold 0 .. 9 poses (the newest slot is their last column), some robots are masked out"""
    batch, B = 100, 70
    targets = list(range(10)) + [100] * (B - 10)
    fused, ref = _ragged(dtype, batch, targets, capacity=128, seed=77)
    apart, _ = _ragged(dtype, batch, targets, capacity=128, seed=77)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    rng = np.random.default_rng(8)
    pose = rng.uniform(-3.0, 9.0, (B, 3)).astype(dtype)
    mask = np.ones(B, dtype=np.int32)
    mask[[4, 20, 69]] = 0
    d_pose, d_mask = _dev(pose), _dev(mask)
    out = []
    for mem in (fused, apart):
        d_cols = torch.full((B, batch, 3), SENTINEL, dtype=tdt, device="cuda")
        d_n = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        if mem is fused:
            mem.append_sample(d_pose, 12, d_cols, d_n, mask=d_mask)
        else:
            mem.append(d_pose, d_mask)
            mem.sample(12, d_cols, d_n)
        torch.cuda.synchronize()
        out.append((d_cols.cpu().numpy(), d_n.cpu().numpy(), mem.counts(), [mem.read(b) for b in range(B)]))
    cols, n = np.full((B, batch, 3), SENTINEL, dtype=dtype), np.full(B, -1, dtype=np.int32)
    ref.append_sample(pose, 12, cols, n, mask)
    slots, _ = ref.indices(12)
    newest = [b for b in range(10, B) if mask[b] and (slots[b] == 100).any()]
    assert len(newest) >= 1, "no robot draws the slot appended in the launch: the case this test is for"
    for b in newest:   # ... and what they got there is the pose of this launch
        j = int(np.nonzero(slots[b] == 100)[0][0])
        assert np.array_equal(out[0][0][b, j], pose[b])
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert out[0][2][0].tolist() == out[1][2][0].tolist() == ref.count.tolist() and out[0][2][1] == out[1][2][1] == 0
    for b in range(B):
        assert np.array_equal(out[0][3][b], out[1][3][b]) and np.array_equal(out[0][3][b], ref.store[b, :ref.count[b]])
    assert np.array_equal(out[0][0], cols) and out[0][1].tolist() == n.tolist()
    fused.close()
    apart.close()


def test_two_shards_draw_what_one_memory_draws():
    """4. two shards of B / 2 robots with the global id of their first robot give the columns of one memory of B"""
    B, batch, cap, seed, first = 64, 16, 64, 31337, 1000
    rng = np.random.default_rng(5)
    poses = rng.uniform(-3.0, 9.0, (40, B, 3))
    whole = capi.ReplayMemory(B, cap, batch, seed=seed, robot0=first)
    lo = capi.ReplayMemory(B // 2, cap, batch, seed=seed, robot0=first)
    hi = capi.ReplayMemory(B // 2, cap, batch, seed=seed, robot0=first + B // 2)
    ref = rr.ReplayMemory(B, cap, batch, seed=seed, robot0=first)
    d_poses = _dev(poses)
    for t in range(40):
        whole.append(d_poses[t])
        lo.append(d_poses[t, :B // 2].contiguous())
        hi.append(d_poses[t, B // 2:].contiguous())
        ref.append(poses[t])
    new = lambda n: (torch.full((n, batch, 3), SENTINEL, dtype=torch.float64, device="cuda"), torch.full((n,), -1, dtype=torch.int32, device="cuda"))
    (c_w, n_w), (c_lo, n_lo), (c_hi, n_hi) = new(B), new(B // 2), new(B // 2)
    whole.sample(21, c_w, n_w)
    lo.sample(21, c_lo, n_lo)
    hi.sample(21, c_hi, n_hi)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([c_lo, c_hi]), c_w) and torch.equal(torch.cat([n_lo, n_hi]), n_w)
    cols, n = np.full((B, batch, 3), SENTINEL), np.full(B, -1, dtype=np.int32)
    ref.sample(21, cols, n)
    assert np.array_equal(c_w.cpu().numpy(), cols) and n_w.cpu().numpy().tolist() == n.tolist() == [batch] * B
    assert not torch.equal(c_lo, c_hi[:, :, :])   # (different robots, different draws)
    for m in (whole, lo, hi):
        m.close()


def _oracle_tick(o, pose, vb, cols):
    """OracleExploration.tick (tests/test_host_mirror.py: the loop body of exploration.hpp:197-292 on the CPU oracle) with the
    columns sampleMemory prepends GIVEN (3 x n) instead of the whole memory: the sampled regime of buffer.cpp:91-108"""
    source = "ergodic"
    if o.follow:
        o.i += 1
        o.follow = o.i != o.dwa_steps
        source = "dwa-follow"
    if not o.follow:
        o.u = o.ec.control(o.bounds, pose, cols)
        source = "ergodic"
    if not po.validate_control(COLL, o.grid, pose, o.u, 0.1, 0.5):
        if o.follow:
            _, o.u, _ = po.dwa_control(DWA[o.model], COLL, o.grid, pose, vb, vref=o.u)
            o.follow = False
            source = "dwa-replan"
        else:
            ok, o.u, _ = po.dwa_control(DWA[o.model], COLL, o.grid, pose, vb, xt_ref=o.ec.opt_traj(), dt_ref=0.1)
            o.follow = ok
            if ok:
                o.i = 0
            source = "dwa-reference"
    return o.u.copy(), source


def _scenario(B, rng):
    """the map, the wall that appears, and collision-free start poses of tests/test_gpu_fleet_tick.py"""
    obstacles = [(2.4, 0.2, 3.0, 2.6), (6.0, 2.0, 6.5, 4.6), (8.8, -0.4, 9.4, 1.2)]
    wall = (4.2, -0.6, 4.5, 4.4)
    grid_a, bounds = _grid_with(obstacles)
    grid_b, _ = _grid_with(obstacles + [wall])
    poses = np.stack([rng.uniform(0.2, 9.5, B), rng.uniform(-0.2, 4.2, B), rng.uniform(-0.6, 0.6, B)], 1)
    poses[:8, 0], poses[:8, 1], poses[:8, 2] = rng.uniform(1.0, 1.6, 8), rng.uniform(0.6, 2.2, 8), rng.uniform(-0.2, 0.2, 8)
    poses[8:14, 0], poses[8:14, 1] = rng.uniform(3.3, 3.7, 6), rng.uniform(0.0, 4.0, 6)
    for b in range(B):
        while not po.validate_control(COLL, grid_b, poses[b], np.zeros(3), 0.1, 0.5):
            poses[b, :2] = rng.uniform(0.2, 9.5), rng.uniform(-0.2, 4.2)
    return grid_a, grid_b, bounds, poses


@pytest.mark.parametrize("model", ["omni", "simple_cart"])
def test_closed_loop_fed_by_append_sample_against_the_oracle(model):
    """5. the scenario of test_fleet_tick_against_independent_oracle_loops with a replay memory of batch size 8 over 30 ticks
    of 28 robots: from tick 9 on the columns are SAMPLED.  tick_batch is fed by append_sample on the device; an oracle loop per
    robot calls control(bounds, pose, columns) with the restated columns.  Assertions and tolerances are that test's."""
    B, ticks, wall_tick, batch, dt = 28, 30, 12, 8, 0.1
    grid_a, grid_b, bounds, poses = _scenario(B, np.random.default_rng(4))
    ccfg = capi.make_collision_cfg(bounds[0], bounds[2], 0.05, grid_a.xsize, grid_a.ysize, *COLL)
    dcfg = capi.DwaCfg(*DWA[model])
    eng = _engine(model)
    eng.config_domain(bounds)
    assert eng.agent_lanes(B) == 64
    T = eng.T
    mem = capi.ReplayMemory(B, 64, batch, seed=2020)
    ref = rr.ReplayMemory(B, 64, batch, seed=2020)
    ors = [OracleExploration(model, grid_a, bounds) for _ in range(B)]
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device="cuda")
    d_ut, d_follow, d_count, d_u, d_traj = z(B, T, 3), z(B, dt=torch.int32), z(B, dt=torch.int32), z(B, 3), z(B, T, 3)
    d_valid, d_skip = z(B, dt=torch.int32), z(B, dt=torch.int32)
    d_source, d_status = torch.full((B,), -1, dtype=torch.int32, device="cuda"), torch.full((B,), -1, dtype=torch.int32, device="cuda")
    d_cols, d_n = torch.full((B, batch, 3), SENTINEL, dtype=torch.float64, device="cuda"), z(B, dt=torch.int32)
    cols, n_mem = np.full((B, batch, 3), SENTINEL), np.zeros(B, dtype=np.int32)
    d_grid_a, d_grid_b = _dev(grid_a.data, torch.int8), _dev(grid_b.data, torch.int8)
    vb = np.zeros((B, 3))
    seen, sampled_ticks = set(), 0
    for t in range(ticks):
        grid, d_grid = (grid_a, d_grid_a) if t < wall_tick else (grid_b, d_grid_b)
        ut_before = d_ut.cpu().numpy()
        d_pose = _dev(poses)
        mem.append_sample(d_pose, t, d_cols, d_n)          # addStateMemory (:209), then the columns of sampleMemory (:232)
        eng.tick_batch(B, d_pose, d_ut, d_follow, d_count, d_u, _dev(vb), d_grid, d_traj, d_valid, d_skip, ccfg, dcfg, 0.1, 0.5,
                       source=d_source, mem_cols=d_cols, n_mem=d_n, mem_stride=batch, status=d_status,
                       grid_epoch=1 if t < wall_tick else 2)
        torch.cuda.synchronize()
        ref.append_sample(poses, t, cols, n_mem)
        assert np.array_equal(d_cols.cpu().numpy(), cols) and d_n.cpu().numpy().tolist() == n_mem.tolist() == [min(t + 1, batch)] * B
        sampled_ticks += int(ref.count[0] > batch)
        u, src, follow, count = d_u.cpu().numpy(), d_source.cpu().numpy(), d_follow.cpu().numpy(), d_count.cpu().numpy()
        valid, ut_after = d_valid.cpu().numpy(), d_ut.cpu().numpy()
        for b in range(B):
            o = ors[b]
            o.grid = grid
            o.ec.ut = ut_before[b].T              # the oracle starts every tick from the engine's warm start
            uo, so = _oracle_tick(o, poses[b], vb[b], cols[b, :n_mem[b]].T.copy())
            assert SOURCES[src[b]] == so, (t, b, SOURCES[src[b]], so)
            assert bool(follow[b]) == o.follow and (not o.follow or int(count[b]) == o.i), (t, b, follow[b], count[b], o.follow, o.i)
            assert bool(valid[b]) == (so in ("ergodic", "dwa-follow")), (t, b, valid[b], so)
            if so in ("ergodic", "dwa-follow"):
                assert np.abs(u[b] - uo).max() <= 1e-9, (t, b, so, u[b], uo)
            elif not np.array_equal(u[b], uo):
                if so == "dwa-replan":
                    raise AssertionError((t, b, so, u[b], uo))
                xt = o.ec.opt_traj()
                ca = po.dwa_objective_traj(DWA[model], COLL, grid, poses[b], u[b], xt, 0.1)
                cb = po.dwa_objective_traj(DWA[model], COLL, grid, poses[b], uo, xt, 0.1)
                assert abs(ca - cb) <= 1e-9 * max(1.0, abs(cb)), (t, b, u[b], uo, ca, cb)
            if so == "dwa-follow":
                assert np.array_equal(ut_after[b], ut_before[b])
            seen.add(so)
        assert (d_status.cpu().numpy()[src == 0] == 0).all()
        for b in range(B):
            poses[b] = po.integrate_twist(poses[b], u[b], dt)
        vb = u.copy()
    assert sampled_ticks == ticks - batch   # sampling starts at tick 9
    assert seen >= {"ergodic", "dwa-follow", "dwa-reference"} and (model != "omni" or "dwa-replan" in seen), seen
    assert mem.counts()[0].tolist() == [ticks] * B
    mem.close()
    eng.close()


def test_fleet_loop_without_a_host_round_trip():
    """6. 4096 robots, batch size 100, 120 ticks (sampled from tick 101 on): append_sample -> tick_batch ->
    integrate_twist_batch, vb = u by a device copy, on ONE stream with NO synchronisation inside the loop -- against the same
    loop run the way the callers had to until now: a synchronisation every tick, the poses read back, the columns built on the
    host (the restatement) and uploaded.  Final poses, warm starts, twists, loop state, counts and the last columns: bitwise."""
    B, batch, ticks, cap, dt, seed, model = 4096, 100, 120, 128, 0.1, 4242, "omni"
    grid_a, _, bounds, poses0 = _scenario(B, np.random.default_rng(6))
    ccfg = capi.make_collision_cfg(bounds[0], bounds[2], 0.05, grid_a.xsize, grid_a.ysize, *COLL)
    dcfg = capi.DwaCfg(*DWA[model])
    eng = _engine(model)
    eng.config_domain(bounds)
    T = eng.T
    d_grid = _dev(grid_a.data, torch.int8)
    stream = torch.cuda.Stream()

    def run(on_device):
        z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device="cuda")
        d_pose, d_vb = _dev(poses0), z(B, 3)
        d_ut, d_follow, d_count, d_u, d_traj = z(B, T, 3), z(B, dt=torch.int32), z(B, dt=torch.int32), z(B, 3), z(B, T, 3)
        d_valid, d_skip, d_source = z(B, dt=torch.int32), z(B, dt=torch.int32), z(B, dt=torch.int32)
        d_cols, d_n = torch.full((B, batch, 3), SENTINEL, dtype=torch.float64, device="cuda"), z(B, dt=torch.int32)
        mem = capi.ReplayMemory(B, cap, batch, seed=seed) if on_device else None
        ref = None if on_device else rr.ReplayMemory(B, cap, batch, seed=seed)
        cols, n_mem = np.full((B, batch, 3), SENTINEL), np.zeros(B, dtype=np.int32)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for t in range(ticks):
                if on_device:
                    mem.append_sample(d_pose, t, d_cols, d_n, stream=stream.cuda_stream)
                else:
                    stream.synchronize()
                    ref.append_sample(d_pose.cpu().numpy(), t, cols, n_mem)
                    d_cols.copy_(torch.from_numpy(cols))
                    d_n.copy_(torch.from_numpy(n_mem))
                eng.tick_batch(B, d_pose, d_ut, d_follow, d_count, d_u, d_vb, d_grid, d_traj, d_valid, d_skip, ccfg, dcfg, 0.1, 0.5,
                               source=d_source, mem_cols=d_cols, n_mem=d_n, mem_stride=batch, stream=stream.cuda_stream, grid_epoch=1)
                capi.integrate_twist_batch(d_pose, d_u, dt, stream=stream.cuda_stream)   # the robots move (numerics.hpp:273-297)
                d_vb.copy_(d_u)                                                           # odometry reports the commanded twist
        stream.synchronize()
        counts = mem.counts() if on_device else (ref.count.astype(np.uint32), ref.dropped)
        if on_device:
            mem.close()
        state = [x.cpu().numpy() for x in (d_pose, d_ut, d_u, d_follow, d_count, d_source, d_cols, d_n)]
        return state, counts

    dev_state, dev_counts = run(True)
    host_state, host_counts = run(False)
    assert dev_counts[0].tolist() == host_counts[0].tolist() == [ticks] * B and dev_counts[1] == host_counts[1] == 0
    for name, a, b in zip(("pose", "ut", "u", "follow", "count", "source", "columns", "n_mem"), dev_state, host_state):
        assert np.array_equal(a, b), name
    assert dev_state[7].tolist() == [batch] * B
    assert not np.array_equal(dev_state[0], poses0)   # (the fleet moved)
    eng.close()

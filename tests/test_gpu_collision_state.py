"""The state the inflated collision map keeps BETWEEN calls (the policy: csrc/hit_map_table.hpp HitMapTable; its effects:
csrc/collision_kernel.hip build_hit_map): one buffer per
(device, stream); a stamp 1..255 per build, the buffer cleared when the stamps wrap; the buffer reallocated for a larger map
and reused as it is for a smaller one with another row pitch; the ring-offset table cached by radii; stream-ordered
allocations once 64 streams hold a buffer; a tick's grid_epoch cache, which any other build on the stream must drop.
A mistake in any of these shows as obstacles of an EARLIER map, hundreds of calls later (tests/test_hit_map_table.py asks
the table itself, without a GPU).

Every call has >= 4096 poses, so the cost model picks the inflated map by itself (the file is skipped when an implementation
is forced).  References: the CPU oracle, once per (grid, radii).  Results are compared on the device, on the call's own
stream, and read back once per test.  The streams are created here (a stream of PyTorch's pool may have held a buffer for
hundreds of builds already) and wrapped as torch.cuda.ExternalStream."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pyoracle as po
from ergodic_exploration_amd import capi

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("EEA_TEST_OPTIONS")), reason="an implementation is forced: no cost model")]

COLL = (0.7, 1.0, 0.2, 0.8)      # the yaml radii: rings 7..10, collision within 9 cells at 0.1 m
COLL2 = (0.3, 0.6, 0.1, 0.5)     # other radii AND another occupancy threshold: rings 3..6, within 4 cells
P = 4096
RES, XMIN, YMIN = 0.1, -2.0, -1.0


class _Streams:
    """streams of this test's own, through the HIP runtime the process already runs on"""

    def __init__(self):
        torch.zeros(1, device="cuda")   # (the device is initialised and current)
        capi.lib()
        paths = sorted({l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l and "/" in l})
        assert len(paths) == 1, paths   # one HIP runtime per process (capi.lib)
        self.hip = C.CDLL(paths[0])
        self.hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.hip.hipStreamDestroy.argtypes = [C.c_void_p]
        self.handles = []

    def new(self):
        h = C.c_void_p()
        assert self.hip.hipStreamCreate(C.byref(h)) == 0 and h.value
        self.handles.append(h.value)
        return torch.cuda.ExternalStream(h.value)

    def close(self):
        torch.cuda.synchronize()
        capi.release_collision_caches()   # (no buffer stays keyed to a handle a later stream may be given again)
        for h in self.handles:
            self.hip.hipStreamDestroy(C.c_void_p(h))
        self.handles = []


@pytest.fixture
def streams():
    s = _Streams()
    yield s
    s.close()


_CASES = {}


def _host_case(name, coll=COLL):
    """(cfg, grid, poses, the oracle's verdicts) of a named map with the given radii, as host arrays"""
    xs, ys = {"small": (40, 30), "large": (200, 150), "pitch": (64, 20)}.get(name, (80, 60))
    rng = np.random.default_rng(sum(name.encode()))
    data = np.zeros((ys, xs), dtype=np.int8)
    if name == "left":
        data[12:50, 4:9] = 100
    elif name == "right":
        data[8:40, 70:75] = 100
    elif name == "scattered":        # (rows the dilation of "centre" does not reach)
        rows = np.concatenate([rng.integers(0, 10, 15), rng.integers(51, 60, 15)])
        data[rows, rng.integers(0, xs, 30)] = rng.choice([100, 80, 55], 30)
    elif name == "centre":           # dilated: rows 19..41, columns 29..51 -- no other 80 x 60 map marks a cell there
        data[28:33, 38:43] = 100
    elif name != "empty":
        for _ in range(max(3, xs * ys // 400)):
            i, j = rng.integers(0, ys - 4), rng.integers(0, xs - 4)
            data[i:i + rng.integers(1, 5), j:j + rng.integers(1, 5)] = rng.choice([100, 80, 79, 55, 49])
        data[rng.integers(0, ys, 4), rng.integers(0, xs, 4)] = 100
    g = po.GridMap(XMIN, XMIN + xs * RES, YMIN, YMIN + ys * RES, RES, data.reshape(-1))
    cfg = capi.make_collision_cfg(XMIN, YMIN, RES, xs, ys, *coll)
    prng = np.random.default_rng(1000 * xs + ys)      # (maps of one size share their poses)
    poses = np.stack([prng.uniform(XMIN - 1.2, XMIN + xs * RES + 1.2, P), prng.uniform(YMIN - 1.2, YMIN + ys * RES + 1.2, P),
                      np.zeros(P)], 1)
    ref = np.array([po.collision_check(coll, g, p)[0] for p in poses], dtype=np.int32)
    assert (ref.sum() == 0) if name == "empty" else (0 < ref.sum() < P), (name, ref.sum())
    return cfg, data, poses, ref


def _case(name, coll=COLL):
    """the same on the device; the oracle runs once per (map, radii)"""
    key = (name, coll)
    if key not in _CASES:
        cfg, data, poses, ref = _host_case(name, coll)
        _CASES[key] = (cfg, torch.as_tensor(data).cuda(), torch.as_tensor(poses).cuda(), torch.as_tensor(ref).cuda())
        torch.cuda.synchronize()
    return _CASES[key]


def _check_on(stream, case, hit, bad, k):
    """one collision_check_batch of `case` on `stream`; bad[k] = verdicts that differ from the reference (device, same stream)"""
    cfg, d_grid, d_pose, d_ref = case
    with torch.cuda.stream(stream):
        hit.fill_(-1)
        capi.collision_check_batch(cfg, d_grid, d_pose, hit, stream=stream.cuda_stream)
        bad[k] = (hit != d_ref).sum()


def test_stamps_wrap_without_showing_an_earlier_map(streams):
    """601 consecutive builds on one stream: the stamps wrap twice.  First ONE call on a map with a block in the centre,
    then 600 calls cycling through obstacles on the left / on the right / none / scattered, none of which marks a cell the
    centre block marked: those marks keep the stamp of call 0 until the buffer is cleared.  255 builds later the same stamp
    is current again -- without the clear at the wrap the centre block is back, on whichever map is looked up then (4 is
    coprime to 255: across the wraps every stamp meets every map).  Every call must equal its own map's reference, the
    empty map all zeros."""
    cycle = [_case(n) for n in ("left", "right", "empty", "scattered")]
    once = _case("centre")
    assert int(cycle[2][3].sum()) == 0
    # (the premise: poses that the centre map reports as hits and each cycled map as free)
    for c in cycle:
        assert torch.equal(c[2], once[2]) and int(((once[3] == 1) & (c[3] == 0)).sum()) > 50
    s = streams.new()
    n = 601
    hit = torch.empty((P,), dtype=torch.int32, device="cuda")
    bad = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _check_on(s, once, hit, bad, 0)
    for k in range(1, n):
        _check_on(s, cycle[(k - 1) % 4], hit, bad, k)
    s.synchronize()
    bad = bad.cpu().numpy()
    assert (bad == 0).all(), (np.nonzero(bad)[0][:10], bad[np.nonzero(bad)[0][:10]])


def test_buffer_grows_and_is_reused_by_smaller_maps(streams):
    """one stream: 40 x 30, then 200 x 150 (the buffer is reallocated), 40 x 30 again, 64 x 20 (another row pitch inside the
    same buffer), 40 x 30 with other radii (another offset table, another pitch: w = xsize + 2 r_col), the first radii again"""
    seq = [_case("small"), _case("large"), _case("small"), _case("pitch"), _case("small", COLL2), _case("small")]
    s = streams.new()
    hits = [torch.empty((P,), dtype=torch.int32, device="cuda") for _ in seq]
    bad = torch.full((2 * len(seq),), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for rep in range(2):      # (the second pass starts from a buffer that has held every layout)
        for k, c in enumerate(seq):
            _check_on(s, c, hits[k], bad, rep * len(seq) + k)
    s.synchronize()
    assert (bad.cpu().numpy() == 0).all(), bad.cpu().numpy()
    assert not torch.equal(_case("small")[3], _case("small", COLL2)[3])    # (the radii matter on this map)


def test_two_streams_keep_their_own_maps(streams):
    """20 rounds, stream 1 on one map and stream 2 on another, enqueued alternately without a host wait in between: the
    buffers are per stream, neither may see the other's map"""
    a, b = _case("left"), _case("pitch")
    s1, s2 = streams.new(), streams.new()
    h1, h2 = (torch.empty((P,), dtype=torch.int32, device="cuda") for _ in range(2))
    bad = torch.full((40,), -1, dtype=torch.int64, device="cuda")
    b1, b2 = bad[:20], bad[20:]
    torch.cuda.synchronize()
    for k in range(20):
        _check_on(s1, a, h1, b1, k)
        _check_on(s2, b, h2, b2, k)
    s1.synchronize()
    s2.synchronize()
    assert (bad.cpu().numpy() == 0).all(), bad.cpu().numpy()


def test_more_streams_than_map_buffers(streams):
    """64 (device, stream) pairs hold a buffer; a call on a further stream builds its map in a stream-ordered allocation.
    After release_collision_caches(): one call on each of 66 new streams -- the last two take that path -- all equal to the
    reference; the caches released again, the next call on the default stream is still right."""
    c = _case("scattered")
    capi.release_collision_caches()
    n = 66
    ss = [streams.new() for _ in range(n)]
    assert len(set(s.cuda_stream for s in ss)) == n
    hits = [torch.empty((P,), dtype=torch.int32, device="cuda") for _ in range(n)]
    bad = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for k, s in enumerate(ss):
        _check_on(s, c, hits[k], bad, k)
    torch.cuda.synchronize()
    capi.release_collision_caches()
    cfg, d_grid, d_pose, d_ref = c
    capi.collision_check_batch(cfg, d_grid, d_pose, hits[0])
    bad[n] = (hits[0] != d_ref).sum()
    torch.cuda.synchronize()
    assert (bad.cpu().numpy() == 0).all(), bad.cpu().numpy()


def test_tick_epoch_cache_is_dropped_by_any_other_build(streams):
    """eea_tick_io::grid_epoch != 0 lets a tick reuse the inflated map of the LAST build on its stream when (grid pointer,
    epoch, parameters) are the same.  Any other build on that stream -- a collision_check_batch on another grid, a tick with
    other radii, a tick with another (pointer, epoch) -- overwrites the buffer, so the key must go with it.  A small fleet
    between two walls: the second tick's d_valid / d_source / d_u / d_follow are bitwise those of the same calls with
    grid_epoch = 0 throughout, and differ from what the stale map would have given."""
    from tests.test_gpu_fleet_tick import _engine
    from tests.test_host_mirror import COLL as YAML, DWA, _grid_with
    assert YAML == COLL
    obstacles = [(2.4, 0.2, 3.0, 2.6), (6.0, 2.0, 6.5, 4.6), (8.8, -0.4, 9.4, 1.2)]
    grid_a, bounds = _grid_with(obstacles)
    grid_b, _ = _grid_with(obstacles + [(4.2, -0.6, 4.5, 4.4)])    # a wall appears
    cfgs = {c: capi.make_collision_cfg(bounds[0], bounds[2], 0.05, grid_a.xsize, grid_a.ysize, *c) for c in (COLL, COLL2)}
    dcfg = capi.DwaCfg(*DWA["omni"])
    eng = _engine("omni")
    eng.config_domain(bounds)
    B, T = 64, eng.T
    rng = np.random.default_rng(8)
    poses = np.stack([rng.uniform(0.2, 9.5, B), rng.uniform(-0.2, 4.2, B), rng.uniform(-0.6, 0.6, B)], 1)
    poses[:16, 0], poses[:16, 1] = rng.uniform(3.5, 4.1, 16), rng.uniform(3.6, 4.2, 16)     # free on A, inside the wall's reach on B
    poses[16:32, 0], poses[16:32, 1] = rng.uniform(3.5, 3.8, 16), rng.uniform(0.5, 2.3, 16)  # 0.5 .. 0.8 m from an obstacle
    dev = lambda a, t=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=t).cuda()
    d_pose, d_vb = dev(poses), torch.zeros((B, 3), dtype=torch.float64, device="cuda")
    grids = {"A": dev(grid_a.data, torch.int8), "B": dev(grid_b.data, torch.int8)}
    scratch = dev(grid_a.data, torch.int8)          # a third buffer whose content the "lying epoch" run changes
    # the foreign call: >= 4096 poses on grid B through the same stream
    far = dev(np.stack([rng.uniform(-1, 11, P), rng.uniform(-1, 5, P), np.zeros(P)], 1))
    far_hit = torch.empty((P,), dtype=torch.int32, device="cuda")
    s = streams.new()
    torch.cuda.synchronize()

    def run(steps):
        """the calls of `steps` on the stream; every tick starts from the same zero state; the outputs of the last tick"""
        out = None
        with torch.cuda.stream(s):
            for step in steps:
                if step[0] == "foreign":
                    capi.collision_check_batch(cfgs[COLL], grids["B"], far, far_hit, stream=s.cuda_stream)
                elif step[0] == "fill":
                    scratch.copy_(grids[step[1]])
                else:
                    _, grid, coll, epoch = step
                    z = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device="cuda")
                    d_ut, d_follow, d_count, d_u, d_traj = z(B, T, 3), z(B, dt=torch.int32), z(B, dt=torch.int32), z(B, 3), z(B, T, 3)
                    d_valid, d_skip, d_source = (torch.full((B,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
                    eng.tick_batch(B, d_pose, d_ut, d_follow, d_count, d_u, d_vb, scratch if grid == "S" else grids[grid], d_traj,
                                   d_valid, d_skip, cfgs[coll], dcfg, 0.1, 0.5, source=d_source, stream=s.cuda_stream,
                                   grid_epoch=epoch)
                    out = (d_valid, d_source, d_u, d_follow)
        s.synchronize()
        return [t.cpu().numpy() for t in out]

    same = lambda x, y: all(np.array_equal(p, q) for p, q in zip(x, y))
    on_a, on_b, on_a2 = run([("tick", "A", COLL, 0)]), run([("tick", "B", COLL, 0)]), run([("tick", "A", COLL2, 0)])
    for o in (on_a, on_b, on_a2):
        assert 0 < o[0].sum() < B and set(np.unique(o[1])) >= {0, 2}     # valid twists and dynamic-window twists
    assert not np.array_equal(on_a[0], on_b[0]) and not np.array_equal(on_a[0], on_a2[0])   # the scene tells the maps apart
    assert same(on_a, run([("tick", "A", COLL, 0)]))                     # (a tick is reproducible bit for bit)
    # the cache is live: the caller vouches that (pointer, epoch) names one content -- a content changed behind its back is
    # not seen (the documented contract; without this the checks below could not fail)
    assert same(on_a, run([("fill", "A"), ("tick", "S", COLL, 7), ("fill", "B"), ("tick", "S", COLL, 7)]))
    assert same(on_b, run([("fill", "A"), ("tick", "S", COLL, 7), ("fill", "B"), ("tick", "S", COLL, 8)]))
    # 1. a foreign build on the stream between two ticks of one (grid, epoch)
    for epoch in (1, 0):
        assert same(on_a, run([("tick", "A", COLL, epoch), ("foreign",), ("tick", "A", COLL, epoch)])), epoch
    # 2. other collision radii under the same (grid, epoch); and back
    for epoch in (1, 0):
        assert same(on_a2, run([("tick", "A", COLL, epoch), ("tick", "A", COLL2, epoch)])), epoch
        assert same(on_a, run([("tick", "A", COLL2, epoch), ("tick", "A", COLL, epoch)])), epoch
    # 3. the epoch moves on, on another grid pointer
    for e1, e2 in ((1, 2), (0, 0)):
        assert same(on_b, run([("tick", "A", COLL, e1), ("tick", "B", COLL, e2)])), (e1, e2)
    eng.close()

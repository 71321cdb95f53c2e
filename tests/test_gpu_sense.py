"""The fleet's range sensor on the device (include/ergodic_amd.h: eea_sense_reveal_batch, eea_grid_census;
csrc/sense_kernel.hip): robots cast rays through a ground-truth grid and the cells the rays cross become known.

Checker: the numpy restatement tests/sense_restatement.py (held to an independent statement in exact fractions by
tests/test_sense.py).  Everything is integers: `known` and `ranges` are compared BITWISE, as whole buffers -- the known grid
and the ranges sit between guard bytes, and hold a sentinel wherever nothing may be written.  The device buffers start 37
bytes into their allocations, so neither grid is aligned to anything."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pyoracle as po
from ergodic_exploration_amd import capi
from tests import sense_restatement as sr

pytestmark = pytest.mark.gpu

GUARD = 37                       # bytes (elements) in front of and behind every checked buffer
G_KNOWN, G_RANGES = 0x3C, -123456789
S_KNOWN, S_RANGES = 77, -77      # what `known` / `ranges` hold before a call: neither a truth value used here nor a range
RES, XMIN, YMIN, THR = 0.25, -1.0, -2.0, 0.8   # (binary fractions: a pose exactly on xmax divides to xsize exactly)


def _geom(xs, ys):
    return sr.Geometry(XMIN, YMIN, RES, xs, ys, THR)


def _cfg(g):
    # (radii Collision::Collision would refuse: the sensor must not look at them)
    return capi.make_collision_cfg(g.xmin, g.ymin, g.resolution, g.xsize, g.ysize, 0.7, 0.1, 0.2, g.occupied_threshold)


def _centre(g, i, j):
    return [g.xmin + (j + 0.5) * g.resolution, g.ymin + (i + 0.5) * g.resolution, 0.3]


def _guarded(values, guard_value, dtype):
    """(host image, device buffer, device view of the payload): the payload between GUARD guard elements on both sides"""
    flat = np.asarray(values, dtype=dtype).reshape(-1)
    img = np.concatenate([np.full(GUARD, guard_value, dtype), flat, np.full(GUARD, guard_value, dtype)])
    buf = torch.as_tensor(img).cuda()
    return img, buf, buf[GUARD:GUARD + flat.size]


class _Device:
    """truth and known of one grid on the device, and the host images the restatement is replayed on"""

    def __init__(self, g, truth, known_fill=S_KNOWN):
        self.g, self.cfg, self.truth = g, _cfg(g), np.ascontiguousarray(truth, dtype=np.int8)
        _, self._tbuf, self.d_truth = _guarded(self.truth, 0x11, np.int8)
        self.known = np.full_like(self.truth, known_fill)
        _, self._kbuf, self.d_known = _guarded(self.known, G_KNOWN, np.int8)

    def reveal(self, R, poses, mask=None, want_ranges=True, stream=None):
        """one call on the device and in the restatement; returns (ranges image of the device, expected image) or None"""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        P = poses.shape[0]
        d_pose = torch.as_tensor(poses).cuda()
        d_mask = None if mask is None else torch.as_tensor(np.asarray(mask, dtype=np.int32)).cuda()
        rows = np.full((P, 8 * R), S_RANGES, dtype=np.int32)
        want_img, rbuf, d_ranges = _guarded(rows, G_RANGES, np.int32)
        torch.cuda.synchronize()     # (the uploads above ran on torch's stream)
        capi.sense_reveal_batch(self.cfg, R, self.d_truth, self.d_known, d_pose, d_ranges if want_ranges else None, d_mask,
                                stream=stream)
        torch.cuda.synchronize()
        sr.reveal(self.g, R, self.truth, self.known, poses, mask, rows)
        if not want_ranges:
            rows[:] = S_RANGES
        want_img[GUARD:GUARD + rows.size] = rows.reshape(-1)
        return rbuf.cpu().numpy(), want_img

    def check_known(self):
        got = self._kbuf.cpu().numpy()
        want = np.concatenate([np.full(GUARD, G_KNOWN, np.int8), self.known.reshape(-1), np.full(GUARD, G_KNOWN, np.int8)])
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "known differs at buffer offsets %s (payload starts at %d): got %s want %s" % (
            bad[:8], GUARD, got[bad[:8]], want[bad[:8]])
        assert np.array_equal(self._tbuf.cpu().numpy()[GUARD:GUARD + self.truth.size], self.truth.reshape(-1))   # read only


def _check_ranges(got, want):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "ranges differ at buffer offsets %s (payload starts at %d): got %s want %s" % (
        bad[:8], GUARD, got[bad[:8]], want[bad[:8]])


def _scene(xs, ys):
    """a grid with a single blocking cell, an L-shaped wall, an unknown patch and the 79 / 80 pair, and robots in the open,
    beside the single cell, on both diagonals of the wall's corner, inside a wall cell, in the four corners, on the four
    edges, exactly on xmax / ymax, and off the grid on every side"""
    g = _geom(xs, ys)
    truth = np.zeros((ys, xs), dtype=np.int8)
    ci, cj = ys // 2, xs // 2
    truth[ci, cj + 3] = 100
    truth[4, 5:11] = 100
    truth[4:10, 10] = 100
    truth[ys - 6:ys - 3, 2:6] = -1
    truth[ci + 2, 3], truth[ci + 3, 3] = 79, 80
    xmax, ymax = XMIN + xs * RES, YMIN + ys * RES
    poses = [_centre(g, ci + 3, cj - 4),                                  # in the open
             _centre(g, ci, cj + 2),                                      # beside the single blocking cell
             _centre(g, 6, 8), _centre(g, 2, 12),                         # the wall's corner (4, 10) on a diagonal, from both sides
             _centre(g, 4, 7),                                            # inside an occupied cell
             _centre(g, 0, 0), _centre(g, 0, xs - 1), _centre(g, ys - 1, 0), _centre(g, ys - 1, xs - 1),
             _centre(g, 0, cj), _centre(g, ys - 1, cj), _centre(g, ci, 0), _centre(g, ci, xs - 1),
             [xmax, ymax, 0.0], [xmax, YMIN + 3.1 * RES, 0.0], [XMIN + 7.5 * RES, ymax, 0.0],   # the decrement rule
             [XMIN, YMIN, 0.0],
             [XMIN - 0.3, 0.0, 0.0], [xmax + 0.3, 0.0, 0.0], [0.0, YMIN - 5.0, 0.0], [0.0, ymax + RES, 0.0],
             [-1.0e6, -1.0e6, 0.0], [float("nan"), 0.0, 0.0]]             # (NaN: x86's conversion gives cell 0)
    return g, truth, poses


@pytest.mark.parametrize("xs,ys", [(23, 19), (64, 41)])
@pytest.mark.parametrize("R", [1, 2, 3, 9, 17])
def test_reveal_is_the_restatement(R, xs, ys):
    """8, 16, 24, 72 and 136 rays per robot on two grids, every placement of _scene at once (their discs overlap)"""
    g, truth, poses = _scene(xs, ys)
    dev = _Device(g, truth)
    got, want = dev.reveal(R, poses)
    _check_ranges(got, want)
    dev.check_known()
    rows = want[GUARD:-GUARD].reshape(len(poses), 8 * R)
    assert (rows[-6:-1] == -1).all()                      # the robots off the grid: a row of -1 ...
    assert (rows[:13] != -1).any() and (dev.known != S_KNOWN).any()
    assert R > 3 or (dev.known == S_KNOWN).any()          # (from R = 9 on the placements' discs cover the smaller grid)
    # ... and every placement alone, on a fresh known grid: nothing but its own disc is written
    for b in (0, 4, 8, 13, 17):
        one = _Device(g, truth)
        _check_ranges(*one.reveal(R, [poses[b]]))
        one.check_known()


@functools.lru_cache(maxsize=None)
def _fleet(P):
    """P robots scattered over a 64 x 41 grid with clutter (some off the grid): R = 9 discs overlap many times at P = 300"""
    rng = np.random.default_rng(1000 + P)
    g = _geom(64, 41)
    truth = rng.choice(np.array([0] * 40 + [100, 100, -1, -1, 79, 80, 50], dtype=np.int8), size=(41, 64))
    poses = np.stack([rng.uniform(XMIN - 0.4, XMIN + 64 * RES + 0.4, P), rng.uniform(YMIN - 0.4, YMIN + 41 * RES + 0.4, P),
                      rng.uniform(-3, 3, P)], 1)
    return g, truth, poses


@pytest.mark.parametrize("P", [1, 3, 65, 300])
def test_fleet_sizes_with_overlapping_discs(P):
    g, truth, poses = _fleet(P)
    dev = _Device(g, truth)
    _check_ranges(*dev.reveal(9, poses))
    dev.check_known()


def test_mask_and_no_ranges():
    """a mask that leaves out the first, the last and alternate robots: their rows of ranges keep the sentinel and their
    discs stay unknown; then d_ranges == NULL; then a mask of zeros (nothing at all is written)"""
    g, truth, poses = _fleet(65)
    mask = np.ones(65, dtype=np.int32)
    mask[0], mask[-1], mask[1::2] = 0, 0, 0
    dev = _Device(g, truth)
    got, want = dev.reveal(9, poses, mask=mask)
    _check_ranges(got, want)
    dev.check_known()
    rows = got[GUARD:-GUARD].reshape(65, 72)
    assert (rows[mask == 0] == S_RANGES).all() and (rows[mask == 1] != S_RANGES).all()
    full = _Device(g, truth)
    full.reveal(9, poses)
    assert (dev.known != full.known).any()      # the masked robots would have revealed more
    none = _Device(g, truth)
    _check_ranges(*none.reveal(9, poses, want_ranges=False))
    none.check_known()
    assert np.array_equal(none.known, full.known)
    idle = _Device(g, truth)
    _check_ranges(*idle.reveal(9, poses, mask=np.zeros(65, dtype=np.int32)))
    idle.check_known()
    assert (idle.known == S_KNOWN).all()


STRIDED = 65536 + 3              # robots: a launch has at most 65536 workgroups, which stride over the robots past that


@functools.lru_cache(maxsize=None)
def _strided_fleet(second_turn_live):
    """65536 + 3 robots on an 8 x 8 grid.  Robots 0 .. 2 and 65536 .. 65538 are the two turns of workgroups 0 .. 2: three stand
    in columns 5 and 6 and work, of the three others the first and the last are masked out -- in cells (5, 6) and (7, 7), which
    the working three do not reach (at R = 1 a robot reveals its cell and the four beside it) -- and the middle one is off the
    grid (a row of -1).  Everybody else stands in columns 0 .. 2
    (a few off the grid, one in eight live), so columns 5 .. 7 are revealed by the working three alone: a turn that is skipped or
    whose stores are lost shows in `known`, not only in the ranges"""
    rng = np.random.default_rng(STRIDED)
    g = _geom(8, 8)
    truth = rng.choice(np.array([0, 0, 0, 100, 50, -1], dtype=np.int8), size=(8, 8))
    cells = np.stack([rng.integers(0, 8, STRIDED), rng.integers(0, 3, STRIDED)], 1)
    poses = np.array([[XMIN + (j + 0.5) * RES, YMIN + (i + 0.5) * RES, 0.0] for i, j in cells.tolist()])
    poses[rng.integers(3, 65536, 40), 0] = XMIN - 0.3                      # off the grid, in the crowd
    mask = (rng.integers(0, 8, STRIDED) == 0).astype(np.int32)
    working, idle = ((65536, 65537, 65538), (0, 1, 2)) if second_turn_live else ((0, 1, 2), (65536, 65537, 65538))
    for b, (i, j) in zip(working, ((0, 6), (3, 6), (7, 5))):
        poses[b], mask[b] = _centre(g, i, j), 1
    poses[idle[0]], mask[idle[0]] = _centre(g, 5, 6), 0
    poses[idle[1]], mask[idle[1]] = [XMIN + 8 * RES + 0.3, 0.0, 0.0], 1
    poses[idle[2]], mask[idle[2]] = _centre(g, 7, 7), 0
    for a in (truth, poses, mask):
        a.setflags(write=False)
    return g, truth, poses, mask, working, idle


@pytest.mark.parametrize("want_ranges", [True, False], ids=["ranges", "no_ranges"])
@pytest.mark.parametrize("second_turn_live", [True, False], ids=["second_turn_works", "first_turn_works"])
def test_workgroups_stride_over_the_robots(second_turn_live, want_ranges):
    """more robots than workgroups in a launch, R = 1 (the LDS kernel, whose loop over a workgroup's robots has a barrier at its
    top and a `continue` for a robot that is masked out or off the grid): workgroups 0 .. 2 skip their first robot and work on
    their second, and the other way round; ranges (or, with d_ranges NULL, their sentinel) and `known` whole against the
    restatement"""
    g, truth, poses, mask, working, idle = _strided_fleet(second_turn_live)
    dev = _Device(g, truth)
    got, want = dev.reveal(1, poses.copy(), mask=mask.copy(), want_ranges=want_ranges)    # (the scene's arrays are read-only)
    _check_ranges(got, want)
    dev.check_known()
    rows = want[GUARD:-GUARD].reshape(STRIDED, 8)
    if want_ranges:
        assert (rows[list(working)] != S_RANGES).all() and (rows[[idle[0], idle[2]]] == S_RANGES).all() and (rows[idle[1]] == -1).all()
    # columns 5 .. 7 are the working three's alone, and the masked robots' own cells stay untouched
    assert (dev.known[:, 5:] != S_KNOWN).sum() == 12 and dev.known[5, 6] == S_KNOWN and dev.known[7, 7] == S_KNOWN
    assert (dev.known[:, :4] != S_KNOWN).all()
    alone = np.full_like(dev.known, S_KNOWN)
    sr.reveal(g, 1, truth, alone, poses[list(working)])
    assert np.array_equal(alone[:, 5:], dev.known[:, 5:])


def test_workgroups_stride_over_the_robots_in_global_memory():
    """the same fleet at R = 128, where the rays march in global memory and the kernel has a loop of its own: d_ranges NULL
    (65539 rows of 1024 ranges are not worth their bytes), `known` whole, second turn working and first turn working"""
    for second_turn_live in (True, False):
        g, truth, poses, mask, working, idle = _strided_fleet(second_turn_live)
        few = np.array(mask)
        few[3:65536] = 0                                                   # the crowd stays out: 1024 rays per robot in the restatement
        dev = _Device(g, truth)
        d_pose, d_mask = torch.as_tensor(poses.copy()).cuda(), torch.as_tensor(few).cuda()
        torch.cuda.synchronize()
        capi.sense_reveal_batch(dev.cfg, 128, dev.d_truth, dev.d_known, d_pose, None, d_mask)
        torch.cuda.synchronize()
        sr.reveal(g, 128, truth, dev.known, poses, few)
        dev.check_known()
        assert (dev.known != S_KNOWN).sum() > 12


@pytest.mark.parametrize("R", [32, 33, 65, 127, 128])
def test_each_side_of_every_switch(R):
    """the workgroup has 256 threads, a thread per ray: R = 32 is exactly one round of rays, 33 one round and a tail, 65 two
    rounds and a tail; R <= 127 marches in an LDS window, R = 128 in global memory.  Grid of 2R + 3 cells per side, three
    robots: in the middle (the whole window), in a corner and beside an edge (a clipped window)"""
    n = 2 * R + 3
    g = _geom(n, n)
    rng = np.random.default_rng(R)
    truth = np.where(rng.random((n, n)) < 0.004, 100, 0).astype(np.int8)
    truth[rng.integers(0, n, 40), rng.integers(0, n, 40)] = -1
    truth[R // 2, :R] = 100
    dev = _Device(g, truth)
    _check_ranges(*dev.reveal(R, [_centre(g, R + 1, R + 1), _centre(g, 0, n - 1), _centre(g, n - 2, R // 3)]))
    dev.check_known()
    assert (dev.known == S_KNOWN).any() and (dev.known == 100).any()


def test_calls_in_a_row_and_on_a_second_stream():
    """two calls in a row on one stream (the second re-reveals part of the first's cells: idempotent), then, after a
    synchronisation, a call on a second stream: the known grid is the restatement replayed in that order"""
    g, truth, poses = _fleet(65)
    dev = _Device(g, truth, known_fill=-1)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    _check_ranges(*dev.reveal(9, poses[:30], stream=s1.cuda_stream))
    _check_ranges(*dev.reveal(17, poses[20:50], stream=s1.cuda_stream))
    dev.check_known()
    before = dev.known.copy()
    _check_ranges(*dev.reveal(17, poses[20:50], stream=s1.cuda_stream))
    dev.check_known()
    assert np.array_equal(before, dev.known)
    _check_ranges(*dev.reveal(3, poses[40:], stream=s2.cuda_stream))
    dev.check_known()
    # P == 0: EEA_OK, nothing launched
    d_pose = torch.as_tensor(poses).cuda()    # (an empty tensor has a null pointer, which is an argument error: P by hand)
    capi.check(capi.lib().eea_sense_reveal_batch(0, dev.cfg, 9, dev.d_truth.data_ptr(), dev.d_known.data_ptr(), d_pose.data_ptr(),
                                                 None, 0, None, None))
    torch.cuda.synchronize()
    dev.check_known()


@pytest.mark.parametrize("xs,ys", [(1, 1), (63, 1), (64, 1), (65, 1), (4099, 3)])
@pytest.mark.parametrize("shift", [0, 5])
def test_census_against_count_nonzero(xs, ys, shift):
    """grids of 1, 63, 64, 65 and 4099 x 3 cells, the grid starting 37 and 42 bytes into its allocation (the kernel loads 16
    bytes at a time from the first 16-byte boundary on); d_counts is overwritten, not added to"""
    rng = np.random.default_rng(xs + shift)
    g = _geom(xs, ys)
    grid = rng.choice(np.array([-1, -1, 0, 0, 0, 79, 80, 100, -128, 127, 50], dtype=np.int8), size=(ys, xs))
    buf = torch.as_tensor(np.concatenate([np.full(GUARD + shift, 100, np.int8), grid.reshape(-1), np.full(GUARD, -1, np.int8)])).cuda()
    counts = torch.full((5,), 123456789, dtype=torch.int64, device="cuda")
    for _ in range(2):
        capi.grid_census(_cfg(g), buf[GUARD + shift:GUARD + shift + grid.size], counts[1:4])
    torch.cuda.synchronize()
    got = counts.cpu().numpy()
    cells = grid.reshape(-1)
    below = cells.astype(np.float64) / 100.0 < THR
    want = (np.count_nonzero(cells < 0), np.count_nonzero((cells >= 0) & below), np.count_nonzero(~below))
    assert tuple(int(v) for v in got[1:4]) == want == sr.census(g, grid)
    assert got[0] == got[4] == 123456789 and want[0] + want[1] + want[2] == grid.size


@pytest.mark.parametrize("shift", [0, 5])
def test_census_past_the_launch_cap(shift):
    """8192 x 1025 cells: 524 800 loads of 16 bytes for the 2048 x 256 threads a launch is capped at, so the first threads take a
    second step of the body loop (every smaller grid gives each thread at most one load).  The grid starts 37 and 42 bytes into
    its allocation; d_counts sits between guard words and is overwritten, not added to"""
    xs, ys = 8192, 1025
    assert xs * ys // 16 - 1 > 2048 * 256
    rng = np.random.default_rng(xs + ys + shift)
    g = _geom(xs, ys)
    grid = rng.choice(np.array([-1, -1, 0, 0, 0, 79, 80, 100, -128, 127, 50], dtype=np.int8), size=(ys, xs))
    grid[-1, -600:] = 100                      # the cells of the second step's last loads and of the tail: unlike the rest
    grid[0, :300] = -1                         # ... and of the head and the first loads
    buf = torch.as_tensor(np.concatenate([np.full(GUARD + shift, 100, np.int8), grid.reshape(-1), np.full(GUARD, -1, np.int8)])).cuda()
    counts = torch.full((5,), 123456789, dtype=torch.int64, device="cuda")
    for _ in range(2):
        capi.grid_census(_cfg(g), buf[GUARD + shift:GUARD + shift + grid.size], counts[1:4])
    torch.cuda.synchronize()
    got = counts.cpu().numpy()
    cells = grid.reshape(-1)
    below = cells.astype(np.float64) / 100.0 < THR
    want = (np.count_nonzero(cells < 0), np.count_nonzero((cells >= 0) & below), np.count_nonzero(~below))
    assert tuple(int(v) for v in got[1:4]) == want == sr.census(g, grid)
    assert got[0] == got[4] == 123456789 and want[0] + want[1] + want[2] == grid.size and min(want) > 1000000


def _entropy_target(occ):
    """the oracle's entropy() of every cell (numerics.hpp:164-179), normalised: the target eea_set_target_occupancy builds"""
    lut = np.array([po.lib().eo_entropy(float(np.int8(np.uint8(b))) / 100.0) for b in range(256)])
    ent = lut[occ.reshape(-1).view(np.uint8)]
    return ent / ent.sum()


def test_closed_loop_reveals_the_map():
    """6 robots, 25 ticks, a 12 x 6 m map at 0.1 m with walls the robots have not seen: per tick reveal -> census ->
    eea_set_target_occupancy(on_device) of the KNOWN grid -> eea_tick_batch on the known grid (grid_epoch = 0: it changes
    every tick) -> eea_integrate_twist_batch.  The final known grid is, bitwise, the restatement replayed over the recorded
    poses; the unknown count never rises and ends below its value after the first reveal; phi_k after the last re-target is
    the oracle's occupancy phi_k of that known grid within the bound of tests/test_gpu_phik_parity.py (1e-11)."""
    B, ticks, R, K, res, dt = 6, 25, 15, 10, 0.1, 0.1
    xs, ys = 120, 60
    g = sr.Geometry(0.0, 0.0, res, xs, ys, THR)
    truth = np.zeros((ys, xs), dtype=np.int8)
    truth[0], truth[-1], truth[:, 0], truth[:, -1] = 100, 100, 100, 100
    truth[:38, 45:47] = 100          # a wall from the bottom with a gap at the top
    truth[25:, 80:82] = 100          # a wall from the top with a gap at the bottom
    truth[28:32, 20:30] = 100        # a block
    ccfg = capi.make_collision_cfg(0.0, 0.0, res, xs, ys, 0.2, 0.4, 0.05, THR)
    dcfg = capi.DwaCfg(0.1, 1.0, 0.2, 2.5, 2.5, 1.0, 1.0, -1.0, 1.0, -1.0, 2.0, -2.0, 3, 8, 5)
    lim = np.array([1.0, 1.0, 2.0])
    eng = capi.Engine(capi.make_config(capi.MODEL_OMNI, dt, 2.0, res, 1.0, K, np.diag([1.0, 1.0, 2.0]), -lim, lim))
    T = eng.T
    lx, ly = (xs - 1) * res, (ys - 1) * res
    poses0 = np.array([[1.5, 1.5, 0.0], [3.0, 4.5, 1.0], [6.2, 1.2, 2.0], [6.5, 4.8, -1.0], [10.0, 3.0, 3.0], [9.2, 1.0, 0.5]])
    zeros = lambda *s, dtype=torch.float64: torch.zeros(s, dtype=dtype, device="cuda")
    d_pose = torch.as_tensor(poses0).cuda()
    d_truth = torch.as_tensor(truth).cuda()
    d_known = torch.full((ys, xs), -1, dtype=torch.int8, device="cuda")
    d_counts = zeros(3, dtype=torch.int64)
    d_ut, d_traj = zeros(B, T, 3), zeros(B, T, 3)
    d_follow, d_count, d_valid, d_skip = (zeros(B, dtype=torch.int32) for _ in range(4))
    d_u, d_vb = zeros(B, 3), zeros(B, 3)
    recorded, unknown = [], []
    for t in range(ticks):
        torch.cuda.synchronize()
        recorded.append(d_pose.cpu().numpy().copy())
        capi.sense_reveal_batch(ccfg, R, d_truth, d_known, d_pose)
        capi.grid_census(ccfg, d_known, d_counts)
        eng.set_target_occupancy(xs, ys, d_known, lx, ly)
        eng.tick_batch(B, d_pose, d_ut, d_follow, d_count, d_u, d_vb, d_known, d_traj, d_valid, d_skip, ccfg, dcfg, 0.1, 0.5,
                       grid_epoch=0)
        capi.integrate_twist_batch(d_pose, d_u, dt, normalize_heading=True)
        d_vb.copy_(d_u)
        torch.cuda.synchronize()
        c = d_counts.cpu().numpy()
        assert int(c.sum()) == xs * ys
        unknown.append(int(c[0]))
    known = np.full((ys, xs), -1, dtype=np.int8)
    for p in recorded:
        sr.reveal(g, R, truth, known, p)
    got = d_known.cpu().numpy()
    assert np.array_equal(got, known)
    print("unknown cells per tick:", unknown)
    assert unknown[-1] == int((known < 0).sum())
    assert all(b <= a for a, b in zip(unknown, unknown[1:])) and unknown[-1] < unknown[0]
    assert np.isfinite(recorded[-1]).all() and np.abs(recorded[-1] - recorded[0]).max() > 0.0
    ref = po.spatial_coeff(lx, ly, K, _entropy_target(known), po.phi_grid(xs, ys, res))
    err = np.abs(eng.phik() - ref).max()
    print("max |phi_k - oracle| after the last re-target: %.3e" % err)
    assert err < 1e-11
    eng.close()


def test_sense_argument_errors():
    g, truth, poses = _fleet(3)
    dev = _Device(g, truth)
    d_pose = torch.as_tensor(poses).cuda()
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    for kw in (dict(truth=None), dict(known=None), dict(pose=None), dict(known="truth"), dict(R=0)):
        a = dict(dict(truth=dev.d_truth, known=dev.d_known, pose=d_pose, R=5), **kw)
        if a["known"] == "truth":
            a["known"] = a["truth"]
        with pytest.raises(capi.EngineError) as ei:
            if a["pose"] is None:    # (the binding reads P from the pose tensor)
                capi.check(capi.lib().eea_sense_reveal_batch(0, dev.cfg, a["R"], a["truth"].data_ptr(), a["known"].data_ptr(), None,
                                                             None, 3, None, None))
            else:
                capi.sense_reveal_batch(dev.cfg, a["R"], a["truth"], a["known"], a["pose"])
        assert ei.value.status == capi.ERR_INVALID_ARGUMENT, kw
    with pytest.raises(capi.EngineError) as ei:
        capi.sense_reveal_batch(dev.cfg, 1025, dev.d_truth, dev.d_known, d_pose)
    assert ei.value.status == capi.ERR_UNSUPPORTED
    for field, bad in (("xsize", 0), ("ysize", 0), ("resolution", 0.0), ("resolution", -1.0)):
        cfg = _cfg(g)
        setattr(cfg, field, bad)
        with pytest.raises(capi.EngineError) as ei:
            capi.sense_reveal_batch(cfg, 5, dev.d_truth, dev.d_known, d_pose)
        assert ei.value.status == capi.ERR_INVALID_ARGUMENT, field
        with pytest.raises(capi.EngineError) as ei:
            capi.grid_census(cfg, dev.d_known, counts)
        assert ei.value.status == capi.ERR_INVALID_ARGUMENT, field
    for grid, out in ((None, counts), (dev.d_known, None)):
        with pytest.raises(capi.EngineError) as ei:
            capi.grid_census(dev.cfg, grid, out)
        assert ei.value.status == capi.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    dev.check_known()               # no refused call wrote anything
    assert (dev.known == S_KNOWN).all()

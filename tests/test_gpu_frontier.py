"""Frontier regions and their goals on the device (include/ergodic_amd.h: eea_frontier_regions, eea_frontier_goals;
csrc/frontier_kernel.hip).

Checker: tests/frontier_restatement.py (a flood fill, held to a two-pass raster union-find and to the records' invariants by
tests/test_frontier.py).  Planes, records and goals are integers (and one double per robot, compared by its bits) compared
BITWISE as whole buffers.  Every output sits between guard elements and holds a sentinel before the call, every input and the
workspace sit between guards and come back unchanged.  Scenes are sized from the tile the header publishes
(tests/frontier_scenes.py); the guarded buffers are tests/test_gpu_geodesic.py's."""
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ergodic_exploration_amd import capi
from tests import frontier_restatement as fr
from tests import frontier_scenes as fs
from tests import geodesic_restatement as geo
from tests import partition_restatement as part
from tests import sense_restatement as sr
from tests import test_gpu_geodesic as tg

pytestmark = pytest.mark.gpu

ROOT = tg.ROOT
T = fs.T
G_IN, G_OUT, S_GEO, S_STATE, S_PATH = tg.G_IN, tg.G_OUT, tg.S_GEO, tg.S_STATE, tg.S_PATH
S_REGION, S_RECORD, S_SCORE = 0x7ACE0FF1, 0x5EED5EED5EED5EED, -3.5e77
WS_GUARD = 64                      # bytes around the workspace (which must stay 8-byte aligned)
WORDS = fr.RECORD.itemsize // 8    # a record as 64-bit words: the record buffer is guarded as int64, which keeps it 8-byte aligned
_guarded, _geom, _bits = tg._guarded, tg._geom, tg._bits


class _Device(tg._Device):
    """tests/test_gpu_geodesic.py's device grid with the frontier's workspace"""

    def __init__(self, g, grid):
        super().__init__(g, grid)
        self.n_fws = capi.frontier_ws_bytes(self.cfg)
        self._fws = torch.full((self.n_fws + 2 * WS_GUARD,), G_IN, dtype=torch.uint8, device="cuda")
        self.d_fws = self._fws[WS_GUARD:WS_GUARD + self.n_fws]
        assert self.d_fws.data_ptr() % 8 == 0

    def check(self, buf, guard=G_OUT):
        w = self._fws.cpu().numpy()
        assert (w[:WS_GUARD] == G_IN).all() and (w[-WS_GUARD:] == G_IN).all(), "a guard byte of the frontier's workspace was written"
        return super().check(buf, guard)

    def regions(self, kind, geo_plane=None, owner=None, max_regions=0, n_records=None, stream=None):
        """one call; (root, region int32 [ysize][xsize], records RECORD [n_records] -- sentinel bytes where nothing was written --,
        state uint32 [4]) after the guards.  n_records: the records the buffer holds (max_regions when None); 0: d_regions NULL"""
        n_records = max_regions if n_records is None else n_records
        d_geo = None if geo_plane is None else self.upload(geo_plane, np.int32)
        d_owner = None if owner is None else self.upload(owner, np.int32)
        _, tbuf, d_root = _guarded(np.full(self.grid.size, S_GEO, np.int32), G_OUT, np.int32)
        _, gbuf, d_region = _guarded(np.full(self.grid.size, S_REGION, np.int32), G_OUT, np.int32)
        _, sbuf, d_state = _guarded(np.full(4, S_STATE, np.uint32).view(np.int32), G_OUT, np.int32)
        rbuf = d_rec = None
        if n_records:
            _, rbuf, d_rec = _guarded(np.full(n_records * WORDS, S_RECORD, np.int64), G_OUT, np.int64)
            assert d_rec.data_ptr() % 8 == 0
        torch.cuda.synchronize()
        capi.frontier_regions(self.cfg, kind, self.d_grid, d_root, d_region, self.d_fws, d_state, regions=d_rec, max_regions=max_regions,
                              geo=d_geo, owner=d_owner, stream=stream)
        torch.cuda.synchronize()
        self.d_rec, self.d_state, self.d_geo, self.d_owner = d_rec, d_state, d_geo, d_owner
        shape = self.grid.shape
        rec = np.zeros(0, dtype=fr.RECORD) if rbuf is None else self.check(rbuf).copy().view(fr.RECORD)
        return (self.check(tbuf).reshape(shape).copy(), self.check(gbuf).reshape(shape).copy(), rec,
                self.check(sbuf).view(np.uint32).copy())

    def goals(self, rec, state, max_regions, P, min_size, w_size, w_cost, stream=None):
        """one call on uploaded records and state; (goal_cell, goal_region int32 [P], goal_score float64 [P]) after the guards"""
        d_rec = self.upload(np.ascontiguousarray(rec).view(np.int64), np.int64)
        d_state = self.upload(np.asarray(state, dtype=np.uint32).view(np.int32), np.int32)
        return self.goals_of(d_rec, d_state, max_regions, P, min_size, w_size, w_cost, stream)

    def goals_of(self, d_rec, d_state, max_regions, P, min_size, w_size, w_cost, stream=None):
        _, cbuf, d_cell = _guarded(np.full(P, S_GEO, np.int32), G_OUT, np.int32)
        _, gbuf, d_region = _guarded(np.full(P, S_REGION, np.int32), G_OUT, np.int32)
        _, sbuf, d_score = _guarded(np.full(P, S_SCORE), 2.5, np.float64)
        torch.cuda.synchronize()
        capi.frontier_goals(d_rec, d_state, max_regions, d_cell, d_region, d_score, min_size=min_size, w_size=w_size, w_cost=w_cost,
                            stream=stream)
        torch.cuda.synchronize()
        self.d_goal_cell = d_cell
        return self.check(cbuf).copy(), self.check(gbuf).copy(), self.check(sbuf, 2.5).copy()


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s differs at %s: got %s want %s" % (what, bad[:6].tolist(), [int(got[tuple(b)]) for b in bad[:6]],
                                                                [int(want[tuple(b)]) for b in bad[:6]])


def _sentinel(n):
    return np.full(n * WORDS, S_RECORD, np.int64).view(fr.RECORD)


def _run(dev, kind, geo_plane=None, owner=None, max_regions=None, spare=3, want=None, **kw):
    """one call against the restatement: both planes and the state as whole buffers, the records written by their bytes, the
    records past min(n, max_regions) (the buffer holds `spare` more than max_regions) still the sentinel.  max_regions None: room
    for every region.  want: the restatement's answer to these arguments where the caller holds it already (the large scenes,
    whose reference is fr.regions_fast, computed once).  Returns the planes, the records written and the state"""
    want_root, want_region, want_rec, want_state = want if want is not None else fr.regions(
        kind, dev.grid, dev.g.occupied_threshold, geo=geo_plane, owner=owner, max_regions=max_regions)
    cap = int(want_state[0]) + 2 if max_regions is None else max_regions
    root, region, rec, state = dev.regions(kind, geo_plane, owner, max_regions=cap, n_records=cap + spare if cap else 0, **kw)
    _same(root, want_root, "root")
    _same(region, want_region, "region")
    assert state.tolist() == [int(want_state[0]), min(int(want_state[0]), cap), int(want_state[2]), 0], (state, want_state)
    kept = int(state[1])
    if cap:
        assert rec[:kept].tobytes() == want_rec[:kept].tobytes(), [(r, rec[r], want_rec[r]) for r in range(kept) if rec[r] != want_rec[r]][:3]
        assert rec[kept:].tobytes() == _sentinel(len(rec) - kept).tobytes(), "a record past min(n, max_regions) was written"
    return root, region, rec[:kept], state


# ---- masks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fs.MASKS))
def test_mask_scenes_are_the_restatement(name):
    """arbitrary shapes through EEA_FRONTIER_OF_MASK: empty and full, a few cells, one row and one column of more than two
    tiles, a serpentine that fills a tile and one that winds through nine, two cells that meet only at a four-tile corner (both
    diagonals), a comb whose teeth are joined in another tile row with a U beside it, a checkerboard (the most unions, one
    region), random masks below, near and above the 8-neighbour percolation threshold, and isolated cells"""
    mask = fs.MASKS[name]()
    dev = _Device(_geom(mask.shape[1], mask.shape[0]), mask)
    root, region, rec, state = _run(dev, capi.FRONTIER_OF_MASK)
    if name == "full":
        assert state[0] == 1 and (root == 0).all() and rec[0]["size"] == mask.size
    if name == "comb_and_u":
        assert state[0] == 2 and rec[0]["root"] == 0 and (root[:T, 0:48:4] == 0).all()
    if name == "checkerboard":
        assert state[0] == 1 and rec[0]["size"] == mask.size // 2
    if name in ("corner_main", "corner_anti"):
        assert state.tolist() == [1, 1, 2, 0]


@pytest.mark.parametrize("max_regions", [5, 0])
def test_more_regions_than_records(max_regions):
    """members at every third cell of 3 T x 3 T: T * T regions of one cell.  With room for five records the state is [n, 5, n, 0],
    the records from the sixth on keep the sentinel and d_region holds the true ranks; max_regions = 0 with d_regions = NULL
    writes the planes and the state"""
    mask = fs.MASKS["every_third"]()
    dev = _Device(_geom(mask.shape[1], mask.shape[0]), mask)
    root, region, rec, state = _run(dev, capi.FRONTIER_OF_MASK, max_regions=max_regions)
    assert state.tolist() == [T * T, max_regions, T * T, 0] and region.max() == T * T - 1 and len(rec) == max_regions
    assert np.array_equal(region[mask != 0], np.arange(T * T))


# ---- grids -----------------------------------------------------------------------------------------------------------------
def test_the_hand_built_grid():
    """values 0, 69, 70 and 100 at occupied_threshold 0.7, unknown cells only diagonal to a free cell, unknown cells at the
    grid's border, a free cell on the grid's edge with no unknown neighbour: the members are the ones written down"""
    grid, members = fs.known_grid()
    g = sr.Geometry(fs.gs.XMIN, fs.gs.YMIN, fs.gs.RES, grid.shape[1], grid.shape[0], 0.7)
    dev = _Device(g, grid)
    root, region, rec, state = _run(dev, capi.FRONTIER_OF_GRID)
    assert np.array_equal(root >= 0, members) and state[2] == members.sum()


def test_a_revealed_map_with_the_partitions_planes():
    """a grid revealed by the sensor's restatement with d_geo / d_owner of the partition's restatement: members with geo -1 cut
    a rim in two, an entry is the member with the least (geo, index) -- a rim in the open has several at the least cost -- and
    entry_owner is the partition's; without the planes the rim is whole and the entries are -1; with d_geo alone the owners are"""
    sc = fs.revealed_scene()
    dev = _Device(sc.g, sc.known)
    root0, _, rec0, state0 = _run(dev, capi.FRONTIER_OF_GRID)
    root, region, rec, state = _run(dev, capi.FRONTIER_OF_GRID, geo_plane=sc.geo, owner=sc.owner)
    assert state[0] > state0[0] and state[2] < state0[2] and (rec0["entry_cell"] == -1).all()
    assert (rec["entry_cell"] >= 0).all() and (rec["entry_owner"] >= 0).all() and len(set(rec["entry_owner"].tolist())) == 3
    flat = sc.geo.reshape(-1)
    assert any(((region.reshape(-1) == r) & (flat == e["entry_cost"])).sum() > 1 for r, e in enumerate(rec))
    _, _, rec1, _ = _run(dev, capi.FRONTIER_OF_GRID, geo_plane=sc.geo)
    assert (rec1["entry_owner"] == -1).all() and np.array_equal(rec1["entry_cell"], rec["entry_cell"])
    _run(dev, capi.FRONTIER_OF_MASK, geo_plane=sc.geo, owner=sc.owner)      # the mask kind takes the planes as well


# ---- repetition ------------------------------------------------------------------------------------------------------------
def test_the_same_call_again_and_on_another_stream_gives_the_same_bits():
    mask = fs.MASKS["random_45"]()
    dev = _Device(_geom(mask.shape[1], mask.shape[0]), mask)
    first = _run(dev, capi.FRONTIER_OF_MASK)
    again = _run(dev, capi.FRONTIER_OF_MASK)
    st = torch.cuda.Stream()
    other = _run(dev, capi.FRONTIER_OF_MASK, stream=st.cuda_stream)
    for run in (again, other):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, run))
    sc = fs.revealed_scene()
    dev = _Device(sc.g, sc.known)
    first = _run(dev, capi.FRONTIER_OF_GRID, geo_plane=sc.geo, owner=sc.owner)
    other = _run(dev, capi.FRONTIER_OF_GRID, geo_plane=sc.geo, owner=sc.owner, stream=st.cuda_stream)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, other))
    P = 3
    want = dev.goals_of(dev.d_rec, dev.d_state, len(first[2]), P, 1, 1.0, 0.125)
    got = dev.goals_of(dev.d_rec, dev.d_state, len(first[2]), P, 1, 1.0, 0.125, stream=st.cuda_stream)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(want, got))


# ---- goals -----------------------------------------------------------------------------------------------------------------
def _records(rows):
    """hand-made records: (size, entry_cost, entry_cell, entry_owner) per row"""
    rec = np.zeros(len(rows), dtype=fr.RECORD)
    for r, (size, cost, cell, owner) in enumerate(rows):
        rec[r]["size"], rec[r]["entry_cost"], rec[r]["entry_cell"], rec[r]["entry_owner"] = size, cost, cell, owner
        rec[r]["root"] = cell
    return rec


def _check_goals(dev, rec, state, max_regions, P, min_size, w_size, w_cost):
    n = min(int(state[1]), max_regions)
    want = fr.goals(rec[:n], P, min_size, w_size, w_cost)
    got = dev.goals(rec, state, max_regions, P, min_size, w_size, w_cost)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (got, want)
    assert np.array_equal(_bits(got[2]), _bits(want[2])), (got[2], want[2])
    return got


def test_goals_are_the_restatement():
    """ties broken by the lowest r, min_size filtering a speckle, owners >= P and < 0 ignored, a record without an entry, a robot
    without a region gets -1 / -1 / 0.0, w_cost = 0, P = 1, records past d_state[1] and past max_regions ignored"""
    dev = _Device(_geom(4, 3), np.zeros((3, 4), dtype=np.int8))
    rows = [(1, 5, 100, 0),      # 0: a speckle next to robot 0
            (40, 35, 200, 0),    # 1
            (40, 35, 300, 0),    # 2: ties with 1 under every weight pair
            (7, 10, 400, 2),     # 3
            (9, 0, 500, 5),      # 4: an owner >= P
            (9, 0, 600, -1),     # 5: nobody's
            (50, 0, -1, 2),      # 6: no entry
            (8, 20, 700, 2),     # 7
            (99, 0, 800, 1)]     # 8: robot 1's only region: past d_state[1] in the second run
    rec = _records(rows)
    n = len(rows)
    full = [n, n, 0, 0]
    cell, region, score = _check_goals(dev, rec, full, n, 4, 2, 1.0, 0.125)
    assert cell.tolist() == [200, 800, 400, -1] and region.tolist() == [1, 8, 3, -1] and score[3] == 0.0 and score[0] == 40 - 0.125 * 35
    cell, region, score = _check_goals(dev, rec, full, n, 4, 1, 0.0, 1.0)       # the nearest: the speckle wins
    assert cell.tolist() == [100, 800, 400, -1] and score[0] == -5.0
    cell, region, score = _check_goals(dev, rec, full, n, 4, 1, 1.0, 0.0)       # w_cost = 0: the largest, ties to the lowest r
    assert region.tolist() == [1, 8, 7, -1]
    cell, region, score = _check_goals(dev, rec, full, n, 4, 1, 0.0, 0.0)       # every score 0.0: the lowest r that is eligible
    assert region.tolist() == [0, 8, 3, -1] and (score == 0.0).all()
    cell, region, score = _check_goals(dev, rec, [n, n - 1, 0, 0], n, 4, 2, 1.0, 0.125)   # d_state[1] is read on the device
    assert cell[1] == -1 and region[0] == 1
    cell, region, score = _check_goals(dev, rec, full, 2, 4, 2, 1.0, 0.125)     # max_regions below d_state[1]
    assert region.tolist() == [1, -1, -1, -1]
    cell, region, score = _check_goals(dev, rec, full, n, 1, 2, 1.0, 0.125)     # P = 1
    assert cell.tolist() == [200]
    cell, region, score = _check_goals(dev, rec, full, n, 300, 100, 1e30, 1e30)  # more than a workgroup of robots, nobody eligible
    assert (cell == -1).all() and (region == -1).all() and (score == 0.0).all()
    _check_goals(dev, rec, [0, 0, 0, 0], n, 4, 1, 1.0, 0.0)


def test_many_records_and_many_robots():
    """more records and robots than a workgroup has lanes, scores full of ties"""
    rng = np.random.default_rng(7)
    n, P = 3000, 700
    rows = [(int(rng.integers(1, 6)), int(rng.integers(0, 4)) * 5, int(rng.integers(0, 1 << 20)) if rng.random() < 0.9 else -1,
             int(rng.integers(-1, P + 5))) for _ in range(n)]
    dev = _Device(_geom(4, 3), np.zeros((3, 4), dtype=np.int8))
    rec = _records(rows)
    for min_size, ws, wc in ((1, 1.0, 0.0), (2, 1.0, 0.2), (1, 0.0, 1.0)):
        cell, region, score = _check_goals(dev, rec, [n, n, 0, 0], n, P, min_size, ws, wc)
        assert (region >= 0).sum() > P // 2


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_reveal_partition_frontier_goals_paths_on_the_device():
    """the loop the frontier closes, device buffers end to end on a 2 T x (T + 16) map: reveal -> eea_geodesic_partition (unknown
    cells block) -> eea_frontier_regions -> eea_frontier_goals -> the existing eea_partition_path_batch.  Every robot with a goal
    has len >= 0, and with n_steps >= cost / 5 the last way-point is the goal cell's centre by its bits"""
    sc = fs.revealed_scene()
    g = sc.g
    dev = _Device(g, sc.truth)
    P = len(sc.poses)
    d_known = torch.full((g.ysize * g.xsize,), -1, dtype=torch.int8, device="cuda")
    d_pose = dev.upload(sc.poses, np.float64).view(-1, 3)
    capi.sense_reveal_batch(dev.cfg, sc.R, dev.d_grid, d_known, d_pose)
    torch.cuda.synchronize()
    assert np.array_equal(d_known.cpu().numpy().reshape(sc.known.shape), sc.known)
    seen = _Device(g, sc.known)
    d_geo = torch.empty(g.ysize * g.xsize, dtype=torch.int32, device="cuda")
    d_owner = torch.empty_like(d_geo)
    d_pws = torch.empty(capi.partition_ws_bytes(seen.cfg), dtype=torch.uint8, device="cuda")
    d_pstate = torch.empty(4, dtype=torch.int32, device="cuda")
    capi.geodesic_partition(seen.cfg, d_known, d_geo, d_owner, d_pws, d_pstate, pose=d_pose, flags=capi.GEODESIC_UNKNOWN_BLOCKS)
    cost, owner = (a.cpu().numpy().reshape(sc.known.shape) for a in (d_geo, d_owner))
    want_cost, want_owner, _ = part.partition(g, sc.known, poses=sc.poses, flags=geo.UNKNOWN_BLOCKS)
    assert np.array_equal(cost, want_cost) and np.array_equal(owner, want_owner)
    root, region, rec, state = _run(seen, capi.FRONTIER_OF_GRID, geo_plane=cost, owner=owner)
    cell, reg, score = seen.goals_of(seen.d_rec, seen.d_state, len(rec), P, 2, 1.0, 0.125)
    want = fr.goals(rec[:int(state[1])], P, 2, 1.0, 0.125)
    assert np.array_equal(cell, want[0]) and np.array_equal(reg, want[1]) and np.array_equal(_bits(score), _bits(want[2]))
    # (the first two robots' rims touch: one region, whose entry the first robot owns -- the second gets no goal: no second round)
    going = [q for q in range(P) if cell[q] >= 0]
    assert len(going) >= 2 and all(owner.reshape(-1)[cell[q]] == q and cost.reshape(-1)[cell[q]] >= 0 for q in going)
    n_steps = int(max(rec["entry_cost"][reg[going]]) // 5) + 3
    assert all(n_steps >= rec["entry_cost"][reg[q]] / 5 for q in going)
    _, pbuf, d_path = _guarded(np.full(P * n_steps * 3, S_PATH), 2.5, np.float64)
    _, lbuf, d_len = _guarded(np.full(P, S_GEO, np.int32), G_OUT, np.int32)
    capi.partition_path_batch(seen.cfg, seen.d_geo, seen.d_owner, d_pose, seen.d_goal_cell, d_path.view(P, n_steps, 3), d_len)
    torch.cuda.synchronize()
    path, length = seen.check(pbuf, 2.5).reshape(P, n_steps, 3), seen.check(lbuf)
    want_path, want_len = part.paths(g, cost, owner, sc.poses, cell, n_steps)
    assert np.array_equal(length, want_len) and np.array_equal(_bits(path), _bits(want_path))
    assert np.array_equal(length >= 0, cell >= 0) and (length > 0).any()
    for q in going:
        cx, cy = geo.cell_centre(g, int(cell[q]) // g.xsize, int(cell[q]) % g.xsize)
        assert np.array_equal(_bits(path[q, -1, :2]), _bits(np.array([cx, cy]))), q


# ---- past 256 chunks: the paths only large inputs reach ----------------------------------------------------------------------
# More than 256 * 1024 cells (tests/frontier_scenes.py asserts it): every thread of frontier_rank_kernel sums share = 2 chunks,
# so its two chunk loops take a second turn, the threads past chunks / 2 clamp lo and hi, and half the scatter workgroups read an
# offset written on that second turn; the stats launch has 129 and more workgroups, merge and flatten see sets that span
# hundreds of tiles.  The reference is fr.regions_fast, held to fr.regions byte for byte by tests/test_frontier.py
@pytest.mark.parametrize("name", sorted(fs.LARGE_MASKS))
def test_large_masks_are_the_restatement(name):
    """506 x 520 (257 chunks, 16 x 17 tiles, ragged both ways): 29 406 regions of one cell, whose ranks run through every chunk
    offset; one serpentine of 131 813 members through all 272 tiles, whose record takes atomics from every stats workgroup;
    random masks at 5 % and 45 %.  33 x 8192 (264 chunks, 256 x 2 tiles): a row united only westwards across 256 tiles, 4096
    regions of one cell, runs of 63.  Planes, state and every record with room for all of them"""
    mask = fs.LARGE_MASKS[name]()
    want = fs.large_mask_regions(name)
    dev = _Device(_geom(mask.shape[1], mask.shape[0]), mask)
    assert dev.n_fws == 2 * 4 * ((mask.size - 1) // 1024 + 1) > 2 * 4 * 256
    root, region, rec, state = _run(dev, capi.FRONTIER_OF_MASK, want=want)
    assert len(rec) == int(want[3][0]) == state[0] and state[2] == np.count_nonzero(mask)
    if name == "large_serpentine":
        assert state[0] == 1 and (root[mask != 0] == 0).all() and rec[0]["size"] == np.count_nonzero(mask)
    if name == "large_rows":
        assert (root[0] == 0).all() and rec[0]["size"] == mask.shape[1] and np.array_equal(region[2, 0::2], np.arange(1, 4097))


@pytest.mark.parametrize("max_regions", [300, 0])
def test_large_every_third_with_fewer_records_than_regions(max_regions):
    """29 406 regions and room for 300 records, or none (d_regions NULL): d_region holds the true ranks past the cut in every
    one of the 257 chunks, the records from the 301st on keep the sentinel"""
    mask = fs.LARGE_MASKS["large_every_third"]()
    dev = _Device(_geom(mask.shape[1], mask.shape[0]), mask)
    root, region, rec, state = _run(dev, capi.FRONTIER_OF_MASK, max_regions=max_regions,
                                    want=fs.large_mask_regions("large_every_third", max_regions))
    n = np.count_nonzero(mask)
    assert state.tolist() == [n, max_regions, n, 0] and len(rec) == max_regions and n == 29406
    assert np.array_equal(region[mask != 0], np.arange(n))


def test_a_large_revealed_map_its_goals_and_their_paths():
    """506 x 520 revealed by 300 robots, with the partition's planes (300 labels): regions and records, then eea_frontier_goals
    for P = 300 (two workgroups of robots) on the device's own records, then eea_partition_path_batch on the goal cells: every
    robot with a goal has len >= 0, way-points and lengths are the restatement's"""
    sc = fs.large_revealed()
    g, P = sc.g, len(sc.poses)
    dev = _Device(g, sc.known)
    root, region, rec, state = _run(dev, capi.FRONTIER_OF_GRID, geo_plane=sc.geo, owner=sc.owner, want=fs.large_revealed_regions())
    assert state[0] > P and (rec["entry_cell"] >= 0).all() and len(set(rec["entry_owner"].tolist())) > 200
    cell, reg, score = dev.goals_of(dev.d_rec, dev.d_state, len(rec), P, 2, 1.0, 0.125)
    want = fr.goals(rec, P, 2, 1.0, 0.125)
    assert np.array_equal(cell, want[0]) and np.array_equal(reg, want[1]) and np.array_equal(_bits(score), _bits(want[2]))
    going = np.flatnonzero(cell >= 0)
    assert len(going) > 200 and (going >= 256).any() and cell[P - 1] == -1
    assert (sc.owner.reshape(-1)[cell[going]] == going).all() and (sc.geo.reshape(-1)[cell[going]] >= 0).all()
    n_steps = int(rec["entry_cost"][reg[going]].max()) // 5 + 3
    d_pose = dev.upload(sc.poses, np.float64).view(-1, 3)
    _, pbuf, d_path = _guarded(np.full(P * n_steps * 3, S_PATH), 2.5, np.float64)
    _, lbuf, d_len = _guarded(np.full(P, S_GEO, np.int32), G_OUT, np.int32)
    torch.cuda.synchronize()
    capi.partition_path_batch(dev.cfg, dev.d_geo, dev.d_owner, d_pose, dev.d_goal_cell, d_path.view(P, n_steps, 3), d_len)
    torch.cuda.synchronize()
    path, length = dev.check(pbuf, 2.5).reshape(P, n_steps, 3), dev.check(lbuf)
    want_path, want_len = part.paths(g, sc.geo, sc.owner, sc.poses, cell, n_steps)
    assert np.array_equal(length, want_len) and np.array_equal(_bits(path), _bits(want_path))
    assert np.array_equal(length >= 0, cell >= 0) and (length > 0).any() and length.max() < n_steps


def test_a_large_call_again_on_another_stream_gives_the_same_bits():
    """the 45 % mask (thousands of unions in flight, records that take atomics from many workgroups) and the revealed map with
    its planes: the second call, on another stream, gives the bits of the first"""
    st = torch.cuda.Stream()
    mask = fs.LARGE_MASKS["large_random_45"]()
    dev = _Device(_geom(mask.shape[1], mask.shape[0]), mask)
    want = fs.large_mask_regions("large_random_45")
    first = _run(dev, capi.FRONTIER_OF_MASK, want=want)
    other = _run(dev, capi.FRONTIER_OF_MASK, want=want, stream=st.cuda_stream)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, other))
    sc = fs.large_revealed()
    dev = _Device(sc.g, sc.known)
    want = fs.large_revealed_regions()
    first = _run(dev, capi.FRONTIER_OF_GRID, geo_plane=sc.geo, owner=sc.owner, want=want)
    other = _run(dev, capi.FRONTIER_OF_GRID, geo_plane=sc.geo, owner=sc.owner, want=want, stream=st.cuda_stream)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, other))


# ---- the host mirror -------------------------------------------------------------------------------------------------------
def _host_map(W, H):
    """the map of host/test/frontier_regions_tests.cpp"""
    d = np.zeros((H, W), dtype=np.int8)
    d[:30, 20] = 100
    d[12, 20] = 0
    d[25, 34:44] = d[34, 34:44] = 100
    d[25:35, 34] = d[25:35, 43] = 100
    d[3:9, 30:36] = -1
    d[:, 46:] = -1
    d[20, 40:46] = 100
    d[22, 5] = -1
    return d


def test_host_mirror_frontier_regions():
    """host/build/frontier_regions_tests (FrontierRegions in frontier_regions.hpp: update with a GeodesicPartition, regions,
    rootAt / regionAt, goals, and the goal cells in eea_partition_path_batch) runs, and its printed answers are the restatement's"""
    exe = os.path.join(ROOT, "ergodic_exploration_amd", "host", "build", "frontier_regions_tests")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    m = {}
    for line in out.stdout.splitlines():
        w = line.split()
        m.setdefault(w[0], []).append(w[1:])
    W, H, res, ox, oy, flags, max_regions, min_size = m["map"][0]
    W, H, flags, max_regions, min_size = int(W), int(H), int(flags), int(max_regions), int(min_size)
    w_size, w_cost = (float(v) for v in m["weights"][0])
    g = sr.Geometry(float(ox), float(oy), float(res), W, H, 0.8)
    grid = _host_map(W, H)
    poses = np.array([[float(v) for v in p[1:4]] for p in m["robot"]])
    cost, owner, _ = part.partition(g, grid, poses=poses, flags=flags)
    root, region, rec, state = fr.regions(fr.OF_GRID, grid, 0.8, geo=cost, owner=owner, max_regions=max_regions)
    rows = lambda key: np.array([[int(v) for v in r[1:]] for r in sorted(m[key], key=lambda r: int(r[0]))], dtype=np.int32)
    _same(rows("root"), root, "root")
    _same(rows("region"), region, "region")
    assert [int(v) for v in m["state"][0]] == [int(state[0]), int(state[1]), int(state[2])] and state[0] > max_regions >= 3
    got = np.zeros(len(m["record"]), dtype=fr.RECORD)
    for r, row in enumerate(m["record"]):
        assert int(row[0]) == r
        got[r] = tuple(int(v) for v in row[1:])
    assert got.tobytes() == rec.tobytes()
    for i, j, a, b in m["at"]:
        assert int(a) == root[int(i), int(j)] and int(b) == region[int(i), int(j)]
    assert any(int(a) >= 0 for _, _, a, _ in m["at"]) and any(int(a) < 0 for _, _, a, _ in m["at"])
    cell, reg, score = fr.goals(rec, len(poses), min_size, w_size, w_cost)
    goal = np.array([[float(v) for v in r] for r in m["goal"]])
    assert np.array_equal(goal[:, 0], np.arange(len(poses))) and np.array_equal(goal[:, 1], cell) and np.array_equal(goal[:, 2], reg)
    assert np.array_equal(_bits(goal[:, 3]), _bits(score)) and (cell >= 0).sum() >= 2 and (cell < 0).any()
    _, want_len = part.paths(g, cost, owner, poses, cell, 64)
    assert [int(r[1]) for r in m["len"]] == want_len.tolist() and all((n >= 0) == (c >= 0) for n, c in zip(want_len, cell))

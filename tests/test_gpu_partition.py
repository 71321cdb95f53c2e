"""The geodesic partition, its goals and its paths on the device (include/ergodic_amd.h: eea_geodesic_partition,
eea_partition_goals, eea_partition_path_batch; csrc/partition_kernel.hip).

Checker: tests/partition_restatement.py (a heapq Dijkstra over (cost, label) keys, held to a second statement and to a model of
the device's round schedule by tests/test_partition.py); in every scene the cost plane is also compared with the device's own
eea_geodesic_field.  Planes, goal cells and areas are integers compared BITWISE as whole buffers; scores and way-points are
doubles compared by their bits.  Every output sits between guard elements and holds a sentinel before the call, every input
sits between guard elements and must come back unchanged.  Scenes are sized from the tile the header publishes; the guarded
buffers and the scenes are tests/test_gpu_geodesic.py's."""
import functools
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pyoracle as po
from ergodic_exploration_amd import capi
from tests import frontier_scenes as fs
from tests import gain_scenes as gs
from tests import geodesic_restatement as geo
from tests import partition_restatement as part
from tests import sense_restatement as sr
from tests import test_gpu_geodesic as tg

pytestmark = pytest.mark.gpu

ROOT = tg.ROOT
TX, TY = capi.GEODESIC_TILE_X, capi.GEODESIC_TILE_Y
G_IN, G_OUT, S_GEO, S_STATE, S_PATH = tg.G_IN, tg.G_OUT, tg.S_GEO, tg.S_STATE, tg.S_PATH
S_OWNER, S_SCORE = 0x7ACE0FF1, -3.5e77
WS_GUARD = 64                      # bytes around the workspace (which must stay 8-byte aligned)
_guarded, _geom, _centre, _bits = tg._guarded, tg._geom, tg._centre, tg._bits


class _Device(tg._Device):
    """tests/test_gpu_geodesic.py's device grid with the partition's workspace beside the field's"""

    def __init__(self, g, grid, with_sq=False):
        super().__init__(g, grid, with_sq)
        self.n_pws = capi.partition_ws_bytes(self.cfg)
        self._pws = torch.full((self.n_pws + 2 * WS_GUARD,), G_IN, dtype=torch.uint8, device="cuda")
        self.d_pws = self._pws[WS_GUARD:WS_GUARD + self.n_pws]
        assert self.d_pws.data_ptr() % 8 == 0

    def check(self, buf, guard=G_OUT):
        w = self._pws.cpu().numpy()
        assert (w[:WS_GUARD] == G_IN).all() and (w[-WS_GUARD:] == G_IN).all(), "a guard byte of the partition's workspace was written"
        return super().check(buf, guard)

    def partition(self, poses=None, cells=None, clear_sq=0, flags=0, max_rounds=0, start=None, use_sq=True, stream=None):
        """one call; (geo, owner int32 [ysize][xsize], state uint32 [4]) after the guards"""
        d_pose = None if poses is None else self.upload(poses, np.float64).view(-1, 3)
        d_cells = None if cells is None else self.upload(cells, np.int32)
        _, gbuf, d_geo = self.geo_buffer(None if start is None else start[0])
        _, obuf, d_owner = _guarded(np.full(self.grid.size, S_OWNER, np.int32) if start is None else start[1], G_OUT, np.int32)
        _, sbuf, d_state = _guarded(np.full(4, S_STATE, np.uint32).view(np.int32), G_OUT, np.int32)
        torch.cuda.synchronize()
        capi.geodesic_partition(self.cfg, self.d_grid, d_geo, d_owner, self.d_pws, d_state, pose=d_pose, cells=d_cells,
                                sq=self.d_sq if use_sq else None, clear_sq=clear_sq, flags=flags, max_rounds=max_rounds, stream=stream)
        torch.cuda.synchronize()
        shape = self.grid.shape
        return (self.check(gbuf).reshape(shape).copy(), self.check(obuf).reshape(shape).copy(),
                self.check(sbuf).view(np.uint32).copy())

    def goals(self, kind, fieldv, stride, cost, owner, n_labels, w_field, w_cost, known=None, stream=None):
        """one call; (goal_cell int32 [n], goal_score float64 [n], area uint32 [n]) after the guards"""
        d_field = self.upload(np.asarray(fieldv).view(np.int32) if kind == 0 else fieldv, np.int32 if kind == 0 else np.float64)
        d_geo, d_owner = self.upload(cost, np.int32), self.upload(owner, np.int32)
        d_known = self.d_grid if known is None else self.upload(known, np.int8)
        _, cbuf, d_cell = _guarded(np.full(n_labels, S_GEO, np.int32), G_OUT, np.int32)
        _, sbuf, d_score = _guarded(np.full(n_labels, S_SCORE), 2.5, np.float64)
        _, abuf, d_area = _guarded(np.full(n_labels, S_OWNER, np.int32), G_OUT, np.int32)
        torch.cuda.synchronize()
        capi.partition_goals(self.cfg, kind, d_field, stride, d_known, d_geo, d_owner, d_cell, d_score, d_area, w_field=w_field,
                             w_cost=w_cost, stream=stream)
        torch.cuda.synchronize()
        return self.check(cbuf).copy(), self.check(sbuf, 2.5).copy(), self.check(abuf).view(np.uint32).copy()

    def paths(self, cost, owner, poses, goal, n_steps, with_len=True):
        d_geo, d_owner = self.upload(cost, np.int32), self.upload(owner, np.int32)
        d_pose = self.upload(poses, np.float64).view(-1, 3)
        d_goal = self.upload(goal, np.int32)
        P = d_pose.shape[0]
        _, pbuf, d_path = _guarded(np.full(P * n_steps * 3, S_PATH), 2.5, np.float64)
        _, lbuf, d_len = _guarded(np.full(P, S_GEO, np.int32), G_OUT, np.int32)
        torch.cuda.synchronize()
        capi.partition_path_batch(self.cfg, d_geo, d_owner, d_pose, d_goal, d_path.view(P, n_steps, 3), d_len if with_len else None)
        torch.cuda.synchronize()
        self.d_path = d_path.view(P, n_steps, 3)
        return self.check(pbuf, 2.5).reshape(P, n_steps, 3).copy(), self.check(lbuf).copy()


def _same(got, want, what="geo"):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s differs at %s: got %s want %s" % (what, bad[:6].tolist(), [int(got[tuple(b)]) for b in bad[:6]],
                                                                [int(want[tuple(b)]) for b in bad[:6]])


_KEYS = ("poses", "cells", "clear_sq", "flags", "use_sq")


def _run(dev, **kw):
    """the waiting call against the restatement and against the device's own eea_geodesic_field: both planes, the state, and
    every element overwritten"""
    cost, owner, state = dev.partition(**kw)
    args = {k: v for k, v in kw.items() if k in _KEYS}
    use_sq = args.pop("use_sq", True)
    want_cost, want_owner, n_src = part.partition(dev.g, dev.grid, sq=dev.sq if use_sq else None, **args)
    _same(cost, want_cost)
    _same(owner, want_owner, "owner")
    assert state[0] == 1 and state[2] == n_src and state[3] == 0, state
    plain, plain_state = dev.field(**{k: v for k, v in kw.items() if k in _KEYS})
    assert np.array_equal(cost, plain) and plain_state[2] == state[2], "d_geo is not eea_geodesic_field's"
    return cost, owner, state


def _cells(g, cs):
    return np.array([i * g.xsize + j for i, j in cs], dtype=np.int32)


# ---- the labelled field ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xs,ys", [(1, 1), (2 * TX + 6, 1), (1, 2 * TY + 6)])
def test_degenerate_grids(xs, ys):
    """one cell, one row and one column of more than two tiles: a source at each end and a third label on the first one's cell"""
    g = _geom(xs, ys)
    dev = _Device(g, np.zeros((ys, xs), dtype=np.int8))
    cost, owner, _ = _run(dev, cells=np.array([0, xs * ys - 1, 0], dtype=np.int32))
    assert owner.reshape(-1)[0] == 0 and (owner != 2).all() and (xs * ys == 1 or owner.reshape(-1)[-1] == 1)
    _run(dev, poses=np.array([_centre(g, ys - 1, xs - 1)]), cells=np.array([0], dtype=np.int32))


@functools.lru_cache(maxsize=None)
def _open():
    xs, ys = 3 * TX + 5, 2 * TY + 3                    # 101 x 67: 4 x 3 tiles, ragged both ways
    grid = np.zeros((ys, xs), dtype=np.int8)
    grid.setflags(write=False)
    return _geom(xs, ys), grid


# mirrored about column TX (a tile's first column): the tie line runs ALONG a tile edge; mirrored about the diagonal: it runs
# ACROSS tile edges and through a tile corner
_MIRRORED = [(20, TX - 9), (20, TX + 9)]
_DIAGONAL = [(TY + 8, TX - 6), (TY - 6, TX + 8)]


@pytest.mark.parametrize("swap", [False, True])
def test_tie_lines_along_and_across_tile_edges(swap):
    g, grid = _open()
    dev = _Device(g, grid)
    a, b = (_MIRRORED[::-1], _DIAGONAL[::-1]) if swap else (_MIRRORED, _DIAGONAL)
    cost, owner, _ = _run(dev, cells=_cells(g, a))
    assert (owner[:, TX] == 0).all() and (owner[:, TX - 1] == (1 if swap else 0)).all() and (owner[:, TX + 1] == (0 if swap else 1)).all()
    cost, owner, _ = _run(dev, cells=_cells(g, b))
    k = np.arange(2, min(g.xsize, g.ysize))
    assert (owner[k, k] == 0).all() and {int(v) for v in owner[k, k - 2]} == {1 if swap else 0}
    cost, owner, _ = _run(dev, poses=np.array([_centre(g, *c) for c in a]), cells=_cells(g, b))
    assert set(np.unique(owner)) == {0, 1, 2, 3}


@functools.lru_cache(maxsize=None)
def _fleet_scene():
    """the clutter with 200 sources -- 120 poses and 80 cells, more than three wavefronts of seeds: some off the grid, some on
    walls, some on unknown cells (waived), one cell twice and one on a pose's cell"""
    g, grid = tg._clutter()
    rng = np.random.default_rng(23)
    poses = np.stack([g.xmin + rng.uniform(-0.02, 1.02, 120) * g.xsize * g.resolution,
                      g.ymin + rng.uniform(-0.02, 1.02, 120) * g.ysize * g.resolution, rng.uniform(-3, 3, 120)], 1)
    cells = rng.integers(-3, g.xsize * g.ysize + 3, size=80).astype(np.int32)
    free = _cells(g, tg._free_cells(grid, 3, seed=9))
    cells[10], cells[50] = free[0], free[0]                                # label 130 and label 170 in one cell
    i, j = sr.world2grid(g, poses[5][0], poses[5][1])
    cells[60] = i * g.xsize + j                                            # label 180 on pose 5's cell
    return g, grid, poses, cells


@pytest.mark.parametrize("flags", [0, capi.GEODESIC_UNKNOWN_BLOCKS])
def test_clutter_with_200_sources(flags):
    g, grid, poses, cells = _fleet_scene()
    dev = _Device(g, grid, with_sq=True)
    cost, owner, state = _run(dev, poses=poses, cells=cells, clear_sq=2, flags=flags)
    assert 120 < state[2] < 200 and (owner != 170).all() and (owner != 180).all() and (owner == 130).any()
    assert len(np.unique(owner)) > 100 and (owner == -1).any()
    _run(dev, poses=poses[:3], flags=flags, use_sq=False)


def test_a_sealed_room_on_a_tile_corner():
    """a room whose walls touch only at their corners is sealed: with a source inside, the room is that source's and nothing else
    is; with none it holds -1 / -1"""
    xs, ys = TX + 9, TY + 6
    g = _geom(xs, ys)
    grid = np.zeros((ys, xs), dtype=np.int8)
    a, b = TY - 4, TX - 5
    grid[a, b + 1:b + 7] = grid[a + 7, b + 1:b + 7] = 100
    grid[a + 1:a + 7, b] = grid[a + 1:a + 7, b + 7] = 100
    dev = _Device(g, grid)
    room = np.zeros_like(grid, dtype=bool)
    room[a + 1:a + 7, b + 1:b + 7] = True
    cost, owner, _ = _run(dev, cells=_cells(g, [(0, 0), (TY, TX), (ys - 1, xs - 1)]))
    assert (owner[room] == 1).all() and (owner[~room] != 1).all() and (owner[a, b] >= 0)
    cost, owner, _ = _run(dev, cells=_cells(g, [(0, 0), (ys - 1, xs - 1)]))
    assert (owner[room] == -1).all() and (cost[room] == -1).all()


def test_serpentine_with_a_source_at_each_end():
    g, grid = tg._serpentine()
    dev = _Device(g, grid)
    cost, owner, state = _run(dev, cells=np.array([0, g.xsize - 1], dtype=np.int32))
    assert (owner == 0).sum() > 1000 and (owner == 1).sum() > 1000 and state[1] > 4


def test_no_accepted_source():
    g, grid = gs.partly_revealed(23, 19)
    dev = _Device(g, grid)
    cost, owner, state = dev.partition(poses=np.array([[g.xmin - 1.0, g.ymin - 1.0, 0.0]]), cells=np.array([-1], dtype=np.int32))
    assert (cost == -1).all() and (owner == -1).all() and state.tolist() == [1, 0, 0, 0]


def test_a_budget_of_one_round_continue_and_a_generous_budget():
    """one round cannot finish the serpentine: d_state[0] = 0, every cell holds -1 / -1 or a cost >= the final one and >= its
    label's own field, nothing where the final field has nothing; EEA_GEODESIC_CONTINUE from those planes ends at the final bits;
    a generous budget on a second stream is the waiting call"""
    g, grid = tg._serpentine()
    dev = _Device(g, grid)
    ends = np.array([0, g.xsize - 1], dtype=np.int32)
    f_cost, f_owner, _ = part.partition(g, grid, cells=ends)
    p_cost, p_owner, state = dev.partition(cells=ends, max_rounds=1)
    assert state[0] == 0 and state[1] == 1 and state[2] == 2 and state[3] == 0, state
    assert np.array_equal(p_cost == -1, p_owner == -1) and ((p_cost == -1) | (p_cost >= f_cost)).all()
    assert (p_cost[f_cost == -1] == -1).all() and (p_cost == -1).sum() > (f_cost == -1).sum()
    for s in (0, 1):
        own, _ = geo.field(g, grid, cells=ends[s:s + 1])
        assert (own[p_owner == s] >= 0).all() and (p_cost[p_owner == s] >= own[p_owner == s]).all()
    cost, owner, state = dev.partition(cells=ends, flags=capi.GEODESIC_CONTINUE, start=(p_cost, p_owner))
    _same(cost, f_cost)
    _same(owner, f_owner, "owner")
    assert state[0] == 1 and state[2] == 2
    cost, owner, state = dev.partition(flags=capi.GEODESIC_CONTINUE, start=(f_cost, f_owner))       # no list: nothing changes
    assert np.array_equal(cost, f_cost) and np.array_equal(owner, f_owner) and state.tolist() == [1, 0, 0, 0]
    waited, _, s0 = dev.partition(cells=ends)
    budget = 4 * int(s0[1]) + 64
    st = torch.cuda.Stream()
    cost, owner, state = dev.partition(cells=ends, max_rounds=budget, stream=st.cuda_stream)
    _same(cost, f_cost)
    _same(owner, f_owner, "owner")
    assert np.array_equal(waited, f_cost) and state[0] == 1 and 0 < state[1] < budget and state[2] == 2 and state[3] == 0, state


# ---- goals -----------------------------------------------------------------------------------------------------------------
_WEIGHTS = ((1.0, 0.0), (0.0, 1.0), (1.0, 0.125), (0.0, 0.0))


def _field_of(kind, n, seed):
    """full of repeated values, zeros among them"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 4, size=n).astype(np.uint32) if kind == 0 else rng.choice(np.array([0.0, 0.5, 0.5, 2.5]), size=n)


def _check_goals(dev, kind, fieldv, stride, cost, owner, n_labels, known=None, weights=_WEIGHTS):
    out = []
    for wf, wc in weights:
        want = part.goals(dev.g, fieldv, stride, dev.grid if known is None else known, cost, owner, n_labels, wf, wc)
        got = dev.goals(kind, fieldv, stride, cost, owner, n_labels, wf, wc, known=known)
        assert np.array_equal(got[2], want[2]), "areas differ"
        assert np.array_equal(got[0], want[0]), (wf, wc, np.argwhere(got[0] != want[0])[:5].tolist())
        assert np.array_equal(_bits(got[1]), _bits(want[1])), (wf, wc)
        out.append(got)
    return out


@functools.lru_cache(maxsize=None)
def _partitions(scene):
    """the restated planes of a scene (held to the device's by the tests above): (g, grid, poses, cells, cost, owner)"""
    if scene == "open":
        g, grid = _open()
        poses, cells = np.array([_centre(g, *c) for c in _MIRRORED]), _cells(g, _DIAGONAL)
        cost, owner, _ = part.partition(g, grid, poses=poses, cells=cells)
    else:
        g, grid, poses, cells = _fleet_scene()
        cost, owner, _ = part.partition(g, grid, poses=poses, cells=cells, flags=capi.GEODESIC_UNKNOWN_BLOCKS)
    for a in (cost, owner):
        a.setflags(write=False)
    return g, grid, poses, cells, cost, owner


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("scene", ["open", "fleet"])
def test_goals_are_the_restatement(scene, kind, stride):
    """uploaded uint32 and double fields full of repeated values under the four weight pairs: areas, goal cells (ties to the
    lowest index) and the bits of the scores.  The fleet scene has labels without a candidate (sources that were refused) and
    labels that share a cell with a lower one (area 0)"""
    g, grid, poses, cells, cost, owner = _partitions(scene)
    dev = _Device(g, grid)
    n_labels = len(poses) + len(cells)
    fieldv = _field_of(kind, grid.size, 5 + kind)
    got = _check_goals(dev, kind, fieldv, stride, cost, owner, n_labels)
    cell, score, area = got[0]
    assert area.sum() == (owner >= 0).sum() and (cell >= 0).sum() > 1
    if scene == "fleet":
        assert area[170] == 0 and area[180] == 0 and cell[170] == -1 and score[180] == 0.0 and area[130] > 0
    # (0, 0): every candidate scores 0.0, so the goal is the label's first candidate; fewer labels than owners: the rest is ignored
    assert (got[3][1][got[3][0] >= 0] == 0.0).all()
    _check_goals(dev, kind, fieldv, stride, cost, owner, 2, weights=_WEIGHTS[2:3])


@pytest.mark.parametrize("kind", [0, 1])
def test_one_label_owns_the_whole_grid(kind):
    """every wavefront sees one label in every chunk: the carried label, across chunks and to the last ragged one"""
    g, grid = _open()
    dev = _Device(g, grid)
    cost, owner, _ = part.partition(g, grid, cells=_cells(g, [(40, 33)]))
    fieldv = _field_of(kind, grid.size, 9)
    got = _check_goals(dev, kind, fieldv, 1, cost, owner, 1)
    assert got[0][2][0] == grid.size and got[0][0][0] == int(np.argmax(fieldv))
    known = np.full(grid.shape, 100, dtype=np.int8)                         # every cell blocks: an area and no candidate
    known[g.ysize - 1, g.xsize - 1] = 0
    (cell, score, area), = _check_goals(dev, kind, np.ones_like(fieldv), 1, cost, owner, 1, known=known, weights=_WEIGHTS[2:3])
    assert cell[0] == grid.size - 1 and area[0] == grid.size


def test_a_different_label_in_every_lane():
    """a hand-made owner plane: 64 consecutive cells hold 64 different values, -2, -1 and labels >= n_labels among them; the cost
    plane is hand-made as well"""
    xs, ys = 2 * TX + 3, TY + 2
    g = _geom(xs, ys)
    dev = _Device(g, np.zeros((ys, xs), dtype=np.int8))
    idx = np.arange(xs * ys)
    owner = ((idx * 11) % 70 - 2).astype(np.int32)
    assert len(set(owner[:64])) == 64
    cost = ((idx * 37) % 101).astype(np.int32)
    for kind in (0, 1):
        _check_goals(dev, kind, _field_of(kind, xs * ys, 3), 1, cost, owner, 64, weights=_WEIGHTS[1:3])
    _check_goals(dev, 0, _field_of(0, xs * ys, 3), 1, cost, np.full(xs * ys, 64, dtype=np.int32), 64, weights=_WEIGHTS[:1])


# ---- more sources and labels than a workgroup has lanes, more tiles than a wavefront ----------------------------------------------
# tests/frontier_scenes.py's large_revealed(): 506 x 520 cells (16 x 17 tiles) revealed by 300 robots, unknown cells block, the
# clearance of the true walls.  300 sources are a second workgroup of partition_seed_kernel / geodesic_seed_kernel, 257 and 300
# labels a second workgroup of goals_init_kernel and goals_finish_kernel, and the rounds run over 272 tiles.  The planes of the
# restatement are computed once, with the scene
def _large():
    sc = fs.large_revealed()
    dev = _Device(sc.g, sc.known)
    dev.use_sq(sc.sq)
    return sc, dev, dict(poses=sc.poses, clear_sq=sc.clear_sq, flags=capi.GEODESIC_UNKNOWN_BLOCKS)


def test_300_sources_on_272_tiles():
    """both planes whole against the restatement, d_state[2] the 300 accepted sources (robots 298 and 299 stand in the cells of
    robots 0 and 1 and own nothing), and d_geo the bits of eea_geodesic_field on the same arguments"""
    sc, dev, args = _large()
    cost, owner, state = dev.partition(**args)
    _same(cost, sc.geo)
    _same(owner, sc.owner, "owner")
    assert state[0] == 1 and state[2] == sc.n_src == 300 and state[3] == 0, state
    assert (owner == 297).any() and (owner < 298).all() and len(np.unique(owner)) == 299
    plain, plain_state = dev.field(**args)
    assert np.array_equal(plain, cost) and plain_state[0] == 1 and plain_state[2] == 300 and plain_state[3] == 0, plain_state
    print("large revealed map: %d rounds of the partition changed something, %d of the field" % (state[1], plain_state[1]))


def test_one_round_at_a_time_on_272_tiles():
    """a budget of one round, then EEA_GEODESIC_CONTINUE calls of one round each from the planes of the call before: unfinished
    until d_state[0] = 1, then the planes of the waiting call"""
    sc, dev, args = _large()
    _, _, waited = dev.partition(**args)
    limit = 4 * int(waited[1]) + 64
    cost, owner, state = dev.partition(max_rounds=1, **args)
    assert state[0] == 0 and state[1] == 1 and state[2] == 300 and state[3] == 0, state
    assert np.array_equal(cost == -1, owner == -1) and ((cost == -1) | (cost >= sc.geo)).all() and (cost[sc.geo == -1] == -1).all()
    calls = 1
    while state[0] == 0:
        assert calls < limit, "no end after %d calls of one round" % calls
        cost, owner, state = dev.partition(max_rounds=1, start=(cost, owner), **dict(args, flags=args["flags"] | capi.GEODESIC_CONTINUE))
        calls += 1
        assert state[1] <= 1 and state[2] == 300 and state[3] == 0, state
    _same(cost, sc.geo)
    _same(owner, sc.owner, "owner")
    assert calls > 2
    print("large revealed map: final after %d calls of one round (the waiting call: %d rounds changed something)" % (calls, waited[1]))


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n_labels", [256, 257, 300])
def test_goals_of_more_labels_than_a_workgroup(n_labels, kind, stride):
    """256 labels are one workgroup of the init and finish launches, 257 one lane of a second, 300 the fleet: areas, goal cells
    and the bits of the scores against the restatement; owners >= n_labels are ignored; labels 298 and 299 own no cell and get
    -1 / 0.0 / area 0"""
    sc = fs.large_revealed()
    dev = _Device(sc.g, sc.known)
    fieldv = _field_of(kind, sc.known.size, 5 + kind)
    (cell, score, area), _ = _check_goals(dev, kind, fieldv, stride, sc.geo, sc.owner, n_labels, weights=_WEIGHTS[1:3])
    assert area.sum() == ((sc.owner >= 0) & (sc.owner < n_labels)).sum() and (cell[200:] >= 0).sum() > 20
    if n_labels == 300:
        assert area[298:].tolist() == [0, 0] and cell[298:].tolist() == [-1, -1] and score[298:].tolist() == [0.0, 0.0]
        assert (area[:298] > 0).all()


# ---- paths -----------------------------------------------------------------------------------------------------------------
def _farthest_goals(cost, owner, P, xs):
    goal = np.full(P, -1, dtype=np.int32)
    for q in range(P):
        mine = np.argwhere(owner == q)
        if len(mine):
            i, j = mine[np.argmax(cost[tuple(mine.T)])]
            goal[q] = i * xs + j
    return goal


@pytest.mark.parametrize("scene", ["open", "fleet"])
def test_paths_are_the_restatement(scene):
    """every robot to the farthest cell of its own region (across tie cells, where the cost-only descent could leave the region):
    way-points by their bits and lengths against the restatement; n_steps shorter than the longest path, equal to it and longer
    (padding); m = 0 (the goal is the robot's own cell); goal -1; a goal that another label owns; a goal off the grid; d_len
    NULL; every consecutive pair of way-points is a legal move inside the robot's region"""
    g, grid, poses, cells, cost, owner = _partitions(scene)
    dev = _Device(g, grid)
    P = len(poses)
    goal = _farthest_goals(cost, owner, P, g.xsize)
    walkers = [q for q in range(P) if goal[q] >= 0]
    assert len(walkers) >= 2
    q0, q1 = walkers[0], walkers[1]
    i, j = sr.world2grid(g, poses[q1][0], poses[q1][1])
    goal = np.concatenate([goal, [goal[q0], i * g.xsize + j, -1, goal[q1], g.xsize * g.ysize]]).astype(np.int32)
    # five more robots, none of which gets a way: twins of q0 and q1 whose labels P .. do not own the goals they are given (q0's
    # goal, q1's own cell, q1's goal), one without a goal and one whose goal is off the grid
    poses = np.concatenate([poses, poses[[q0, q1, q0, q0, q1]]])
    own = goal.copy()
    own[q1] = i * g.xsize + j                                              # m = 0
    trav = geo.traversable(g, grid, None, 0, 0 if scene == "open" else capi.GEODESIC_UNKNOWN_BLOCKS)
    longest = max(len(part.descend(cost, owner, goal[q] // g.xsize, goal[q] % g.xsize)) for q in walkers)
    assert longest >= 3
    for n_steps, gl in ((longest - 2, goal), (longest, own), (longest + 5, goal)):
        want, want_len = part.paths(g, cost, owner, poses, gl, n_steps)
        got, got_len = dev.paths(cost, owner, poses, gl, n_steps)
        assert np.array_equal(got_len, want_len), (got_len, want_len)
        assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:5]
        assert (want_len[P:] == -1).all() and want_len.max() <= n_steps and (want_len[walkers] >= 0).all()
        assert want_len[q1] == 0 if gl is own else want_len.max() == min(longest, n_steps)
        for q in walkers:
            a = sr.world2grid(g, poses[q][0], poses[q][1])
            way = [a] + [sr.world2grid(g, x, y) for x, y, _ in got[q, :got_len[q]]]
            assert all(geo.legal_move(trav, cost, c, d) for c, d in zip(way, way[1:])) and all(owner[c] == q for c in way)
            if got_len[q] < n_steps:
                assert way[-1] == (gl[q] // g.xsize, gl[q] % g.xsize)
    got, untouched = dev.paths(cost, owner, poses, goal, longest, with_len=False)
    assert np.array_equal(_bits(got), _bits(part.paths(g, cost, owner, poses, goal, longest)[0])) and (untouched == S_GEO).all()


def test_goals_feed_paths_on_the_device():
    """the loop the partition closes, device buffers end to end: partition -> goals -> paths"""
    g, grid, poses, cells, _, _ = _partitions("fleet")
    dev = _Device(g, grid)
    cost, owner, _ = dev.partition(poses=poses, cells=cells, flags=capi.GEODESIC_UNKNOWN_BLOCKS)
    fieldv = _field_of(0, grid.size, 4)
    n = len(poses) + len(cells)
    cell, score, area = dev.goals(0, fieldv, 1, cost, owner, n, 1.0, 0.125)
    want, want_len = part.paths(g, cost, owner, poses, cell, 24)
    got, got_len = dev.paths(cost, owner, poses, cell[:len(poses)], 24)
    assert np.array_equal(got_len, want_len) and np.array_equal(_bits(got), _bits(want)) and (got_len > 0).sum() > 20
    assert np.array_equal(got_len >= 0, cell[:len(poses)] >= 0)


def test_a_path_batch_is_a_reference_trajectory_of_the_dynamic_window():
    """the serpentine's paths as d_xt_ref of eea_dwa_control_batch in trajectory mode, as tests/test_gpu_geodesic.py does for the
    descent: u_opt / found are the bits of the oracle's DynamicWindow given the same reference"""
    g, grid = tg._serpentine()
    dev = _Device(g, grid)
    coll = (0.05, 0.3, 0.02, gs.THR)
    dwa = (0.1, 1.0, 0.2, 1.0, 1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 2.0, -2.0, 3, 8, 5)
    n_ref, dt_ref = 16, 0.1
    robots = [(3, 1), (TY - 2, 5), (TY, 9), (1, 13), (TY // 2, 2 * TX + 1), (5, 4 * TX + 1)]
    assert all(grid[c] == 0 for c in robots)
    x0 = np.array([_centre(g, i, j, th=0.4 * k - 1.0, fx=0.37, fy=0.61) for k, (i, j) in enumerate(robots)])
    vb = np.array([[0.2 * (k % 3) - 0.2, 0.1 * (k % 2), 0.3 * k - 0.6] for k in range(len(robots))])
    cost, owner, _ = dev.partition(poses=x0)
    goal = _farthest_goals(cost, owner, len(robots), g.xsize)
    want_path, want_len = part.paths(g, cost, owner, x0, goal, n_ref)
    got_path, got_len = dev.paths(cost, owner, x0, goal, n_ref)
    assert np.array_equal(_bits(got_path), _bits(want_path)) and np.array_equal(got_len, want_len) and (got_len > 0).all()
    P = len(robots)
    d_u = torch.full((P, 3), 7.0, dtype=torch.float64, device="cuda")
    d_f = torch.full((P,), -1, dtype=torch.int32, device="cuda")
    capi.dwa_control_batch(dev.cfg, capi.DwaCfg(*dwa), dev.d_grid, torch.as_tensor(x0).cuda(), torch.as_tensor(vb).cuda(), d_u, d_f,
                           xt_ref=dev.d_path, dt_ref=dt_ref)
    torch.cuda.synchronize()
    u, f = d_u.cpu().numpy(), d_f.cpu().numpy()
    gm = po.GridMap(g.xmin, g.xmin + g.xsize * g.resolution, g.ymin, g.ymin + g.ysize * g.resolution, g.resolution, grid.reshape(-1))
    found = 0
    for q in range(P):
        ok, uo, _ = po.dwa_control(dwa, coll, gm, x0[q], vb[q], xt_ref=want_path[q].T, dt_ref=dt_ref)
        assert bool(f[q]) == ok and np.array_equal(_bits(u[q]), _bits(uo)), (q, u[q], uo)
        found += ok
    assert found > 0


# ---- the host mirror -------------------------------------------------------------------------------------------------------
def _host_map(W, H):
    """the map of host/test/geodesic_partition_tests.cpp"""
    d = np.zeros((H, W), dtype=np.int8)
    d[:30, 20] = 100
    d[12, 20] = 0
    d[25, 34:44] = d[34, 34:44] = 100
    d[25:35, 34] = d[25:35, 43] = 100
    d[3:9, 30:36] = -1
    return d


def test_host_mirror_geodesic_partition():
    """host/build/geodesic_partition_tests (GeodesicPartition in geodesic_partition.hpp: update, owners, costs, area, goals,
    paths) runs, and its printed answers are the restatement's"""
    exe = os.path.join(ROOT, "ergodic_exploration_amd", "host", "build", "geodesic_partition_tests")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    m = {}
    for line in out.stdout.splitlines():
        w = line.split()
        m.setdefault(w[0], []).append(w[1:])
    W, H, res, ox, oy, flags, n_src, stride, n_steps = m["map"][0]
    W, H, flags, n_src, stride, n_steps = int(W), int(H), int(flags), int(n_src), int(stride), int(n_steps)
    w_field, w_cost = (float(v) for v in m["weights"][0])
    g = sr.Geometry(float(ox), float(oy), float(res), W, H, 0.8)
    grid = _host_map(W, H)
    poses = np.array([[float(v) for v in p[1:4]] for p in m["robot"]])
    want_cost, want_owner, want_src = part.partition(g, grid, poses=poses, flags=flags)
    rows = lambda key: np.array([[int(v) for v in r[1:]] for r in sorted(m[key], key=lambda r: int(r[0]))], dtype=np.int32)
    _same(rows("geo"), want_cost)
    _same(rows("owner"), want_owner, "owner")
    assert n_src == want_src and len(np.unique(want_owner)) >= 4
    fieldv = ((np.arange(W * H) * 7 + 3) % 5).astype(np.uint32)
    cell, score, area = part.goals(g, fieldv, stride, grid, want_cost, want_owner, len(poses), w_field, w_cost)
    got = np.array([[float(v) for v in r] for r in m["goal"]])
    assert np.array_equal(got[:, 0], np.arange(len(poses))) and np.array_equal(got[:, 1], area) and np.array_equal(got[:, 2], cell)
    assert np.array_equal(_bits(got[:, 3]), _bits(score))
    want_path, want_len = part.paths(g, want_cost, want_owner, poses, cell, n_steps)
    way = np.array([[float(v) for v in r[2:]] for r in m["way"]]).reshape(len(poses), n_steps, 3)
    assert np.array_equal(_bits(way), _bits(want_path))
    assert [int(r[1]) for r in m["len"]] == want_len.tolist() and -1 in want_len.tolist() and max(want_len) > 3

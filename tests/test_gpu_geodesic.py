"""The geodesic field, its paths and the reachable target on the device (include/ergodic_amd.h: eea_geodesic_field,
eea_geodesic_path_batch, eea_set_target_reachable; csrc/geodesic_kernel.hip).

Checker: tests/geodesic_restatement.py (a heapq Dijkstra under the header's definitions, held to a second statement and to a
model of the device's round schedule by tests/test_geodesic.py).  The field is integers and is compared BITWISE as a whole
buffer; way-points are doubles compared by their bits.  Every output sits between guard elements and holds a sentinel before
the call, every input sits between guard elements and must come back unchanged.  Scenes are sized from the tile the header
publishes."""
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
from tests import sense_restatement as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TX, TY = capi.GEODESIC_TILE_X, capi.GEODESIC_TILE_Y
GUARD = 37
WS_GUARD = 64                      # bytes around the workspace (which must stay 4-byte aligned)
G_IN, G_OUT, S_GEO, S_STATE = 0x3C, 0x5A5A5A5A, 0x7BCDEF01, 0x6A6A6A6A
S_PATH = -7.25e33


def _cfg(g):
    return capi.make_collision_cfg(g.xmin, g.ymin, g.resolution, g.xsize, g.ysize, 0.05, 0.3, 0.02, g.occupied_threshold)


def _guarded(values, guard_value, dtype):
    flat = np.asarray(values, dtype=dtype).reshape(-1)
    img = np.concatenate([np.full(GUARD, guard_value, dtype), flat, np.full(GUARD, guard_value, dtype)])
    buf = torch.as_tensor(img).cuda()
    return img, buf, buf[GUARD:GUARD + flat.size]


class _Device:
    """one grid on the device between guard bytes, its distance plane, a workspace, and guarded outputs per call"""

    def __init__(self, g, grid, with_sq=False):
        self.g, self.cfg, self.grid = g, _cfg(g), np.ascontiguousarray(grid, dtype=np.int8).reshape(g.ysize, g.xsize)
        self.inputs = [_guarded(self.grid, G_IN, np.int8)]
        self.d_grid = self.inputs[0][2]
        self.n_ws = capi.geodesic_ws_bytes(self.cfg)
        self._ws = torch.full((self.n_ws + 2 * WS_GUARD,), G_IN, dtype=torch.uint8, device="cuda")
        self.d_ws = self._ws[WS_GUARD:WS_GUARD + self.n_ws]
        self.sq = self.d_sq = None
        if with_sq:
            d_sq = torch.empty(self.grid.size, dtype=torch.int32, device="cuda")
            capi.distance_field(self.cfg, self.d_grid, d_sq)
            torch.cuda.synchronize()
            self.use_sq(d_sq.cpu().numpy().reshape(self.grid.shape))

    def use_sq(self, sq):
        self.sq = np.ascontiguousarray(sq, dtype=np.int32)
        self.inputs.append(_guarded(self.sq, G_OUT, np.int32))
        self.d_sq = self.inputs[-1][2]

    def upload(self, values, dtype):
        self.inputs.append(_guarded(values, 0x11 if dtype == np.int32 else 1.5, dtype))
        return self.inputs[-1][2]

    def geo_buffer(self, start=None):
        return _guarded(np.full(self.grid.size, S_GEO, np.int32) if start is None else start, G_OUT, np.int32)

    def check(self, buf, guard=G_OUT):
        got = buf.cpu().numpy()
        assert (got[:GUARD] == guard).all() and (got[-GUARD:] == guard).all(), "a guard element was written"
        for img, ibuf, _ in self.inputs:
            assert np.array_equal(ibuf.cpu().numpy(), img), "an input was written"
        w = self._ws.cpu().numpy()
        assert (w[:WS_GUARD] == G_IN).all() and (w[-WS_GUARD:] == G_IN).all(), "a guard byte of the workspace was written"
        return got[GUARD:-GUARD]

    def field(self, poses=None, cells=None, clear_sq=0, flags=0, max_rounds=0, start=None, use_sq=True, stream=None):
        """one call; (geo int32 [ysize][xsize], state uint32 [4]) after the guards"""
        d_pose = None if poses is None else self.upload(poses, np.float64).view(-1, 3)
        d_cells = None if cells is None else self.upload(cells, np.int32)
        _, gbuf, d_geo = self.geo_buffer(start)
        _, sbuf, d_state = _guarded(np.full(4, S_STATE, np.uint32).view(np.int32), G_OUT, np.int32)
        torch.cuda.synchronize()
        capi.geodesic_field(self.cfg, self.d_grid, d_geo, self.d_ws, d_state, pose=d_pose, cells=d_cells,
                            sq=self.d_sq if use_sq else None, clear_sq=clear_sq, flags=flags, max_rounds=max_rounds, stream=stream)
        torch.cuda.synchronize()
        self.d_geo = d_geo
        return self.check(gbuf).reshape(self.grid.shape).copy(), self.check(sbuf).view(np.uint32).copy()

    def restated(self, poses=None, cells=None, clear_sq=0, flags=0, use_sq=True):
        return geo.field(self.g, self.grid, poses, cells, self.sq if use_sq else None, clear_sq, flags)

    def path(self, geo_field, poses, n_steps, with_len=True):
        d_geo = self.upload(geo_field, np.int32)
        d_pose = self.upload(poses, np.float64).view(-1, 3)
        P = d_pose.shape[0]
        _, pbuf, d_path = _guarded(np.full(P * n_steps * 3, S_PATH), 2.5, np.float64)
        _, lbuf, d_len = _guarded(np.full(P, S_GEO, np.int32), G_OUT, np.int32)
        torch.cuda.synchronize()
        capi.geodesic_path_batch(self.cfg, d_geo, d_pose, d_path.view(P, n_steps, 3), d_len if with_len else None)
        torch.cuda.synchronize()
        self.d_path = d_path.view(P, n_steps, 3)
        return self.check(pbuf, 2.5).reshape(P, n_steps, 3).copy(), self.check(lbuf).copy()


def _same(got, want):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "geo differs at %s: got %s want %s" % (bad[:6].tolist(), [int(got[tuple(b)]) for b in bad[:6]],
                                                                  [int(want[tuple(b)]) for b in bad[:6]])


def _run(dev, **kw):
    """the waiting call against the restatement: field, state, and every element overwritten"""
    got, state = dev.field(**kw)
    want, n_src = dev.restated(**{k: v for k, v in kw.items() if k in ("poses", "cells", "clear_sq", "flags", "use_sq")})
    _same(got, want)
    assert state[0] == 1 and state[2] == n_src and state[3] == 0, state
    return got, state


def _centre(g, i, j, th=0.3, fx=0.5, fy=0.5):
    return [g.xmin + (j + fx) * g.resolution, g.ymin + (i + fy) * g.resolution, th]


def _geom(xs, ys):
    return sr.Geometry(gs.XMIN, gs.YMIN, gs.RES, xs, ys, gs.THR)


@functools.lru_cache(maxsize=None)
def _clutter():
    """3 TY + 5 by 3 TX + 7: blocks of 3 x 5 cells, 25 % unknown, 60 % free, walls, and the 79 / 80 pair sprinkled in"""
    xs, ys = 3 * TX + 7, 3 * TY + 5
    rng = np.random.default_rng(11)
    blocks = rng.choice(np.array([-1, 0, 100], dtype=np.int8), size=(ys // 3 + 1, xs // 5 + 1), p=[0.25, 0.6, 0.15])
    grid = np.ascontiguousarray(np.kron(blocks, np.ones((3, 5), dtype=np.int8))[:ys, :xs])
    grid[rng.integers(0, ys, 12), rng.integers(0, xs, 12)] = 79
    grid[rng.integers(0, ys, 12), rng.integers(0, xs, 12)] = 80
    grid.setflags(write=False)
    return _geom(xs, ys), grid


@functools.lru_cache(maxsize=None)
def _serpentine():
    """one tile high plus one row, five tiles wide plus three cells: the shortest path runs the height between every two walls,
    across the tile edge at row TY, back and forth"""
    xs, ys = 5 * TX + 3, TY + 1
    grid = geo.serpentine(xs, ys)
    grid.setflags(write=False)
    return _geom(xs, ys), grid


def _scene(name):
    if name == "clutter":
        return _clutter()
    if name == "serpentine":
        return _serpentine()
    xs, ys = name
    return gs.partly_revealed(xs, ys)


def _free_cells(grid, n, seed=3):
    """n distinct cells with value 0, spread over the grid"""
    free = np.argwhere(np.asarray(grid) == 0)
    pick = np.random.default_rng(seed).choice(len(free), size=n, replace=False)
    return [tuple(int(v) for v in free[k]) for k in sorted(pick)]


# ---- the field ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, capi.GEODESIC_UNKNOWN_BLOCKS])
@pytest.mark.parametrize("cell", [0, -1])
@pytest.mark.parametrize("xs,ys", [(1, 1), (TX + 1, 1), (1, TY + 1), (TX + 1, TY + 1)])
def test_degenerate_grids(xs, ys, cell, flags):
    """one cell, one row and one column a cell longer than a tile, a grid a cell larger than a tile both ways; all free and all
    unknown, with and without EEA_GEODESIC_UNKNOWN_BLOCKS (then only the waived source has a value)"""
    g = _geom(xs, ys)
    dev = _Device(g, np.full((ys, xs), cell, dtype=np.int8))
    got, _ = _run(dev, cells=np.array([xs * ys - 1], dtype=np.int32), flags=flags)
    assert got[-1, -1] == 0 and ((got >= 0).sum() == 1) == (xs * ys == 1 or (cell < 0 and flags != 0))
    _run(dev, poses=np.array([_centre(g, 0, 0)]), flags=flags)


@pytest.mark.parametrize("flags", [0, capi.GEODESIC_UNKNOWN_BLOCKS])
@pytest.mark.parametrize("scene", [(23, 19), (64, 41), "clutter"])
def test_field_is_the_restatement(scene, flags):
    """the partly revealed scenes of tests/gain_scenes.py and a clutter of more than three tiles each way, ragged: from one
    source, from several (ties between sources), from d_cells only, from both lists; with a source off the grid, on a blocking
    cell (skipped: d_state[2] says so) and on a cell that fails the clearance (seeded, the tests waived)"""
    g, grid = _scene(scene)
    dev = _Device(g, grid, with_sq=True)
    src = _free_cells(grid, 4)
    idx = lambda cs: np.array([i * g.xsize + j for i, j in cs], dtype=np.int32)
    one = np.array([_centre(g, *src[0], fx=0.9, fy=0.1)])
    several = np.array([_centre(g, *c) for c in src])
    got, state = _run(dev, poses=one, flags=flags, use_sq=False)
    assert state[2] == 1 and (got > 0).any() and (got == -1).any()
    _run(dev, poses=several, flags=flags, use_sq=False)
    _run(dev, cells=idx(src[1:3]), flags=flags, use_sq=False)
    _run(dev, poses=several[:2], cells=idx(src[2:]), flags=flags, use_sq=False)
    # off the grid, a negative and a too large index, a blocking cell, and a free cell beside a wall (fails clear_sq = 2)
    wall = tuple(int(v) for v in np.argwhere(np.asarray(grid) >= 80)[0])
    near = [c for c in map(tuple, np.argwhere((dev.sq > 0) & (dev.sq <= 2) & (np.asarray(grid) == 0)))][0]
    odd_poses = np.array([[g.xmin - 0.3, g.ymin + 0.1, 0.0], _centre(g, *wall), _centre(g, int(near[0]), int(near[1]))])
    odd_cells = np.array([-3, g.xsize * g.ysize, wall[0] * g.xsize + wall[1], src[3][0] * g.xsize + src[3][1]], dtype=np.int32)
    got, state = _run(dev, poses=odd_poses, cells=odd_cells, clear_sq=2, flags=flags)
    assert state[2] == 2 and got[near[0], near[1]] == 0 and got[wall] == -1
    assert not geo.traversable(g, grid, dev.sq, 2, flags)[near[0], near[1]]


def test_a_sealed_room_and_a_diagonal_gap():
    """a room whose walls touch only at their corners is sealed (the corner rule: no move between two wall cells); with one
    wall cell of a second room removed there is a way in"""
    xs, ys = TX + 9, TY + 6
    g = _geom(xs, ys)
    grid = np.zeros((ys, xs), dtype=np.int8)
    a, b = TY - 4, TX - 5                         # the room straddles the tile corner
    grid[a, b + 1:b + 7] = grid[a + 7, b + 1:b + 7] = 100
    grid[a + 1:a + 7, b] = grid[a + 1:a + 7, b + 7] = 100      # corners (a, b) .. stay free: diagonal gaps only
    dev = _Device(g, grid)
    got, _ = _run(dev, cells=np.array([0], dtype=np.int32))
    assert (got[a + 1:a + 7, b + 1:b + 7] == -1).all() and got[a, b] > 0 and got[ys - 1, xs - 1] > 0
    grid[a + 3, b] = 0
    got, _ = _run(_Device(g, grid), cells=np.array([0], dtype=np.int32))
    assert (got[a + 1:a + 7, b + 1:b + 7] > 0).all()


def test_inflation_by_the_distance_field():
    """d_sq from eea_distance_field on the same grid: with clear_sq = 1 a corridor of two cells closes and one of five stays
    open; with d_sq all -1 (no occupied cell) the clearance refuses nothing"""
    xs, ys = TX + 12, TY + 3
    g = _geom(xs, ys)
    grid = np.zeros((ys, xs), dtype=np.int8)
    grid[TY - 1, :] = 100
    grid[TY - 1, 4:6] = 0
    grid[TY - 1, TX + 3:TX + 8] = 0
    dev = _Device(g, grid, with_sq=True)
    src = np.array([2 * xs + 2], dtype=np.int32)
    got, _ = _run(dev, cells=src, clear_sq=1)
    assert got[TY - 1, 4] == -1 and got[TY - 1, 5] == -1 and got[TY - 1, TX + 5] > 0 and got[ys - 1, 4] > 0
    closed = grid.copy()
    closed[TY - 1, TX + 3:TX + 8] = 100
    dev2 = _Device(g, closed, with_sq=True)
    got, _ = _run(dev2, cells=src, clear_sq=1)
    assert (got[TY:, :] == -1).all()
    got, _ = _run(dev2, cells=src, clear_sq=0)
    assert got[ys - 1, 4] > 0                         # without inflation the two-cell corridor is a way through
    empty = _Device(g, np.zeros((ys, xs), dtype=np.int8), with_sq=True)
    assert (empty.sq == -1).all()
    got, _ = _run(empty, cells=src, clear_sq=1 << 20)
    assert (got >= 0).all()


def test_serpentine_carries_values_both_ways_across_an_edge():
    g, grid = _serpentine()
    dev = _Device(g, grid)
    got, state = _run(dev, cells=np.array([0], dtype=np.int32))
    lanes = (g.xsize - 2) // 4
    assert got[0, g.xsize - 1] >= 5 * (TY - 1) * lanes and state[1] >= lanes // 2, (got[0, g.xsize - 1], state)
    print("serpentine %d x %d: %d rounds changed something" % (g.xsize, g.ysize, state[1]))


def test_no_accepted_source():
    g, grid = _scene((23, 19))
    wall = np.argwhere(np.asarray(grid) >= 80)[0]
    dev = _Device(g, grid)
    got, state = dev.field(poses=np.array([[g.xmin - 1.0, g.ymin - 1.0, 0.0]]),
                           cells=np.array([-1, int(wall[0]) * g.xsize + int(wall[1])], dtype=np.int32))
    assert (got == -1).all() and state.tolist() == [1, 0, 0, 0]


# ---- budgets ------------------------------------------------------------------------------------------------------------
def test_a_budget_of_one_round_and_continue():
    """one round cannot finish the serpentine (its path crosses a tile edge in every lane): d_state[0] = 0, every element is -1
    or >= the final value, and nothing unreachable has a value; EEA_GEODESIC_CONTINUE ends at the final bits, and after adding
    a source at the bits of a fresh call with both"""
    g, grid = _serpentine()
    dev = _Device(g, grid)
    a = np.array([0], dtype=np.int32)
    both = np.array([0, (g.ysize - 1) * g.xsize + g.xsize - 1], dtype=np.int32)
    final, _ = dev.restated(cells=a)
    part, state = dev.field(cells=a, max_rounds=1)
    assert state[0] == 0 and state[1] == 1 and state[2] == 1 and state[3] == 0, state
    assert ((part == -1) | (part >= final)).all() and (part[final == -1] == -1).all() and (part == -1).sum() > (final == -1).sum()
    got, state = dev.field(cells=a, flags=capi.GEODESIC_CONTINUE, start=part)
    _same(got, final)
    assert state[0] == 1 and state[2] == 1
    got, state = dev.field(cells=both, flags=capi.GEODESIC_CONTINUE, start=part)
    _same(got, dev.restated(cells=both)[0])
    assert state[0] == 1 and state[2] == 2
    # continuing a final field with no source list at all changes nothing
    got, state = dev.field(flags=capi.GEODESIC_CONTINUE, start=final)
    _same(got, final)
    assert state.tolist() == [1, 0, 0, 0]


def test_a_generous_budget_is_the_waiting_call():
    g, grid = _serpentine()
    dev = _Device(g, grid)
    a = np.array([0], dtype=np.int32)
    waited, s0 = dev.field(cells=a)
    budget = 4 * int(s0[1]) + 64
    st = torch.cuda.Stream()
    got, state = dev.field(cells=a, max_rounds=budget, stream=st.cuda_stream)
    _same(got, waited)
    assert state[0] == 1 and 0 < state[1] < budget and state[2] == 1 and state[3] == 0, state


# ---- more sources than a workgroup has lanes, more tiles than a wavefront -------------------------------------------------
def test_300_sources_on_272_tiles_and_one_round_at_a_time():
    """tests/frontier_scenes.py's large_revealed(): 506 x 520 cells (16 x 17 tiles) revealed by 300 robots -- a second workgroup
    of geodesic_seed_kernel --, unknown cells block, the clearance of the true walls.  The field is the cost plane of the
    partition's restatement (computed once, with the scene); a budget of one round and EEA_GEODESIC_CONTINUE calls of one round
    each end at the same bits"""
    sc = fs.large_revealed()
    dev = _Device(sc.g, sc.known)
    dev.use_sq(sc.sq)
    args = dict(poses=sc.poses, clear_sq=sc.clear_sq)
    flags = capi.GEODESIC_UNKNOWN_BLOCKS
    got, waited = dev.field(flags=flags, **args)
    _same(got, sc.geo)
    assert waited[0] == 1 and waited[2] == sc.n_src == 300 and waited[3] == 0, waited
    limit = 4 * int(waited[1]) + 64
    got, state = dev.field(flags=flags, max_rounds=1, **args)
    assert state[0] == 0 and state[1] == 1 and state[2] == 300 and state[3] == 0, state
    assert ((got == -1) | (got >= sc.geo)).all() and (got[sc.geo == -1] == -1).all()
    calls = 1
    while state[0] == 0:
        assert calls < limit, "no end after %d calls of one round" % calls
        got, state = dev.field(flags=flags | capi.GEODESIC_CONTINUE, max_rounds=1, start=got, **args)
        calls += 1
        assert state[1] <= 1 and state[2] == 300 and state[3] == 0, state
    _same(got, sc.geo)
    assert calls > 2
    print("large revealed map: final after %d calls of one round (the waiting call: %d rounds changed something)" % (calls, waited[1]))


# ---- paths ---------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("scene", [(64, 41), "clutter", "sealed", "serpentine"])
def test_paths_are_the_restatement(scene):
    """way-points by their bits and lengths against the restatement: reachable poses, unreachable ones, one off the grid, one on
    a source cell; n_steps shorter than the longest path, equal to it and longer (padding); d_len NULL is accepted; every
    consecutive pair of way-points is a legal move on the traversability the restatement computed"""
    if scene == "sealed":
        xs, ys = TX + 9, TY + 6
        g, grid = _geom(xs, ys), np.zeros((ys, xs), dtype=np.int8)
        grid[TY - 4, TX - 5:TX + 3] = grid[TY + 3, TX - 5:TX + 3] = 100
        grid[TY - 4:TY + 4, TX - 5] = grid[TY - 4:TY + 4, TX + 2] = 100
    else:
        g, grid = _scene(scene)
    dev = _Device(g, grid)
    src = _free_cells(grid, 2, seed=5)
    cells = np.array([src[0][0] * g.xsize + src[0][1]], dtype=np.int32)
    flags = capi.GEODESIC_UNKNOWN_BLOCKS
    field, _ = dev.restated(cells=cells, flags=flags)
    trav = geo.traversable(g, grid, None, 0, flags)
    reach, unreach = np.argwhere(field > 0), np.argwhere(field < 0)
    far = reach[np.argsort(field[tuple(reach.T)])[[-1, len(reach) // 2, 0]]]
    poses = [_centre(g, int(i), int(j), th=0.1 * k - 1.0, fx=0.2, fy=0.7) for k, (i, j) in enumerate(far)]
    poses += [_centre(g, int(i), int(j), th=2.0) for i, j in unreach[[0, -1]]]
    poses += [[g.xmin - 0.4, g.ymin + 0.2, -0.5], _centre(g, *src[0], th=1.25, fx=0.1, fy=0.1)]
    poses = np.array(poses)
    longest = len(geo.path_cells(field, int(far[0][0]), int(far[0][1]), g.xsize * g.ysize))
    assert longest >= 3
    for n_steps in (longest - 2, longest, longest + 5):
        want, want_len = geo.path(g, field, poses, n_steps)
        got, got_len = dev.path(field, poses, n_steps)
        assert np.array_equal(got_len, want_len), (got_len, want_len)
        assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:5]
        assert want_len[0] == min(longest, n_steps) and (want_len[3:6] == -1).all() and want_len[6] == 0
        for q in range(3):
            i, j = sr.world2grid(g, poses[q][0], poses[q][1])
            way = [(i, j)] + [sr.world2grid(g, x, y) for x, y, _ in got[q, :got_len[q]]]
            assert all(geo.legal_move(trav, field, a, b) for a, b in zip(way, way[1:]))
    got, untouched = dev.path(field, poses, longest, with_len=False)
    assert np.array_equal(_bits(got), _bits(geo.path(g, field, poses, longest)[0])) and (untouched == S_GEO).all()


def test_a_path_is_a_reference_trajectory_of_the_dynamic_window():
    """the serpentine's paths as d_xt_ref of eea_dwa_control_batch in trajectory mode: accepted (n_ref columns every dt_ref, the
    rollout of horizon / dt steps stays inside n_ref dt_ref), and u_opt / found are the bits of the oracle's DynamicWindow given
    the same reference.  No new kernel runs here beyond the path: the test pins the layout [P][n_steps][3]"""
    g, grid = _serpentine()
    dev = _Device(g, grid)
    goal = np.array([(g.ysize - 1) * g.xsize + g.xsize - 1], dtype=np.int32)
    field, _ = dev.field(cells=goal)
    coll = (0.05, 0.3, 0.02, gs.THR)
    dwa = (0.1, 1.0, 0.2, 1.0, 1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 2.0, -2.0, 3, 8, 5)
    n_ref, dt_ref = 16, 0.1                        # 10 rollout steps of 0.1 s read columns <= round(15 * 0.9 / 1.6) = 8
    cells = [(3, 1), (TY - 2, 5), (TY, 9), (1, 13), (TY // 2, 2 * TX + 1), (5, 4 * TX + 1)]
    assert all(grid[c] == 0 for c in cells)
    x0 = np.array([_centre(g, i, j, th=0.4 * k - 1.0, fx=0.37, fy=0.61) for k, (i, j) in enumerate(cells)])
    vb = np.array([[0.2 * (k % 3) - 0.2, 0.1 * (k % 2), 0.3 * k - 0.6] for k in range(len(cells))])
    want_path, want_len = geo.path(g, field, x0, n_ref)
    got_path, got_len = dev.path(field, x0, n_ref)
    assert np.array_equal(_bits(got_path), _bits(want_path)) and (got_len == n_ref).all() and np.array_equal(got_len, want_len)
    P = len(cells)
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


# ---- the reachable target ------------------------------------------------------------------------------------------------
def _engine(K, res, precision):
    lim = np.array([1.0, 1.0, 2.0])
    return capi.Engine(capi.make_config(capi.MODEL_OMNI, 0.1, 2.0, res, 1.0, K, np.diag([1.0, 1.0, 2.0]), -lim, lim,
                                        precision=precision))


@functools.lru_cache(maxsize=None)
def _target_scene():
    """(64, 41) partly revealed, with a sealed room of unknown cells (full of gain) drawn into it"""
    g, known = gs.partly_revealed(64, 41)
    known = known.copy()
    known[28:36, 44:54] = 100
    known[29:35, 45:53] = -1
    known[31, 48] = 0                              # a free candidate inside, unreachable
    known.setflags(write=False)
    return g, known


@pytest.mark.parametrize("precision", [pytest.param(capi.PREC_F64, id="fp64"), pytest.param(capi.PREC_F32, id="fp32")])
@pytest.mark.parametrize("floor", [0.0, 0.5])
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("kind", [0, 1])
def test_set_target_reachable(kind, stride, floor, precision):
    """phi_k is BITWISE that of eea_spatial_coeff_rows (whole grid) + eea_set_phik_from_sums fed the restated value grid; with
    geo >= 0 on every candidate it is bitwise eea_set_target_gain / eea_set_target_mi; a sealed room full of gain contributes
    nothing (its cells are 0 in the value grid although their field is not)"""
    R, K = 5, 6
    g, known = _target_scene()
    xs, ys = g.xsize, g.ysize
    npt, tt = (np.float32, torch.float32) if precision == capi.PREC_F32 else (np.float64, torch.float64)
    lx, ly = (xs - 1) * g.resolution, (ys - 1) * g.resolution
    dev = _Device(g, known)
    # the field the caller already has: the existing field entries' own output
    d_field = torch.empty(xs * ys, dtype=torch.int32 if kind == 0 else torch.float64, device="cuda")
    if kind == 0:
        capi.sense_gain_field(dev.cfg, R, stride, dev.d_grid, d_field)
    else:
        capi.sense_mi_field(dev.cfg, R, stride, dev.d_grid, d_field, p_unknown=0.5)
    torch.cuda.synchronize()
    field = d_field.cpu().numpy().reshape(ys, xs)
    field = field.view(np.uint32) if kind == 0 else field
    d_field = dev.upload(field.view(np.int32) if kind == 0 else field, np.int32 if kind == 0 else np.float64)
    src = np.array([_centre(g, 20, 31)])
    assert known[20, 31] == 0
    geo_field, _ = dev.field(poses=src)
    _same(geo_field, dev.restated(poses=src)[0])
    d_geo = dev.upload(geo_field, np.int32)
    v = geo.reachable_values(g, stride, known, field, geo_field, floor, npt)
    room = np.zeros_like(known, dtype=bool)
    room[29:35, 45:53] = True
    assert (geo_field[room] == -1).all() and (v[room] == 0).all() and field[room].sum() > 0 and v.sum() > 0
    eng = _engine(K, g.resolution, precision)
    eng.set_target_reachable(dev.cfg, kind, d_field, stride, dev.d_grid, d_geo, lx, ly, floor=floor)
    torch.cuda.synchronize()
    got = eng.phik()
    sums = torch.empty(K * K, dtype=tt, device="cuda")
    eng.spatial_coeff_rows(xs, ys, 0, ys, torch.as_tensor(v).cuda(), lx, ly, sums)
    eng.set_phik_from_sums(sums, lx, ly)
    torch.cuda.synchronize()
    want = eng.phik()
    assert np.isfinite(want).all() and np.array_equal(got, want), np.abs(got - want).max()
    # everything reachable: the existing targets' bits
    d_all = dev.upload(np.zeros(xs * ys, dtype=np.int32), np.int32)
    st = torch.cuda.Stream()
    eng.set_target_reachable(dev.cfg, kind, d_field, stride, dev.d_grid, d_all, lx, ly, floor=floor, stream=st.cuda_stream)
    torch.cuda.synchronize()
    got_all = eng.phik()
    if kind == 0:
        eng.set_target_gain(dev.cfg, R, stride, dev.d_grid, lx, ly, floor=floor)
    else:
        eng.set_target_mi(dev.cfg, R, stride, dev.d_grid, lx, ly, p_unknown=0.5, floor=floor)
    torch.cuda.synchronize()
    assert np.array_equal(got_all, eng.phik()) and not np.array_equal(got_all, got)
    # nothing reachable: non-finite, as an all-zero grid is
    d_none = dev.upload(np.full(xs * ys, -1, dtype=np.int32), np.int32)
    eng.set_target_reachable(dev.cfg, kind, d_field, stride, dev.d_grid, d_none, lx, ly, floor=floor)
    torch.cuda.synchronize()
    assert not np.isfinite(eng.phik()).any()
    dev.check(dev.inputs[0][1], G_IN)
    eng.close()


# ---- the host mirror -------------------------------------------------------------------------------------------------------
def test_host_mirror_geodesic_field():
    """host/build/geodesic_field_tests (GeodesicField in geodesic_field.hpp: update on two maps in turn -- the second smaller
    and inflated through a DistanceField --, reachable, cost, path) runs, and its printed answers are the restatement's"""
    exe = os.path.join(ROOT, "ergodic_exploration_amd", "host", "build", "geodesic_field_tests")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    maps = {}
    for line in out.stdout.splitlines():
        w = line.split()
        maps.setdefault(int(w[1]), {}).setdefault(w[0], []).append(w[2:])
    assert sorted(maps) == [0, 1]
    from tests import distance_restatement as dr
    for n, m in maps.items():
        W, H, res, ox, oy, clear_sq, flags, n_src = m["map"][0]
        W, H, clear_sq, flags, n_src = int(W), int(H), int(clear_sq), int(flags), int(n_src)
        g = sr.Geometry(float(ox), float(oy), float(res), W, H, 0.8)
        grid = _host_map(n, W, H)
        sources = np.array([[float(x), float(y), 0.0] for x, y in m["source"]])
        sq = None
        if clear_sq >= 0:
            sq = dr.brute_force(grid, 0.8)[0]
        want, want_src = geo.field(g, grid, sources, None, sq, max(clear_sq, 0), flags)
        got = np.array([[int(v) for v in row[1:]] for row in sorted(m["geo"], key=lambda r: int(r[0]))], dtype=np.int32)
        _same(got, want)
        assert n_src == want_src and (got > 0).any() and (got[grid == 0] == -1).any()
        poses = np.array([[float(v) for v in p[1:4]] for p in m["pose"]])
        n_steps = len(m["way"]) // len(poses)
        want_path, want_len = geo.path(g, want, poses, n_steps)
        way = np.array([[float(v) for v in r[2:]] for r in m["way"]]).reshape(len(poses), n_steps, 3)
        assert np.array_equal(_bits(way), _bits(want_path))
        for q, p in enumerate(m["pose"]):
            i, j = sr.world2grid(g, poses[q][0], poses[q][1])
            cost = int(want[i, j]) if (i <= H - 1 and j <= W - 1) else -1
            assert [int(p[4]), int(p[5]), int(p[6])] == [int(cost >= 0), cost, int(want_len[q])], (n, q)
        assert {int(p[4]) for p in m["pose"]} == {0, 1}


def _host_map(n, W, H):
    """the two maps of host/test/geodesic_field_tests.cpp"""
    d = np.zeros((H, W), dtype=np.int8)
    if n == 0:
        d[:30, 20] = 100
        d[12, 20] = 0
        d[25, 34:44] = d[34, 34:44] = 100
        d[25:35, 34] = d[25:35, 43] = 100
        d[3:9, 30:36] = -1
        d[36, 5], d[37, 5] = 80, 79
    else:
        d[8, :] = 100
        d[8, 4:6] = 0
        d[8, 12:17] = 0
    return d

"""The frontier auction (include/ergodic_amd.h: eea_frontier_auction_ws_bytes, eea_frontier_auction; csrc/auction_kernel.hip)
without a GPU: tests/auction_restatement.py against a second statement that is independent of it -- one multi-seed Dijkstra per
open region, every robot takes the least (cost, label) over them, a sort per region accepts -- on the scenes the GPU tests draw
and on random grids; what any answer must obey; that the scenes hold the cases they were drawn for; the entry points, the
workspace size, every refusal that comes before the device is selected, and the kernels in the build."""
import ctypes as C
import heapq
import os
import subprocess
import sys

import numpy as np
import pytest

from ergodic_exploration_amd import capi

from tests import auction_restatement as ar
from tests import auction_scenes as scn
from tests import frontier_restatement as fr
from tests import frontier_scenes as fs
from tests import geodesic_restatement as geo
from tests import sense_restatement as sr

ENTRIES = {"eea_frontier_auction_ws_bytes": 4, "eea_frontier_auction": 25}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ((0, 1, 5), (1, 0, 5), (0, -1, 5), (-1, 0, 5), (1, 1, 7), (1, -1, 7), (-1, -1, 7), (-1, 1, 7))   # the walk's order


# ---- the second statement ----------------------------------------------------------------------------------------------------
def _open_cells(g, grid, poses, sq, clear_sq, flags):
    """the enterable cells, cell by cell from the header's words"""
    ok = np.zeros((g.ysize, g.xsize), dtype=bool)
    for i in range(g.ysize):
        for j in range(g.xsize):
            v = int(grid[i, j])
            t = v / 100.0 < g.occupied_threshold and not (flags & 1 and v < 0)
            if t and sq is not None:
                t = sq[i, j] == -1 or sq[i, j] > clear_sq
            ok[i, j] = t
    cells = []
    for p in poses:
        i, j = sr.world2grid(g, p[0], p[1])
        placed = i < g.ysize and j < g.xsize and int(grid[i, j]) / 100.0 < g.occupied_threshold
        cells.append((i, j) if placed else None)
        if placed:
            ok[i, j] = True
    return ok, cells


def _one_region_costs(ok, seeds):
    """costs from the seeds of ONE region: -1 where no move sequence arrives"""
    ys, xs = ok.shape
    d = np.full((ys, xs), -1, dtype=np.int64)
    heap = [(0, c) for c in seeds]
    done = set()
    while heap:
        c0, (i, j) = heapq.heappop(heap)
        if (i, j) in done:
            continue
        done.add((i, j))
        d[i, j] = c0
        for di, dj, w in STEPS:
            a, b = i + di, j + dj
            if not (0 <= a < ys and 0 <= b < xs) or not ok[a, b] or (a, b) in done:
                continue
            if di and dj and not (ok[i + di, j] and ok[i, j + dj]):
                continue
            heapq.heappush(heap, (c0 + w, (a, b)))
    return d


def second_statement(g, grid, region, rec, fstate, max_regions, poses, n_auction, min_size, cells_per_robot, n_steps, sq, clear_sq,
                     flags):
    """(goal_region, goal_cell, goal_cost, path, length, assigned, rounds that were not idle)"""
    grid = np.asarray(grid).reshape(g.ysize, g.xsize)
    region = np.asarray(region).reshape(g.ysize, g.xsize)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    P = len(poses)
    ok, cells = _open_cells(g, grid, poses, sq, clear_sq, flags)
    n = min(int(fstate[1]), max_regions)
    rem = {}
    for r in range(n):
        size = int(rec[r]["size"])
        if size >= min_size:
            rem[r] = 1 if cells_per_robot == 0 else -(-size // cells_per_robot)
    goal_region, goal_cell, goal_cost, length = (np.full(P, -1, dtype=np.int32) for _ in range(4))
    path = np.repeat(poses[:, None, :], n_steps, axis=1).copy()
    busy = 0
    for _ in range(n_auction):
        waiting = [q for q in range(P) if cells[q] is not None and goal_region[q] < 0]
        open_regions = sorted(r for r in rem if rem[r] > 0)
        if not waiting or not open_regions:
            continue
        busy += 1
        fields = {}
        for r in open_regions:
            members = [(int(i), int(j)) for i, j in np.argwhere(region == r) if int(grid[i, j]) / 100.0 < g.occupied_threshold]
            fields[r] = _one_region_costs(ok, members)
        big = 1 << 60
        stack = np.stack([np.where(fields[r] < 0, big, fields[r]) for r in open_regions])
        cost = stack.min(axis=0)
        owner = np.array(open_regions)[stack.argmin(axis=0)]          # (the first least: the lowest rank)
        owner = np.where(cost == big, -1, owner)
        cost = np.where(cost == big, -1, cost)
        bidders = {}
        for q in waiting:
            if cost[cells[q]] >= 0:
                bidders.setdefault(int(owner[cells[q]]), []).append((int(cost[cells[q]]), q))
        for r, who in bidders.items():
            who.sort()
            for d, q in who[:rem[r]]:
                i, j = cells[q]
                goal_region[q], goal_cost[q] = r, d
                last = geo.cell_centre(g, i, j) + (poses[q, 2],)
                moves = 0
                while cost[i, j] > 0:
                    for k, (di, dj, w) in enumerate(STEPS):
                        a, b = i + di, j + dj
                        if not (0 <= a < g.ysize and 0 <= b < g.xsize) or cost[a, b] < 0 or cost[a, b] + w != cost[i, j] or owner[a, b] != r:
                            continue
                        if k >= 4 and (cost[i + di, j] < 0 or cost[i, j + dj] < 0):
                            continue
                        break
                    else:
                        raise AssertionError("no step")
                    i, j = a, b
                    if moves < n_steps:
                        last = geo.cell_centre(g, i, j) + (geo.HEADINGS[k],)
                        path[q, moves] = last
                    moves += 1
                path[q, min(moves, n_steps):] = last
                goal_cell[q], length[q] = i * g.xsize + j, min(moves, n_steps)
            rem[r] -= min(rem[r], len(who))
    return goal_region, goal_cell, goal_cost, path, length, int((goal_region >= 0).sum()), busy


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _agree(res, other):
    assert np.array_equal(res.goal_region, other[0]) and np.array_equal(res.goal_cell, other[1]) and np.array_equal(res.goal_cost, other[2])
    assert np.array_equal(_bits(res.path), _bits(other[3])) and np.array_equal(res.length, other[4])
    assert res.state.tolist() == [1, 0, other[5], other[6]]


# ---- what any answer must obey ---------------------------------------------------------------------------------------------
def check_invariants(g, grid, region, rec, fstate, max_regions, poses, res, n_auction, min_size, cells_per_robot, n_steps, sq,
                     clear_sq, flags):
    grid = np.asarray(grid).reshape(g.ysize, g.xsize)
    region = np.asarray(region).reshape(g.ysize, g.xsize)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    cap = ar.capacities(rec, fstate, max_regions, min_size, cells_per_robot)
    cells = ar.robot_cells(g, grid, poses)
    ok = ar.enterable(g, grid, poses, sq, clear_sq, flags)
    going = np.flatnonzero(res.goal_region >= 0)
    # no region gets more than cap_r robots, and only an eligible one gets any
    for r in set(res.goal_region[going].tolist()):
        assert 0 < (res.goal_region == r).sum() <= cap[r], r
    for q in range(len(poses)):
        if res.goal_region[q] < 0:
            assert res.goal_cell[q] == res.goal_cost[q] == res.length[q] == -1 and res.assigned_in[q] == -1
            assert np.array_equal(_bits(res.path[q]), _bits(np.repeat(poses[q][None], n_steps, axis=0)))
            continue
        r = int(res.goal_region[q])
        assert cells[q] is not None
        # the goal cell is a member of the region, and one that does not block
        gi, gj = divmod(int(res.goal_cell[q]), g.xsize)
        assert region[gi, gj] == r and not sr.blocks(int(grid[gi, gj]), g.occupied_threshold)
        # every row follows the move rule: one of the eight moves into an enterable cell (or a seed), a diagonal between two
        # such cells; the row is the cell's centre with the move's heading; the costs of the moves add up to goal_cost when the
        # whole walk fits
        at, total = cells[q], 0
        for t in range(int(res.length[q])):
            x, y, th = res.path[q, t]
            nxt = sr.world2grid(g, x, y)
            assert (x, y) == geo.cell_centre(g, *nxt)
            di, dj = nxt[0] - at[0], nxt[1] - at[1]
            assert (di, dj) in geo.MOVES and th == geo.HEADINGS[geo.MOVES.index((di, dj))]
            free = lambda c: bool(ok[c]) or region[c] >= 0
            assert free(nxt) and (di == 0 or dj == 0 or (free((at[0] + di, at[1])) and free((at[0], at[1] + dj))))
            total += 5 if di == 0 or dj == 0 else 7
            at = nxt
        if res.length[q] < n_steps:
            assert total == res.goal_cost[q] and at == (gi, gj)
            rest = res.path[q, int(res.length[q]):]
            want = res.path[q, int(res.length[q]) - 1] if res.length[q] else np.array(geo.cell_centre(g, *cells[q]) + (poses[q, 2],))
            assert np.array_equal(_bits(rest), _bits(np.repeat(want[None], len(rest), axis=0)))
        else:
            assert total <= res.goal_cost[q]
        if res.goal_cost[q] == 0:
            assert res.length[q] == 0 and (gi, gj) == cells[q]
    # a robot accepted in round a > 0 lost every earlier round it bid in to robots with a smaller (cost, index), or had no key
    for q in going:
        for b in range(int(res.assigned_in[q])):
            if q in res.bids[b]:
                d, r = res.bids[b][q]
                winners = [p for p in np.flatnonzero((res.goal_region == r) & (res.assigned_in == b))]
                assert all((int(res.goal_cost[p]), int(p)) < (d, int(q)) for p in winners)
    assert res.state[2] == len(going) and res.state[3] == len(res.bids) <= n_auction
    # the first round alone is the nearest-frontier rule: a robot bids for the least (cost, rank) over the eligible regions
    first = ar.auction(g, grid, region, rec, fstate, max_regions, poses, n_auction=1, min_size=min_size, cells_per_robot=cells_per_robot,
                       n_steps=0, sq=sq, clear_sq=clear_sq, flags=flags)
    if first.bids:
        costs = {r: _one_region_costs(ok, [c for rr, c in ar.seeds(g, grid, region, cap) if rr == r]) for r in range(max_regions) if cap[r]}
        for q, (d, r) in first.bids[0].items():
            assert (d, r) == min((int(f[cells[q]]), rr) for rr, f in costs.items() if f[cells[q]] >= 0), q
        for q in np.flatnonzero(first.goal_region >= 0):
            assert (int(first.goal_cost[q]), int(first.goal_region[q])) == first.bids[0][int(q)]


def _scene_inputs(name):
    sc = scn.scene(name)
    _, region, rec, fstate = scn.regions(name)
    return sc, region, rec, fstate


@pytest.mark.parametrize("name", scn.NAMES)
def test_the_second_statement_agrees_on_the_scenes(name):
    sc, region, rec, fstate = _scene_inputs(name)
    res = scn.answer(name)
    _agree(res, second_statement(sc.g, sc.grid, region, rec, fstate, sc.max_regions, sc.poses, sc.n_auction, sc.min_size,
                                 sc.cells_per_robot, sc.n_steps, sc.sq, sc.clear_sq, sc.flags))
    check_invariants(sc.g, sc.grid, region, rec, fstate, sc.max_regions, sc.poses, res, sc.n_auction, sc.min_size, sc.cells_per_robot,
                     sc.n_steps, sc.sq, sc.clear_sq, sc.flags)


@pytest.mark.parametrize("seed", range(24))
def test_the_second_statement_agrees_on_random_grids(seed):
    """grids of free, unknown and blocking cells with values on both sides of the threshold; regions of the grid's frontier or
    of a random mask plane; robots on and off the grid, on walls and on unknown cells; every argument drawn"""
    rng = np.random.default_rng(7100 + seed)
    ys, xs = int(rng.integers(1, 26)), int(rng.integers(1, 26))
    g = sr.Geometry(-1.0, 0.5, 0.25, xs, ys, 0.8)
    grid = rng.choice(np.array([0, 0, 0, 0, 0, -1, -1, 100, 79, 80], dtype=np.int8), size=(ys, xs))
    if seed % 3 == 2:
        mask = (rng.random((ys, xs)) < 0.15).astype(np.int8)
        _, region, rec, fstate = fr.regions(fr.OF_MASK, mask, 0.8)
    else:
        _, region, rec, fstate = fr.regions(fr.OF_GRID, grid, 0.8)
    max_regions = int(rng.integers(0, int(fstate[0]) + 3))
    rec = rec[:max_regions]
    fstate = np.array([fstate[0], min(int(fstate[0]), max_regions), fstate[2], 0], dtype=np.uint32)
    P = int(rng.integers(1, 12))
    poses = np.stack([rng.uniform(-1.3, -1.0 + 0.25 * xs + 0.3, P), rng.uniform(0.2, 0.5 + 0.25 * ys + 0.3, P), rng.uniform(-3, 3, P)], 1)
    sq = fs._squared_distances(grid, 0.8) if seed % 2 else None
    args = dict(n_auction=int(rng.integers(1, 5)), min_size=int(rng.integers(0, 4)), cells_per_robot=int(rng.integers(0, 4)),
                n_steps=int(rng.integers(0, 7)), sq=sq, clear_sq=int(rng.integers(0, 3)), flags=int(rng.integers(0, 2)))
    res = ar.auction(g, grid, region, rec, fstate, max_regions, poses, **args)
    _agree(res, second_statement(g, grid, region, rec, fstate, max_regions, poses, **args))
    check_invariants(g, grid, region, rec, fstate, max_regions, poses, res, **args)


def test_the_scenes_are_what_their_names_say():
    """the cases the scenes were drawn for are in them"""
    sc, region, rec, fstate = _scene_inputs("hall")
    res = scn.answer("hall")
    cells = ar.robot_cells(sc.g, sc.grid, sc.poses)
    cap = ar.capacities(rec, fstate, sc.max_regions, sc.min_size, sc.cells_per_robot)
    ok = ar.enterable(sc.g, sc.grid, sc.poses, sc.sq, sc.clear_sq, sc.flags)
    assert sc.grid.shape == (2 * scn.T, 3 * scn.T) and scn.scene("maze").grid.shape == (3 * scn.T, 3 * scn.T)
    # (i) a robot assigned in a round >= 1, (ii) robots left over after the last round: capacity < placed robots
    assert res.assigned_in.tolist() == [-1, -1, 0, -1, 0, 0, 0, 1, -1, 0, -1] and res.state.tolist() == [1, 0, 6, 2]
    assert sum(cap) == 6 < sum(c is not None for c in cells) == 9 and sc.n_auction == 3
    assert all(cells[q] is not None and q in res.bids[1] for q in (8, 10)) and res.goal_region[8] == res.goal_region[10] == -1
    # (iii) equal cost for one region, settled by the index
    assert res.bids[0][6] == res.bids[0][7] == (15, 2) and cap[2] == 1 and res.goal_region[6] == 2 and res.assigned_in[7] == 1
    # (iv) equidistant from two regions: the lower rank
    seeds = ar.seeds(sc.g, sc.grid, region, cap)
    d2, d3 = (_one_region_costs(ok, [c for r, c in seeds if r == k]) for k in (2, 3))
    assert d2[cells[8]] == d3[cells[8]] == 45 and res.bids[0][8] == (45, 2)
    # (v) a capacity above 1, used up
    assert cap == [0, 4, 1, 1] and (res.goal_region == 1).sum() == 4
    # (vi) off the grid, on a blocking cell, on an unknown cell under UNKNOWN_BLOCKS (placed through the waiver), cut off
    assert cells[0] is None and cells[1] is None and sr.blocks(int(sc.grid[30, 5]), sc.g.occupied_threshold)
    assert sc.flags == geo.UNKNOWN_BLOCKS and sc.grid[cells[2]] == -1 and not geo.traversable(sc.g, sc.grid, flags=sc.flags)[cells[2]]
    assert res.goal_region[2] == 1 and res.goal_cost[2] == 5 and res.length[2] == 1
    assert cells[3] is not None and all(3 not in b for b in res.bids) and res.goal_region[3] == -1
    # (vii) a robot on a member cell
    assert region[cells[4]] == 1 and (res.goal_cost[4], res.length[4], res.goal_cell[4]) == (0, 0, cells[4][0] * sc.g.xsize + cells[4][1])
    # (viii) a region below min_size, and regions of a rank >= max_regions: neither seeds nor goals
    assert rec[0]["size"] == 2 < sc.min_size and fstate[0] == 6 > sc.max_regions == 4 and region.max() == 5
    assert not {0, 4, 5} & {r for r, _ in seeds} and not {0, 4, 5} & set(res.goal_region.tolist())
    assert region[60, 21] == 4 and res.bids[0][10][1] != 4
    # (x) a path longer than n_steps whose goal cell lies beyond the last row
    assert res.length[7] == sc.n_steps and res.goal_cost[7] > 7 * sc.n_steps
    assert sr.world2grid(sc.g, *res.path[7, -1, :2]) != divmod(int(res.goal_cell[7]), sc.g.xsize)
    # (ix) a grid with no region at all
    assert scn.regions("no_region")[3].tolist() == [0, 0, 0, 0] and scn.answer("no_region").state.tolist() == [1, 0, 0, 0]
    # the maze: a seed that is not enterable, a second round whose winner comes from corridors away, an idle third round
    mz, mregion, mrec, mstate = _scene_inputs("maze")
    mres = scn.answer("maze")
    mok = ar.enterable(mz.g, mz.grid, mz.poses, mz.sq, mz.clear_sq, mz.flags)
    assert any(not mok[c] for _, c in ar.seeds(mz.g, mz.grid, mregion, ar.capacities(mrec, mstate, mz.max_regions, 1, 30)))
    assert mres.state.tolist() == [1, 0, 6, 2] and (mres.assigned_in == 1).sum() == 1 and mz.n_auction == 3
    late = int(np.flatnonzero(mres.assigned_in == 1)[0])
    assert mres.goal_cost[late] > 5 * 2 * scn.T and ar.robot_cells(mz.g, mz.grid, mz.poses)[-1] is None
    # the crowd: 300 bidders for 7 places, costs that repeat among the winners and at the cut
    cres = scn.answer("crowd")
    assert len(cres.bids) == 1 and len(cres.bids[0]) == 300 and cres.state.tolist() == [1, 0, 7, 1]
    ranked = sorted((d, q) for q, (d, r) in cres.bids[0].items())
    assert [q for _, q in ranked[:7]] == sorted(np.flatnonzero(cres.goal_region == 0).tolist(), key=lambda q: (cres.goal_cost[q], q))
    assert ranked[6][0] == ranked[7][0], "the cut falls between two robots of equal cost: the index decides"


# ---- the entries -------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    raw = C.CDLL(capi.LIB_PATH)
    L = capi.lib()
    for name, n_args in ENTRIES.items():
        assert name in capi.declared_symbols() and hasattr(raw, name), name
        assert len(getattr(L, name).argtypes) == n_args, name
    for name in ("frontier_auction_ws_bytes", "frontier_auction"):
        assert callable(getattr(capi, name)), name
    assert L.eea_abi_version() == 6


def test_workspace_bytes_are_positive_and_monotone():
    sizes = [(1, 1), (1, 33), (33, 1), (33, 33), (64, 41), (200, 100), (1024, 1024), (8192, 8192)]
    cfgs = [capi.make_collision_cfg(0.0, 0.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 0.8) for xs, ys in sizes]
    got = [capi.frontier_auction_ws_bytes(c, 0, 0) for c in cfgs]
    assert got[0] > 0 and all(a <= b for a, b in zip(got, got[1:])) and got[-1] > got[0]
    by_p = [capi.frontier_auction_ws_bytes(cfgs[3], P, 5) for P in (0, 1, 2, 255, 256, 257, 4096, 65536)]
    by_r = [capi.frontier_auction_ws_bytes(cfgs[3], 7, n) for n in (0, 1, 2, 255, 256, 257, 4096, (1 << 31) - 1)]
    for seq in (by_p, by_r):
        assert all(a < b for a, b in zip(seq, seq[1:])) and all(v % 4 == 0 for v in seq)
    # the planes the header names fit: a key, a cost and a label per cell, a bid per robot, three words per record slot
    assert capi.frontier_auction_ws_bytes(cfgs[3], 10, 20) >= 33 * 33 * 17 + 10 * 16 + 20 * 12
    L = capi.lib()
    assert L.eea_frontier_auction_ws_bytes(None, 1, 1, C.byref(C.c_size_t())) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_frontier_auction_ws_bytes(C.byref(cfgs[0]), 1, 1, None) == capi.ERR_INVALID_ARGUMENT


def test_argument_errors_come_before_the_device():
    """every refusal of the header is answered without a device: the buffers are host arrays that hold a sentinel nothing may
    touch"""
    L = capi.lib()
    xs, ys, P, R, n_steps = 40, 30, 3, 4, 5
    good = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 0.8)
    grid = np.zeros(xs * ys, dtype=np.int8)
    sq, region = (np.full((ys, xs), 7, dtype=np.int32) for _ in range(2))
    recs, fstate = np.full(R * 56, 7, dtype=np.uint8), np.full(4, 7, dtype=np.uint32)
    pose = np.full((P, 3), 7.0)
    g_region, g_cell, g_cost, length = (np.full(P, 7, dtype=np.int32) for _ in range(4))
    path = np.full((P, n_steps, 3), 7.0)
    ws, state = np.full(capi.frontier_auction_ws_bytes(good, P, R) + 8, 7, dtype=np.uint8), np.full(4, 7, dtype=np.uint32)
    off = (-ws.ctypes.data) % 8
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    ref = lambda c: None if c is None else C.byref(c)
    INV, UNS = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED

    def call(cfg=good, g=grid, s=sq, clear_sq=0, flags=0, rg=region, rc=recs, fs_=fstate, n=R, ps=pose, P_=P, n_auction=2, min_size=1,
             cpr=0, max_rounds=0, steps=n_steps, gr=g_region, gc=g_cell, gk=g_cost, pt=path, ln=length, w=off, st=state):
        wp = None if w is None else C.c_void_p(ws.ctypes.data + w)
        return L.eea_frontier_auction(0, ref(cfg), p(g), p(s), clear_sq, flags, p(rg), p(rc), p(fs_), n, p(ps), P_, n_auction, min_size,
                                      cpr, max_rounds, steps, p(gr), p(gc), p(gk), p(pt), p(ln), wp, p(st), None)

    assert call(cfg=None) == INV
    for kw in (dict(g=None), dict(rg=None), dict(fs_=None), dict(ps=None), dict(gr=None), dict(gc=None), dict(gk=None), dict(w=None),
               dict(st=None)):
        assert call(**kw) == INV and b"null" in L.eea_last_error(), kw
    assert call(rc=None) == INV and b"d_regions" in L.eea_last_error()
    assert call(pt=None) == INV and b"d_path" in L.eea_last_error()
    assert call(clear_sq=-1) == INV and b"clear_sq" in L.eea_last_error()
    for flags in (2, 3, 4, 1 << 31):
        assert call(flags=flags) == INV and b"flag" in L.eea_last_error(), flags
    assert call(n_auction=0) == INV and b"n_auction" in L.eea_last_error()
    for w in (off + 4, off + 2, off + 1):
        assert call(w=w) == INV and b"8-byte aligned" in L.eea_last_error(), w
    assert call(P_=65537) == UNS and b"65536" in L.eea_last_error()
    assert call(n=1 << 31) == UNS and b"2^31 - 1" in L.eea_last_error()
    # the refusals hold for both forms of max_rounds, and with the optional buffers absent
    assert call(max_rounds=3, n_auction=0) == INV and call(max_rounds=3, ln=None, s=None, gr=None) == INV
    # the configuration errors and the limits of the geodesic calls
    swapped = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 1.0, 0.7, 0.2, 0.8)
    assert call(cfg=swapped) == INV and b"Search radius" in L.eea_last_error()
    for bad in (capi.make_collision_cfg(-2.0, -1.0, 0.1, 0, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, 0, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.0, xs, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 100.5)):
        assert call(cfg=bad) == INV and L.eea_frontier_auction_ws_bytes(C.byref(bad), P, R, C.byref(C.c_size_t())) == INV
    side = capi.DISTANCE_MAX_SIDE
    for big in (capi.make_collision_cfg(-2.0, -1.0, 0.1, side + 1, 4, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, 4, side + 1, 0.7, 1.0, 0.2, 0.8)):
        assert call(cfg=big) == UNS and b"EEA_DISTANCE_MAX_SIDE" in L.eea_last_error()
        assert L.eea_frontier_auction_ws_bytes(C.byref(big), P, R, C.byref(C.c_size_t())) == UNS
    for a, v in ((sq, 7), (region, 7), (recs, 7), (fstate, 7), (pose, 7.0), (g_region, 7), (g_cell, 7), (g_cost, 7), (length, 7),
                 (path, 7.0), (ws, 7), (state, 7)):
        assert (a == v).all()
    assert not grid.any()


def test_auction_kernels_are_in_the_library():
    """the kernels of csrc/auction_kernel.hip are gfx950 code in the build and use no scratch; the rank launch's tile of bids (a
    region and a key per lane of the workgroup) and the round's staged tile are static LDS well inside 64 KB"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    obj = os.path.join(os.path.dirname(capi.LIB_PATH), "..", "csrc", "build", "auction_kernel.o")
    names = {}
    for k in kr.kernels(obj):
        if "vgpr_count" in k:
            names[subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.strip()] = k
    for w in ("auction_plane_kernel(", "auction_state_kernel(", "auction_robots_kernel(", "auction_capacity_kernel(",
              "auction_begin_kernel(", "auction_round_kernel(", "auction_close_kernel(", "auction_unpack_kernel(", "auction_bid_kernel(",
              "auction_rank_kernel(", "auction_update_kernel("):
        found = [k for n, k in names.items() if w in n]
        assert len(found) == 1, (w, sorted(names))
        assert int(found[0]["private_segment_fixed_size"]) == 0, found[0]
    lds = lambda w: int([k for n, k in names.items() if w in n][0]["group_segment_fixed_size"])
    assert 12 * 256 <= lds("auction_rank_kernel(") <= 4 * 1024
    T2 = (capi.GEODESIC_TILE_X + 2) * (capi.GEODESIC_TILE_Y + 2)
    assert 9 * T2 <= lds("auction_round_kernel(") <= 16 * 1024

"""Goal paths without a device (include/ergodic_amd.h: eea_geodesic_goto_batch; csrc/goto_kernel.hip).

tests/goto_restatement.py -- Dijkstra on the window's graph and the walk -- is what tests/test_gpu_goto.py holds the device to;
here it is held to a second, independent statement (crop the grid and the distance plane to the window, make the robot's cell
enterable in the copies, run tests/geodesic_restatement.py's field and path_cells on the crop, map the cells back) and to the
invariants of any answer, on the scenes of tests/goto_scenes.py and on random grids.  Then the entry itself: declared,
exported, bound, every refusal answered before the device is selected, and the kernel in the build without scratch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from ergodic_exploration_amd import capi

from tests import frontier_scenes as fs
from tests import gain_scenes as gs
from tests import geodesic_restatement as geo
from tests import goto_restatement as gr
from tests import goto_scenes as scn
from tests import sense_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"eea_geodesic_goto_batch": 18}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the second statement ----------------------------------------------------------------------------------------------------
def second_statement(g, grid, poses, goals, margin, n_steps, sq=None, clear_sq=0, flags=0, mask=None, untouched=(0, 0, 0.0, 0)):
    """gr.goto's first five results through geo.field / geo.path_cells on a crop of the grid"""
    grid = np.asarray(grid, dtype=np.int8).reshape(g.ysize, g.xsize)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    P = len(poses)
    cost, status = np.full(P, untouched[0], np.int32), np.full(P, untouched[1], np.int32)
    path, length = np.full((P, n_steps, 3), untouched[2]), np.full(P, untouched[3], np.int32)
    counts = {k: 0 for k in range(5)}
    blocking = ~(grid.astype(np.float64) / 100.0 < g.occupied_threshold)
    for q in range(P):
        if mask is not None and not mask[q]:
            continue
        x, y, th = poses[q]
        ci, cj = sr.world2grid(g, x, y)
        k = int(goals[q])
        if ci >= g.ysize or cj >= g.xsize or blocking[ci, cj]:
            st = gr.NO_ROBOT
        elif not 0 <= k < grid.size or blocking.flat[k]:
            st = gr.NO_GOAL
        else:
            gi, gj = k // g.xsize, k % g.xsize
            rows = range(max(0, min(ci, gi) - margin), min(g.ysize, max(ci, gi) + margin + 1))
            cols = range(max(0, min(cj, gj) - margin), min(g.xsize, max(cj, gj) + margin + 1))
            st = gr.WINDOW if len(rows) * len(cols) > capi.GOTO_MAX_CELLS else gr.OK
        if st == gr.OK:
            i0, j0 = rows[0], cols[0]
            crop = grid[i0:i0 + len(rows), j0:j0 + len(cols)].copy()
            crop[ci - i0, cj - j0] = 0                                       # the robot's cell: known, free ...
            csq = None
            if sq is not None:
                csq = np.asarray(sq).reshape(g.ysize, g.xsize)[i0:i0 + len(rows), j0:j0 + len(cols)].copy()
                csq[ci - i0, cj - j0] = -1                                   # ... and clear of everything
            cg = sr.Geometry(0.0, 0.0, 1.0, len(cols), len(rows), g.occupied_threshold)
            field, n_src = geo.field(cg, crop, cells=[(gi - i0) * len(cols) + (gj - j0)], sq=csq, clear_sq=clear_sq, flags=flags)
            assert n_src == 1
            if field[ci - i0, cj - j0] < 0:
                st = gr.CUT_OFF
        counts[st] += 1
        status[q] = st
        if st != gr.OK:
            cost[q] = length[q] = -1
            path[q, :] = poses[q]
            continue
        cost[q] = field[ci - i0, cj - j0]
        steps = geo.path_cells(field, ci - i0, cj - j0, n_steps)
        length[q] = len(steps)
        rows_out = [(float(cj) * g.resolution + g.resolution / 2.0 + g.xmin, float(ci) * g.resolution + g.resolution / 2.0 + g.ymin, th)]
        for i, j, m in steps:
            rows_out.append((float(j + j0) * g.resolution + g.resolution / 2.0 + g.xmin,
                             float(i + i0) * g.resolution + g.resolution / 2.0 + g.ymin, geo.HEADINGS[m]))
        for t in range(n_steps):
            path[q, t] = rows_out[min(t + 1, len(steps))]
    state = np.array([counts[gr.OK], counts[gr.WINDOW], counts[gr.CUT_OFF], counts[gr.NO_ROBOT] + counts[gr.NO_GOAL]], dtype=np.uint32)
    return cost, status, path, length, state


def _agree(res, other):
    for k, name in enumerate(("cost", "status")):
        assert res[k].dtype == other[k].dtype == np.int32 and np.array_equal(res[k], other[k]), (name, np.flatnonzero(res[k] != other[k])[:8])
    assert res[2].shape == other[2].shape and np.array_equal(_bits(res[2]), _bits(other[2])), np.argwhere(_bits(res[2]) != _bits(other[2]))[:5]
    assert np.array_equal(res[3], other[3]) and res[4].tolist() == other[4].tolist(), (res[4], other[4])


# ---- the invariants of any answer --------------------------------------------------------------------------------------------
def check_invariants(g, grid, poses, goals, res, margin, n_steps, sq, clear_sq, flags, mask, untouched):
    """what holds for every right answer, from the inputs alone: the rows are centres of cells joined by legal moves inside the
    window, the first from the robot's cell, the cost is the sum of the moves when the walk is whole, the rows past the end
    repeat, the counts are the statuses'"""
    grid = np.asarray(grid, dtype=np.int8).reshape(g.ysize, g.xsize)
    trav = geo.traversable(g, grid, sq, clear_sq, flags)
    live = np.ones(len(poses), bool) if mask is None else np.asarray(mask) != 0
    assert [int((res.status[live] == s).sum()) for s in (gr.OK, gr.WINDOW, gr.CUT_OFF)] == res.state[:3].tolist()
    assert int(((res.status[live] == gr.NO_ROBOT) | (res.status[live] == gr.NO_GOAL)).sum()) == res.state[3]
    for q in range(len(poses)):
        if not live[q]:
            assert (res.cost[q], res.status[q], res.length[q]) == (np.int32(untouched[0]), np.int32(untouched[1]), np.int32(untouched[3]))
            assert (res.path[q] == untouched[2]).all()
            continue
        if res.status[q] != gr.OK:
            assert res.cost[q] == res.length[q] == -1
            assert np.array_equal(_bits(res.path[q]), _bits(np.repeat(poses[q][None], n_steps, axis=0)))
            continue
        ci, cj = sr.world2grid(g, poses[q][0], poses[q][1])
        gi, gj = divmod(int(goals[q]), g.xsize)
        i0, i1, j0, j1 = res.windows[q]
        assert (i1 - i0 + 1) * (j1 - j0 + 1) <= gr.MAX_CELLS and i0 <= min(ci, gi) and i1 >= max(ci, gi) and j0 <= min(cj, gj) and j1 >= max(cj, gj)
        enter = lambda c: bool(trav[c]) or c == (ci, cj)
        n = int(res.length[q])
        assert 0 <= n <= n_steps and res.cost[q] >= 0
        at, total = (ci, cj), 0
        for t in range(n):
            x, y, th = res.path[q, t]
            nxt = sr.world2grid(g, x, y)
            assert (x, y) == geo.cell_centre(g, *nxt) and i0 <= nxt[0] <= i1 and j0 <= nxt[1] <= j1
            di, dj = nxt[0] - at[0], nxt[1] - at[1]
            m = geo.MOVES.index((di, dj))
            assert th == geo.HEADINGS[m]
            # forward along the walk the move leaves `at` for `nxt`: the field's move is the reverse one, INTO `at`
            assert enter(at) or t == 0
            assert nxt == (gi, gj) or enter(nxt)
            if m >= 4:
                assert enter((at[0] + di, at[1])) or (at[0] + di, at[1]) == (gi, gj)
                assert enter((at[0], at[1] + dj)) or (at[0], at[1] + dj) == (gi, gj)
            total += geo.COSTS[m]
            at = nxt
        if n < n_steps:                                                     # the walk is whole
            assert at == (gi, gj) and total == res.cost[q]
            last = res.path[q, n - 1] if n else np.array(geo.cell_centre(g, ci, cj) + (poses[q][2],))
            assert np.array_equal(_bits(res.path[q, n:]), _bits(np.repeat(last[None], n_steps - n, axis=0)))
        else:
            assert total <= res.cost[q]
        # no path is cheaper than the straight chamfer distance
        a, b = abs(ci - gi), abs(cj - gj)
        assert res.cost[q] >= 7 * min(a, b) + 5 * abs(a - b)


def _inputs(name):
    sc = scn.scene(name)
    return dict(g=sc.g, grid=sc.grid, poses=sc.poses, goals=sc.goals, n_steps=sc.n_steps, sq=sc.sq, mask=sc.mask, **scn.call_args(sc))


@pytest.mark.parametrize("name", scn.NAMES)
def test_the_second_statement_agrees_on_the_scenes(name):
    kw = _inputs(name)
    res = scn.answer(name)
    _agree(res, second_statement(untouched=scn.UNTOUCHED, **kw))
    check_invariants(res=res, untouched=scn.UNTOUCHED, **kw)


def _random_case(seed):
    rng = np.random.default_rng(1000 + seed)
    xs, ys = int(rng.integers(1, 40)), int(rng.integers(1, 40))
    g = sr.Geometry(-1.5, 0.75, 0.2, xs, ys, 0.65)
    grid = rng.choice(np.array([0, 0, 0, 0, 30, 64, 65, 100, -1, -1], dtype=np.int8), size=(ys, xs))
    sq = fs._squared_distances(grid, g.occupied_threshold) if seed % 3 else None
    P = 30
    poses = np.stack([rng.uniform(-1.5 - 0.3, -1.5 + xs * 0.2 + 0.3, P), rng.uniform(0.75 - 0.3, 0.75 + ys * 0.2 + 0.3, P),
                      rng.uniform(-3, 3, P)], 1)
    goals = rng.integers(-2, xs * ys + 2, P).astype(np.int32)
    mask = None if seed % 4 == 0 else (rng.random(P) < 0.8).astype(np.int32)
    return dict(g=g, grid=grid, poses=poses, goals=goals, margin=int(rng.choice([0, 1, 2, 3, 7, 40])), n_steps=int(rng.integers(0, 25)),
                sq=sq, clear_sq=int(rng.choice([0, 1, 2])), flags=int(seed % 2), mask=mask)


@pytest.mark.parametrize("seed", range(24))
def test_the_second_statement_agrees_on_random_grids(seed):
    kw = _random_case(seed)
    res = gr.goto(untouched=scn.UNTOUCHED, **kw)
    _agree(res, second_statement(untouched=scn.UNTOUCHED, **kw))
    check_invariants(res=res, untouched=scn.UNTOUCHED, **kw)


def test_the_cost_does_not_rise_with_the_margin_and_ends_at_the_whole_grids():
    """among OK answers the cost is non-increasing in margin (a window holds every smaller one's paths); once the window is the
    grid it is geo.field's from the goal, for a robot on a traversable cell (the field waives nothing for a cell that is no
    source)"""
    seen = 0
    for seed in (1, 2, 5, 7, 10, 11):
        kw = _random_case(seed)
        kw["mask"] = None
        g = kw["g"]
        by_margin = [gr.goto(**dict(kw, margin=m)) for m in (0, 1, 2, 3, 5, 8, 13, 40)]
        for a, b in zip(by_margin, by_margin[1:]):
            both = (a.status == gr.OK) & (b.status == gr.OK)
            assert (b.cost[both] <= a.cost[both]).all()
            assert not ((a.status == gr.OK) & (b.status == gr.CUT_OFF)).any()
        whole = by_margin[-1]
        assert all(w is None or w == (0, g.ysize - 1, 0, g.xsize - 1) for w in whole.windows)
        trav = geo.traversable(g, kw["grid"], kw["sq"], kw["clear_sq"], kw["flags"])
        for q in np.flatnonzero((whole.status == gr.OK) | (whole.status == gr.CUT_OFF)):
            ci, cj = sr.world2grid(g, kw["poses"][q][0], kw["poses"][q][1])
            if trav[ci, cj]:
                field, _ = geo.field(g, kw["grid"], cells=[int(kw["goals"][q])], sq=kw["sq"], clear_sq=kw["clear_sq"], flags=kw["flags"])
                assert whole.cost[q] == field[ci, cj]
                seen += 1
    assert seen >= 12


# ---- the scenes hold the cases they were drawn for ---------------------------------------------------------------------------
def test_the_scenes_are_what_their_names_say():
    OK, NR, NG, WIN, CUT = gr.OK, gr.NO_ROBOT, gr.NO_GOAL, gr.WINDOW, gr.CUT_OFF
    shape = lambda w: (w[1] - w[0] + 1, w[3] - w[2] + 1)
    # open: everything OK; the windows are clipped on each side; 1 x N and N x 1; robot == goal; ties pinned by the move order
    o0, o1, o5, omax = (scn.answer("open_m%s" % m) for m in ("0", "1", "5", "max"))
    for o in (o0, o1, o5, omax):
        assert (o.status == OK).all() and o.state.tolist() == [len(scn.OPEN_PAIRS), 0, 0, 0]
        assert np.array_equal(o.cost, o0.cost), "free space: the box of the two cells holds a shortest path"
        assert o.cost[12] == o.cost[13] == 0 and o.length[12] == 0
    assert shape(o0.windows[14]) == (1, 26) and shape(o0.windows[15]) == (26, 1) and shape(o0.windows[12]) == (1, 1)
    assert shape(o0.windows[0]) == (37, 40) and all(w == (0, 36, 0, 39) for w in omax.windows)
    assert o5.windows[6] == (0, 11, 0, 12) and o5.windows[7] == (25, 36, 25, 39)
    assert o1.windows[8][0] == 0 and o1.windows[9][2] == 0 and o1.windows[10][1] == 36 and o1.windows[11][3] == 39
    assert (o0.length == 12).sum() >= 8 and (o0.length < 12).sum() >= 8, "walks longer and shorter than n_steps"
    # (20, 20) -> (27, 31): 7 diagonal and 4 axis moves in any order cost the same; the walk takes the axis moves first
    assert o0.cost[18] == 7 * 7 + 4 * 5 and [float(v) for v in o0.path[18, :4, 2]] == [0.0] * 4 and o0.path[18, 4, 2] == geo.HEADINGS[4]
    assert [float(o0.path[q, 0, 2]) for q in (22, 23, 24, 25)] == [geo.HEADINGS[m] for m in (4, 6, 5, 7)]
    # wall: cut off until the margin reaches the gap, then the detour; the diagonal wall is never passed; the corner costs 10
    w0, w11, w12 = (scn.answer("wall_m%d" % m) for m in (0, 11, 12))
    assert w0.status[:3].tolist() == [CUT] * 3 and w11.status[:3].tolist() == [CUT] * 3 and w12.status[:3].tolist() == [CUT, OK, OK]
    assert w12.cost[1] > 2 * 5 * 12 and w12.cost[1] == w12.cost[2]
    for w in (w0, w11, w12):
        assert w.status[3:6].tolist() == [CUT] * 3 and w.cost[6] == w.cost[7] == 10 and w.status[9] == OK
    assert w0.status[8] == CUT and w11.status[8] == OK and w11.cost[8] == 4 * 5, "row 19 alone ends at the wall; round its end in row 20 without cutting the corner"
    assert w0.state.tolist() == [3, 0, 7, 0] and w12.state.tolist() == [6, 0, 4, 0]
    # serpentine: the path is many times the window's side
    s0, s2 = scn.answer("serpentine_m0"), scn.answer("serpentine_m2")
    assert s0.status.tolist() == [OK, OK, CUT, CUT, CUT] and s2.status.tolist() == [OK, OK, CUT, CUT, CUT]
    assert s0.cost[0] > 5 * 6 * 31 and s0.length[0] > 6 * 31 and s0.cost[0] == s0.cost[1]
    # waivers
    wp, wb = scn.answer("waivers_pass"), scn.answer("waivers_block")
    sc = scn.scene("waivers_block")
    assert wp.status[0] == OK and wp.cost[0] == 45 and wb.status[0] == CUT
    assert wb.status[1:5].tolist() == [OK] * 4 and wb.cost[1:5].tolist() == [25, 25, 20, 0]
    assert wb.status[5:9].tolist() == [OK] * 4 and wb.cost[7] == 5 and wb.status[9] == CUT
    # the 80 cell blocks and puts its four neighbours, the 79 cell among them, into the band: round it in 4 moves; from band cell
    # to band cell (both waived) in 6; out of the 79 cell in one
    assert wb.status[10:13].tolist() == [OK] * 3 and wb.cost[10:13].tolist() == [20, 30, 5] and wp.cost[3] == 10
    assert wb.status[13:17].tolist() == [NG, NG, NR, NR] and wb.status[17:21].tolist() == [NG] * 4
    assert wb.status[21] == NR and (wb.status[22:26] != NR).all(), "a NaN or a huge coordinate is cell 0 in the x86 conversion"
    assert wb.status[26] == OK and wb.status[27] == np.int32(scn.UNTOUCHED[1]) and sc.mask[27] == 0 and sc.mask[3] == 7
    assert wb.state.sum() == len(sc.poses) - 1
    # cap
    c0, c50, cmax = scn.answer("cap_m0"), scn.answer("cap_m50"), scn.answer("cap_mmax")
    assert c0.status.tolist() == [OK, WIN, WIN, OK, OK] and shape(c0.windows[0]) == (128, 128) and c0.cost[0] == 7 * 127
    assert shape(c0.windows[3]) == (128, 128) and shape(c0.windows[4]) == (1, 130)
    assert c50.status.tolist() == [OK, WIN, OK] and shape(c50.windows[0]) == (111, 111) and 161 * 161 > gr.MAX_CELLS
    assert cmax.status.tolist() == [WIN] and shape(cmax.windows[0]) == (130, 130)
    # many and stride: past the workgroups of the largest launch; every status but WINDOW among many
    m, s = scn.answer("many"), scn.answer("stride")
    assert len(m.cost) == 3000 > scn.MAX_BLOCKS and len(s.cost) == 5000 > 2 * scn.MAX_BLOCKS
    assert all((m.status == k).sum() > 10 for k in (OK, NR, NG, CUT)) and (scn.scene("many").mask == 0).sum() > 100
    assert max(shape(w)[0] * shape(w)[1] for w in m.windows if w is not None) > 1500
    assert all(w is None or max(shape(w)) <= 3 for w in s.windows) and (s.status == OK).sum() > 2000 and (s.status == CUT).sum() > 10


# ---- the entry ---------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    raw = C.CDLL(capi.LIB_PATH)
    L = capi.lib()
    for name, n_args in ENTRIES.items():
        assert name in capi.declared_symbols() and hasattr(raw, name), name
        assert len(getattr(L, name).argtypes) == n_args, name
    assert callable(capi.geodesic_goto_batch)
    assert capi.GOTO_MAX_CELLS == gr.MAX_CELLS == 16384
    assert (capi.GOTO_OK, capi.GOTO_NO_ROBOT, capi.GOTO_NO_GOAL, capi.GOTO_WINDOW, capi.GOTO_CUT_OFF) == (gr.OK, gr.NO_ROBOT, gr.NO_GOAL, gr.WINDOW, gr.CUT_OFF)
    with open(capi.HEADER_PATH) as f:
        text = f.read()
    assert "#define EEA_GOTO_MAX_CELLS 16384" in text
    assert "EEA_GOTO_OK = 0, EEA_GOTO_NO_ROBOT = 1, EEA_GOTO_NO_GOAL = 2, EEA_GOTO_WINDOW = 3, EEA_GOTO_CUT_OFF = 4" in text
    assert L.eea_abi_version() == 6


def test_argument_errors_come_before_the_device():
    """every refusal of the header is answered without a device: the buffers are host arrays that hold a sentinel nothing may
    touch"""
    L = capi.lib()
    xs, ys, P, n_steps = 40, 30, 3, 5
    good = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 0.8)
    grid = np.zeros(xs * ys, dtype=np.int8)
    sq = np.full((ys, xs), 7, dtype=np.int32)
    pose, path = np.full((P, 3), 7.0), np.full((P, n_steps, 3), 7.0)
    goal, mask, cost, status, length = (np.full(P, 7, dtype=np.int32) for _ in range(5))
    state = np.full(4, 7, dtype=np.uint32)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    ref = lambda c: None if c is None else C.byref(c)
    INV, UNS = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED

    def call(cfg=good, g=grid, s=sq, clear_sq=0, flags=0, ps=pose, gl=goal, mk=mask, P_=P, margin=2, steps=n_steps, co=cost, stt=status,
             pt=path, ln=length, st=state):
        return L.eea_geodesic_goto_batch(0, ref(cfg), p(g), p(s), clear_sq, flags, p(ps), p(gl), p(mk), P_, margin, steps, p(co), p(stt),
                                         p(pt), p(ln), p(st), None)

    assert call(cfg=None) == INV
    for kw in (dict(g=None), dict(co=None), dict(stt=None), dict(st=None)):
        assert call(**kw) == INV and b"null" in L.eea_last_error(), kw
    for kw in (dict(ps=None), dict(gl=None), dict(ps=None, gl=None)):
        assert call(**kw) == INV and b"d_pose or d_goal" in L.eea_last_error(), kw
    assert call(pt=None) == INV and b"d_path" in L.eea_last_error()
    assert call(clear_sq=-1) == INV and b"clear_sq" in L.eea_last_error()
    for flags in (2, 3, 4, 1 << 31):
        assert call(flags=flags) == INV and b"flag" in L.eea_last_error(), flags
    assert call(P_=1 << 31) == UNS and b"2^31 - 1" in L.eea_last_error()
    assert call(P_=0xFFFFFFFF) == UNS
    # ... with the optional buffers absent and every margin, too
    assert call(clear_sq=-1, s=None, mk=None, ln=None, margin=0xFFFFFFFF) == INV
    assert call(pt=None, steps=1, ln=None) == INV
    # the configuration errors and the limits of the geodesic calls
    swapped = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 1.0, 0.7, 0.2, 0.8)
    assert call(cfg=swapped) == INV and b"Search radius" in L.eea_last_error()
    for bad in (capi.make_collision_cfg(-2.0, -1.0, 0.1, 0, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, 0, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.0, xs, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 100.5)):
        assert call(cfg=bad) == INV
    side = capi.DISTANCE_MAX_SIDE
    for big in (capi.make_collision_cfg(-2.0, -1.0, 0.1, side + 1, 4, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, 4, side + 1, 0.7, 1.0, 0.2, 0.8)):
        assert call(cfg=big) == UNS and b"EEA_DISTANCE_MAX_SIDE" in L.eea_last_error()
    for a, v in ((sq, 7), (pose, 7.0), (goal, 7), (mask, 7), (cost, 7), (status, 7), (length, 7), (path, 7.0), (state, 7)):
        assert (a == v).all()
    assert not grid.any()


def test_the_goto_kernel_is_in_the_library_without_scratch():
    """the kernels of csrc/goto_kernel.hip are gfx950 code in the build and use no scratch; the window is dynamic LDS, so the
    static part is a few words; few enough registers for eight wavefronts per SIMD (the LDS, not the registers, bounds the
    workgroups per CU)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    obj = os.path.join(os.path.dirname(capi.LIB_PATH), "..", "csrc", "build", "goto_kernel.o")
    names = {}
    for k in kr.kernels(obj):
        if "vgpr_count" in k:
            names[subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.strip()] = k
    for w in ("goto_state_kernel(", "goto_kernel("):
        found = [k for n, k in names.items() if w in n]
        assert len(found) == 1, (w, sorted(names))
        assert int(found[0]["private_segment_fixed_size"]) == 0, found[0]
    main = [k for n, k in names.items() if "goto_kernel(" in n][0]
    assert int(main["group_segment_fixed_size"]) <= 1024 and int(main["vgpr_count"]) <= 64, main

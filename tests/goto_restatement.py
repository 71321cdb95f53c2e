"""eea_geodesic_goto_batch (include/ergodic_amd.h) restated in numpy and heapq, for tests/test_goto.py (CPU) and
tests/test_gpu_goto.py.  Independent of the library: the definition only -- the robot's cell, the goal, the window in whole
numbers and its clipping, Dijkstra on the graph of the window's cells with the goal as the one source and the robot's cell
enterable, the walk with its move order, and the way-point arithmetic on the whole grid's indices."""
import collections
import heapq

import numpy as np

from tests import geodesic_restatement as geo
from tests import sense_restatement as sr

MAX_CELLS = 16384
OK, NO_ROBOT, NO_GOAL, WINDOW, CUT_OFF = range(5)
MOVES, COSTS, HEADINGS = geo.MOVES, geo.COSTS, geo.HEADINGS

Result = collections.namedtuple("Result", "cost status path length state windows")


def window(g, ci, cj, gi, gj, margin):
    """(i0, i1, j0, j1), both ends included: the box of the two cells grown by margin, clipped to the grid (Python's integers)"""
    i0, i1 = max(min(ci, gi) - margin, 0), min(max(ci, gi) + margin, g.ysize - 1)
    j0, j1 = max(min(cj, gj) - margin, 0), min(max(cj, gj) + margin, g.xsize - 1)
    return i0, i1, j0, j1


def window_field(ok, si, sj):
    """dict (i, j) -> cost on the cells of the bool array `ok` (a move may enter the cell) from the source (si, sj): Dijkstra; a
    move goes into an enterable cell of the array, a diagonal one between two enterable cells"""
    h, w = ok.shape
    ok = ok.tolist()
    best = {(si, sj): 0}
    done = {}
    heap = [(0, si, sj)]
    while heap:
        d, i, j = heapq.heappop(heap)
        if (i, j) in done:
            continue
        done[(i, j)] = d
        for (di, dj), c in zip(MOVES, COSTS):
            ni, nj = i + di, j + dj
            if not (0 <= ni < h and 0 <= nj < w) or not ok[ni][nj]:
                continue
            if di != 0 and dj != 0 and not (ok[ni][j] and ok[i][nj]):
                continue
            if d + c < best.get((ni, nj), 1 << 62):
                best[(ni, nj)] = d + c
                heapq.heappush(heap, (d + c, ni, nj))
    return done


def walk(cost, i, j, n_steps):
    """[(ni, nj, k), ...], at most n_steps: from (i, j) the first of the eight moves onto a cell that accounts for the cost, a
    diagonal one only between two cells that have a cost"""
    out = []
    while cost[(i, j)] > 0 and len(out) < n_steps:
        for k, ((di, dj), c) in enumerate(zip(MOVES, COSTS)):
            n = cost.get((i + di, j + dj))
            if n is None or n + c != cost[(i, j)]:
                continue
            if k >= 4 and ((i + di, j) not in cost or (i, j + dj) not in cost):
                continue
            i, j = i + di, j + dj
            out.append((i, j, k))
            break
        else:
            raise AssertionError("a final field has a step from every cell with a cost")
    return out


def goto(g, grid, poses, goals, margin, n_steps, sq=None, clear_sq=0, flags=0, mask=None, untouched=(0, 0, 0.0, 0)):
    """Result of one call: cost, status, length int32 [P], path float64 [P][n_steps][3], state uint32 [4], and per robot the
    window (i0, i1, j0, j1) or None.  A masked-out robot's elements hold `untouched` (cost, status, path, length)"""
    grid = np.asarray(grid, dtype=np.int8).reshape(g.ysize, g.xsize)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    P = len(poses)
    trav = geo.traversable(g, grid, sq, clear_sq, flags)
    cost = np.full(P, untouched[0], dtype=np.int32)
    status = np.full(P, untouched[1], dtype=np.int32)
    path = np.full((P, n_steps, 3), untouched[2], dtype=np.float64)
    length = np.full(P, untouched[3], dtype=np.int32)
    state = np.zeros(4, dtype=np.uint32)
    windows = [None] * P
    for q, p in enumerate(poses):
        if mask is not None and mask[q] == 0:
            continue
        cost[q] = length[q] = -1
        path[q, :] = p
        ci, cj = sr.world2grid(g, p[0], p[1])
        if not (ci <= g.ysize - 1 and cj <= g.xsize - 1) or sr.blocks(int(grid[ci, cj]), g.occupied_threshold):
            status[q] = NO_ROBOT
            state[3] += 1
            continue
        k = int(goals[q])
        if k < 0 or k >= g.xsize * g.ysize or sr.blocks(int(grid.flat[k]), g.occupied_threshold):
            status[q] = NO_GOAL
            state[3] += 1
            continue
        gi, gj = divmod(k, g.xsize)
        i0, i1, j0, j1 = windows[q] = window(g, ci, cj, gi, gj, int(margin))
        if (i1 - i0 + 1) * (j1 - j0 + 1) > MAX_CELLS:
            status[q] = WINDOW
            state[1] += 1
            continue
        ok = trav[i0:i1 + 1, j0:j1 + 1].copy()
        ok[ci - i0, cj - j0] = True
        field = window_field(ok, gi - i0, gj - j0)
        if (ci - i0, cj - j0) not in field:
            status[q] = CUT_OFF
            state[2] += 1
            continue
        status[q] = OK
        state[0] += 1
        cost[q] = field[(ci - i0, cj - j0)]
        steps = walk(field, ci - i0, cj - j0, n_steps)
        last = geo.cell_centre(g, ci, cj) + (p[2],)
        for t in range(n_steps):
            if t < len(steps):
                last = geo.cell_centre(g, steps[t][0] + i0, steps[t][1] + j0) + (HEADINGS[steps[t][2]],)
            path[q, t] = last
        length[q] = len(steps)
    return Result(cost, status, path, length, state, windows)

"""eea_geodesic_field / eea_geodesic_path_batch / the value grid of eea_set_target_reachable (include/ergodic_amd.h) restated in
numpy and heapq, for tests/test_geodesic.py (CPU) and tests/test_gpu_geodesic.py.  Independent of the library: the
definitions only -- the traversable test, the waived sources, the corner rule, the path rule with its move order and the
way-point arithmetic.  tile_rounds() is a model of the device's schedule (tiles relaxed round by round from a stale halo),
which tests/test_geodesic.py holds to the same bits."""
import heapq
import math

import numpy as np

from tests import sense_restatement as sr

UNKNOWN_BLOCKS, CONTINUE = 1, 2
# the eight moves (di, dj) in the order the path tries them, their costs and headings (atan2(di, dj) as k pi / 4 in [-pi, pi))
MOVES = ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, -1), (-1, 1))
COSTS = (5, 5, 5, 5, 7, 7, 7, 7)
HEADINGS = (0.0, 1.5707963267948966, -3.141592653589793, -1.5707963267948966, 0.7853981633974483, 2.356194490192345,
            -2.356194490192345, -0.7853981633974483)


def traversable(g, grid, sq=None, clear_sq=0, flags=0):
    """bool [ysize][xsize]: a move may enter the cell"""
    grid = np.asarray(grid, dtype=np.int8).reshape(g.ysize, g.xsize)
    ok = grid.astype(np.float64) / 100.0 < g.occupied_threshold          # !blocks
    if flags & UNKNOWN_BLOCKS:
        ok &= grid >= 0
    if sq is not None:
        sq = np.asarray(sq).reshape(g.ysize, g.xsize)
        ok &= (sq == -1) | (sq > clear_sq)
    return ok


def source_cells(g, grid, poses=None, cells=None):
    """the accepted sources, one (i, j) per accepted entry of the two lists (poses first): on the grid and not blocking"""
    grid = np.asarray(grid, dtype=np.int8).reshape(g.ysize, g.xsize)
    out = []
    for p in ([] if poses is None else np.asarray(poses, dtype=np.float64).reshape(-1, 3)):
        i, j = sr.world2grid(g, p[0], p[1])
        if i <= g.ysize - 1 and j <= g.xsize - 1:                          # gridBounds
            out.append((i, j))
    for k in ([] if cells is None else np.asarray(cells).reshape(-1).tolist()):
        if 0 <= k < g.xsize * g.ysize:
            out.append((k // g.xsize, k % g.xsize))
    return [(i, j) for i, j in out if not sr.blocks(int(grid[i, j]), g.occupied_threshold)]


def _moves_into(trav, i, j):
    """(ni, nj, cost) of the moves that may be made FROM (i, j): into a traversable cell, a diagonal between traversable cells"""
    ys, xs = len(trav), len(trav[0])
    for (di, dj), w in zip(MOVES, COSTS):
        ni, nj = i + di, j + dj
        if not (0 <= ni < ys and 0 <= nj < xs) or not trav[ni][nj]:
            continue
        if di != 0 and dj != 0 and not (trav[i + di][j] and trav[i][j + dj]):
            continue
        yield ni, nj, w


def field(g, grid, poses=None, cells=None, sq=None, clear_sq=0, flags=0):
    """(geo int32 [ysize][xsize], number of accepted sources): Dijkstra from the accepted sources"""
    trav = traversable(g, grid, sq, clear_sq, flags).tolist()
    src = source_cells(g, grid, poses, cells)
    geo = np.full((g.ysize, g.xsize), -1, dtype=np.int32)
    best = {}
    heap = []
    for c in set(src):
        best[c] = 0
        heap.append((0, c))
    heapq.heapify(heap)
    while heap:
        d, (i, j) = heapq.heappop(heap)
        if d != best[(i, j)]:
            continue
        geo[i, j] = d
        for ni, nj, w in _moves_into(trav, i, j):
            if d + w < best.get((ni, nj), 1 << 62):
                best[(ni, nj)] = d + w
                heapq.heappush(heap, (d + w, (ni, nj)))
    return geo, len(src)


def cell_centre(g, i, j):
    """grid2World's arithmetic, every operation rounded on its own"""
    return float(j) * g.resolution + g.resolution / 2.0 + g.xmin, float(i) * g.resolution + g.resolution / 2.0 + g.ymin


def path_cells(geo, i, j, n_steps):
    """the cells and move indices of the descent from (i, j): [(ni, nj, k), ...], at most n_steps of them"""
    ys, xs = geo.shape
    at = lambda a, b: int(geo[a, b]) if (0 <= a < ys and 0 <= b < xs) else -1
    out = []
    while at(i, j) > 0 and len(out) < n_steps:
        for k, ((di, dj), w) in enumerate(zip(MOVES, COSTS)):
            n = at(i + di, j + dj)
            if n < 0 or n + w != at(i, j):
                continue
            if k >= 4 and (at(i + di, j) < 0 or at(i, j + dj) < 0):
                continue
            i, j = i + di, j + dj
            out.append((i, j, k))
            break
        else:
            break                                                          # (a field that is not final: the walk ends)
    return out


def path(g, geo, poses, n_steps):
    """(path float64 [P][n_steps][3], len int32 [P]) of eea_geodesic_path_batch"""
    geo = np.asarray(geo, dtype=np.int32).reshape(g.ysize, g.xsize)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((len(poses), n_steps, 3))
    lens = np.zeros(len(poses), dtype=np.int32)
    for q, p in enumerate(poses):
        i, j = sr.world2grid(g, p[0], p[1])
        if not (i <= g.ysize - 1 and j <= g.xsize - 1) or geo[i, j] < 0:
            out[q, :] = p
            lens[q] = -1
            continue
        steps = path_cells(geo, i, j, n_steps)
        last = cell_centre(g, i, j) + (p[2],)
        for t in range(n_steps):
            if t < len(steps):
                last = cell_centre(g, steps[t][0], steps[t][1]) + (HEADINGS[steps[t][2]],)
            out[q, t] = last
        lens[q] = len(steps)
    return out, lens


def legal_move(trav, geo, a, b):
    """is a -> b (cells) one of the eight moves, into a traversable or source cell, a diagonal between such cells"""
    ok = lambda c: bool(trav[c[0]][c[1]]) or geo[c[0], c[1]] == 0
    di, dj = b[0] - a[0], b[1] - a[1]
    if (di, dj) not in MOVES or not ok(b):
        return False
    return di == 0 or dj == 0 or (ok((a[0] + di, a[1])) and ok((a[0], a[1] + dj)))


def reachable_values(g, stride, known, fieldv, geo, floor, dtype=np.float64):
    """v[i][j] = (real)((double)field[i][j] + floor) on the candidates whose cell does not block and has geo >= 0, 0 elsewhere"""
    known = np.asarray(known, dtype=np.int8).reshape(g.ysize, g.xsize)
    cand = np.zeros((g.ysize, g.xsize), dtype=bool)
    cand[::stride, ::stride] = True
    cand &= known.astype(np.float64) / 100.0 < g.occupied_threshold
    cand &= np.asarray(geo).reshape(g.ysize, g.xsize) >= 0
    v = np.where(cand, np.asarray(fieldv, dtype=np.float64).reshape(g.ysize, g.xsize) + np.float64(floor), 0.0)
    return v.astype(dtype)


def bellman_ford(g, grid, poses=None, cells=None, sq=None, clear_sq=0, flags=0):
    """a second statement of the field: whole-grid relaxation `geo[c] = min over moves n -> c of geo[n] + cost` to a fixed point"""
    trav = traversable(g, grid, sq, clear_sq, flags)
    INF = 1 << 40
    d = np.full((g.ysize, g.xsize), INF, dtype=np.int64)
    for i, j in source_cells(g, grid, poses, cells):
        d[i, j] = 0
    while True:
        new = d.copy()
        for i in range(g.ysize):
            for j in range(g.xsize):
                if not trav[i, j]:
                    continue
                for (di, dj), w in zip(MOVES, COSTS):
                    a, b = i - di, j - dj                                   # the move comes from (a, b)
                    if not (0 <= a < g.ysize and 0 <= b < g.xsize) or d[a, b] >= INF:
                        continue
                    if di != 0 and dj != 0 and not (trav[a + di, b] and trav[a, b + dj]):
                        continue
                    new[i, j] = min(new[i, j], d[a, b] + w)
        if np.array_equal(new, d):
            break
        d = new
    return np.where(d >= INF, -1, d).astype(np.int32)


def tile_rounds(g, grid, tx, ty, poses=None, cells=None, sq=None, clear_sq=0, flags=0, start=None, max_rounds=None):
    """A model of the device's schedule: (geo, final, rounds that changed something).  Tiles of ty x tx cells; in a round every
    pending tile is relaxed to its own fixed point reading the field AS IT STOOD BEFORE THE ROUND outside itself (the most stale
    halo a workgroup can see), and marks the neighbouring tiles whose halo holds a cell it lowered for the next round."""
    trav = traversable(g, grid, sq, clear_sq, flags)
    INF = 1 << 40
    d = np.full((g.ysize, g.xsize), INF, dtype=np.int64)
    if start is not None:
        start = np.asarray(start, dtype=np.int64).reshape(g.ysize, g.xsize)
        d = np.where(start < 0, INF, start)
    for i, j in source_cells(g, grid, poses, cells):
        d[i, j] = 0
    nty, ntx = (g.ysize - 1) // ty + 1, (g.xsize - 1) // tx + 1
    pending = {(a, b) for a in range(nty) for b in range(ntx)}
    changed_rounds, r = 0, 0
    while pending and (max_rounds is None or r < max_rounds):
        before, nxt, any_change = d.copy(), set(), False
        for a, b in sorted(pending):
            i0, i1, j0, j1 = a * ty, min((a + 1) * ty, g.ysize), b * tx, min((b + 1) * tx, g.xsize)
            lowered = set()
            while True:
                again = False
                for i in range(i0, i1):
                    for j in range(j0, j1):
                        if not trav[i, j]:
                            continue
                        for (di, dj), w in zip(MOVES, COSTS):
                            p, q = i - di, j - dj
                            if not (0 <= p < g.ysize and 0 <= q < g.xsize):
                                continue
                            if di != 0 and dj != 0 and not (trav[p + di, q] and trav[p, q + dj]):
                                continue
                            src = d[p, q] if (i0 <= p < i1 and j0 <= q < j1) else before[p, q]
                            if src < INF and src + w < d[i, j]:
                                d[i, j] = src + w
                                lowered.add((i, j))
                                again = True
                if not again:
                    break
            any_change |= bool(lowered)
            for i, j in lowered:
                for da in (-1, 0, 1):
                    for db in (-1, 0, 1):
                        if (da, db) == (0, 0):
                            continue
                        if (da == -1 and i != i0) or (da == 1 and i != a * ty + ty - 1) or (db == -1 and j != j0) or \
                           (db == 1 and j != b * tx + tx - 1):
                            continue
                        if 0 <= a + da < nty and 0 <= b + db < ntx:
                            nxt.add((a + da, b + db))
        changed_rounds += 1 if any_change else 0
        pending, r = nxt, r + 1
    return np.where(d >= INF, -1, d).astype(np.int32), not pending, changed_rounds


def serpentine(xs, ys, gap=1, pitch=4):
    """int8 [ysize][xsize]: vertical walls every `pitch` columns, each open for `gap` cells at alternating ends: the shortest
    path from the left to the right runs the grid's height between every two walls"""
    grid = np.zeros((ys, xs), dtype=np.int8)
    for n, j in enumerate(range(pitch - 1, xs - 1, pitch)):
        grid[:, j] = 100
        if n % 2 == 0:
            grid[ys - gap:, j] = 0
        else:
            grid[:gap, j] = 0
    return grid

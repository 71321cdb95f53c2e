"""eea_geodesic_partition / eea_partition_goals / eea_partition_path_batch (include/ergodic_amd.h) restated in numpy and heapq,
for tests/test_partition.py (CPU) and tests/test_gpu_partition.py.  Independent of the library: the definitions only -- labels,
the (cost, label) key, the candidates and their score, the owner-constrained descent and the reversed way-points.  The grid, the
traversable set, the moves and the accepted sources are tests/geodesic_restatement.py's.  tile_rounds() is a model of the
device's schedule on keys, which tests/test_partition.py holds to the same bits."""
import heapq

import numpy as np

from tests import geodesic_restatement as geo
from tests import sense_restatement as sr

MOVES, COSTS, HEADINGS = geo.MOVES, geo.COSTS, geo.HEADINGS
OPPOSITE = (2, 3, 0, 1, 6, 7, 4, 5)          # the move that undoes move k
NONE = (1 << 64) - 1                          # the key of a cell without a move sequence


def labelled_sources(g, grid, poses=None, cells=None):
    """[(label, (i, j)), ...] of the accepted entries: pose q has label q, cell k has label P + k; on the grid, not blocking"""
    grid = np.asarray(grid, dtype=np.int8).reshape(g.ysize, g.xsize)
    poses = np.zeros((0, 3)) if poses is None else np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    out = []
    for q, p in enumerate(poses):
        i, j = sr.world2grid(g, p[0], p[1])
        if i <= g.ysize - 1 and j <= g.xsize - 1:
            out.append((q, (i, j)))
    for n, k in enumerate([] if cells is None else np.asarray(cells).reshape(-1).tolist()):
        if 0 <= k < g.xsize * g.ysize:
            out.append((len(poses) + n, (k // g.xsize, k % g.xsize)))
    return [(s, c) for s, c in out if not sr.blocks(int(grid[c]), g.occupied_threshold)]


def _planes(keys):
    keys = np.asarray(keys, dtype=object)
    none = keys == NONE
    geo_plane = np.where(none, -1, keys // (1 << 32)).astype(np.int64).astype(np.int32)
    owner = np.where(none, -1, keys % (1 << 32)).astype(np.int64).astype(np.int32)
    return geo_plane, owner


def partition(g, grid, poses=None, cells=None, sq=None, clear_sq=0, flags=0):
    """(geo int32, owner int32 [ysize][xsize], accepted sources): Dijkstra over (cost, label) keys"""
    trav = geo.traversable(g, grid, sq, clear_sq, flags).tolist()
    src = labelled_sources(g, grid, poses, cells)
    best, heap = {}, []
    for s, c in src:
        if (0, s) < best.get(c, (1 << 62, 0)):
            best[c] = (0, s)
    for c, k in best.items():
        heap.append((k, c))
    heapq.heapify(heap)
    geo_plane = np.full((g.ysize, g.xsize), -1, dtype=np.int32)
    owner = np.full((g.ysize, g.xsize), -1, dtype=np.int32)
    while heap:
        k, (i, j) = heapq.heappop(heap)
        if k != best[(i, j)]:
            continue
        geo_plane[i, j], owner[i, j] = k
        for ni, nj, w in geo._moves_into(trav, i, j):
            cand = (k[0] + w, k[1])
            if cand < best.get((ni, nj), (1 << 62, 0)):
                best[(ni, nj)] = cand
                heapq.heappush(heap, (cand, (ni, nj)))
    return geo_plane, owner, len(src)


def by_single_sources(g, grid, poses=None, cells=None, sq=None, clear_sq=0, flags=0):
    """a second statement: one field of geodesic_restatement.field per accepted source; the cost is the least of them and the
    owner the smallest label among the sources at that cost"""
    poses = np.zeros((0, 3)) if poses is None else np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    big = np.iinfo(np.int64).max
    cost = np.full((g.ysize, g.xsize), big, dtype=np.int64)
    owner = np.full((g.ysize, g.xsize), -1, dtype=np.int32)
    for s, (i, j) in sorted(labelled_sources(g, grid, poses, cells)):
        one, n = geo.field(g, grid, cells=np.array([i * g.xsize + j], dtype=np.int32), sq=sq, clear_sq=clear_sq, flags=flags)
        assert n == 1
        d = np.where(one < 0, big, one.astype(np.int64))
        lower = d < cost                                                    # (labels rise: a tie keeps the smaller one)
        cost[lower], owner[lower] = d[lower], s
    return np.where(cost == big, -1, cost).astype(np.int32), owner


def tile_rounds(g, grid, tx, ty, poses=None, cells=None, sq=None, clear_sq=0, flags=0, start=None, max_rounds=None):
    """geodesic_restatement.tile_rounds on keys: (geo, owner, final, rounds that changed something).  start: (geo, owner) planes
    the keys are rebuilt from (EEA_GEODESIC_CONTINUE).  In a round every pending tile is relaxed to its own fixed point reading
    the keys AS THEY STOOD BEFORE THE ROUND outside itself -- whole keys, never a cost of one time with a label of another"""
    trav = geo.traversable(g, grid, sq, clear_sq, flags)
    d = np.full((g.ysize, g.xsize), NONE, dtype=object)
    if start is not None:
        s_geo, s_owner = (np.asarray(a).reshape(g.ysize, g.xsize) for a in start)
        for i in range(g.ysize):
            for j in range(g.xsize):
                if s_geo[i, j] >= 0:
                    d[i, j] = (int(s_geo[i, j]) << 32) | (int(s_owner[i, j]) & 0xFFFFFFFF)
    for s, c in labelled_sources(g, grid, poses, cells):
        d[c] = min(d[c], s)
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
                            if src != NONE and src + (w << 32) < d[i, j]:
                                d[i, j] = src + (w << 32)
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
    return _planes(d) + (not pending, changed_rounds)


def descend(geo_plane, owner, i, j):
    """the owner-constrained descent from (i, j): [(ni, nj, k), ...] down to a geo == 0 cell, or None when some cell has no step"""
    ys, xs = geo_plane.shape
    at = lambda a, b: int(geo_plane[a, b]) if (0 <= a < ys and 0 <= b < xs) else -1
    label, out = int(owner[i, j]), []
    while at(i, j) > 0:
        for k, ((di, dj), w) in enumerate(zip(MOVES, COSTS)):
            n = at(i + di, j + dj)
            if n < 0 or n + w != at(i, j) or int(owner[i + di, j + dj]) != label:
                continue
            if k >= 4 and (at(i + di, j) < 0 or at(i, j + dj) < 0):
                continue
            i, j = i + di, j + dj
            out.append((i, j, k))
            break
        else:
            return None
    return out


def goals(g, fieldv, stride, known, geo_plane, owner, n_labels, w_field, w_cost):
    """(goal_cell int32 [n], goal_score float64 [n], area uint32 [n]) by brute force over the cells in row-major order"""
    known = np.asarray(known, dtype=np.int8).reshape(-1)
    fieldv, geo_plane, owner = (np.asarray(a).reshape(-1) for a in (fieldv, geo_plane, owner))
    cell = np.full(n_labels, -1, dtype=np.int32)
    score = np.zeros(n_labels, dtype=np.float64)
    area = np.zeros(n_labels, dtype=np.uint32)
    wf, wc = np.float64(w_field), np.float64(w_cost)
    for c in range(g.xsize * g.ysize):
        r = int(owner[c])
        if not 0 <= r < n_labels:
            continue
        area[r] += 1
        if (c % g.xsize) % stride or (c // g.xsize) % stride or sr.blocks(int(known[c]), g.occupied_threshold) or not fieldv[c] > 0:
            continue
        s = wf * np.float64(fieldv[c]) - wc * np.float64(int(geo_plane[c]))
        if cell[r] < 0 or s > score[r]:
            cell[r], score[r] = c, s
    return cell, score, area


def paths(g, geo_plane, owner, poses, goal_cell, n_steps):
    """(path float64 [P][n_steps][3], len int32 [P]) of eea_partition_path_batch"""
    geo_plane = np.asarray(geo_plane, dtype=np.int32).reshape(g.ysize, g.xsize)
    owner = np.asarray(owner, dtype=np.int32).reshape(g.ysize, g.xsize)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((len(poses), n_steps, 3))
    lens = np.zeros(len(poses), dtype=np.int32)
    for q, p in enumerate(poses):
        i, j = sr.world2grid(g, p[0], p[1])
        goal = int(goal_cell[q])
        steps = None
        if i <= g.ysize - 1 and j <= g.xsize - 1 and 0 <= goal < g.xsize * g.ysize:
            gi, gj = goal // g.xsize, goal % g.xsize
            if owner[gi, gj] == q and geo_plane[gi, gj] >= 0:
                steps = descend(geo_plane, owner, gi, gj)
                end = (steps[-1][0], steps[-1][1]) if steps else (gi, gj)
                if steps is not None and end != (i, j):
                    steps = None
        if steps is None:
            out[q, :] = p
            lens[q] = -1
            continue
        # the cells reversed: c_0 = (i, j) .. c_m = the goal; way-point k is c_{k+1} with the heading of the move into it
        cells = [(gi, gj)] + [(a, b) for a, b, _ in steps]
        m = len(steps)
        way = [geo.cell_centre(g, *cells[m - k - 1]) + (HEADINGS[OPPOSITE[steps[m - k - 1][2]]],) for k in range(m)]
        last = geo.cell_centre(g, i, j) + (p[2],)
        for t in range(n_steps):
            if t < m:
                last = way[t]
            elif m:
                last = way[m - 1]
            out[q, t] = last
        lens[q] = min(m, n_steps)
    return out, lens

"""eea_frontier_auction (include/ergodic_amd.h) restated in numpy and heapq, for tests/test_auction.py (CPU),
tests/test_gpu_auction.py and tools/auction_cost.py.  Independent of the library: the definition only -- placed robots and their
waived cells, capacities, the seeds of a round, the (cost, label) field on the enterable cells, bids, acceptance by (cost, robot)
and the forward walk with eea_geodesic_path_batch's rows.  The traversable set, the moves and the way-point arithmetic are
tests/geodesic_restatement.py's, the owner-constrained step is tests/partition_restatement.py's."""
import collections
import heapq

import numpy as np

from tests import geodesic_restatement as geo
from tests import partition_restatement as part
from tests import sense_restatement as sr

Result = collections.namedtuple("Result", "goal_region goal_cell goal_cost path length state assigned_in bids")


def robot_cells(g, grid, poses):
    """per robot its cell (i, j), or None where it is not placed: off the grid, or on a blocking cell"""
    grid = np.asarray(grid, dtype=np.int8).reshape(g.ysize, g.xsize)
    out = []
    for p in np.asarray(poses, dtype=np.float64).reshape(-1, 3):
        i, j = sr.world2grid(g, p[0], p[1])
        ok = i <= g.ysize - 1 and j <= g.xsize - 1 and not sr.blocks(int(grid[i, j]), g.occupied_threshold)
        out.append((i, j) if ok else None)
    return out


def enterable(g, grid, poses, sq=None, clear_sq=0, flags=0):
    """bool [ysize][xsize]: traversable as the geodesic field has it, or the cell of a placed robot"""
    ok = geo.traversable(g, grid, sq, clear_sq, flags).copy()
    for c in robot_cells(g, grid, poses):
        if c is not None:
            ok[c] = True
    return ok


def capacities(rec, fstate, max_regions, min_size, cells_per_robot):
    """cap_r per record slot r < max_regions: 0 where r is not eligible"""
    n = min(int(fstate[1]), max_regions)
    cap = [0] * max_regions
    for r in range(n):
        size = int(rec[r]["size"])
        if size >= min_size:
            cap[r] = 1 if cells_per_robot == 0 else (size + cells_per_robot - 1) // cells_per_robot
    return cap


def seeds(g, grid, region, rem):
    """[(r, (i, j)), ...]: the members of the regions with room left that do not block"""
    grid = np.asarray(grid, dtype=np.int8).reshape(g.ysize, g.xsize)
    region = np.asarray(region).reshape(g.ysize, g.xsize)
    out = []
    for i, j in np.argwhere(region >= 0):
        r = int(region[i, j])
        if r < len(rem) and rem[r] > 0 and not sr.blocks(int(grid[i, j]), g.occupied_threshold):
            out.append((r, (int(i), int(j))))
    return out


def field(open_cells, seed_list):
    """(geo, owner int32 [ysize][xsize]) of the keys (cost, label): Dijkstra from the seeds over moves into open cells; a seed
    keeps (0, r) whether it is open or not"""
    ys, xs = open_cells.shape
    trav = open_cells.tolist()
    best = {c: (0, r) for r, c in seed_list}
    heap = [(k, c) for c, k in best.items()]
    heapq.heapify(heap)
    cost = np.full((ys, xs), -1, dtype=np.int32)
    owner = np.full((ys, xs), -1, dtype=np.int32)
    while heap:
        k, (i, j) = heapq.heappop(heap)
        if k != best[(i, j)]:
            continue
        cost[i, j], owner[i, j] = k
        for ni, nj, w in geo._moves_into(trav, i, j):
            cand = (k[0] + w, k[1])
            if cand < best.get((ni, nj), (1 << 62, 0)):
                best[(ni, nj)] = cand
                heapq.heappush(heap, (cand, (ni, nj)))
    return cost, owner


def auction(g, grid, region, rec, fstate, max_regions, poses, n_auction=1, min_size=1, cells_per_robot=0, n_steps=0, sq=None,
            clear_sq=0, flags=0):
    """Result of eea_frontier_auction with every field built to the end.  assigned_in [P]: the auction round a robot was accepted
    in, -1 for none; bids: per round that was not idle {robot: (cost, region)}"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    P = len(poses)
    goal_region, goal_cell, goal_cost, length = (np.full(P, -1, dtype=np.int32) for _ in range(4))
    path = np.repeat(poses[:, None, :], n_steps, axis=1).copy()
    assigned_in = np.full(P, -1, dtype=np.int32)
    if P == 0:
        return Result(goal_region, goal_cell, goal_cost, path, length, np.array([1, 0, 0, 0], dtype=np.uint32), assigned_in, [])
    cells = robot_cells(g, grid, poses)
    open_cells = enterable(g, grid, poses, sq, clear_sq, flags)
    rem = capacities(rec, fstate, max_regions, min_size, cells_per_robot)
    bids_of_round = []
    for a in range(n_auction):
        waiting = [q for q in range(P) if cells[q] is not None and goal_region[q] < 0]
        if not waiting or not any(rem):
            break                                                          # idle, and so is every round behind it
        cost, owner = field(open_cells, seeds(g, grid, region, rem))
        bids = {q: (int(cost[cells[q]]), int(owner[cells[q]])) for q in waiting if cost[cells[q]] >= 0}
        bids_of_round.append(bids)
        for r in sorted({b[1] for b in bids.values()}):
            ranked = sorted((b[0], q) for q, b in bids.items() if b[1] == r)
            for d, q in ranked[:rem[r]]:
                steps = part.descend(cost, owner, *cells[q])
                assert steps is not None, "a final field has a step for every cell with a key"
                end = (steps[-1][0], steps[-1][1]) if steps else cells[q]
                goal_region[q], goal_cost[q], goal_cell[q] = r, d, end[0] * g.xsize + end[1]
                last = geo.cell_centre(g, *cells[q]) + (poses[q, 2],)
                for t in range(n_steps):
                    if t < len(steps):
                        last = geo.cell_centre(g, steps[t][0], steps[t][1]) + (geo.HEADINGS[steps[t][2]],)
                    path[q, t] = last
                length[q] = min(len(steps), n_steps)
                assigned_in[q] = a
            rem[r] -= min(rem[r], len(ranked))
    state = np.array([1, 0, int((goal_region >= 0).sum()), len(bids_of_round)], dtype=np.uint32)
    return Result(goal_region, goal_cell, goal_cost, path, length, state, assigned_in, bids_of_round)

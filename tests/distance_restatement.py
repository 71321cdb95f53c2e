"""The exact Euclidean distance transform of a grid's occupied cells (eea_distance_field) and the queries through it
(eea_distance_query_batch, eea_distance_traj_min) restated in numpy, for tests/test_distance_field.py (CPU) and
tests/test_gpu_distance_field.py.

sq (i, j) = the smallest (i - i')^2 + (j - j')^2 over the occupied cells (i', j'), nearest (i, j) = the row-major index of the
cell that attains it, the smallest index among equals; -1 / -1 everywhere when no cell is occupied.  Two forms: all pairs
(brute force, the definition) and an independent separable one for larger grids."""
import numpy as np

from tests import clearance_restatement as cr

CRASH, OBSTACLE, NONE, OFF_GRID = 0, 1, 2, 3
DBL_MAX = cr.DBL_MAX
occupied = cr.occupied


def brute_force(data, threshold):
    """(sq, nearest) int32 [ysize][xsize]: all pairs, key sq * (xsize * ysize) + index, minimum"""
    ys, xs = data.shape
    n = xs * ys
    oi, oj = np.nonzero(occupied(data, threshold))
    sq = np.full((ys, xs), -1, dtype=np.int32)
    nearest = np.full((ys, xs), -1, dtype=np.int32)
    if len(oi) == 0:
        return sq, nearest
    oi, oj = oi.astype(np.int64), oj.astype(np.int64)
    oidx = oi * xs + oj
    jj = np.arange(xs, dtype=np.int64)
    for i in range(ys):          # one row of cells against all occupied cells
        key = ((i - oi[None, :]) ** 2 + (jj[:, None] - oj[None, :]) ** 2) * n + oidx[None, :]
        best = key.min(1)
        sq[i], nearest[i] = best // n, best % n
    return sq, nearest


def separable(data, threshold):
    """the same by two passes: per column the signed row offset to its nearest occupied cell (the smaller row on a tie), then
    per row the minimum over the columns of the key ((j - j')^2 + dy^2) * n + index"""
    ys, xs = data.shape
    n = xs * ys
    occ = occupied(data, threshold)
    sq = np.full((ys, xs), -1, dtype=np.int32)
    nearest = np.full((ys, xs), -1, dtype=np.int32)
    if not occ.any():
        return sq, nearest
    far = 4 * (xs + ys)
    rows = np.arange(ys, dtype=np.int64)[:, None]
    up = np.maximum.accumulate(np.where(occ, rows, -far), axis=0)                      # nearest occupied row at or above
    down = np.minimum.accumulate(np.where(occ, rows, far)[::-1], axis=0)[::-1]         # ... at or below
    near_row = np.where(rows - up <= down - rows, up, down)                            # the smaller row on a tie
    has = occ.any(0)
    jj = np.arange(xs, dtype=np.int64)[None, :]
    big = np.iinfo(np.int64).max
    best = np.full((ys, xs), big, dtype=np.int64)
    for jc in np.nonzero(has)[0]:
        r = near_row[:, jc][:, None]
        key = ((jj - jc) ** 2 + (rows - r) ** 2) * n + (r * xs + jc)
        np.minimum(best, key, out=best)
    return (best // n).astype(np.int32), (best % n).astype(np.int32)


def on_grid(cx, cy, xs, ys):
    """gridBounds (grid.cpp:96-100) of cells given as signed reinterpretations of the unsigned indices"""
    return (cx >= 0) & (cx < xs) & (cy >= 0) & (cy < ys)


def query(res, coll, g, sq, nearest, poses):
    """(out int32 [P][4] = msg, sqrd_obs, dx, dy; dmin [P]; disp [P][2]) of eea_distance_query_batch: the poses' cells by the
    oracle's world2Grid; dmin = sqrt(sq) * res - boundary_radius, disp = res * (dx, dy) as IEEE doubles"""
    ys, xs = sq.shape
    r_col = cr.radii(res, coll)[1]
    cx, cy = cr.centres(g, poses)
    P = len(poses)
    out = np.zeros((P, 4), dtype=np.int32)
    out[:, 0], out[:, 1] = OFF_GRID, -1
    dmin, disp = np.zeros(P), np.zeros((P, 2))
    on = on_grid(cx, cy, xs, ys)
    q = np.nonzero(on)[0]
    s = sq[cy[q], cx[q]].astype(np.int64)
    empty = s < 0
    out[q[empty], 0] = NONE
    dmin[q[empty]] = DBL_MAX
    disp[q[empty]] = DBL_MAX
    q, s = q[~empty], s[~empty]
    near = nearest[cy[q], cx[q]].astype(np.int64)
    out[q, 0] = np.where(s <= r_col * r_col, CRASH, OBSTACLE)
    out[q, 1] = s
    out[q, 2] = near % xs - cx[q]
    out[q, 3] = near // xs - cy[q]
    dmin[q] = np.sqrt(s.astype(np.float64)) * np.float64(res) - np.float64(coll[0])
    disp[q] = np.float64(res) * out[q, 2:].astype(np.float64)
    return out, dmin, disp


def worst_step(res, coll, g, sq, nearest, traj):
    """(out int32 [B][4], step int32 [B], dmin [B]) of eea_distance_traj_min for traj [B][T][3]: an off-grid step is worse than
    any on-grid one, among on-grid steps the smallest sq, among equals the earliest; an empty field: none at the first step
    that is on the grid"""
    B, T = traj.shape[:2]
    out, dmin, _ = query(res, coll, g, sq, nearest, traj.reshape(B * T, 3))
    out, dmin = out.reshape(B, T, 4), dmin.reshape(B, T)
    msg, s = out[:, :, 0].astype(np.int64), out[:, :, 1].astype(np.int64)
    cls = np.where(msg == OFF_GRID, 0, np.where(msg == NONE, 1 << 40, 1 + s))
    step = np.argmin(cls * (1 << 20) + np.arange(T)[None, :], axis=1)          # (argmin alone would do: the first among equals)
    b = np.arange(B)
    return out[b, step], step.astype(np.int32), dmin[b, step]


# ---- the shapes and scenes the GPU test builds --------------------------------------------------------------------------
SHAPES = [(1, 7), (7, 1), (1, 300), (300, 1), (5, 300), (300, 5), (64, 64), (63, 65), (129, 257)]      # ysize x xsize
VALUES = np.array([100, 80, 79, 50, 49, -1, -128, 127], dtype=np.int8)


def random_grid(ys, xs, seed, fraction=0.02):
    """about `fraction` of the cells take one of VALUES (occupied or not by the threshold), the rest 0; one cell is 100"""
    rng = np.random.default_rng(seed)
    data = np.zeros((ys, xs), dtype=np.int8)
    mark = rng.random((ys, xs)) < max(fraction, 2.0 / (xs * ys))
    data[mark] = rng.choice(VALUES, int(mark.sum()))
    if xs * ys > 1:
        data[rng.integers(0, ys), rng.integers(0, xs)] = 100          # never empty
    return data

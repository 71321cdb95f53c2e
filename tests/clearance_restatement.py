"""Collision::minDistance / minDirection (reference collision.cpp:65-124) restated in numpy in their ORDER-FREE form, and the
scenes the clearance tests share (tests/test_clearance.py checks this file against the oracle on the CPU;
tests/test_gpu_clearance.py uses it as the second opinion beside the oracle).

The search walks the Bresenham rings r_bnd..r_max, four cells per step (Q1 Q2 Q3 Q4, collision.cpp:175-193), keeps the first
visited occupied cell of the smallest squared distance and stops with "crash" at the first cell within r_col.  Enumerate the
walk once as offsets d_0..d_{n-1} in visit order, duplicates included; an occupied in-grid cell reached through offset k
has the key (|d_k|^2, k), here the integer |d_k|^2 * n + k; the answer of a centre is its smallest key."""
import math

import numpy as np

from oracle import pyoracle as po

CRASH, OBSTACLE, NONE = 0, 1, 2
DBL_MAX = float(np.finfo(np.float64).max)

# (resolution, (boundary, search, obstacle threshold, occupied threshold)) -> the number of cells the walk visits
SETS = [(0.05, (0.7, 1.0, 0.2, 0.8), 744), (0.25, (0.7, 1.0, 0.2, 0.8), 48), (0.1, (0.3, 0.6, 0.1, 0.5), 76),
        (0.1, (0.0, 0.5, 0.3, 0.8), 80), (0.1, (0.4, 0.4, 0.5, 0.8), 20), (0.1, (0.2, 1.2, 0.1, 0.8), 360)]


def radii(res, coll):
    """r_bnd, r_col, r_max in cells (collision.cpp:130-133)"""
    return math.floor(coll[0] / res), math.floor((coll[0] + coll[2]) / res), math.floor(coll[1] / res)


def walk(r_bnd, r_max):
    """the offsets (cell - centre) of the search in visit order, [n][2] = (dx, dy)"""
    out = []
    for r0 in range(r_bnd, r_max + 1):
        x, y, err = -r0, 0, 2 - 2 * r0
        while x < 0:
            out += [(-x, y), (-y, -x), (x, -y), (y, x)]
            r = err
            if r <= y:
                y += 1
                err += 2 * y + 1
            if r > x or err > y:
                x += 1
                err += 2 * x + 1
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def occupied(data, threshold):
    """checkCell's test (collision.cpp:228, grid.cpp:177-184): not (cell / 100 < threshold)"""
    return ~(data.astype(np.float64) / 100.0 < threshold)


def key_map(data, threshold, offs):
    """keys [ysize + 2R][xsize + 2R] over the centres [-R, size + R): the smallest |d_k|^2 * n + k, -1 where no cell is seen"""
    n = len(offs)
    R = int(np.abs(offs).max()) if n else 0
    ys, xs = data.shape
    big = np.iinfo(np.int64).max
    keys = np.full((ys + 2 * R, xs + 2 * R), big, dtype=np.int64)
    ii, jj = np.nonzero(occupied(data, threshold))
    if n and len(ii):
        key = (offs ** 2).sum(1) * n + np.arange(n)
        rows = (ii[:, None] - offs[None, :, 1] + R).reshape(-1)       # centre = cell - d
        cols = (jj[:, None] - offs[None, :, 0] + R).reshape(-1)
        np.minimum.at(keys, (rows, cols), np.broadcast_to(key, (len(ii), n)).reshape(-1))
    keys[keys == big] = -1
    return keys, R


def decode(keys_at, offs, r_col):
    """(msg, sqrd_obs, dx, dy) int32 [.][4] of the keys keys_at [.] (-1: none)"""
    n = max(len(offs), 1)
    out = np.zeros((len(keys_at), 4), dtype=np.int32)
    out[:, 0], out[:, 1] = NONE, -1
    seen = keys_at >= 0
    sq, k = keys_at // n, keys_at % n
    crash = seen & (sq <= r_col * r_col)
    obst = seen & ~crash
    out[crash] = (CRASH, 0, 0, 0)
    out[obst, 0] = OBSTACLE
    out[obst, 1] = sq[obst]
    if len(offs):
        out[obst, 2:] = offs[k[obst]]
    return out


def centres(g, poses):
    """the poses' cells (x, y) as signed 32-bit integers, by the oracle's world2Grid (the unsigned indices reinterpreted)"""
    ij = np.array([g.world2grid(float(p[0]), float(p[1])) for p in poses], dtype=np.uint32).reshape(-1, 2)
    return ij[:, 1].astype(np.int32).astype(np.int64), ij[:, 0].astype(np.int32).astype(np.int64)


def restate(res, coll, g, data, poses):
    """the canonical form for the poses [P][3]: int32 [P][4]"""
    r_bnd, r_col, r_max = radii(res, coll)
    offs = walk(r_bnd, r_max)
    keys, R = key_map(data, coll[3], offs)
    cx, cy = centres(g, poses)
    hx, hy = cx + R, cy + R
    inside = (hx >= 0) & (hy >= 0) & (hx < keys.shape[1]) & (hy < keys.shape[0])
    at = np.full(len(poses), -1, dtype=np.int64)
    at[inside] = keys[hy[inside], hx[inside]]
    return decode(at, offs, r_col)


def oracle(coll, g, poses):
    """(msg, sqrd_obs, dx, dy) int32 [P][4] from pyoracle.collision_check's state after the search; crash and none carry the
    constants of eea_clearance (crash: 0, 0, 0; none: -1, 0, 0)"""
    out = np.zeros((len(poses), 4), dtype=np.int32)
    for q, p in enumerate(poses):
        hit, sq, dx, dy = po.collision_check(coll, g, np.asarray(p, dtype=np.float64))
        if hit:
            out[q] = (CRASH, 0, 0, 0)
        elif sq == -1:
            out[q] = (NONE, -1, 0, 0)
        else:
            out[q] = (OBSTACLE, sq, dx, dy)
    return out


def doubles(res, coll, ans):
    """dmin [P] and disp [P][2] of the answers ans [P][4] as the reference forms them (collision.cpp:79-92, 107-123): IEEE
    double sqrt, one product, one difference"""
    msg = ans[:, 0]
    dmin = np.full(len(ans), DBL_MAX)
    disp = np.full((len(ans), 2), DBL_MAX)
    dmin[msg == CRASH] = 0.0
    disp[msg == CRASH] = 0.0
    o = msg == OBSTACLE
    dmin[o] = np.sqrt(ans[o, 1].astype(np.float64)) * np.float64(res) - np.float64(coll[0])
    disp[o] = np.float64(res) * ans[o, 2:].astype(np.float64)
    return dmin, disp


# ---- scenes --------------------------------------------------------------------------------------------------------

def scene(res, coll, P=3000):
    """the 90 x 70 grid of tests/test_gpu_collision_parity.py::test_inflated_map_and_ring_search_agree_with_oracle with P poses
    up to 30 cells outside the map, the first eight the edge poses of test_collision_check_bit_exact's kind: the map's corners,
    just outside the lower edge, far outside, NaN.  Returns (GridMap, data [70][90] int8, poses [P][3], xmin, ymin)"""
    rng = np.random.default_rng(int(res * 1000) + int(coll[0] * 10))
    xs, ys = 90, 70
    xmin, ymin = -2.0, -1.5
    data = np.zeros((ys, xs), dtype=np.int8)
    for _ in range(12):
        i, j = rng.integers(0, ys - 6), rng.integers(0, xs - 6)
        data[i:i + rng.integers(1, 6), j:j + rng.integers(1, 6)] = rng.choice([100, 80, 79, 55, 50, 49])
    data[rng.integers(0, ys, 30), rng.integers(0, xs, 30)] = 100
    data[0, :] = 100
    data[:, xs - 1] = 100
    g = po.GridMap(xmin, xmin + xs * res, ymin, ymin + ys * res, res, data.reshape(-1))
    poses = np.empty((P, 3))
    poses[:, 0] = rng.uniform(xmin - 30 * res, xmin + (xs + 30) * res, P)
    poses[:, 1] = rng.uniform(ymin - 30 * res, ymin + (ys + 30) * res, P)
    poses[:, 2] = 0.0
    edge = np.array([[xmin, ymin, 0], [xmin + xs * res, ymin + ys * res, 0], [xmin - 0.5 * res, 0.0, 0], [1e9, 0.0, 0],
                     [xmin + 12.5 * res, ymin + 6.5 * res, 0], [0.0, -1e9, 0], [float("nan"), 0.0, 0], [xmin - 1e-12, ymin, 0]])
    poses[:len(edge)] = edge
    return g, data, poses, xmin, ymin


# Hand-made scenes on a 41 x 41 grid at 0.1 m around the centre cell (20, 20): occupied cells as offsets (dx, dy) from it, and
# the answer at the centre.  FACT_COLLS: the radii 3, 4, 12 in cells, and (0.3, 1.2, 0.1, 0.8), whose quotients 0.3 / 0.1 and
# 1.2 / 0.1 fall just below 3 and 12 in doubles (radii 2, 4, 11): every fact holds for both.
N41, RES41, XMIN41, YMIN41 = 41, 0.1, -2.0, -1.0
FACT_COLLS = [(0.35, 1.25, 0.1, 0.8), (0.3, 1.2, 0.1, 0.8)]
FACTS = [
    ([(5, 0), (-5, 0), (0, 5), (0, -5)], (OBSTACLE, 25, 5, 0)),       # Q1 of the ring's first step wins
    ([(7, 0), (-7, 0), (0, 7), (0, -7)], (OBSTACLE, 49, 7, 0)),
    ([(10, 0), (-10, 0), (0, 10), (0, -10)], (OBSTACLE, 100, 10, 0)),
    ([(3, 4), (-5, 0), (-4, -3)], (OBSTACLE, 25, -5, 0)),             # the axis cells of ring 5 come before its (3, 4)
    ([(4, 3), (3, 4), (3, -4), (-4, 3)], (OBSTACLE, 25, 4, 3)),
    ([(6, 6)], (NONE, -1, 0, 0)),                                     # the rings have gaps
    ([(5, 6)], (OBSTACLE, 61, 5, 6)),
    ([(7, 5)], (OBSTACLE, 74, 7, 5)),
    ([(8, 4)], (OBSTACLE, 80, 8, 4)),
    ([(4, 8)], (OBSTACLE, 80, 4, 8)),
    ([(1, 0)], (NONE, -1, 0, 0)),                                     # inside r_bnd
    ([(4, 0)], (CRASH, 0, 0, 0)),
]


def fact_scene(cells):
    """(GridMap, data [41][41], the pose at the centre of cell (20, 20))"""
    data = np.zeros((N41, N41), dtype=np.int8)
    for dx, dy in cells:
        data[20 + dy, 20 + dx] = 100
    g = po.GridMap(XMIN41, XMIN41 + N41 * RES41, YMIN41, YMIN41 + N41 * RES41, RES41, data.reshape(-1))
    pose = np.array([[XMIN41 + 20.5 * RES41, YMIN41 + 20.5 * RES41, 0.0]])
    assert g.world2grid(pose[0, 0], pose[0, 1]) == (20, 20)
    return g, data, pose


def cell_centres(g, xs, ys):
    """the world centre of every cell, row-major [ys * xs][3] (grid.cpp:126-131), each inside its own cell"""
    poses = np.zeros((ys * xs, 3))
    for i in range(ys):
        for j in range(xs):
            poses[i * xs + j, :2] = g.grid2world(i, j)
            assert g.world2grid(poses[i * xs + j, 0], poses[i * xs + j, 1]) == (i, j)
    return poses

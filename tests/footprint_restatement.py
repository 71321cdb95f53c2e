"""Footprint collision (eea_footprint_radii / eea_footprint_check_batch / eea_footprint_traj_first: csrc/footprint_planes.hpp,
csrc/footprint_kernel.hip) restated in numpy, for tests/test_footprint.py (CPU) and tests/test_gpu_footprint.py.

A pose (px, py, th) with three finite components collides iff some occupied in-grid cell has its centre in the closed polygon
placed at the pose.  brute is that definition over all occupied cells; filtered is the same through the distance field (one
int per pose with a cell decides most of them, the rest test the cells of a box around their own); both form every value in
the order include/ergodic_amd.h writes down, numpy's sin / cos in place of the device's."""
import math

import numpy as np

from tests import clearance_restatement as cr
from tests import distance_restatement as dr

MAX_VERTICES = 16
FOOTPRINTS = {
    "rect": [(0.45, -0.25), (0.45, 0.25), (-0.45, 0.25), (-0.45, -0.25)],
    "tri": [(0.6, 0.0), (-0.3, 0.35), (-0.3, -0.35)],
    "oct": [(0.5 * math.cos(k * math.pi / 4 + 0.1), 0.5 * math.sin(k * math.pi / 4 + 0.1)) for k in range(8)],
    "offc": [(0.9, -0.2), (0.9, 0.2), (-0.1, 0.2), (-0.1, -0.2)],       # the body origin 0.1 m from the rear edge
}
DECIDED = 1e-9          # metres: a pose is decided when no occupied centre lies closer than this to the footprint's boundary
FREE, HIT, AMBIGUOUS, NO_CELL, NO_CELL_REJECTED = range(5)          # the classes of `filtered`


def planes(vertices):
    """(nx [n], ny [n], h [n], r_in, r_out): edge k from vertex k to k + 1; single IEEE operations, no hypot, no FMA"""
    v = np.asarray(vertices, dtype=np.float64)
    x, y = v[:, 0], v[:, 1]
    x1, y1 = np.roll(x, -1), np.roll(y, -1)
    ex, ey = x1 - x, y1 - y
    length = np.sqrt(ex * ex + ey * ey)
    nx, ny = ey / length, -ex / length
    h = nx * x + ny * y
    return nx, ny, h, h.min(), np.sqrt(x * x + y * y).max()


def valid(vertices):
    """the footprint's refusals: 3..16 finite vertices, every turn strictly left, every h_k > 0"""
    v = np.asarray(vertices, dtype=np.float64)
    if v.ndim != 2 or not 3 <= len(v) <= MAX_VERTICES or not np.isfinite(v).all():
        return False
    e = np.roll(v, -1, axis=0) - v
    e1 = np.roll(e, -1, axis=0)
    if not (e[:, 0] * e1[:, 1] - e[:, 1] * e1[:, 0] > 0.0).all():
        return False
    return bool((planes(vertices)[2] > 0.0).all())


def thresholds(r_in, r_out, res):
    """(sq_hit, sq_free, box): 0 <= sq <= sq_hit is a sure hit (-1: none is), sq > sq_free is surely free, the exact test covers
    the cells within box of the pose's"""
    a = np.float64(r_in) / np.float64(res) - 0.7072 - 1e-6
    sq_hit = int(math.floor(a)) ** 2 if a >= 0.0 else -1
    sq_free = int(math.ceil(np.float64(r_out) / np.float64(res) + 0.7072 + 1e-6)) ** 2
    return sq_hit, sq_free, int(math.ceil(np.float64(r_out) / np.float64(res))) + 1


def _signed(res, xmin, ymin, pl, poses, ii, jj):
    """max_k (n_k . b - h_k) [P][cells] of the centres of the cells (ii, jj) in the body frames of the poses, and the closed
    test itself (every n_k . b <= h_k) -- NaN poses fail every comparison"""
    nx, ny, h = pl[:3]
    res = np.float64(res)
    cxw = jj.astype(np.float64) * res + res / 2.0 + np.float64(xmin)
    cyw = ii.astype(np.float64) * res + res / 2.0 + np.float64(ymin)
    with np.errstate(invalid="ignore"):
        s, c = np.sin(poses[:, 2])[:, None], np.cos(poses[:, 2])[:, None]
        dx, dy = cxw[None, :] - poses[:, 0][:, None], cyw[None, :] - poses[:, 1][:, None]
        bx, by = c * dx + s * dy, (-s) * dx + c * dy
        worst = np.full(bx.shape, -np.inf)
        inside = np.ones(bx.shape, dtype=bool)
        for k in range(len(h)):
            d = nx[k] * bx + ny[k] * by
            inside &= d <= h[k]
            worst = np.fmax(worst, d - h[k])
    return worst, inside


def brute(res, xmin, ymin, data, threshold, vertices, poses):
    """(hit bool [P], margin [P]): the definition over every occupied cell; margin = the smallest |max_k (n_k . b - h_k)| over
    the occupied cells (inf: no occupied cell, or a pose that is not finite)"""
    poses = np.asarray(poses, dtype=np.float64)
    ii, jj = np.nonzero(cr.occupied(data, threshold))
    hit = np.zeros(len(poses), dtype=bool)
    margin = np.full(len(poses), np.inf)
    if len(ii) == 0 or len(poses) == 0:
        return hit, margin
    worst, inside = _signed(res, xmin, ymin, planes(vertices), poses, ii, jj)
    hit = inside.any(1)
    fin = np.isfinite(poses).all(1)
    margin[fin] = np.abs(worst[fin]).min(1)
    return hit & fin, margin


def cells(res, xmin, ymin, xs, ys, poses):
    """(has [P], fx [P], fy [P]): fx = floor((px - xmin) / res) as a double, no wrap and no step at the upper edge; a pose has
    a cell when it is finite and fx, fy are on the grid"""
    poses = np.asarray(poses, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        fx = np.floor((poses[:, 0] - np.float64(xmin)) / np.float64(res))
        fy = np.floor((poses[:, 1] - np.float64(ymin)) / np.float64(res))
        has = np.isfinite(poses).all(1) & (fx >= 0) & (fx <= xs - 1) & (fy >= 0) & (fy <= ys - 1)
    return has, fx, fy


def filtered(res, xmin, ymin, data, threshold, vertices, poses, sq=None):
    """(hit bool [P], cls [P]) through the field sq (distance_restatement.brute_force's by default): FREE / HIT by one int,
    AMBIGUOUS and NO_CELL by the exact test over the box, NO_CELL_REJECTED when the box misses the grid (or the pose is not
    finite)"""
    poses = np.asarray(poses, dtype=np.float64)
    ys, xs = data.shape
    if sq is None:
        sq = dr.brute_force(data, threshold)[0]
    pl = planes(vertices)
    sq_hit, sq_free, box = thresholds(pl[3], pl[4], res)
    has, fx, fy = cells(res, xmin, ymin, xs, ys, poses)
    occ = cr.occupied(data, threshold)
    hit = np.zeros(len(poses), dtype=bool)
    cls = np.full(len(poses), NO_CELL_REJECTED)
    fin = np.isfinite(poses).all(1)
    for q in range(len(poses)):
        if not fin[q]:
            continue
        if has[q]:
            s = int(sq[int(fy[q]), int(fx[q])])
            if s < 0 or s > sq_free:
                cls[q] = FREE
                continue
            if s <= sq_hit:
                cls[q], hit[q] = HIT, True
                continue
        if not (fx[q] + box >= 0 and fx[q] - box <= xs - 1 and fy[q] + box >= 0 and fy[q] - box <= ys - 1):
            continue
        cls[q] = AMBIGUOUS if has[q] else NO_CELL
        x0, x1 = int(max(fx[q] - box, 0.0)), int(min(fx[q] + box, xs - 1.0))
        y0, y1 = int(max(fy[q] - box, 0.0)), int(min(fy[q] + box, ys - 1.0))
        ii, jj = np.nonzero(occ[y0:y1 + 1, x0:x1 + 1])
        if len(ii):
            hit[q] = _signed(res, xmin, ymin, pl, poses[q:q + 1], ii + y0, jj + x0)[1].any()
    return hit, cls


def first_step(hits):
    """int32 [B]: the first True of every row of hits [B][T], -1 where there is none"""
    hits = np.asarray(hits, dtype=bool)
    return np.where(hits.any(1), hits.argmax(1), -1).astype(np.int32)


# ---- scenes -----------------------------------------------------------------------------------------------------------------

def scene(res, coll, P=3000):
    """clearance_restatement.scene with every heading, the eight edge poses' included, drawn from (-pi, pi).  Returns
    (data [70][90] int8, poses [P][3], xmin, ymin)"""
    _, data, poses, xmin, ymin = cr.scene(res, coll, P)
    poses = poses.copy()
    poses[:, 2] = np.random.default_rng(5).uniform(-np.pi, np.pi, P)
    return data, poses, xmin, ymin


def wrap_poses(res, xmin, ymin):
    """Poses 2^32 cells away that world2Grid's x86 wrap (grid.cpp:143-159 as gcc compiles the cast: low 32 bits of the 64-bit
    integer) folds on to cell (row 0, column 5) of the grid: in x, in y and in both, upwards and downwards.  floor((px - xmin) /
    res) is +-2^32 + 5 (in y: +-2^32) for them, so they have no cell here, and their box misses the grid.  [6][3], any heading.  No scene of
    clearance_restatement holds such a pose (its far poses, 1e9 m, wrap to cells far off the grid), so the tests add these"""
    res = np.float64(res)
    up_x, dn_x = xmin + (2.0 ** 32 + 5.5) * res, xmin - (2.0 ** 32 - 5.5) * res
    up_y, dn_y = ymin + (2.0 ** 32 + 0.5) * res, ymin - (2.0 ** 32 - 0.5) * res
    in_x, in_y = xmin + 5.5 * res, ymin + 0.5 * res
    return np.array([[up_x, in_y, 0.3], [dn_x, in_y, -2.0], [in_x, up_y, 1.0], [in_x, dn_y, 3.0], [up_x, up_y, -0.7], [dn_x, dn_y, 2.2]])


def fact_scene(walls):
    """the 41 x 41 grid at 0.1 m of clearance_restatement with the cells walls [(i0, i1, j0, j1), ...] (inclusive) at 100"""
    data = np.zeros((cr.N41, cr.N41), dtype=np.int8)
    for i0, i1, j0, j1 in walls:
        data[i0:i1 + 1, j0:j1 + 1] = 100
    return data


def centre41(j, i):
    return cr.XMIN41 + (j + 0.5) * cr.RES41, cr.YMIN41 + (i + 0.5) * cr.RES41


# A corridor along x, 0.7 m wide between the faces of its wall cells (rows 16 and 24 of occupied centres, 0.8 m apart), with
# `rect` (0.9 m x 0.5 m) at the centre of cell (20, 20): along the corridor the nearest wall centres are 0.4 m from the axis,
# 0.15 m outside the 0.25 m half-width; across it they are 0.4 m from the centre, 0.05 m inside the 0.45 m half-length.
CORRIDOR = [(16, 16, 0, 40), (24, 24, 0, 40)]
CORRIDOR_POSE = centre41(20, 20)
# A wall across x at column 27, its centres 0.7 m ahead of cell (20, 20): `offc` reaches 0.9 m forward (0.2 m past them) and
# 0.1 m backward (0.6 m short of them).  The pose stands 0.05 m above the cell's centre, so that the wall's centres are 0.05 m
# and more from the sides y = +-0.2 m of the base.
WALL_AHEAD = [(0, 40, 27, 27)]
WALL_POSE = (centre41(20, 20)[0], centre41(20, 20)[1] + 0.05)

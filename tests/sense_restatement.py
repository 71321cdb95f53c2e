"""numpy restatement of eea_sense_reveal_batch / eea_grid_census (include/ergodic_amd.h): what the calls are defined to
compute, written for clarity.  Integers throughout; the only floating-point steps are world2Grid (reference grid.cpp:143-159,
with the wrap of x86-64's double -> unsigned conversion) and checkCell's `cell / 100.0 < occupied_threshold`
(collision.cpp:216-243 with GridMap::getCell, grid.cpp:177-184), both in IEEE doubles as the device computes them."""
import collections
import math

import numpy as np

# the part of eea_collision_cfg the sensor reads (the radii are ignored)
Geometry = collections.namedtuple("Geometry", "xmin ymin resolution xsize ysize occupied_threshold")


def cast_u32_x86(v):
    """static_cast<unsigned>(double) of an x86-64 build: cvttsd2si to 64 bits, low 32 bits; out of range / NaN give 0"""
    if not (v > -9.2233720368547758e18 and v < 9.2233720368547758e18):
        return 0
    return int(v) & 0xFFFFFFFF


def world2grid(g, x, y):
    """(i, j) = (row, column) of a world point; a point exactly on the upper edge is taken into the last cell"""
    qx, qy = (float(x) - g.xmin) / g.resolution, (float(y) - g.ymin) / g.resolution
    j = cast_u32_x86(math.floor(qx) if math.isfinite(qx) else qx)
    i = cast_u32_x86(math.floor(qy) if math.isfinite(qy) else qy)
    if j == g.xsize:
        j -= 1
    if i == g.ysize:
        i -= 1
    return i, j


def blocks(cell, occupied_threshold):
    """checkCell's rule: the cell stops a ray unless getCell < occupied_threshold (an unknown cell, -1, is -0.01: it does not)"""
    return not (float(cell) / 100.0 < occupied_threshold)


def ray_target(q, R):
    """the offset (tx, ty) on the perimeter of [-R, R]^2 that ray q of the 8R rays aims at"""
    side, k = divmod(q, 2 * R)
    return ((R, -R + k), (R - k, R), (-R, R - k), (-R + k, -R))[side]


def step_offset(m, s, R):
    """d(m, s) = sgn(m) ((2 s |m| + R) div 2R): s |m| / R rounded half away from zero"""
    return (1 if m > 0 else -1 if m < 0 else 0) * ((2 * s * abs(m) + R) // (2 * R))


def ray_offsets(R):
    """[8R][R][2] ints: (dx, dy) of step s = 1 .. R of every ray (before the range and grid tests cut the ray)"""
    out = np.empty((8 * R, R, 2), dtype=np.int64)
    for q in range(8 * R):
        tx, ty = ray_target(q, R)
        for s in range(1, R + 1):
            out[q, s - 1] = step_offset(tx, s, R), step_offset(ty, s, R)
    return out


def reveal(g, R, truth, known, poses, mask=None, ranges=None):
    """known (int8 [ysize][xsize]) is updated in place from truth; returns ranges int32 [P][8R] (`ranges` itself when given:
    the rows of robots the mask leaves out are not written)"""
    P = len(poses)
    if ranges is None:
        ranges = np.full((P, 8 * R), -1, dtype=np.int32)
    off = ray_offsets(R)
    for b in range(P):
        if mask is not None and mask[b] == 0:
            continue
        ranges[b, :] = -1
        i0, j0 = world2grid(g, poses[b][0], poses[b][1])
        if not (i0 <= g.ysize - 1 and j0 <= g.xsize - 1):     # gridBounds: the robot reveals nothing and hits nothing
            continue
        known[i0, j0] = truth[i0, j0]                          # the robot's own cell; it never blocks
        for q in range(8 * R):
            for s in range(1, R + 1):
                dx, dy = int(off[q, s - 1, 0]), int(off[q, s - 1, 1])
                if dx * dx + dy * dy > R * R:
                    break
                i, j = i0 + dy, j0 + dx
                if not (0 <= i < g.ysize and 0 <= j < g.xsize):
                    break
                known[i, j] = truth[i, j]
                if blocks(truth[i, j], g.occupied_threshold):
                    ranges[b, q] = s
                    break
    return ranges


def census(g, grid):
    """(unknown cells, known cells below the threshold, blocking cells) of an int8 grid"""
    cells = np.asarray(grid, dtype=np.int8).reshape(-1)
    below = cells.astype(np.float64) / 100.0 < g.occupied_threshold
    return (int(np.count_nonzero(cells < 0)), int(np.count_nonzero((cells >= 0) & below)), int(np.count_nonzero(~below)))

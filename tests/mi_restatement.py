"""Restatement of eea_sense_mi_table / eea_sense_mi_field / the value grid of eea_set_target_mi (include/ergodic_amd.h): what the
calls are defined to compute, written as the contract's loops in Python floats (IEEE doubles, every product and sum rounded on
its own), in the contract's order.  The rays, step offsets, disc test, grid test and blocks() are those of
tests/sense_restatement.py, imported unchanged.  The field takes the table as an argument: fed the library's own table it must
equal the device bit for bit, whatever libm evaluated the logs."""
import math

import numpy as np

from tests import sense_restatement as sr


def table(g, p_unknown):
    """(h, pass_): two lists of 256 floats, entry v + 128 for the int8 value v"""
    h, pass_ = [], []
    for v in range(-128, 128):
        o = float(p_unknown) if v < 0 else float(min(v, 100)) / 100.0
        h.append(0.0 if o == 0.0 or o == 1.0 else -o * math.log(o) - (1.0 - o) * math.log(1.0 - o))
        pass_.append(0.0 if sr.blocks(v, g.occupied_threshold) else 1.0 - o)
    return h, pass_


def beam(g, R, known, h, pass_, i0, j0, ray):
    """one ray from (i0, j0): (its value, the cell values it crossed up to and including a blocking one)"""
    reach, value, crossed = 1.0, 0.0, []
    for dx, dy in ray:
        if dx * dx + dy * dy > R * R:
            break
        i, j = i0 + dy, j0 + dx
        if not (0 <= i < g.ysize and 0 <= j < g.xsize):
            break
        v = known[i][j]
        crossed.append(v)
        value = value + reach * h[v + 128]
        reach = reach * pass_[v + 128]
        if sr.blocks(v, g.occupied_threshold):
            break                                           # (reach is +0.0: going on would add +0.0 per step)
    return value, crossed


def mi_field_loops(g, R, stride, known, h, pass_):
    """the contract, candidate by candidate and beam by beam in Python floats (slow: small grids only)"""
    cells = np.asarray(known, dtype=np.int8).reshape(g.ysize, g.xsize).tolist()
    h, pass_ = [float(x) for x in h], [float(x) for x in pass_]
    rays = [[(int(dx), int(dy)) for dx, dy in ray] for ray in sr.ray_offsets(R)]
    mi = np.zeros((g.ysize, g.xsize), dtype=np.float64)
    for i0 in range(0, g.ysize, stride):
        for j0 in range(0, g.xsize, stride):
            if sr.blocks(cells[i0][j0], g.occupied_threshold):
                continue                                    # a robot cannot stand there
            total = h[cells[i0][j0] + 128]
            for ray in rays:
                total = total + beam(g, R, cells, h, pass_, i0, j0, ray)[0]
            mi[i0, j0] = total
    return mi


def mi_field(g, R, stride, known, h, pass_, rows=None, cols=None):
    """float64 [ysize][xsize]: for every candidate (i0 % stride == 0 and j0 % stride == 0) whose own cell does not block,
    h(own) + the beams of its 8R rays, added in ray order; +0.0 everywhere else.  rows / cols (ranges, optional): only the
    candidates inside them are evaluated (a sub-window of a large grid; the rest of the result stays 0).
    The loops of mi_field_loops with the candidates side by side in numpy arrays: per candidate the same doubles, the same
    operations (numpy's float64 product and sum are IEEE, one rounding each) in the same order"""
    cells = np.asarray(known, dtype=np.int8).reshape(g.ysize, g.xsize).astype(np.int64)
    h, pass_ = np.asarray(h, dtype=np.float64), np.asarray(pass_, dtype=np.float64)
    block = np.array([sr.blocks(v, g.occupied_threshold) for v in range(-128, 128)])
    ii, jj = np.meshgrid(np.arange(0, g.ysize, stride), np.arange(0, g.xsize, stride), indexing="ij")
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    keep = ~block[cells[ii, jj] + 128]                      # a robot cannot stand in a blocking cell
    if rows is not None:
        keep &= np.isin(ii, np.asarray(list(rows)))
    if cols is not None:
        keep &= np.isin(jj, np.asarray(list(cols)))
    ii, jj = ii[keep], jj[keep]
    total = h[cells[ii, jj] + 128].copy()
    for ray in sr.ray_offsets(R):
        reach, value = np.ones(ii.size), np.zeros(ii.size)
        on = np.ones(ii.size, dtype=bool)                   # the candidates whose ray has not ended
        for dx, dy in ray:
            dx, dy = int(dx), int(dy)
            if dx * dx + dy * dy > R * R:
                break
            i, j = ii + dy, jj + dx
            on &= (i >= 0) & (i < g.ysize) & (j >= 0) & (j < g.xsize)
            if not on.any():
                break
            v = cells[np.where(on, i, 0), np.where(on, j, 0)] + 128
            value = np.where(on, value + reach * h[v], value)
            reach = np.where(on, reach * pass_[v], reach)
            on &= ~block[v]
        total = total + value
    mi = np.zeros((g.ysize, g.xsize), dtype=np.float64)
    mi[ii, jj] = total
    return mi


def value_grid(g, stride, known, mi, floor, dtype=np.float64):
    """v[i][j] = (real)(mi[i][j] + floor) on the candidates whose cell does not block, 0 elsewhere"""
    known = np.asarray(known, dtype=np.int8).reshape(g.ysize, g.xsize)
    cand = np.zeros((g.ysize, g.xsize), dtype=bool)
    cand[::stride, ::stride] = True
    cand &= known.astype(np.float64) / 100.0 < g.occupied_threshold
    v = np.where(cand, np.asarray(mi, dtype=np.float64) + np.float64(floor), 0.0)
    return v.astype(dtype)

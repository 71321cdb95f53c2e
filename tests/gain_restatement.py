"""numpy restatement of eea_sense_gain_field / the value grid of eea_set_target_gain (include/ergodic_amd.h): what the calls
are defined to compute, written as the contract's loops.  The rays, step offsets, disc test, grid test and blocks() are those of
tests/sense_restatement.py, imported unchanged.  Integers throughout."""
import numpy as np

from tests import sense_restatement as sr


def gain_field(g, R, stride, known, rows=None, cols=None):
    """uint32 [ysize][xsize]: for every candidate (i0 % stride == 0 and j0 % stride == 0) whose own cell does not block,
    [known[i0][j0] < 0] + the unknown cells its 8R rays cross through `known`, counted per beam (a blocking cell is visited,
    counted if negative, and ends the ray); 0 everywhere else.  rows / cols (ranges, optional): only the candidates inside
    them are evaluated (a sub-window of a large grid; the rest of the result stays 0)"""
    cells = np.asarray(known, dtype=np.int8).reshape(g.ysize, g.xsize).tolist()    # (plain ints: the loops below are long)
    block = {v: sr.blocks(v, g.occupied_threshold) for v in range(-128, 128)}
    rays = [[(int(dx), int(dy)) for dx, dy in ray] for ray in sr.ray_offsets(R)]
    gain = np.zeros((g.ysize, g.xsize), dtype=np.uint32)
    for i0 in range(0, g.ysize, stride):
        for j0 in range(0, g.xsize, stride):
            if (rows is not None and i0 not in rows) or (cols is not None and j0 not in cols):
                continue
            if block[cells[i0][j0]]:
                continue                                   # a robot cannot stand there
            n = 1 if cells[i0][j0] < 0 else 0
            for ray in rays:
                for dx, dy in ray:
                    if dx * dx + dy * dy > R * R:
                        break
                    i, j = i0 + dy, j0 + dx
                    if not (0 <= i < g.ysize and 0 <= j < g.xsize):
                        break
                    v = cells[i][j]
                    if v < 0:
                        n += 1
                    if block[v]:
                        break
            gain[i0, j0] = n
    return gain


def value_grid(g, stride, known, gain, floor, dtype=np.float64):
    """v[i][j] = (real)((double)gain[i][j] + floor) on the candidates whose cell does not block, 0 elsewhere"""
    known = np.asarray(known, dtype=np.int8).reshape(g.ysize, g.xsize)
    cand = np.zeros((g.ysize, g.xsize), dtype=bool)
    cand[::stride, ::stride] = True
    cand &= known.astype(np.float64) / 100.0 < g.occupied_threshold
    v = np.where(cand, np.asarray(gain, dtype=np.float64) + np.float64(floor), 0.0)
    return v.astype(dtype)

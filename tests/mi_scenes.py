"""Graded grids the mutual-information tests share (tests/test_mi.py, tests/test_gpu_mi.py): the partly revealed scenes of
tests/gain_scenes.py with occupancy probabilities laid over part of the free area -- a ramp of the values 1 .. 99, the 79 / 80
pair side by side, one cell of 127 and one of -128 -- so that every class of cell value meets rays from every side."""
import functools

import numpy as np

from tests import gain_scenes as gs


@functools.lru_cache(maxsize=None)
def _graded(xs, ys):
    g, base = gs.partly_revealed(xs, ys)
    known = base.copy()
    free = np.argwhere(known == 0)
    assert len(free) >= 8, "the scene has no free area to grade"
    ramp = free[::2]                                        # every second free cell, in row-major order
    for n, (i, j) in enumerate(ramp):
        known[i, j] = 1 + (n * 7) % 99                      # 1 .. 99, each value met (7 and 99 are coprime) once there are 99
    (i, j), (i2, j2) = free[1], free[3]
    known[i, j], known[i2, j2] = 127, -128
    # the threshold pair next to each other, in a row of the free area
    pair = [(a, b) for a, b in free.tolist() if b + 1 < xs and base[a, b + 1] == 0]
    a, b = pair[len(pair) // 2]
    known[a, b], known[a, b + 1] = 79, 80
    known.setflags(write=False)
    return g, known


def graded(xs, ys):
    """(geometry, known): read-only, computed once per size"""
    return _graded(xs, ys)

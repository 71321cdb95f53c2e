"""Partly revealed grids the information-gain tests share (tests/test_gain.py, tests/test_gpu_gain.py): a truth grid in the
manner of test_gpu_sense.py's _scene -- a single blocking cell, an L-shaped wall, a patch that is unknown in truth itself and
the 79 / 80 pair -- revealed from a few poses by the restatement, so that `known` has frontiers in the open, frontiers behind
walls, known pockets and a rim nobody has seen."""
import functools

import numpy as np

from tests import sense_restatement as sr

RES, XMIN, YMIN, THR = 0.25, -1.0, -2.0, 0.8


def geom(xs, ys):
    return sr.Geometry(XMIN, YMIN, RES, xs, ys, THR)


def centre(g, i, j):
    return [g.xmin + (j + 0.5) * g.resolution, g.ymin + (i + 0.5) * g.resolution, 0.3]


@functools.lru_cache(maxsize=None)
def _partly_revealed(xs, ys):
    g = geom(xs, ys)
    truth = np.zeros((ys, xs), dtype=np.int8)
    ci, cj = ys // 2, xs // 2
    truth[ci, min(cj + 3, xs - 1)] = 100
    truth[min(4, ys - 1), 5:11] = 100
    truth[4:10, min(10, xs - 1)] = 100
    truth[max(ys - 6, 0):max(ys - 3, 0), 2:6] = -1
    truth[min(ci + 2, ys - 1), min(3, xs - 1)], truth[min(ci + 3, ys - 1), min(3, xs - 1)] = 79, 80
    known = np.full_like(truth, -1)
    R = max(2, min(xs, ys) // 4)
    sr.reveal(g, R, truth, known, [centre(g, ci, cj - 1), centre(g, 2, 7), centre(g, ys - 1, 0)])
    sr.reveal(g, 2, truth, known, [centre(g, 0, xs - 1), centre(g, 6, min(12, xs - 1))])
    known.setflags(write=False)
    return g, known


def partly_revealed(xs, ys):
    """(geometry, known): read-only, computed once per size"""
    return _partly_revealed(xs, ys)

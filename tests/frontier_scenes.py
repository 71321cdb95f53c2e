"""The scenes tests/test_frontier.py (CPU) and tests/test_gpu_frontier.py share, sized from the tile the header publishes: masks
that draw arbitrary shapes for EEA_FRONTIER_OF_MASK, a hand-built occupancy grid with its members written down, and a map
revealed by the sensor's restatement with the planes of the partition's restatement.  Read-only, computed once."""
import collections
import functools

import numpy as np

from ergodic_exploration_amd import capi
from tests import frontier_restatement as fr
from tests import gain_scenes as gs
from tests import geodesic_restatement as geo
from tests import partition_restatement as part
from tests import sense_restatement as sr

T = capi.GEODESIC_TILE_X
assert capi.GEODESIC_TILE_Y == T
THR = gs.THR


def _frozen(f):
    @functools.lru_cache(maxsize=None)
    def once():
        m = np.ascontiguousarray(f(), dtype=np.int8)
        m.setflags(write=False)
        return m
    return once


def _cells(shape, cells):
    m = np.zeros(shape, dtype=np.int8)
    for c in cells:
        m[c] = 1
    return m


def _comb_and_u():
    """teeth in tile row 0 that are separate there, joined by a spine in tile row 1: many unions at once, which must all end on
    tooth 0's root, cell 0; to the right a U on its side whose arms are separate in tile column 1 and joined in tile column 2"""
    teeth = 12
    m = np.zeros((T + 4, 2 * T + 8), dtype=np.int8)
    m[:T + 2, 0:4 * teeth:4] = 1
    m[T + 1, :4 * teeth - 3] = 1
    m[3, T + 20:2 * T + 5] = m[9, T + 20:2 * T + 5] = 1
    m[3:10, 2 * T + 4] = 1
    return m


def _random(density, seed):
    return lambda: (np.random.default_rng(seed).random((3 * T, 2 * T + 6)) < density).astype(np.int8) * np.int8(-5)


def _every_third():
    m = np.zeros((3 * T, 3 * T), dtype=np.int8)
    m[0::3, 0::3] = 1
    return m


def _checkerboard():
    i, j = np.indices((3 * T, 2 * T))
    return ((i + j) % 2 == 0).astype(np.int8) * np.int8(100)


MASKS = {
    "empty": _frozen(lambda: np.zeros((T + 13, 2 * T + 6))),
    "full": _frozen(lambda: np.ones((T + 13, 2 * T + 6))),
    "tiny": _frozen(lambda: _cells((3, 5), [(0, 0), (1, 1), (0, 4), (2, 3), (2, 4)])),
    "row_alternating": _frozen(lambda: np.arange(2 * T + 6).reshape(1, -1) % 2 == 0),
    "column": _frozen(lambda: np.ones((2 * T + 6, 1))),
    "serpentine_tile": _frozen(lambda: fr.serpentine_mask(T, T)),
    "serpentine_3x3": _frozen(lambda: fr.serpentine_mask(3 * T, 3 * T)),
    "corner_main": _frozen(lambda: _cells((2 * T, 2 * T), [(T - 1, T - 1), (T, T)])),
    "corner_anti": _frozen(lambda: _cells((2 * T, 2 * T), [(T - 1, T), (T, T - 1)])),
    "comb_and_u": _frozen(_comb_and_u),
    "checkerboard": _frozen(_checkerboard),
    "random_30": _frozen(_random(0.3, 31)),
    "random_45": _frozen(_random(0.45, 32)),
    "random_60": _frozen(_random(0.6, 33)),
    "every_third": _frozen(_every_third),
}


@functools.lru_cache(maxsize=None)
def known_grid():
    """(grid int8 [7][8], members bool) at occupied_threshold 0.7: 69 is free and 70 blocks; the unknown cell (0, 7) sits at
    the grid's border, (6, 0) in its corner; the free cell (5, 5) has unknown cells only diagonally; the free cells of row 0
    left of column 5 lie on the grid's edge with no unknown neighbour (off the grid is not unknown)"""
    U = -1
    grid = np.array([[0, 0, 0, 0, 0, 0, 69, U],
                     [0, 0, 0, 0, 0, 0, 70, U],
                     [0, 0, U, 69, 0, 0, 100, 0],
                     [0, 70, U, U, 100, 0, 0, 0],
                     [0, 0, 69, 0, U, 0, U, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0],
                     [U, 0, 0, 0, U, 0, U, 69]], dtype=np.int8)
    want = np.zeros(grid.shape, dtype=bool)
    for c in ((0, 6), (1, 2), (2, 1), (2, 3), (4, 2), (4, 3), (4, 5), (4, 7), (5, 0), (5, 4), (5, 6), (6, 1), (6, 3), (6, 5), (6, 7), (2, 7),
              (3, 6)):
        want[c] = True
    grid.setflags(write=False)
    want.setflags(write=False)
    return grid, want


Revealed = collections.namedtuple("Revealed", "g truth known poses R sq clear_sq geo owner")


def _squared_distances(known, thr):
    """the plane eea_distance_field defines, by brute force: the squared cell distance to the nearest blocking cell, -1 for none"""
    ys, xs = known.shape
    walls = np.argwhere(~(known.astype(np.float64) / 100.0 < thr))
    sq = np.full((ys, xs), -1, dtype=np.int32)
    if len(walls):
        i, j = np.indices((ys, xs))
        d = (i[..., None] - walls[:, 0]) ** 2 + (j[..., None] - walls[:, 1]) ** 2
        sq = d.min(axis=2).astype(np.int32)
    return sq


@functools.lru_cache(maxsize=None)
def revealed_scene():
    """2 T rows by T + 16 columns, three robots with a sensor of 10 cells in a map with two walls: the frontier is the rims of
    the revealed discs.  The clearance plane is the building plan's (the true walls, which the fleet has although it has not
    seen them all): two pillars stand one cell outside the second robot's range, left and right of it, so the rim's two tips
    there are members within clear_sq of a wall -- geo -1 in the partition (unknown cells block) --, which cuts that rim into
    two regions; and a rim in the open has several cells at its least cost"""
    ys, xs, R = 2 * T, T + 16, 10
    g = gs.geom(xs, ys)
    truth = np.zeros((ys, xs), dtype=np.int8)
    truth[14, 10:40] = 100                                                  # through the first robot's disc
    truth[T + 4:T + 30, 30] = 100                                           # beside the third's
    truth[T + 2, 12 - R - 1] = truth[T + 2, 12 + R + 1] = 100               # the pillars
    poses = np.array([gs.centre(g, 18, 20), gs.centre(g, T + 2, 12), gs.centre(g, T + 16, 36)])
    known = np.full_like(truth, -1)
    sr.reveal(g, R, truth, known, poses)
    assert known[T + 2, 12 - R - 1] == -1 and known[T + 2, 12 + R + 1] == -1
    sq = _squared_distances(truth, g.occupied_threshold)
    clear_sq = 2
    cost, owner, n_src = part.partition(g, known, poses=poses, sq=sq, clear_sq=clear_sq, flags=geo.UNKNOWN_BLOCKS)
    assert n_src == 3
    for a in (truth, known, sq, cost, owner, poses):
        a.setflags(write=False)
    return Revealed(g, truth, known, poses, R, sq, clear_sq, cost, owner)

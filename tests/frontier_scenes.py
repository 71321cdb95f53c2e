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


# ---- scenes past the sizes at which the kernels take another path -------------------------------------------------------------
# frontier_rank_kernel sums share = (chunks - 1) / 256 + 1 consecutive chunks of 1024 cells per thread: only past 256 * 1024
# cells is share >= 2 (here 2), do the trailing threads clamp lo / hi, and does a scatter workgroup read an offset its rank
# thread wrote on the second turn of its loop.  Built on first use, like the others
RANK_SINGLE_SHARE_CELLS = 256 * 1024
LARGE_YS, LARGE_XS = 506, 520      # 257 chunks (thread 128 of the rank scan owns one trailing chunk), 16 x 17 tiles, ragged both ways


def _large(f):
    def build():
        m = np.asarray(f())
        assert m.size > RANK_SINGLE_SHARE_CELLS, "the rank kernel's share must be >= 2: more than 256 chunks of 1024 cells"
        return m
    return _frozen(build)


def _large_every_third():
    m = np.zeros((LARGE_YS, LARGE_XS), dtype=np.int8)
    m[0::3, 0::3] = 1
    return m


def _large_rows():
    """33 rows of 8192 columns (the widest grid the entry takes): 256 x 2 tiles, the second tile row one cell high, 264 chunks.
    Row 0 is one region, united only westwards across 256 tiles; row 2 holds 4096 regions of one cell; row 32 holds runs of 63
    members and one gap: a run that starts on a tile's first column crosses the next tile border in its middle"""
    m = np.zeros((T + 1, capi.DISTANCE_MAX_SIDE), dtype=np.int8)
    m[0, :] = 1
    m[2, 0::2] = 1
    m[T, :] = np.arange(m.shape[1]) % 64 != 63
    return m


def _large_random(density, seed):
    return lambda: (np.random.default_rng(seed).random((LARGE_YS, LARGE_XS)) < density).astype(np.int8) * np.int8(-5)


LARGE_MASKS = {
    "large_every_third": _large(_large_every_third),                       # 29 406 regions of one cell: ranks through every offset
    "large_serpentine": _large(lambda: fr.serpentine_mask(LARGE_YS, LARGE_XS)),  # one region through all 272 tiles: deep trees
    "large_rows": _large(_large_rows),
    "large_random_05": _large(_large_random(0.05, 41)),
    "large_random_45": _large(_large_random(0.45, 42)),
}


@functools.lru_cache(maxsize=None)
def large_mask_regions(name, max_regions=None):
    """fr.regions_fast of a large mask, computed once per (scene, max_regions); read-only"""
    out = fr.regions_fast(fr.OF_MASK, LARGE_MASKS[name](), THR, max_regions=max_regions)
    for a in out:
        a.setflags(write=False)
    return out


LargeRevealed = collections.namedtuple("LargeRevealed", "g truth known poses R sq clear_sq geo owner n_src")


@functools.lru_cache(maxsize=None)
def large_revealed():
    """506 x 520: border walls, four long walls with gaps and 1 % clutter; 300 robots on free cells with a sensor of 10 cells.
    300 sources are two workgroups of the seed and goal launches (a lane per source or label, 256 per workgroup), and the map
    spans 16 x 17 tiles of the round machinery.  Robots 298 and 299 stand in the cells of robots 0 and 1: labels that own no
    cell.  The clearance plane is the true walls', as in revealed_scene"""
    from tests import distance_restatement as dr
    ys, xs, R, P = LARGE_YS, LARGE_XS, 10, 300
    assert ys * xs > RANK_SINGLE_SHARE_CELLS, "the rank kernel's share must be >= 2: more than 256 chunks of 1024 cells"
    g = gs.geom(xs, ys)
    rng = np.random.default_rng(506520)
    truth = np.zeros((ys, xs), dtype=np.int8)
    truth[rng.random((ys, xs)) < 0.01] = 100
    truth[0, :] = truth[-1, :] = truth[:, 0] = truth[:, -1] = 100
    truth[120, 30:400] = truth[300, 100:500] = 100
    truth[40:380, 170] = truth[150:480, 350] = 100
    truth[120, 90:96] = truth[120, 250:256] = truth[300, 200:206] = truth[300, 420:426] = 0
    truth[200:206, 170] = truth[330:336, 170] = truth[220:226, 350] = truth[400:406, 350] = 0
    free = np.argwhere(truth == 0)
    at = free[np.sort(rng.choice(len(free), size=P - 2, replace=False))]
    at = np.concatenate([at, at[:2]])
    poses = np.array([gs.centre(g, int(i), int(j)) for i, j in at])
    poses[:, 2] = rng.uniform(-3, 3, P)
    known = np.full_like(truth, -1)
    sr.reveal(g, R, truth, known, poses)
    sq = dr.separable(truth, g.occupied_threshold)[0]
    clear_sq = 2
    cost, owner, n_src = part.partition(g, known, poses=poses, sq=sq, clear_sq=clear_sq, flags=geo.UNKNOWN_BLOCKS)
    assert n_src == P and not (owner == P - 1).any() and not (owner == P - 2).any() and (owner == P - 3).any()
    for a in (truth, known, sq, cost, owner, poses):
        a.setflags(write=False)
    return LargeRevealed(g, truth, known, poses, R, sq, clear_sq, cost, owner, n_src)


@functools.lru_cache(maxsize=None)
def large_revealed_regions():
    """fr.regions_fast of large_revealed() with the partition's planes, computed once; read-only"""
    sc = large_revealed()
    out = fr.regions_fast(fr.OF_GRID, sc.known, sc.g.occupied_threshold, geo=sc.geo, owner=sc.owner)
    for a in out:
        a.setflags(write=False)
    return out


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

"""The scenes tests/test_goto.py (CPU) and tests/test_gpu_goto.py share: the smallest shapes at which the window kernel of
eea_geodesic_goto_batch can go wrong.  A scene is a grid, the robots with their goals and what one call is given; a family of
scenes shares the grid and the robots and differs in the margin or the flags.  Read-only, computed once."""
import collections
import functools

import numpy as np

from tests import frontier_scenes as fs
from tests import gain_scenes as gs
from tests import geodesic_restatement as geo
from tests import goto_restatement as gr

Scene = collections.namedtuple("Scene", "g grid poses goals margin n_steps sq clear_sq flags mask")
MARGIN_MAX = 0xFFFFFFFF
MAX_BLOCKS = 2048                       # the workgroups of the largest launch (csrc/common.hpp, kGotoMaxBlocks)


def _poses(g, cells):
    """robots at cell centres (a pair of floats is a world point as it is), headings that differ"""
    out = [gs.centre(g, int(c[0]), int(c[1])) if isinstance(c[0], (int, np.integer)) else [c[0], c[1], 0.0] for c in cells]
    out = np.array(out, dtype=np.float64)
    out[:, 2] = -2.5 + 0.37 * (np.arange(len(out)) % 14)
    return out


def _scene(g, grid, pairs, margin, n_steps, sq=None, clear_sq=0, flags=0, mask=None):
    """pairs: (robot, goal), a robot a cell (i, j) or a world point, a goal a cell (i, j) or a raw index"""
    goals = [k[0] * g.xsize + k[1] if isinstance(k, tuple) else k for _, k in pairs]
    return Scene(g, grid, _poses(g, [r for r, _ in pairs]), np.array(goals, dtype=np.int32), margin, n_steps, sq, clear_sq, flags,
                 None if mask is None else np.array(mask, dtype=np.int32))


# ---- open: 40 x 37, free ---------------------------------------------------------------------------------------------------
OPEN_PAIRS = [((0, 0), (36, 39)), ((36, 39), (0, 0)), ((0, 39), (36, 0)), ((36, 0), (0, 39)),      # corners
              ((0, 20), (18, 0)), ((36, 5), (20, 39)),                                            # edges
              ((2, 2), (6, 7)), ((34, 37), (30, 30)),                                             # margin 5 clips two sides each
              ((0, 10), (3, 12)), ((10, 0), (12, 3)), ((36, 20), (33, 22)), ((20, 39), (22, 36)),  # margin 1 clips one side each
              ((15, 15), (15, 15)), ((0, 0), (0, 0)),                                             # robot == goal
              ((10, 5), (10, 30)), ((5, 12), (30, 12)), ((10, 30), (10, 5)), ((30, 12), (5, 12)),  # collinear: 1 x N, N x 1
              ((20, 20), (27, 31)), ((27, 31), (20, 20)), ((25, 10), (12, 17)), ((12, 30), (25, 22)),  # many equal-cost moves
              ((8, 8), (9, 9)), ((9, 9), (8, 8)), ((8, 9), (9, 8)), ((9, 8), (8, 9))]              # one diagonal move each way


def _open(margin):
    g = gs.geom(40, 37)
    return _scene(g, np.zeros((37, 40), dtype=np.int8), OPEN_PAIRS, margin, 12)


# ---- wall: a wall with a gap below, a sealed triangle behind a diagonal wall, a one-sided corner -----------------------------
WALL_PAIRS = [((5, 10), (5, 20)), ((3, 10), (8, 20)), ((8, 20), (3, 10)),      # the gap (rows 20-23) is 12 rows below the box
              ((1, 1), (4, 4)), ((4, 4), (1, 1)), ((1, 3), (2, 4)),             # across the diagonal wall: only by cutting corners
              ((12, 2), (13, 3)), ((13, 3), (12, 2)),                           # one blocked cell beside the diagonal: 10, not 7
              ((19, 14), (19, 16)), ((21, 13), (21, 17))]                       # beside the wall's end and through the gap


def _wall(margin):
    g = gs.geom(30, 24)
    grid = np.zeros((24, 30), dtype=np.int8)
    grid[0:20, 15] = 100
    for k in range(6):
        grid[k, 5 - k] = 100
    grid[12, 3] = 100
    return _scene(g, grid, WALL_PAIRS, margin, 40)


# ---- serpentine: the path is many times the window's side --------------------------------------------------------------------
def _serpentine(margin):
    g = gs.geom(31, 31)
    grid = geo.serpentine(31, 31).copy()
    pairs = [((0, 0), (30, 30)), ((30, 30), (0, 0)), ((0, 1), (15, 29)), ((15, 13), (16, 17)), ((0, 0), (0, 30))]
    return _scene(g, grid, pairs, margin, 300)


# ---- waivers: unknown cells, a clearance band, robots and goals on cells nothing may enter, and the statuses -----------------
def _waivers(flags):
    g = gs.geom(22, 20)
    grid = np.zeros((20, 22), dtype=np.int8)
    grid[:, 8] = -1                                                             # an unknown strip, the grid's height
    grid[15, 10:20] = 100                                                       # a wall; with clear_sq = 1 its band is rows 14-16
    grid[3, 14] = 79
    grid[3, 15] = 80                                                            # the 79 / 80 pair: 0.79 < 0.8 passes, 0.80 blocks
    sq = fs._squared_distances(grid, g.occupied_threshold)
    nan = float("nan")
    pairs = [((5, 3), (5, 12)),                                                 # across the strip
             ((5, 3), (5, 8)), ((7, 8), (7, 3)), ((9, 8), (11, 8)), ((12, 8), (12, 8)),   # goal / robot / both on unknown cells
             ((14, 12), (12, 17)), ((18, 13), (16, 16)), ((14, 11), (14, 12)), ((16, 18), (14, 18)),   # ... in the band
             ((13, 12), (17, 12)),                                              # round the wall's end, through the band: no
             ((2, 14), (4, 14)), ((2, 15), (4, 15)), ((3, 14), (3, 13)),        # over the 79 cell; the 80 cell blocks
             ((6, 12), (15, 12)), ((6, 12), (3, 15)), ((15, 13), (6, 12)), ((3, 15), (6, 12)),    # blocking goal, blocking robot cell
             ((6, 12), -1), ((6, 12), 22 * 20), ((6, 12), -(1 << 31)), ((6, 12), (1 << 31) - 1),  # goal outside the grid
             ((-3.0e3, 0.5), (6, 12)), ((1.0e300, 0.5), (6, 12)), ((nan, 0.5), (1, 2)), ((nan, nan), (2, 1)), ((0.5, nan), (0, 0)),
             ((6, 13), (9, 16)), ((6, 13), (9, 16))]                            # the last one is masked out
    mask = [1] * (len(pairs) - 1) + [0]
    mask[3] = 7                                                                 # (any non-zero word)
    return _scene(g, grid, pairs, 3, 9, sq=sq, clear_sq=1, flags=flags, mask=mask)


# ---- cap: 130 x 130, free ----------------------------------------------------------------------------------------------------
def _cap(margin):
    g = gs.geom(130, 130)
    pairs = {0: [((0, 0), (127, 127)), ((0, 0), (127, 128)), ((0, 0), (128, 127)), ((129, 129), (2, 2)), ((1, 0), (1, 129))],
             50: [((0, 0), (60, 60)), ((0, 0), (127, 127)), ((129, 129), (69, 75))],
             MARGIN_MAX: [((3, 3), (5, 5))]}[margin]
    return _scene(g, np.zeros((130, 130), dtype=np.int8), pairs, margin, 6)


# ---- many: 96 x 96 with random obstacles; more robots than the largest launch has workgroups ---------------------------------
def _many():
    rng = np.random.default_rng(96)
    g = gs.geom(96, 96)
    grid = np.where(rng.random((96, 96)) < 0.2, 100, 0).astype(np.int8)
    grid[rng.random((96, 96)) < 0.05] = -1
    P = 3000
    assert P > MAX_BLOCKS
    at = rng.integers(0, 96, size=(P, 2))
    to = np.clip(at + rng.integers(-7, 8, size=(P, 2)), 0, 95)
    to[:24] = rng.integers(0, 96, size=(24, 2))                                  # a few goals anywhere: large windows
    pairs = [((int(a[0]), int(a[1])), (int(b[0]), int(b[1]))) for a, b in zip(at, to)]
    return _scene(g, grid, pairs, 2, 5, flags=geo.UNKNOWN_BLOCKS, mask=(rng.random(P) < 0.9).astype(np.int32))


def _stride():
    """5000 robots on a 64 x 64 grid, windows of at most 3 x 3 cells: every workgroup of the largest launch takes a second and a
    third robot"""
    rng = np.random.default_rng(5000)
    g = gs.geom(64, 64)
    grid = np.where(rng.random((64, 64)) < 0.25, 100, 0).astype(np.int8)
    P = 5000
    at = rng.integers(0, 64, size=(P, 2))
    to = np.clip(at + rng.integers(-2, 3, size=(P, 2)), 0, 63)
    pairs = [((int(a[0]), int(a[1])), (int(b[0]), int(b[1]))) for a, b in zip(at, to)]
    return _scene(g, grid, pairs, 0, 2)


_BUILDERS = {"open_m0": lambda: _open(0), "open_m1": lambda: _open(1), "open_m5": lambda: _open(5), "open_mmax": lambda: _open(MARGIN_MAX),
             "wall_m0": lambda: _wall(0), "wall_m11": lambda: _wall(11), "wall_m12": lambda: _wall(12),
             "serpentine_m0": lambda: _serpentine(0), "serpentine_m2": lambda: _serpentine(2),
             "waivers_pass": lambda: _waivers(0), "waivers_block": lambda: _waivers(geo.UNKNOWN_BLOCKS),
             "cap_m0": lambda: _cap(0), "cap_m50": lambda: _cap(50), "cap_mmax": lambda: _cap(MARGIN_MAX),
             "many": _many, "stride": _stride}
NAMES = sorted(_BUILDERS)
UNTOUCHED = (0x6B0B0B0B, 0x5C5C5C5C, -7.25e33, 0x7BCDEF01)       # what a masked-out robot's elements hold before and after


@functools.lru_cache(maxsize=None)
def scene(name):
    sc = _BUILDERS[name]()
    for a in (sc.grid, sc.poses, sc.goals) + tuple(a for a in (sc.sq, sc.mask) if a is not None):
        a.setflags(write=False)
    return sc


def call_args(sc):
    """what the restatement and the entry take beside the buffers"""
    return dict(margin=sc.margin, clear_sq=sc.clear_sq, flags=sc.flags)


@functools.lru_cache(maxsize=None)
def answer(name, n_steps=None):
    """the restatement's Result for the scene (with another n_steps if given), computed once; read-only"""
    sc = scene(name)
    out = gr.goto(sc.g, sc.grid, sc.poses, sc.goals, n_steps=sc.n_steps if n_steps is None else n_steps, sq=sc.sq, mask=sc.mask,
                  untouched=UNTOUCHED, **call_args(sc))
    for a in out[:5]:
        a.setflags(write=False)
    return out

"""The geodesic field (include/ergodic_amd.h: eea_geodesic_ws_bytes, eea_geodesic_field, eea_geodesic_path_batch,
eea_set_target_reachable; csrc/geodesic_kernel.hip) without a GPU: the restatement tests/geodesic_restatement.py against a
second statement and against the closed form of the 5-7 chamfer, the path rule on random grids, a model of the device's
round schedule against the same bits, the entry points, and every refusal that comes before the device is selected."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ergodic_exploration_amd import capi

from tests import geodesic_restatement as geo
from tests import sense_restatement as sr

ENTRIES = {"eea_geodesic_ws_bytes": 2, "eea_geodesic_field": 15, "eea_geodesic_path_batch": 9, "eea_set_target_reachable": 11}
RES, XMIN, YMIN, THR = 0.25, -1.0, -2.0, 0.8


def _geom(xs, ys):
    return sr.Geometry(XMIN, YMIN, RES, xs, ys, THR)


def _random_case(seed):
    """a grid of up to 12 x 12 with walls, unknown cells and the 79 / 80 pair, a clearance plane, sources as poses and as
    cells -- some off the grid, some on blocking cells, some on cells the unknown or the clearance test would refuse"""
    rng = np.random.default_rng(seed)
    ys, xs = int(rng.integers(1, 13)), int(rng.integers(1, 13))
    g = _geom(xs, ys)
    grid = rng.choice(np.array([0, 0, 0, -1, 100, 79, 80], dtype=np.int8), size=(ys, xs))
    sq = rng.integers(-1, 6, size=(ys, xs)).astype(np.int32) if seed % 3 else None
    flags = geo.UNKNOWN_BLOCKS if seed % 2 else 0
    n = int(rng.integers(1, 4))
    poses = np.stack([XMIN + rng.uniform(-0.5, xs + 0.5, n) * RES, YMIN + rng.uniform(-0.5, ys + 0.5, n) * RES, rng.uniform(-3, 3, n)], 1)
    cells = rng.integers(-2, xs * ys + 2, size=int(rng.integers(0, 3))).astype(np.int32)
    return g, grid, dict(poses=poses, cells=cells, sq=sq, clear_sq=2, flags=flags)


@pytest.mark.parametrize("seed", range(40))
def test_dijkstra_is_the_fixed_point_of_bellman_ford(seed):
    g, grid, kw = _random_case(seed)
    got, n_src = geo.field(g, grid, **kw)
    assert np.array_equal(got, geo.bellman_ford(g, grid, **kw))
    assert n_src == len(geo.source_cells(g, grid, kw["poses"], kw["cells"]))
    trav = geo.traversable(g, grid, kw["sq"], kw["clear_sq"], kw["flags"])
    src = set(geo.source_cells(g, grid, kw["poses"], kw["cells"]))
    assert ((got >= 0) <= (trav | (got == 0))).all()                       # a value only on traversable cells and sources
    assert all(got[c] == 0 for c in src) and {tuple(c) for c in np.argwhere(got == 0)} == src


def test_costs_on_an_empty_grid_are_the_chamfer():
    g = _geom(17, 13)
    grid = np.zeros((13, 17), dtype=np.int8)
    got, n_src = geo.field(g, grid, cells=np.array([5 * 17 + 6], dtype=np.int32))
    di, dj = np.abs(np.arange(13) - 5)[:, None], np.abs(np.arange(17) - 6)[None, :]
    assert n_src == 1 and np.array_equal(got, 5 * np.maximum(di, dj) + 2 * np.minimum(di, dj))


def test_no_corner_cutting_and_waived_sources():
    """a diagonal gap between two wall cells is closed; a source on a cell the clearance refuses is seeded and left, but
    nothing moves into or diagonally past it"""
    g = _geom(4, 4)
    grid = np.zeros((4, 4), dtype=np.int8)
    grid[1:, 2] = 100                                                      # a wall with a door at (0, 2)
    got, _ = geo.field(g, grid, cells=np.array([0], dtype=np.int32))
    assert got[0, 1] == 5 and got[0, 2] == 10 and got[0, 3] == 15 and got[1, 3] == 20     # round the corner, never across it
    grid2 = np.zeros((3, 3), dtype=np.int8)
    grid2[0, 1], grid2[1, 0] = 100, 100
    g3 = _geom(3, 3)
    assert (geo.field(g3, grid2, cells=np.array([0], dtype=np.int32))[0] == np.array([[0, -1, -1]] + [[-1] * 3] * 2)).all()
    sq = np.full((3, 3), 9, dtype=np.int32)
    sq[1, 1] = 1                                                           # the centre fails the clearance
    free = np.zeros((3, 3), dtype=np.int8)
    from_centre, _ = geo.field(g3, free, cells=np.array([4], dtype=np.int32), sq=sq, clear_sq=1)
    assert np.array_equal(from_centre, [[7, 5, 7], [5, 0, 5], [7, 5, 7]])
    from_corner, _ = geo.field(g3, free, cells=np.array([0, 4], dtype=np.int32), sq=sq, clear_sq=1)
    assert np.array_equal(from_corner, [[0, 5, 7], [5, 0, 5], [7, 5, 7]])
    only_corner, _ = geo.field(g3, free, cells=np.array([0], dtype=np.int32), sq=sq, clear_sq=1)
    assert np.array_equal(only_corner, [[0, 5, 10], [5, -1, 15], [10, 15, 20]])


@pytest.mark.parametrize("seed", range(40))
def test_every_reachable_cell_has_a_path_step(seed):
    """on random grids (waived sources included) every reachable non-source cell has a step by the path rule, costs fall
    strictly along the path, it ends on a geo == 0 cell, every move is legal, and the way-points are the cells' centres"""
    g, grid, kw = _random_case(seed)
    field, _ = geo.field(g, grid, **kw)
    trav = geo.traversable(g, grid, kw["sq"], kw["clear_sq"], kw["flags"])
    n_steps = g.xsize * g.ysize
    for i, j in np.argwhere(field > 0):
        steps = geo.path_cells(field, int(i), int(j), n_steps)
        assert steps, (i, j)
        cells = [(int(i), int(j))] + [(a, b) for a, b, _ in steps]
        costs = [int(field[c]) for c in cells]
        assert all(x > y for x, y in zip(costs, costs[1:])) and costs[-1] == 0
        assert all(geo.legal_move(trav, field, a, b) for a, b in zip(cells, cells[1:]))
        pose = [XMIN + (j + 0.3) * RES, YMIN + (i + 0.6) * RES, 0.7]
        p, n = geo.path(g, field, [pose], len(steps) + 2)
        assert n[0] == len(steps) and np.array_equal(p[0, -1], p[0, len(steps) - 1])
        assert tuple(p[0, len(steps) - 1, :2]) == geo.cell_centre(g, *cells[-1])
        assert p[0, 0, 2] == geo.HEADINGS[steps[0][2]]
    for k, (di, dj) in enumerate(geo.MOVES):
        assert abs(geo.HEADINGS[k] - np.arctan2(di, dj)) < 1e-15 or (k == 2 and geo.HEADINGS[k] == -np.pi)
    off = geo.path(g, field, [[XMIN - 1.0, YMIN, 0.2]], 3)
    assert off[1][0] == -1 and (off[0][0] == [XMIN - 1.0, YMIN, 0.2]).all()


@pytest.mark.parametrize("seed", range(12))
def test_the_round_schedule_ends_at_dijkstra(seed):
    """tiles relaxed round by round from the halo as it stood before the round (geodesic_restatement.tile_rounds, the device's
    schedule at its most stale) end at the same bits; a budgeted run only holds -1 or upper bounds, and continuing it -- also with
    a source added -- ends at the bits of a fresh run"""
    rng = np.random.default_rng(100 + seed)
    ys, xs = int(rng.integers(5, 20)), int(rng.integers(5, 20))
    g = _geom(xs, ys)
    grid = rng.choice(np.array([0, 0, 0, 0, -1, 100], dtype=np.int8), size=(ys, xs))
    cells = rng.integers(0, xs * ys, size=2).astype(np.int32)
    want, _ = geo.field(g, grid, cells=cells[:1])
    got, final, _ = geo.tile_rounds(g, grid, 4, 3, cells=cells[:1])
    assert final and np.array_equal(got, want)
    part, _, _ = geo.tile_rounds(g, grid, 4, 3, cells=cells[:1], max_rounds=1)
    assert ((part == -1) | (part >= want)).all() and (part[want == -1] == -1).all()
    assert np.array_equal(geo.tile_rounds(g, grid, 4, 3, cells=cells[:1], start=part)[0], want)
    assert np.array_equal(geo.tile_rounds(g, grid, 4, 3, cells=cells, start=part)[0], geo.field(g, grid, cells=cells)[0])


def test_one_round_cannot_finish_a_serpentine():
    grid = geo.serpentine(40, 33)
    g = _geom(40, 33)
    want, _ = geo.field(g, grid, cells=np.array([0], dtype=np.int32))
    got, final, rounds = geo.tile_rounds(g, grid, 8, 8, cells=np.array([0], dtype=np.int32))
    assert final and np.array_equal(got, want) and rounds > 10 and want[0, 39] > 5 * 9 * 30
    assert not geo.tile_rounds(g, grid, 8, 8, cells=np.array([0], dtype=np.int32), max_rounds=1)[1]


def test_entries_are_declared_exported_and_bound(tmp_path):
    raw = C.CDLL(capi.LIB_PATH)
    L = capi.lib()
    for name, n_args in ENTRIES.items():
        assert name in capi.declared_symbols() and hasattr(raw, name), name
        assert len(getattr(L, name).argtypes) == n_args, name
    for name in ("geodesic_ws_bytes", "geodesic_field", "geodesic_path_batch"):
        assert callable(getattr(capi, name)), name
    assert callable(capi.Engine.set_target_reachable)
    assert L.eea_abi_version() == 6
    src = tmp_path / "tile.c"
    src.write_text('#include <stdio.h>\n#include "ergodic_amd.h"\nint main(void) {\n'
                   'printf("%d %d %d %d\\n", EEA_GEODESIC_TILE_X, EEA_GEODESIC_TILE_Y, EEA_GEODESIC_UNKNOWN_BLOCKS, EEA_GEODESIC_CONTINUE);\n'
                   'return 0; }\n')
    exe = tmp_path / "tile"
    subprocess.run(["gcc", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)], check=True)
    got = [int(w) for w in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [capi.GEODESIC_TILE_X, capi.GEODESIC_TILE_Y, capi.GEODESIC_UNKNOWN_BLOCKS, capi.GEODESIC_CONTINUE]
    assert got[0] >= 1 and got[1] >= 1


def test_workspace_bytes_are_positive_and_monotone():
    sizes = [(1, 1), (1, 33), (33, 1), (33, 33), (64, 41), (200, 100), (1024, 1024), (8192, 8192)]
    got = [capi.geodesic_ws_bytes(capi.make_collision_cfg(0.0, 0.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 0.8)) for xs, ys in sizes]
    assert got[0] > 0 and all(a <= b for a, b in zip(got, got[1:])) and got[-1] > got[0]
    assert all(b >= xs * ys for b, (xs, ys) in zip(got, sizes))
    L = capi.lib()
    good = capi.make_collision_cfg(0.0, 0.0, 0.1, 8, 8, 0.7, 1.0, 0.2, 0.8)
    assert L.eea_geodesic_ws_bytes(None, C.byref(C.c_size_t())) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_geodesic_ws_bytes(C.byref(good), None) == capi.ERR_INVALID_ARGUMENT


def test_argument_errors_come_before_the_device():
    """every refusal of the header is answered without a device: the buffers are host arrays that hold a sentinel nothing may
    touch, the engine is a pointer nothing may follow"""
    L = capi.lib()
    xs, ys = 40, 30
    good = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 0.8)
    grid = np.zeros(xs * ys, dtype=np.int8)
    geo_buf, sq = np.full((ys, xs), 7, dtype=np.int32), np.full((ys, xs), 7, dtype=np.int32)
    ws, state = np.full(capi.geodesic_ws_bytes(good), 7, dtype=np.uint8), np.full(4, 7, dtype=np.uint32)
    pose, cells = np.zeros((2, 3)), np.zeros(2, dtype=np.int32)
    path, length = np.full((2, 5, 3), 7.0), np.full(2, 7, dtype=np.int32)
    field = np.full((ys, xs), 7, dtype=np.uint32)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    ref = lambda c: None if c is None else C.byref(c)
    INV, UNS = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED

    def build(cfg=good, g=grid, s=sq, clear=4, flags=0, ps=pose, P=2, cl=cells, n=2, rounds=3, out=geo_buf, w=ws, st=state):
        return L.eea_geodesic_field(0, ref(cfg), p(g), p(s), clear, flags, p(ps), P, p(cl), n, rounds, p(out), p(w), p(st), None)

    def walk(cfg=good, gf=geo_buf, ps=pose, P=2, n_steps=5, out=path, ln=length):
        return L.eea_geodesic_path_batch(0, ref(cfg), p(gf), p(ps), P, n_steps, p(out), p(ln), None)

    def target(e=C.c_void_p(64), cfg=good, kind=0, f=field, stride=2, known=grid, gf=geo_buf, floor=0.5, lx=3.9, ly=2.9):
        return L.eea_set_target_reachable(e, ref(cfg), kind, p(f), stride, p(known), p(gf), floor, lx, ly, None)

    assert build(cfg=None) == INV and walk(cfg=None) == INV and target(cfg=None) == INV
    for kw in (dict(g=None), dict(out=None), dict(w=None), dict(st=None)):
        assert build(**kw) == INV and b"null" in L.eea_last_error(), kw
    for kw in (dict(ps=None, cl=None), dict(P=0, n=0), dict(ps=None, n=0), dict(P=0, cl=None)):
        assert build(**kw) == INV and b"source" in L.eea_last_error(), kw
        assert build(flags=capi.GEODESIC_UNKNOWN_BLOCKS, **kw) == INV
    assert build(clear=-1) == INV and b"clear_sq" in L.eea_last_error()
    assert L.eea_geodesic_field(0, ref(good), p(grid), None, 0, 0, p(pose), 2, None, 0, 3, p(geo_buf), C.c_void_p(ws.ctypes.data + 2),
                                p(state), None) == INV and b"aligned" in L.eea_last_error()
    assert build(flags=4) == INV and build(flags=1 << 31) == INV and b"flag" in L.eea_last_error()
    for kw in (dict(gf=None), dict(ps=None), dict(out=None)):
        assert walk(**kw) == INV and b"null" in L.eea_last_error(), kw
    assert walk(n_steps=0) == INV and walk(n_steps=0, P=0) == INV and b"n_steps" in L.eea_last_error()
    assert walk(P=0) == capi.OK and walk(P=0, ln=None) == capi.OK
    for kw in (dict(e=None), dict(f=None), dict(known=None), dict(gf=None)):
        assert target(**kw) == INV and b"null" in L.eea_last_error(), kw
    assert target(kind=2) == INV and target(kind=-1) == INV and b"kind" in L.eea_last_error()
    assert target(stride=0) == INV and b"stride" in L.eea_last_error()
    for bad in (-0.5, float("nan"), float("inf")):
        assert target(floor=bad) == INV and b"floor" in L.eea_last_error(), bad
    for kw in (dict(lx=0.0), dict(ly=-1.0), dict(lx=float("nan"))):
        assert target(**kw) == INV, kw
    # the configuration errors of the distance calls
    swapped = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 1.0, 0.7, 0.2, 0.8)
    assert build(cfg=swapped) == INV and walk(cfg=swapped) == INV and b"Search radius" in L.eea_last_error()
    for bad in (capi.make_collision_cfg(-2.0, -1.0, 0.1, 0, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, 0, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.0, xs, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 100.5)):
        assert build(cfg=bad) == INV and walk(cfg=bad) == INV
    for bad in (capi.make_collision_cfg(-2.0, -1.0, 0.1, 0, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.0, xs, ys, 0.7, 1.0, 0.2, 0.8)):
        assert target(cfg=bad) == INV
    # the limits: a side above EEA_DISTANCE_MAX_SIDE, more than 2^26 cells (8192 x 8192 is exactly 2^26: accepted)
    side = capi.DISTANCE_MAX_SIDE
    for big, word in ((capi.make_collision_cfg(-2.0, -1.0, 0.1, side + 1, 4, 0.7, 1.0, 0.2, 0.8), b"EEA_DISTANCE_MAX_SIDE"),
                      (capi.make_collision_cfg(-2.0, -1.0, 0.1, 4, side + 1, 0.7, 1.0, 0.2, 0.8), b"EEA_DISTANCE_MAX_SIDE")):
        assert build(cfg=big) == UNS and word in L.eea_last_error()
        assert walk(cfg=big) == UNS and L.eea_geodesic_ws_bytes(C.byref(big), C.byref(C.c_size_t())) == UNS
    assert side * side == 1 << 26 and 7 * (1 << 26) < 1 << 31
    widest = capi.make_collision_cfg(-2.0, -1.0, 0.1, side, side, 0.7, 1.0, 0.2, 0.8)
    assert walk(cfg=widest, P=0) == capi.OK
    huge = capi.make_collision_cfg(0.0, 0.0, 0.1, 1 << 16, (1 << 15) + 1, 0.7, 0.1, 0.2, 0.8)
    assert target(cfg=huge) == UNS and b"2^31" in L.eea_last_error()
    for a, v in ((geo_buf, 7), (sq, 7), (ws, 7), (state, 7), (path, 7.0), (length, 7), (field, 7)):
        assert (a == v).all()
    assert not grid.any() and not pose.any() and not cells.any()


def test_geodesic_kernels_are_in_the_library():
    """the kernels of csrc/geodesic_kernel.hip are gfx950 code in the build and use no scratch; a round's tile with its halo is
    static LDS well inside 64 KB"""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import kernel_resources as kr
    obj = os.path.join(os.path.dirname(capi.LIB_PATH), "..", "csrc", "build", "geodesic_kernel.o")
    names = {}
    for k in kr.kernels(obj):
        if "vgpr_count" in k:
            names[subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.strip()] = k
    for w in ("geodesic_init_kernel(", "geodesic_seed_kernel(", "geodesic_round_kernel(", "geodesic_close_kernel(",
              "geodesic_path_kernel(", "reachable_values_kernel<double, unsigned int>(", "reachable_values_kernel<float, double>("):
        found = [k for n, k in names.items() if w in n]
        assert len(found) == 1, (w, sorted(names))
        assert int(found[0]["private_segment_fixed_size"]) == 0, found[0]
    tile = (capi.GEODESIC_TILE_X + 2) * (capi.GEODESIC_TILE_Y + 2)
    lds = int([k for n, k in names.items() if "geodesic_round_kernel(" in n][0]["group_segment_fixed_size"])
    assert 5 * tile <= lds <= 8 * 1024          # (an int and a byte per staged cell, and the words of the workgroup's votes)

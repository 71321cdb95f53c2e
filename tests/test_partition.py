"""The geodesic partition (include/ergodic_amd.h: eea_partition_ws_bytes, eea_geodesic_partition, eea_partition_goals,
eea_partition_path_batch; csrc/partition_kernel.hip) without a GPU: the restatement tests/partition_restatement.py against a
second statement built from single-source fields of tests/geodesic_restatement.py, a model of the device's round schedule on
keys against the same bits, the owner-constrained descent, goals and reversed paths on random grids, the entry points, and
every refusal that comes before the device is selected."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from ergodic_exploration_amd import capi

from tests import geodesic_restatement as geo
from tests import partition_restatement as part
from tests import sense_restatement as sr

ENTRIES = {"eea_partition_ws_bytes": 2, "eea_geodesic_partition": 16, "eea_partition_goals": 15, "eea_partition_path_batch": 11}
RES, XMIN, YMIN, THR = 0.25, -1.0, -2.0, 0.8
SEEDS = range(48)


def _geom(xs, ys):
    return sr.Geometry(XMIN, YMIN, RES, xs, ys, THR)


@functools.lru_cache(maxsize=None)
def _random_case(seed):
    """test_geodesic.py's random grids (walls, unknown cells, the 79 / 80 pair, a clearance plane; sources off the grid, on
    blocking cells, on cells the unknown or the clearance test would refuse) with more sources, and every third seed a cell
    source put on the first pose's cell: two labels in one cell"""
    rng = np.random.default_rng(1000 + seed)
    ys, xs = int(rng.integers(1, 13)), int(rng.integers(1, 13))
    g = _geom(xs, ys)
    grid = rng.choice(np.array([0, 0, 0, 0, -1, 100, 79, 80], dtype=np.int8), size=(ys, xs))
    sq = rng.integers(-1, 6, size=(ys, xs)).astype(np.int32) if seed % 3 else None
    flags = geo.UNKNOWN_BLOCKS if seed % 2 else 0
    n = int(rng.integers(1, 5))
    poses = np.stack([XMIN + rng.uniform(-0.5, xs + 0.5, n) * RES, YMIN + rng.uniform(-0.5, ys + 0.5, n) * RES, rng.uniform(-3, 3, n)], 1)
    cells = rng.integers(-2, xs * ys + 2, size=int(rng.integers(0, 4))).astype(np.int32)
    if seed % 3 == 0:
        i, j = sr.world2grid(g, poses[0][0], poses[0][1])
        if i <= ys - 1 and j <= xs - 1:
            cells = np.append(cells, np.int32(i * xs + j))
    kw = dict(poses=poses, cells=cells, sq=sq, clear_sq=2, flags=flags)
    return g, grid, kw, part.partition(g, grid, **kw)


@pytest.mark.parametrize("seed", SEEDS)
def test_two_statements_agree_and_the_cost_plane_is_the_plain_field(seed):
    g, grid, kw, (cost, owner, n_src) = _random_case(seed)
    plain, plain_src = geo.field(g, grid, **kw)
    assert np.array_equal(cost, plain) and n_src == plain_src
    cost2, owner2 = part.by_single_sources(g, grid, **kw)
    assert np.array_equal(cost, cost2) and np.array_equal(owner, owner2)
    assert np.array_equal(owner == -1, cost == -1)
    src = part.labelled_sources(g, grid, kw["poses"], kw["cells"])
    for c in {c for _, c in src}:
        assert cost[c] == 0 and owner[c] == min(s for s, cc in src if cc == c)
    assert set(np.unique(owner)) <= {-1} | {s for s, _ in src}


def test_the_random_cases_hold_ties_shared_cells_and_refused_sources():
    ties = shared = refused = 0
    for seed in SEEDS:
        g, grid, kw, (cost, owner, n_src) = _random_case(seed)
        src = part.labelled_sources(g, grid, kw["poses"], kw["cells"])
        refused += len(kw["poses"]) + len(kw["cells"]) - len(src)
        shared += len(src) - len({c for _, c in src})
        for s, (i, j) in src:
            one, _ = geo.field(g, grid, cells=np.array([i * g.xsize + j], dtype=np.int32), sq=kw["sq"], clear_sq=2, flags=kw["flags"])
            ties += int(((one == cost) & (cost > 0) & (owner != s)).sum())
    assert ties > 50 and shared > 5 and refused > 20, (ties, shared, refused)


@pytest.mark.parametrize("seed", SEEDS)
def test_the_constrained_descent_ends_on_the_owners_cell(seed):
    """every reachable cell has a step that stays in its region, costs fall strictly, every move is legal, and the walk ends on a
    cell of the owner's own (the cost-only rule of eea_geodesic_path_batch need not: counted below)"""
    g, grid, kw, (cost, owner, _) = _random_case(seed)
    trav = geo.traversable(g, grid, kw["sq"], kw["clear_sq"], kw["flags"])
    src = dict()
    for s, c in part.labelled_sources(g, grid, kw["poses"], kw["cells"]):
        src.setdefault(c, s)
        src[c] = min(src[c], s)
    for i, j in np.argwhere(cost >= 0):
        steps = part.descend(cost, owner, int(i), int(j))
        assert steps is not None, (i, j)
        cells = [(int(i), int(j))] + [(a, b) for a, b, _ in steps]
        assert all(owner[c] == owner[i, j] for c in cells) and cost[cells[-1]] == 0 and src[cells[-1]] == owner[i, j]
        assert all(cost[a] > cost[b] for a, b in zip(cells, cells[1:]))
        assert all(geo.legal_move(trav, cost, b, a) for a, b in zip(cells, cells[1:]))      # walked forwards: b -> a


def test_the_cost_only_descent_can_end_on_another_robot():
    """why the owner condition is there: an open row, sources at both ends, the middle cell a tie owned by label 0 -- the plain
    path rule tries the move (0, +1) first and walks to label 1"""
    g = _geom(5, 1)
    grid = np.zeros((1, 5), dtype=np.int8)
    cost, owner, _ = part.partition(g, grid, cells=np.array([0, 4], dtype=np.int32))
    assert cost.tolist() == [[0, 5, 10, 5, 0]] and owner.tolist() == [[0, 0, 0, 1, 1]]
    assert geo.path_cells(cost, 0, 2, 9)[-1][:2] == (0, 4) and part.descend(cost, owner, 0, 2)[-1][:2] == (0, 0)


@pytest.mark.parametrize("seed", range(12))
def test_the_round_schedule_on_keys_ends_at_dijkstra(seed):
    """tiles relaxed round by round from the keys as they stood before the round end at the same bits; a budgeted run holds -1 /
    -1 or the cost and label of a real move sequence (cost >= the final one and >= that label's own field), nothing where the
    final field has nothing; continuing it ends at the bits of a fresh run"""
    rng = np.random.default_rng(300 + seed)
    ys, xs = int(rng.integers(5, 20)), int(rng.integers(5, 20))
    g = _geom(xs, ys)
    grid = rng.choice(np.array([0, 0, 0, 0, -1, 100], dtype=np.int8), size=(ys, xs))
    cells = rng.integers(0, xs * ys, size=4).astype(np.int32)
    cells[3] = cells[0]                                                     # two labels in one cell
    cost, owner, _ = part.partition(g, grid, cells=cells)
    got = part.tile_rounds(g, grid, 4, 3, cells=cells)
    assert got[2] and np.array_equal(got[0], cost) and np.array_equal(got[1], owner)
    p_cost, p_owner, _, _ = part.tile_rounds(g, grid, 4, 3, cells=cells, max_rounds=1)
    assert np.array_equal(p_cost == -1, p_owner == -1) and ((p_cost == -1) | (p_cost >= cost)).all() and (p_cost[cost == -1] == -1).all()
    for s in np.unique(p_owner[p_owner >= 0]):
        own, _ = geo.field(g, grid, cells=cells[s:s + 1])
        assert (own[p_owner == s] >= 0).all() and (p_cost[p_owner == s] >= own[p_owner == s]).all()
    again = part.tile_rounds(g, grid, 4, 3, cells=cells, start=(p_cost, p_owner))
    assert again[2] and np.array_equal(again[0], cost) and np.array_equal(again[1], owner)


def test_a_torn_key_would_stick():
    """the hazard the single 64-bit word excludes: a new cost paired with an old, smaller label is a key below every real one,
    and since keys only go down the rounds keep it"""
    g = _geom(6, 1)
    grid = np.zeros((1, 6), dtype=np.int8)
    cells = np.array([5, 0], dtype=np.int32)                                # label 0 at the right end, label 1 at the left
    cost, owner, _ = part.partition(g, grid, cells=cells)
    assert owner.tolist() == [[1, 1, 1, 0, 0, 0]]
    torn_cost, torn_owner = cost.copy(), owner.copy()
    torn_owner[0, 1] = 0                                                    # cost 5 is label 1's; label 0 never had it
    got = part.tile_rounds(g, grid, 2, 1, cells=cells, start=(torn_cost, torn_owner))
    assert got[2] and got[1][0, 1] == 0 and not np.array_equal(got[1], owner)


@pytest.mark.parametrize("seed", SEEDS)
def test_goals_are_the_argmax_with_ties(seed):
    """against a second brute force written with numpy masks: repeated field values make ties, which go to the lowest index"""
    g, grid, kw, (cost, owner, _) = _random_case(seed)
    rng = np.random.default_rng(seed)
    n_labels = len(kw["poses"]) + len(kw["cells"])
    flat_o, flat_c = owner.reshape(-1), cost.reshape(-1)
    for kind, stride, (wf, wc) in ((0, 1, (1.0, 0.0)), (1, 1, (1.0, 0.125)), (0, 3, (0.0, 1.0)), (1, 2, (0.0, 0.0))):
        fieldv = rng.integers(0, 3, size=g.xsize * g.ysize).astype(np.uint32) if kind == 0 else \
            rng.choice(np.array([0.0, 0.5, 2.5]), size=g.xsize * g.ysize)
        cell, score, area = part.goals(g, fieldv, stride, grid, cost, owner, n_labels, wf, wc)
        idx = np.arange(g.xsize * g.ysize)
        cand = ((idx % g.xsize) % stride == 0) & ((idx // g.xsize) % stride == 0) & (fieldv > 0) & \
               (grid.reshape(-1).astype(np.float64) / 100.0 < THR)
        s_all = np.float64(wf) * fieldv.astype(np.float64) - np.float64(wc) * flat_c.astype(np.float64)
        for r in range(n_labels):
            mine = cand & (flat_o == r)
            assert area[r] == (flat_o == r).sum()
            if not mine.any():
                assert cell[r] == -1 and score[r] == 0.0
            else:
                top = s_all[mine].max()
                assert score[r] == top and cell[r] == idx[mine & (s_all == top)][0]
        assert area.sum() == (flat_o >= 0).sum()


@pytest.mark.parametrize("seed", SEEDS)
def test_paths_run_from_the_robot_to_its_goal(seed):
    g, grid, kw, (cost, owner, _) = _random_case(seed)
    poses = kw["poses"]
    P = len(poses)
    trav = geo.traversable(g, grid, kw["sq"], kw["clear_sq"], kw["flags"])
    # the farthest cell of each robot's region as its goal; the last robot gets a cell of somebody else's, or none
    goal = np.full(P, -1, dtype=np.int32)
    for q in range(P):
        mine = np.argwhere(owner == q)
        if len(mine):
            i, j = mine[np.argmax(cost[tuple(mine.T)])]
            goal[q] = i * g.xsize + j
    others = np.argwhere((owner >= 0) & (owner != P - 1))
    goal[P - 1] = -1 if not len(others) or seed % 2 else others[0][0] * g.xsize + others[0][1]
    for n_steps in (1, 3, g.xsize * g.ysize):
        way, lens = part.paths(g, cost, owner, poses, goal, n_steps)
        assert lens[P - 1] == -1 and np.array_equal(way[P - 1], np.tile(poses[P - 1], (n_steps, 1)))
        for q in range(P - 1):
            if goal[q] < 0:
                assert lens[q] == -1
                continue
            i, j = sr.world2grid(g, poses[q][0], poses[q][1])
            m = len(part.descend(cost, owner, goal[q] // g.xsize, goal[q] % g.xsize))
            assert lens[q] == min(m, n_steps)
            cells = [(i, j)] + [sr.world2grid(g, x, y) for x, y, _ in way[q, :lens[q]]]
            assert all(geo.legal_move(trav, cost, a, b) for a, b in zip(cells, cells[1:]))
            assert all(owner[c] == q for c in cells)
            for (a, b), th in zip(zip(cells, cells[1:]), way[q, :lens[q], 2]):
                assert th == geo.HEADINGS[geo.MOVES.index((b[0] - a[0], b[1] - a[1]))]
            if m <= n_steps:
                assert cells[-1] == (goal[q] // g.xsize, goal[q] % g.xsize)
            if m == 0:
                assert tuple(way[q, 0]) == geo.cell_centre(g, i, j) + (poses[q][2],)
            assert (way[q, lens[q]:] == way[q, max(lens[q] - 1, 0)]).all()


def test_entries_are_declared_exported_and_bound():
    raw = C.CDLL(capi.LIB_PATH)
    L = capi.lib()
    for name, n_args in ENTRIES.items():
        assert name in capi.declared_symbols() and hasattr(raw, name), name
        assert len(getattr(L, name).argtypes) == n_args, name
    for name in ("partition_ws_bytes", "geodesic_partition", "partition_goals", "partition_path_batch"):
        assert callable(getattr(capi, name)), name
    assert L.eea_abi_version() == 6


def test_workspace_bytes_hold_a_key_per_cell_and_are_monotone():
    sizes = [(1, 1), (1, 33), (33, 1), (33, 33), (64, 41), (200, 100), (1024, 1024), (8192, 8192)]
    cfgs = [capi.make_collision_cfg(0.0, 0.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 0.8) for xs, ys in sizes]
    got = [capi.partition_ws_bytes(c) for c in cfgs]
    assert got[0] > 0 and all(a <= b for a, b in zip(got, got[1:])) and got[-1] > got[0]
    assert all(b >= 8 * xs * ys + capi.geodesic_ws_bytes(c) for b, c, (xs, ys) in zip(got, cfgs, sizes))
    L = capi.lib()
    assert L.eea_partition_ws_bytes(None, C.byref(C.c_size_t())) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_partition_ws_bytes(C.byref(cfgs[0]), None) == capi.ERR_INVALID_ARGUMENT


def test_argument_errors_come_before_the_device():
    """every refusal of the header is answered without a device: the buffers are host arrays that hold a sentinel nothing may
    touch"""
    L = capi.lib()
    xs, ys = 40, 30
    good = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 0.8)
    grid = np.zeros(xs * ys, dtype=np.int8)
    geo_buf, own_buf, sq = (np.full((ys, xs), 7, dtype=np.int32) for _ in range(3))
    ws, state = np.full(capi.partition_ws_bytes(good) + 8, 7, dtype=np.uint8), np.full(4, 7, dtype=np.uint32)
    off = (-ws.ctypes.data) % 8
    pose, cells = np.zeros((2, 3)), np.zeros(2, dtype=np.int32)
    path, length = np.full((2, 5, 3), 7.0), np.full(2, 7, dtype=np.int32)
    field = np.full((ys, xs), 7, dtype=np.uint32)
    g_cell, g_score, area = np.full(3, 7, dtype=np.int32), np.full(3, 7.0), np.full(3, 7, dtype=np.uint32)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    ref = lambda c: None if c is None else C.byref(c)
    INV, UNS = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED

    def build(cfg=good, g=grid, s=sq, clear=4, flags=0, ps=pose, P=2, cl=cells, n=2, rounds=3, out=geo_buf, own=own_buf, w=off, st=state):
        wp = None if w is None else C.c_void_p(ws.ctypes.data + w)
        return L.eea_geodesic_partition(0, ref(cfg), p(g), p(s), clear, flags, p(ps), P, p(cl), n, rounds, p(out), p(own), wp, p(st), None)

    def pick(cfg=good, kind=0, f=field, stride=2, known=grid, gf=geo_buf, own=own_buf, n=3, wf=1.0, wc=0.5, gc=g_cell, gs=g_score, ar=area):
        return L.eea_partition_goals(0, ref(cfg), kind, p(f), stride, p(known), p(gf), p(own), n, wf, wc, p(gc), p(gs), p(ar), None)

    def walk(cfg=good, gf=geo_buf, own=own_buf, ps=pose, P=2, gc=g_cell, n_steps=5, out=path, ln=length):
        return L.eea_partition_path_batch(0, ref(cfg), p(gf), p(own), p(ps), P, p(gc), n_steps, p(out), p(ln), None)

    assert build(cfg=None) == INV and pick(cfg=None) == INV and walk(cfg=None) == INV
    for kw in (dict(g=None), dict(out=None), dict(own=None), dict(w=None), dict(st=None)):
        assert build(**kw) == INV and b"null" in L.eea_last_error(), kw
    for kw in (dict(ps=None, cl=None), dict(P=0, n=0), dict(ps=None, n=0), dict(P=0, cl=None)):
        assert build(**kw) == INV and b"source" in L.eea_last_error(), kw
    assert build(clear=-1) == INV and b"clear_sq" in L.eea_last_error()
    assert build(flags=4) == INV and build(flags=1 << 31) == INV and b"flag" in L.eea_last_error()
    for w in (off + 4, off + 2, off + 1):                                   # 4-byte alignment is not enough here
        assert build(w=w) == INV and b"8-byte aligned" in L.eea_last_error(), w
    assert build(P=(1 << 31) - 1, n=1) == UNS and b"2^31 - 1" in L.eea_last_error()
    assert build(P=0xFFFFFFFF, n=0xFFFFFFFF) == UNS
    for kw in (dict(f=None), dict(known=None), dict(gf=None), dict(own=None), dict(gc=None), dict(gs=None), dict(ar=None)):
        assert pick(**kw) == INV and b"null" in L.eea_last_error(), kw
    assert pick(kind=2) == INV and pick(kind=-1) == INV and b"kind" in L.eea_last_error()
    assert pick(stride=0) == INV and b"stride" in L.eea_last_error()
    for bad in (-0.5, float("nan"), float("inf"), -float("inf"), 1.0000001e30):
        assert pick(wf=bad) == INV and b"weight" in L.eea_last_error(), bad
        assert pick(wc=bad) == INV and b"weight" in L.eea_last_error(), bad
    assert pick(n=0) == capi.OK and pick(n=0, wf=1e30, wc=0.0) == capi.OK
    for kw in (dict(gf=None), dict(own=None), dict(ps=None), dict(gc=None), dict(out=None)):
        assert walk(**kw) == INV and b"null" in L.eea_last_error(), kw
    assert walk(n_steps=0) == INV and walk(n_steps=0, P=0) == INV and b"n_steps" in L.eea_last_error()
    assert walk(P=0) == capi.OK and walk(P=0, ln=None) == capi.OK
    assert walk(P=1 << 31) == UNS and b"2^31 - 1" in L.eea_last_error()
    # the configuration errors and the limits of the geodesic calls
    swapped = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 1.0, 0.7, 0.2, 0.8)
    assert build(cfg=swapped) == INV and walk(cfg=swapped) == INV and pick(cfg=swapped) == INV and b"Search radius" in L.eea_last_error()
    for bad in (capi.make_collision_cfg(-2.0, -1.0, 0.1, 0, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, 0, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.0, xs, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 100.5)):
        assert build(cfg=bad) == INV and walk(cfg=bad) == INV and pick(cfg=bad) == INV
    side = capi.DISTANCE_MAX_SIDE
    for big in (capi.make_collision_cfg(-2.0, -1.0, 0.1, side + 1, 4, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, 4, side + 1, 0.7, 1.0, 0.2, 0.8)):
        assert build(cfg=big) == UNS and b"EEA_DISTANCE_MAX_SIDE" in L.eea_last_error()
        assert walk(cfg=big) == UNS and pick(cfg=big) == UNS and L.eea_partition_ws_bytes(C.byref(big), C.byref(C.c_size_t())) == UNS
    widest = capi.make_collision_cfg(-2.0, -1.0, 0.1, side, side, 0.7, 1.0, 0.2, 0.8)
    assert walk(cfg=widest, P=0) == capi.OK and pick(cfg=widest, n=0) == capi.OK
    for a, v in ((geo_buf, 7), (own_buf, 7), (sq, 7), (ws, 7), (state, 7), (path, 7.0), (length, 7), (field, 7), (g_cell, 7),
                 (g_score, 7.0), (area, 7)):
        assert (a == v).all()
    assert not grid.any() and not pose.any() and not cells.any()


def test_partition_kernels_are_in_the_library():
    """the kernels of csrc/partition_kernel.hip are gfx950 code in the build and use no scratch; a round's tile of keys with its
    halo is static LDS well inside 64 KB; the round kernel reads and writes the key plane with 64-bit accesses that bypass the
    L1 (the relaxed agent-scope atomics of the source), and the goal passes hold 64-bit atomic max and 32-bit atomic min"""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import kernel_resources as kr
    obj = os.path.join(os.path.dirname(capi.LIB_PATH), "..", "csrc", "build", "partition_kernel.o")
    names = {}
    for k in kr.kernels(obj):
        if "vgpr_count" in k:
            names[subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.strip()] = k
    for w in ("partition_init_kernel(", "partition_seed_kernel(", "partition_round_kernel(", "partition_close_kernel(",
              "partition_unpack_kernel(", "goals_init_kernel(", "goals_pass_kernel<unsigned int, 0>(", "goals_pass_kernel<unsigned int, 1>(",
              "goals_pass_kernel<double, 0>(", "goals_pass_kernel<double, 1>(", "goals_finish_kernel(", "partition_path_kernel("):
        found = [k for n, k in names.items() if w in n]
        assert len(found) == 1, (w, sorted(names))
        assert int(found[0]["private_segment_fixed_size"]) == 0, found[0]
    tile = (capi.GEODESIC_TILE_X + 2) * (capi.GEODESIC_TILE_Y + 2)
    lds = int([k for n, k in names.items() if "partition_round_kernel(" in n][0]["group_segment_fixed_size"])
    assert 9 * tile <= lds <= 12 * 1024         # (a key and a byte per staged cell, and the words of the workgroup's votes)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        text = subprocess.run([kr.LLVM + "/llvm-objdump", "-d", kr.code_object(obj, tmp)], check=True, capture_output=True, text=True).stdout
    body = {}
    for line in text.splitlines():
        if line.endswith(">:"):
            cur = body.setdefault(line.split("<")[1][:-2], [])
        elif line.strip() and body:
            cur.append(line.split("//")[0])
    of = lambda w: [b for n, b in body.items() if w in n]
    (rnd,) = of("partition_round_kernel")
    wide = [l for l in rnd if "global_load_dwordx2" in l or "global_store_dwordx2" in l]
    assert any("load" in l for l in wide) and any("store" in l for l in wide) and all(" sc1" in l for l in wide), wide
    assert not any("flat_" in l for l in rnd)
    (seed,) = of("partition_seed_kernel")
    assert any("global_atomic_umin_x2" in l for l in seed)
    for b in of("goals_pass_kernelIjLi0E") + of("goals_pass_kernelIdLi0E"):
        assert any("global_atomic_umax_x2" in l for l in b) and any("global_atomic_add" in l for l in b)
    for b in of("goals_pass_kernelIjLi1E") + of("goals_pass_kernelIdLi1E"):
        assert any("global_atomic_smin" in l for l in b) and not any("global_atomic_add" in l for l in b)

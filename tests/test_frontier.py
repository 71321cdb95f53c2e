"""Frontier regions (include/ergodic_amd.h: eea_frontier_ws_bytes, eea_frontier_regions, eea_frontier_goals;
csrc/frontier_kernel.hip) without a GPU: the two statements of tests/frontier_restatement.py against one another on every scene
the GPU tests draw and on random grids, the records' invariants, the goals against a second brute force, the lock-free union of
the merge launch under random interleavings, the record's layout as gcc sees it, the entry points, and every refusal that comes
before the device is selected."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from ergodic_exploration_amd import capi

from tests import frontier_restatement as fr
from tests import frontier_scenes as fs

ENTRIES = {"eea_frontier_ws_bytes": 2, "eea_frontier_regions": 13, "eea_frontier_goals": 12}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(fs.MASKS))
def test_two_statements_agree_on_the_mask_scenes(name):
    mask = fs.MASKS[name]()
    m = fr.members(fr.OF_MASK, mask, fs.THR)
    a, b = fr.roots_by_flood_fill(m), fr.roots_by_raster_union_find(m)
    assert np.array_equal(a, b)
    root, region, rec, state = fr.regions(fr.OF_MASK, mask, fs.THR)
    fr.check_invariants(m, root, region, rec, state)
    assert (rec["entry_cell"] == -1).all() and (rec["entry_cost"] == -1).all() and (rec["entry_owner"] == -1).all()


def test_the_mask_scenes_are_what_their_names_say():
    T = fs.T
    n = lambda name: int(fr.regions(fr.OF_MASK, fs.MASKS[name](), fs.THR)[3][0])
    assert n("empty") == 0 and n("full") == 1 and n("checkerboard") == 1 and n("corner_main") == 1 and n("corner_anti") == 1
    assert n("serpentine_tile") == 1 and n("serpentine_3x3") == 1 and n("comb_and_u") == 2 and n("row_alternating") == T + 3
    root, region, rec, state = fr.regions(fr.OF_MASK, fs.MASKS["serpentine_tile"](), fs.THR)
    assert rec[0]["size"] == T * T // 2 + T // 2 and rec[0]["root"] == 0
    root, region, rec, state = fr.regions(fr.OF_MASK, fs.MASKS["checkerboard"](), fs.THR)
    assert rec[0]["size"] == 3 * T * T
    root, region, rec, state = fr.regions(fr.OF_MASK, fs.MASKS["every_third"](), fs.THR, max_regions=5)
    assert state.tolist() == [T * T, 5, T * T, 0] and len(rec) == 5 and region.max() == T * T - 1
    # 0.45 is near the 8-neighbour percolation threshold: a region that winds through most of the grid beside many small ones
    root, region, rec, state = fr.regions(fr.OF_MASK, fs.MASKS["random_45"](), fs.THR)
    assert rec["size"].max() > 500 and state[0] > 20


def test_the_hand_built_grid():
    """values 0, 69, 70, 100 at threshold 0.7; unknown cells only diagonal to a free cell; unknown cells at the grid's border; a
    free cell on the grid's edge with no unknown neighbour"""
    grid, want = fs.known_grid()
    m = fr.members(fr.OF_GRID, grid, 0.7)
    assert np.array_equal(m, want)
    assert np.array_equal(fr.roots_by_flood_fill(m), fr.roots_by_raster_union_find(m))
    fr.check_invariants(m, *fr.regions(fr.OF_GRID, grid, 0.7))


def test_the_revealed_scene_splits_on_unreachable_members_and_has_an_entry_tie():
    sc = fs.revealed_scene()
    plain = fr.regions(fr.OF_GRID, sc.known, sc.g.occupied_threshold)
    root, region, rec, state = fr.regions(fr.OF_GRID, sc.known, sc.g.occupied_threshold, geo=sc.geo, owner=sc.owner)
    m = fr.members(fr.OF_GRID, sc.known, sc.g.occupied_threshold, sc.geo)
    fr.check_invariants(m, root, region, rec, state)
    assert np.array_equal(fr.roots_by_raster_union_find(m), root)
    assert state[2] < plain[3][2] and state[0] > 1
    # members with geo -1 split a region of the plain labelling in two
    split = [r for r in np.unique(plain[0][plain[0] >= 0]) if len(np.unique(root[(plain[0] == r) & (root >= 0)])) > 1]
    assert split, "no region was split by unreachable members"
    # a tie in geo between two entry candidates: the lower index wins
    ties = 0
    flat_geo, flat_region = sc.geo.reshape(-1), region.reshape(-1)
    for r, e in enumerate(rec):
        at = np.flatnonzero((flat_region == r) & (flat_geo == e["entry_cost"]))
        assert e["entry_cell"] == at[0] and e["entry_owner"] == sc.owner.reshape(-1)[at[0]] and e["entry_cost"] == flat_geo[flat_region == r].min()
        ties += len(at) > 1
    assert ties > 0


@pytest.mark.parametrize("seed", range(24))
def test_two_statements_agree_on_random_grids(seed):
    rng = np.random.default_rng(500 + seed)
    ys, xs = int(rng.integers(1, 40)), int(rng.integers(1, 40))
    if seed % 2:
        grid = (rng.random((ys, xs)) < rng.choice([0.3, 0.45, 0.6])).astype(np.int8) * np.int8(rng.choice([1, -3, 100]))
        kind = fr.OF_MASK
    else:
        grid = rng.choice(np.array([0, 0, 0, -1, -1, 100, 79, 80], dtype=np.int8), size=(ys, xs))
        kind = fr.OF_GRID
    geo = rng.integers(-1, 4, size=(ys, xs)).astype(np.int32) if seed % 3 == 0 else None
    owner = None if geo is None else rng.integers(0, 3, size=(ys, xs)).astype(np.int32)
    m = fr.members(kind, grid, 0.8, geo)
    assert np.array_equal(fr.roots_by_flood_fill(m), fr.roots_by_raster_union_find(m))
    root, region, rec, state = fr.regions(kind, grid, 0.8, geo=geo, owner=owner)
    fr.check_invariants(m, root, region, rec, state)
    if kind == fr.OF_GRID and geo is None:
        # the definition once more, cell by cell
        for i in range(ys):
            for j in range(xs):
                v = int(grid[i, j])
                near = any(0 <= i + a < ys and 0 <= j + b < xs and grid[i + a, j + b] < 0 for a, b in ((0, 1), (1, 0), (0, -1), (-1, 0)))
                assert m[i, j] == (v >= 0 and v / 100.0 < 0.8 and near)


# ---- regions_fast, the reference of the large scenes, against regions, the definition ----------------------------------------
def _identical(fast, slow):
    for a, b, what in zip(fast, slow, ("root", "region", "records", "state")):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("name", sorted(fs.MASKS))
def test_regions_fast_is_regions_on_the_mask_scenes(name):
    mask = fs.MASKS[name]()
    n = int(fr.regions(fr.OF_MASK, mask, fs.THR)[3][0])
    for max_regions in (None, 0, 1, 5, n, n + 1):
        _identical(fr.regions_fast(fr.OF_MASK, mask, fs.THR, max_regions=max_regions),
                   fr.regions(fr.OF_MASK, mask, fs.THR, max_regions=max_regions))


def test_regions_fast_is_regions_on_the_grids():
    """the hand-built grid; the revealed scene without the partition's planes, with d_geo alone and with both (entries with
    ties in geo), each with room for every record, for some, for one and for none"""
    grid, _ = fs.known_grid()
    for max_regions in (None, 0, 3):
        _identical(fr.regions_fast(fr.OF_GRID, grid, 0.7, max_regions=max_regions), fr.regions(fr.OF_GRID, grid, 0.7, max_regions=max_regions))
    sc = fs.revealed_scene()
    for planes in ({}, dict(geo=sc.geo), dict(geo=sc.geo, owner=sc.owner)):
        for kind in (fr.OF_MASK, fr.OF_GRID):
            for max_regions in (None, 0, 1, 2):
                fast = fr.regions_fast(kind, sc.known, sc.g.occupied_threshold, max_regions=max_regions, **planes)
                _identical(fast, fr.regions(kind, sc.known, sc.g.occupied_threshold, max_regions=max_regions, **planes))
    assert fast[3][0] > 2 and (fast[2]["entry_owner"] >= 0).all()


@pytest.mark.parametrize("seed", range(24))
def test_regions_fast_is_regions_on_random_grids(seed):
    """the grids of test_two_statements_agree_on_random_grids: both kinds, a third of them with geo (-1 among its values) and an
    owner plane"""
    rng = np.random.default_rng(500 + seed)
    ys, xs = int(rng.integers(1, 40)), int(rng.integers(1, 40))
    if seed % 2:
        grid = (rng.random((ys, xs)) < rng.choice([0.3, 0.45, 0.6])).astype(np.int8) * np.int8(rng.choice([1, -3, 100]))
        kind = fr.OF_MASK
    else:
        grid = rng.choice(np.array([0, 0, 0, -1, -1, 100, 79, 80], dtype=np.int8), size=(ys, xs))
        kind = fr.OF_GRID
    geo = rng.integers(-1, 4, size=(ys, xs)).astype(np.int32) if seed % 3 == 0 else None
    owner = None if geo is None else rng.integers(0, 3, size=(ys, xs)).astype(np.int32)
    for max_regions in (None, 2):
        _identical(fr.regions_fast(kind, grid, 0.8, geo=geo, owner=owner, max_regions=max_regions),
                   fr.regions(kind, grid, 0.8, geo=geo, owner=owner, max_regions=max_regions))


@pytest.mark.parametrize("name", sorted(fs.LARGE_MASKS))
def test_the_large_masks_are_what_their_names_say(name):
    """more than 256 chunks of 1024 cells each; the labels of regions_fast (a raster union-find) are the flood fill's; the
    counts the scenes were drawn for"""
    mask = fs.LARGE_MASKS[name]()
    root, region, rec, state = fs.large_mask_regions(name)
    assert (mask.size - 1) // 1024 + 1 > 256 and not mask.flags.writeable
    assert np.array_equal(root, fr.roots_by_flood_fill(fr.members(fr.OF_MASK, mask, fs.THR)))
    assert state[0] == state[1] == len(rec) and rec["size"].sum() == state[2] == np.count_nonzero(mask)
    assert np.array_equal(region.reshape(-1)[rec["root"]], np.arange(len(rec))) and (np.diff(rec["root"]) > 0).all()
    if name == "large_every_third":
        assert mask.shape == (506, 520) and state[0] == 29406 and (rec["size"] == 1).all()
    if name == "large_serpentine":
        assert state.tolist() == [1, 1, 131813, 0] and (rec[0]["i_max"], rec[0]["j_max"]) == (505, 519)
    if name == "large_rows":
        assert mask.shape == (33, 8192) and state[0] == 1 + 4096 + 128 and rec[0]["size"] == 8192 and (rec[1:4097]["size"] == 1).all()
        assert (rec[4097:]["size"] == 63).all()
    if name.startswith("large_random"):
        assert state[0] > 1000
    cut = fs.large_mask_regions(name, 300) if name == "large_every_third" else None
    if cut is not None:
        assert cut[3].tolist() == [29406, 300, 29406, 0] and cut[2].tobytes() == rec[:300].tobytes() and np.array_equal(cut[1], region)


def test_the_large_revealed_scene():
    """300 accepted sources, the last two without a cell of their own; frontier regions owned by most robots"""
    sc = fs.large_revealed()
    root, region, rec, state = fs.large_revealed_regions()
    assert sc.known.shape == (506, 520) and sc.n_src == 300 and len(sc.poses) == 300
    assert set(np.unique(sc.owner)) == set(range(-1, 298))
    assert state[0] > 300 and len(set(rec["entry_owner"].tolist())) > 200 and (rec["entry_cell"] >= 0).all()
    cell, reg, score = fr.goals(rec, 300, 2, 1.0, 0.125)
    assert (cell >= 0).sum() > 200 and cell[298] == cell[299] == -1


@pytest.mark.parametrize("seed", range(12))
def test_goals_are_the_argmax_with_ties_to_the_lowest_record(seed):
    rng = np.random.default_rng(seed)
    n, P = int(rng.integers(0, 40)), int(rng.integers(1, 6))
    rec = np.zeros(n, dtype=fr.RECORD)
    rec["size"] = rng.integers(1, 5, n)
    rec["entry_cost"] = rng.integers(0, 4, n) * 5
    rec["entry_cell"] = np.where(rng.random(n) < 0.85, rng.integers(0, 1000, n), -1)
    rec["entry_owner"] = rng.integers(-1, P + 2, n)
    for min_size, ws, wc in ((1, 1.0, 0.0), (2, 1.0, 0.2), (1, 0.0, 1.0), (3, 0.0, 0.0), (1, 1e30, 1e30)):
        cell, region, score = fr.goals(rec, P, min_size, ws, wc)
        s_all = np.float64(ws) * rec["size"].astype(np.float64) - np.float64(wc) * rec["entry_cost"].astype(np.float64)
        for q in range(P):
            ok = (rec["entry_owner"] == q) & (rec["entry_cell"] >= 0) & (rec["size"] >= min_size)
            if not ok.any():
                assert (cell[q], region[q], score[q]) == (-1, -1, 0.0)
            else:
                top = s_all[ok].max()
                r = np.flatnonzero(ok & (s_all == top))[0]
                assert (cell[q], region[q], score[q]) == (rec["entry_cell"][r], r, top)


@pytest.mark.parametrize("seed", range(40))
def test_the_lock_free_union_under_random_interleavings(seed):
    """the merge launch's loop as a state machine per lane, stepped one memory access at a time in a random order: every
    interleaving ends, and at the sets of a flood fill with every root its set's least index.  Parents start as the tile-local
    roots of a 3 x 3-tile grid with tiles of 4 x 4 cells"""
    rng = np.random.default_rng(900 + seed)
    T, ys, xs = 4, 11, 10
    m = rng.random((ys, xs)) < 0.55
    want = fr.roots_by_flood_fill(m)
    parent = np.full(ys * xs, -1, dtype=np.int64)
    for a in range(0, ys, T):
        for b in range(0, xs, T):
            local = fr.roots_by_flood_fill(m[a:a + T, b:b + T])
            h, w = local.shape
            for i in range(h):
                for j in range(w):
                    if local[i, j] >= 0:
                        parent[(a + i) * xs + b + j] = (a + local[i, j] // w) * xs + b + local[i, j] % w
    pairs = [(i * xs + j, (i + da) * xs + j + db) for i in range(ys) for j in range(xs) for da, db in ((0, -1), (-1, -1), (-1, 0), (-1, 1))
             if m[i, j] and 0 <= i + da and 0 <= j + db < xs and m[i + da, j + db] and (i // T, j // T) != ((i + da) // T, (j + db) // T)]

    def lane(a, b):
        while True:
            while True:                                                     # a = find(a)
                p = parent[a]
                yield
                if p == a:
                    break
                a = p
            while True:                                                     # b = find(b)
                p = parent[b]
                yield
                if p == b:
                    break
                b = p
            if a == b:
                return
            if a < b:
                a, b = b, a
            old = parent[a]                                                 # atomicMin: one step
            parent[a] = min(old, b)
            yield
            if old == a:
                return
            a = old

    live = [lane(a, b) for a, b in pairs]
    steps = 0
    while live:
        k = int(rng.integers(len(live)))
        try:
            next(live[k])
        except StopIteration:
            live.pop(k)
        steps += 1
        assert steps < 200000
    got = np.full(ys * xs, -1, dtype=np.int64)
    for c in np.flatnonzero(parent >= 0):
        x = c
        while parent[x] != x:
            assert parent[x] < x
            x = parent[x]
        got[c] = x
    assert np.array_equal(got.reshape(ys, xs), want)


def test_entries_are_declared_exported_and_bound():
    raw = C.CDLL(capi.LIB_PATH)
    L = capi.lib()
    for name, n_args in ENTRIES.items():
        assert name in capi.declared_symbols() and hasattr(raw, name), name
        assert len(getattr(L, name).argtypes) == n_args, name
    for name in ("frontier_ws_bytes", "frontier_regions", "frontier_goals"):
        assert callable(getattr(capi, name)), name
    assert L.eea_abi_version() == 6 and (capi.FRONTIER_OF_GRID, capi.FRONTIER_OF_MASK) == (0, 1)


def test_the_record_as_gcc_lays_it_out_is_the_ctypes_mirror_and_the_numpy_record():
    fields = [n for n, _ in capi.FrontierRegion._fields_]
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "ergodic_amd.h"\nint main(void) {\n' \
          '  printf("%zu %zu\\n", sizeof(eea_frontier_region), _Alignof(eea_frontier_region));\n' + \
          "".join('  printf("%s %%zu\\n", offsetof(eea_frontier_region, %s));\n' % (f, f) for f in fields) + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "layout.c"), "w") as f:
            f.write(src)
        exe = os.path.join(tmp, "layout")
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "layout.c"), "-o", exe], check=True)
        lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    size, align = (int(v) for v in lines[0].split())
    assert (size, align) == (56, 8) == (C.sizeof(capi.FrontierRegion), C.alignment(capi.FrontierRegion))
    assert fr.RECORD.itemsize == 56 and list(fr.RECORD.names) == fields
    for line in lines[1:1 + len(fields)]:
        name, off = line.split()
        assert getattr(capi.FrontierRegion, name).offset == int(off) == fr.RECORD.fields[name][1], name
    # the entry is one aligned 8-byte word, cost << 32 | cell
    assert capi.FrontierRegion.entry_cell.offset % 8 == 0 and capi.FrontierRegion.entry_cost.offset == capi.FrontierRegion.entry_cell.offset + 4


def test_workspace_bytes_are_positive_and_monotone():
    sizes = [(1, 1), (1, 33), (33, 1), (33, 33), (64, 41), (200, 100), (1024, 1024), (8192, 8192)]
    cfgs = [capi.make_collision_cfg(0.0, 0.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 0.8) for xs, ys in sizes]
    got = [capi.frontier_ws_bytes(c) for c in cfgs]
    assert got[0] > 0 and all(a <= b for a, b in zip(got, got[1:])) and got[-1] > got[0]
    L = capi.lib()
    assert L.eea_frontier_ws_bytes(None, C.byref(C.c_size_t())) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_frontier_ws_bytes(C.byref(cfgs[0]), None) == capi.ERR_INVALID_ARGUMENT


def test_argument_errors_come_before_the_device():
    """every refusal of the header is answered without a device: the buffers are host arrays that hold a sentinel nothing may
    touch"""
    L = capi.lib()
    xs, ys = 40, 30
    good = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 0.8)
    grid = np.zeros(xs * ys, dtype=np.int8)
    geo_buf, own_buf, root, region = (np.full((ys, xs), 7, dtype=np.int32) for _ in range(4))
    ws, state = np.full(capi.frontier_ws_bytes(good) + 8, 7, dtype=np.uint8), np.full(4, 7, dtype=np.uint32)
    off = (-ws.ctypes.data) % 8
    recs = np.full(3 * 56, 7, dtype=np.uint8)
    g_cell, g_region, g_score = np.full(3, 7, dtype=np.int32), np.full(3, 7, dtype=np.int32), np.full(3, 7.0)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    ref = lambda c: None if c is None else C.byref(c)
    INV, UNS = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED

    def label(cfg=good, kind=0, g=grid, gf=geo_buf, own=own_buf, n=3, rt=root, rg=region, rc=recs, w=off, st=state):
        wp = None if w is None else C.c_void_p(ws.ctypes.data + w)
        return L.eea_frontier_regions(0, ref(cfg), kind, p(g), p(gf), p(own), n, p(rt), p(rg), p(rc), wp, p(st), None)

    def pick(rc=recs, st=state, n=3, P=3, min_size=1, ws_=1.0, wc=0.5, gc=g_cell, gr=g_region, gs=g_score):
        return L.eea_frontier_goals(0, p(rc), p(st), n, P, min_size, ws_, wc, p(gc), p(gr), p(gs), None)

    assert label(cfg=None) == INV
    for kw in (dict(g=None), dict(rt=None), dict(rg=None), dict(w=None), dict(st=None)):
        assert label(**kw) == INV and b"null" in L.eea_last_error(), kw
    assert label(rc=None) == INV and label(rc=None, n=1) == INV and b"d_regions" in L.eea_last_error()
    assert label(gf=None) == INV and b"d_owner" in L.eea_last_error()
    for kind in (2, -1, 1 << 30):
        assert label(kind=kind) == INV and b"kind" in L.eea_last_error(), kind
    for w in (off + 4, off + 2, off + 1):
        assert label(w=w) == INV and b"8-byte aligned" in L.eea_last_error(), w
    for kw in (dict(rc=None), dict(st=None), dict(gc=None), dict(gr=None), dict(gs=None)):
        assert pick(**kw) == INV and b"null" in L.eea_last_error(), kw
    for bad in (-0.5, float("nan"), float("inf"), -float("inf"), 1.0000001e30):
        assert pick(ws_=bad) == INV and b"weight" in L.eea_last_error(), bad
        assert pick(wc=bad) == INV and b"weight" in L.eea_last_error(), bad
    assert pick(P=1 << 31) == UNS and b"2^31 - 1" in L.eea_last_error()
    assert pick(P=0) == capi.OK and pick(P=0, ws_=1e30, wc=0.0, n=0) == capi.OK
    # the configuration errors and the limits of the geodesic calls
    swapped = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 1.0, 0.7, 0.2, 0.8)
    assert label(cfg=swapped) == INV and b"Search radius" in L.eea_last_error()
    for bad in (capi.make_collision_cfg(-2.0, -1.0, 0.1, 0, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, 0, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.0, xs, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 100.5)):
        assert label(cfg=bad) == INV and L.eea_frontier_ws_bytes(C.byref(bad), C.byref(C.c_size_t())) == INV
    side = capi.DISTANCE_MAX_SIDE
    assert side == 8192
    for big in (capi.make_collision_cfg(-2.0, -1.0, 0.1, side + 1, 4, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, 4, side + 1, 0.7, 1.0, 0.2, 0.8)):
        assert label(cfg=big) == UNS and b"EEA_DISTANCE_MAX_SIDE" in L.eea_last_error()
        assert L.eea_frontier_ws_bytes(C.byref(big), C.byref(C.c_size_t())) == UNS
    widest = capi.make_collision_cfg(-2.0, -1.0, 0.1, side, side, 0.7, 1.0, 0.2, 0.8)
    n = C.c_size_t()
    assert L.eea_frontier_ws_bytes(C.byref(widest), C.byref(n)) == capi.OK and n.value >= capi.frontier_ws_bytes(good)
    for a, v in ((geo_buf, 7), (own_buf, 7), (root, 7), (region, 7), (ws, 7), (state, 7), (recs, 7), (g_cell, 7), (g_region, 7),
                 (g_score, 7.0)):
        assert (a == v).all()
    assert not grid.any()


def test_frontier_kernels_are_in_the_library():
    """the kernels of csrc/frontier_kernel.hip are gfx950 code in the build and use no scratch; the local launch's tile (a byte
    per staged cell and a parent per cell) is static LDS well inside 64 KB"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    obj = os.path.join(os.path.dirname(capi.LIB_PATH), "..", "csrc", "build", "frontier_kernel.o")
    names = {}
    for k in kr.kernels(obj):
        if "vgpr_count" in k:
            names[subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.strip()] = k
    for w in ("frontier_local_kernel(", "frontier_merge_kernel(", "frontier_flatten_kernel(", "frontier_rank_kernel(",
              "frontier_scatter_kernel(", "frontier_stats_kernel(", "frontier_finish_kernel(", "frontier_goals_init_kernel(",
              "frontier_goals_pass_kernel<0>(", "frontier_goals_pass_kernel<1>(", "frontier_goals_finish_kernel("):
        found = [k for n, k in names.items() if w in n]
        assert len(found) == 1, (w, sorted(names))
        assert int(found[0]["private_segment_fixed_size"]) == 0, found[0]
    T2 = capi.GEODESIC_TILE_X * capi.GEODESIC_TILE_Y
    lds = int([k for n, k in names.items() if "frontier_local_kernel(" in n][0]["group_segment_fixed_size"])
    assert 5 * T2 <= lds <= 8 * 1024

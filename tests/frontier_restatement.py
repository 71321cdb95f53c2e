"""eea_frontier_regions / eea_frontier_goals (include/ergodic_amd.h) restated in numpy, for tests/test_frontier.py (CPU),
tests/test_gpu_frontier.py and tools/frontier_cost.py.  Independent of the library: the definitions only -- the members of the
two kinds, the 8-connected regions by a flood fill, a second and independent statement by a two-pass raster union-find, the
records, and the goals with the score in numpy fp64."""
import numpy as np

OF_GRID, OF_MASK = 0, 1
RECORD = np.dtype([("sum_i", "<u8"), ("sum_j", "<u8"), ("entry_cell", "<i4"), ("entry_cost", "<i4"), ("root", "<i4"), ("size", "<u4"),
                   ("i_min", "<i4"), ("i_max", "<i4"), ("j_min", "<i4"), ("j_max", "<i4"), ("entry_owner", "<i4"), ("reserved", "<i4")])
NEIGHBOURS8 = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def members(kind, grid, occupied_threshold, geo=None):
    """bool [ysize][xsize].  OF_GRID: value >= 0, !(value / 100.0 < threshold) false, and an axis neighbour inside the grid with
    a value < 0; OF_MASK: value != 0; with geo also geo >= 0"""
    grid = np.asarray(grid, dtype=np.int8)
    if kind == OF_MASK:
        m = grid != 0
    else:
        free = (grid >= 0) & (grid.astype(np.float64) / 100.0 < occupied_threshold)
        unknown = grid < 0
        near = np.zeros_like(unknown)
        near[1:, :] |= unknown[:-1, :]
        near[:-1, :] |= unknown[1:, :]
        near[:, 1:] |= unknown[:, :-1]
        near[:, :-1] |= unknown[:, 1:]
        m = free & near
    if geo is not None:
        m = m & (np.asarray(geo).reshape(grid.shape) >= 0)
    return m


def roots_by_flood_fill(m):
    """int32 [ysize][xsize]: the least row-major index of the cell's 8-connected region, -1 for a non-member.  Cells are
    visited in row-major order, so the cell a fill starts from is its region's least"""
    ys, xs = m.shape
    root = np.full((ys, xs), -1, dtype=np.int32)
    mem = m.tolist()
    for i in range(ys):
        for j in range(xs):
            if not mem[i][j] or root[i, j] >= 0:
                continue
            label, stack = i * xs + j, [(i, j)]
            root[i, j] = label
            while stack:
                a, b = stack.pop()
                for da, db in NEIGHBOURS8:
                    p, q = a + da, b + db
                    if 0 <= p < ys and 0 <= q < xs and mem[p][q] and root[p, q] < 0:
                        root[p, q] = label
                        stack.append((p, q))
    return root


def roots_by_raster_union_find(m):
    """the second statement: one raster pass gives every member a provisional label and records the equivalences of its W, NW,
    N and NE neighbours in a union-find that keeps the smaller index as the parent; a second pass resolves them"""
    ys, xs = m.shape
    parent = {}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    mem = m.tolist()
    for i in range(ys):
        for j in range(xs):
            if not mem[i][j]:
                continue
            c = i * xs + j
            parent[c] = c
            for da, db in ((0, -1), (-1, -1), (-1, 0), (-1, 1)):
                p, q = i + da, j + db
                if 0 <= p < ys and 0 <= q < xs and mem[p][q]:
                    a, b = find(c), find(p * xs + q)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    root = np.full((ys, xs), -1, dtype=np.int32)
    for c in parent:
        root[c // xs, c % xs] = find(c)
    return root


def regions(kind, grid, occupied_threshold, geo=None, owner=None, max_regions=None):
    """(root int32, region int32 [ysize][xsize], records RECORD [min(n, max_regions)], state uint32 [4]); max_regions None: n"""
    m = members(kind, grid, occupied_threshold, geo)
    ys, xs = m.shape
    root = roots_by_flood_fill(m)
    labels = np.unique(root[root >= 0])                                      # ascending
    rank = {int(r): k for k, r in enumerate(labels)}
    region = np.full((ys, xs), -1, dtype=np.int32)
    for i, j in np.argwhere(m):
        region[i, j] = rank[int(root[i, j])]
    n = len(labels)
    kept = n if max_regions is None else min(n, max_regions)
    rec = np.zeros(kept, dtype=RECORD)
    flat_geo = None if geo is None else np.asarray(geo).reshape(-1)
    flat_owner = None if owner is None else np.asarray(owner).reshape(-1)
    for r in range(kept):
        cells = np.argwhere(region == r)
        ii, jj = cells[:, 0].astype(np.int64), cells[:, 1].astype(np.int64)
        e = rec[r]
        e["sum_i"], e["sum_j"], e["size"], e["root"] = ii.sum(), jj.sum(), len(cells), labels[r]
        e["i_min"], e["i_max"], e["j_min"], e["j_max"] = ii.min(), ii.max(), jj.min(), jj.max()
        e["entry_cell"] = e["entry_cost"] = e["entry_owner"] = -1
        if flat_geo is not None:
            idx = ii * xs + jj
            cost, cell = min((int(flat_geo[c]), int(c)) for c in idx)
            e["entry_cell"], e["entry_cost"] = cell, cost
            if flat_owner is not None:
                e["entry_owner"] = flat_owner[cell]
    state = np.array([n, kept, int(m.sum()), 0], dtype=np.uint32)
    return root, region, rec, state


def regions_fast(kind, grid, occupied_threshold, geo=None, owner=None, max_regions=None):
    """regions() for grids where a pass per region is too slow: the same four values, byte for byte (tests/test_frontier.py holds
    it to regions(), which stays the definition).  Labels from the raster union-find -- regions() takes the flood fill's --, ranks
    by ascending root, and every record field by one array operation over the members"""
    m = members(kind, grid, occupied_threshold, geo)
    ys, xs = m.shape
    root = roots_by_raster_union_find(m)
    flat = root.reshape(-1)
    idx = np.flatnonzero(flat >= 0).astype(np.int64)                         # the members, row-major
    labels, rank = np.unique(flat[idx], return_inverse=True)                 # ascending roots; a member's rank
    rank = rank.reshape(-1).astype(np.int64)
    region = np.full(ys * xs, -1, dtype=np.int32)
    region[idx] = rank
    n = len(labels)
    kept = n if max_regions is None else min(n, max_regions)
    rec = np.zeros(kept, dtype=RECORD)
    rec["root"] = labels[:kept]
    rec["entry_cell"] = rec["entry_cost"] = rec["entry_owner"] = -1
    has = rank < kept
    idx, rank = idx[has], rank[has]
    ii, jj = idx // xs, idx % xs
    rec["size"] = np.bincount(rank, minlength=kept)
    for name, v in (("sum_i", ii), ("sum_j", jj)):
        total = np.zeros(kept, dtype=np.int64)
        np.add.at(total, rank, v)
        rec[name] = total
    for name, v, op, start in (("i_min", ii, np.minimum, ys), ("i_max", ii, np.maximum, -1), ("j_min", jj, np.minimum, xs),
                               ("j_max", jj, np.maximum, -1)):
        edge = np.full(kept, start, dtype=np.int64)
        op.at(edge, rank, v)
        rec[name] = edge
    if geo is not None and kept:
        cost = np.asarray(geo).reshape(-1)[idx].astype(np.int64)
        order = np.lexsort((idx, cost, rank))                                # by rank, then the least (geo, index) first
        first = order[np.searchsorted(rank[order], np.arange(kept))]         # (every kept rank has a member)
        rec["entry_cell"], rec["entry_cost"] = idx[first], cost[first]
        if owner is not None:
            rec["entry_owner"] = np.asarray(owner).reshape(-1)[idx[first]]
    state = np.array([n, kept, int(m.sum()), 0], dtype=np.uint32)
    return root, region.reshape(ys, xs), rec, state


def goals(rec, P, min_size, w_size, w_cost):
    """(goal_cell int32 [P], goal_region int32 [P], goal_score float64 [P]): brute force over the records in ascending order"""
    cell = np.full(P, -1, dtype=np.int32)
    region = np.full(P, -1, dtype=np.int32)
    score = np.zeros(P, dtype=np.float64)
    ws, wc = np.float64(w_size), np.float64(w_cost)
    for r, e in enumerate(rec):
        q = int(e["entry_owner"])
        if not 0 <= q < P or e["entry_cell"] < 0 or e["size"] < min_size:
            continue
        s = ws * np.float64(int(e["size"])) - wc * np.float64(int(e["entry_cost"]))
        if region[q] < 0 or s > score[q]:
            cell[q], region[q], score[q] = e["entry_cell"], r, s
    return cell, region, score


def check_invariants(m, root, region, rec, state):
    """what any answer must obey, whatever computed it"""
    ys, xs = m.shape
    idx = np.arange(ys * xs, dtype=np.int64).reshape(ys, xs)
    assert np.array_equal(root >= 0, m) and np.array_equal(region >= 0, m)
    assert (root[m] <= idx[m]).all()
    flat = root.reshape(-1)
    assert (flat[flat[flat >= 0]] == flat[flat >= 0]).all()                  # root[root] == root
    labels = np.unique(flat[flat >= 0])
    assert state[0] == len(labels) and state[2] == m.sum() and state[3] == 0 and state[1] == len(rec)
    assert np.array_equal(region.reshape(-1)[labels], np.arange(len(labels)))  # ranks ascend with the roots
    assert int(sum(int(e["size"]) for e in rec)) == int((m & (region < len(rec))).sum())
    for r, e in enumerate(rec):
        assert e["root"] == labels[r] and e["reserved"] == 0 and e["size"] > 0
        assert e["i_min"] * xs + e["j_min"] <= e["root"] and e["i_min"] == e["root"] // xs
        assert e["i_min"] * e["size"] <= e["sum_i"] <= e["i_max"] * e["size"]
        assert e["j_min"] * e["size"] <= e["sum_j"] <= e["j_max"] * e["size"]


# ---- scenes both test files draw -------------------------------------------------------------------------------------------
def serpentine_mask(ys, xs):
    """a one-cell-wide path that fills the rectangle: every even row is full, an odd row holds one cell, at alternating ends"""
    m = np.zeros((ys, xs), dtype=np.int8)
    m[0::2, :] = 1
    for i in range(1, ys, 2):
        m[i, xs - 1 if (i // 2) % 2 == 0 else 0] = 1
    return m


def comb_mask(T, teeth=8):
    """(T + 4) x (teeth * 4): teeth of tile row 0 (columns 0, 4, 8, ..., rows 0 .. T - 1, separate inside tile row 0) joined by a
    spine in tile row 1 (row T + 1), which they reach through rows T .. T + 1"""
    m = np.zeros((T + 4, teeth * 4), dtype=np.int8)
    m[:T + 2, 0::4] = 1
    m[T + 1, :teeth * 4 - 3] = 1
    return m

"""Scenes that pin the exact test of the footprint kernels at its edges (csrc/footprint_plan_kernel.hip: row_span, the masks
in_box / l2 / h2, the mapping j = wx0 + 64 k + bit, the four-row read-ahead of resolve_window; csrc/footprint_cell_test.hpp:
resolve), and a 50-digit reference of the verdict, for tests/test_footprint_edges.py (CPU) and
tests/test_gpu_footprint_edges.py.

A scene is a grid, a few start poses x0, and the verdict of every pose.  The pose a kernel judges is
footprint_plan_restatement.rollout(x0, zero twist, DT, one step): the position unchanged, the heading through the wrap.  The
verdict is `some occupied cell has exact_signed <= 0`, exact_signed = max_k (n_k . b - h_k) at 50 digits over the doubles of
footprint_restatement.planes -- the device's polygon is those rounded planes.

Families (the tag of a scene says which):
  A  one occupied cell, its centre a body point pulled inward / outward of the boundary by m at every vertex (along the ray to
     the origin) and at a point of every edge (along the normal), random headings;
  B  A's edge probes with the heading chosen so that the edge is within a few 1e-3 of parallel to the grid rows;
  C  a hollow block: every cell of the pose's box occupied except those within m of the polygon (free), and the same plus one
     occupied cell inside (hit) at the first / last inside column of a row, the top / bottom inside row, a one-cell row;
  D  A and C with the pose's cell near the grid's edges, so that the window starts at column 0 and the box's first column in
     it (c0) and the clipped box height take the listed values;
  E  a fan: N headings of one body, the lanes of one workgroup, against two or three cells in the annulus r_in .. r_out.

The pull m of a probe is measured in exact_signed itself (the smaller of the two adjacent half-plane values at a vertex), and
a candidate is kept only when the 50-digit value has the intended sign with |exact_signed| >= MARGIN, and the pose is one
`classify` calls ambiguous (sq_hit < sq <= sq_free), so that the exact test is what answers."""
import functools
import math

import mpmath as mp
import numpy as np

from tests import footprint_plan_restatement as pr
from tests import footprint_restatement as fr

DT = 0.1                      # one step: horizon = dt
MARGIN = 1e-7                 # metres: what the families A - D keep between every occupied centre and the boundary
RES = (0.1, 0.05, 0.01, 0.0017, 0.0013)
RES_NO_WINDOW = 0.0013        # rect: box 397, a window of 2 * 398 + 1 columns does not fit
W_DEFAULT = 6                 # the reach in cells a launch reserves unless a scene says otherwise
W_MEMORY = 400                # a reach no window fits the LDS with: side >= 801, 801 * 13 * 8 bytes
LDS_LIMIT = 64 * 1024
EPS_PARALLEL = tuple(s * f * 1e-3 for f in (0.5, 0.9, 0.999, 1.001, 1.1, 2.0, 5.0) for s in (1.0, -1.0))
C0_LIST = (0, 1, 62, 63, 64, 65, 127, 128)

POLYGONS = dict(fr.FOOTPRINTS)
POLYGONS["needle"] = [(0.6, 0.0), (-0.3, 0.02), (-0.3, -0.02)]
POLYGONS["gon16"] = [(0.5 * math.cos(k * math.pi / 8 + 0.05), 0.5 * math.sin(k * math.pi / 8 + 0.05)) for k in range(16)]
POLYGONS["tiny"] = [(0.12, 0.0), (-0.06, 0.1), (-0.06, -0.1)]          # r_in = 0.06 m: sq_hit == -1 at 0.1 m
NAMES = ("rect", "tri", "oct", "offc", "needle", "gon16", "tiny")


# ---- the reference ---------------------------------------------------------------------------------------------------------------

def exact_signed(res, xmin, ymin, i, j, vertices, pose):
    """max_k (n_k . b - h_k) in metres for the centre of cell (row i, column j) and the polygon placed at `pose`: the planes are
    the doubles of footprint_restatement.planes, everything else is formed at 50 digits"""
    nx, ny, h = fr.planes(vertices)[:3]
    with mp.workdps(50):
        M = mp.mpf
        r = M(float(res))
        cx, cy = M(int(j)) * r + r / 2 + M(float(xmin)), M(int(i)) * r + r / 2 + M(float(ymin))
        dx, dy = cx - M(float(pose[0])), cy - M(float(pose[1]))
        s, c = mp.sin(M(float(pose[2]))), mp.cos(M(float(pose[2])))
        bx, by = c * dx + s * dy, -s * dx + c * dy
        return +max(M(float(nx[k])) * bx + M(float(ny[k])) * by - M(float(h[k])) for k in range(len(h)))


# The double evaluation of the same value (footprint_restatement._signed) is off by a few ulp of the operands: coordinates below
# 2 m, about ten operations, under 1e-14 m.  signed_many trusts it outside a band of GUARD around the values a decision is
# made at and asks the 50-digit form inside.
GUARD = 1e-9


def signed_many(w, vertices, pose, ii, jj, at=(0.0,)):
    """exact_signed of the cells (ii, jj) as doubles: footprint_restatement._signed, replaced by the 50-digit value wherever it
    lies within GUARD of one of the values `at`"""
    pose = np.asarray(pose, dtype=np.float64).reshape(1, 3)
    v = fr._signed(w.res, w.xmin, w.ymin, fr.planes(vertices), pose, np.asarray(ii), np.asarray(jj))[0][0].copy()
    close = np.zeros(len(v), dtype=bool)
    for t in at:
        close |= np.abs(v - t) < GUARD
    for q in np.nonzero(close)[0]:
        v[q] = float(exact_signed(w.res, w.xmin, w.ymin, ii[q], jj[q], vertices, pose[0]))
    return v


def judged(x0):
    """the poses the planning kernels judge: one step of a zero twist"""
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1, 3)
    return np.array([pr.rollout(x, np.zeros(3), DT, 1)[0] for x in x0]).reshape(-1, 3)


NEAREST = 32                  # the cells per pose exact_verdicts evaluates at 50 digits
DOUBLE_ERROR = 1e-12          # metres: what the double value may differ from the 50-digit one by (observed: below 1e-15)


def exact_verdicts(w, vertices, poses, nearest=NEAREST):
    """(hit bool [P], margin [P], n): the verdict of every pose over the occupied cells of w and the smallest |exact_signed|
    (inf: no occupied cell), from exact_signed ITSELF on the cells that decide: per pose the `nearest` occupied cells with the
    smallest |double value| and the eight with the smallest double value (every occupied cell when there are no more than
    that: the scenes of one cell, the fans).  On those cells the double value is held to the 50-digit one within DOUBLE_ERROR
    -- an AssertionError otherwise --, which is what lets the cells farther out, whose double value is farther from 0 than any
    evaluated one, keep the sign of their double value.  n = the number of 50-digit evaluations"""
    ii, jj = np.nonzero(fr.cr.occupied(w.data, w.threshold))
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    hit, margin, n = np.zeros(len(poses), dtype=bool), np.full(len(poses), np.inf), 0
    if len(ii) == 0:
        return hit, margin, n
    pl = fr.planes(vertices)
    for q, p in enumerate(poses):
        v = fr._signed(w.res, w.xmin, w.ymin, pl, p[None], ii, jj)[0][0]
        pick = np.arange(len(v))
        if len(v) > nearest + 8:
            pick = np.union1d(np.argpartition(np.abs(v), nearest)[:nearest], np.argpartition(v, 8)[:8])
        e = np.array([float(exact_signed(w.res, w.xmin, w.ymin, ii[c], jj[c], vertices, p)) for c in pick])
        n += len(pick)
        assert np.abs(e - v[pick]).max() < DOUBLE_ERROR, (p, float(np.abs(e - v[pick]).max()))
        rest = np.delete(v, pick)
        assert len(rest) == 0 or (np.abs(rest).min() >= np.abs(v[pick]).min() and rest.min() >= v[pick].min())
        # (the cells left out are no nearer to the boundary and no deeper inside than an evaluated one)
        hit[q], margin[q] = bool((e <= 0.0).any()), float(np.abs(e).min())
    return hit, margin, n


# ---- geometry of a launch ----------------------------------------------------------------------------------------------------------

def radii(name):
    pl = fr.planes(POLYGONS[name])
    return float(pl[3]), float(pl[4])


def box_of(name, res):
    return fr.thresholds(*radii(name), res)[2]


def window_bytes(box, W, nsamp=1):
    """what footprint_dwa_kernel asks of the LDS for a reach of W cells: the costs and the bit rows"""
    side = 2 * (W + box) + 1
    return side * ((side + 63) // 64) * 8 + 8 * nsamp


def fits(name, res, W=W_DEFAULT, nsamp=1):
    return window_bytes(box_of(name, res), W, nsamp) <= LDS_LIMIT


def names_at(res):
    """the polygons a resolution is run with: all at the coarse ones, below 0.01 m those whose window fits (and at the one
    resolution where none does, the two smallest of those)"""
    if res >= 0.01:
        return NAMES
    if res == RES_NO_WINDOW:
        return ("rect", "oct")
    return tuple(n for n in NAMES if fits(n, res))


def dwa_cfg(res, W=W_DEFAULT, ns=(1, 1, 1), acc=1.0, rot=0.0):
    """a DWA tuple (footprint_plan_restatement.FIELDS) of one step whose limits reserve a reach of exactly W >= 2 cells: every
    minimum 0, max_vel_y 0, so reach = ceil(DT * max_vel_x / res) + 1 with DT * max_vel_x / res = W - 1.5.  vb = 0 gives
    lower = 0 on every axis with a minimum of 0: the one sample is the zero twist.  rot: +-rot as the yaw limits (the fan)"""
    mx = (W - 1.5) * res / DT
    return (DT, DT, 1.0, acc, 0.0, max(rot, 1.0), mx, 0.0, 0.0, 0.0, rot, -rot if rot else 0.0, ns[0], ns[1], ns[2])


class EdgeScene:
    """family 'A'..'E', tag, polygon name, World, x0 [P][3], hit bool [P] (the 50-digit verdicts), margin [P], W"""

    def __init__(self, family, tag, name, w, x0, hit, margin, W=W_DEFAULT, info=None):
        self.family, self.tag, self.name, self.w, self.W = family, tag, name, w, W
        self.x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1, 3)
        self.hit, self.margin = np.asarray(hit, dtype=bool), np.asarray(margin, dtype=np.float64)
        self.info = info or {}
        self.verts = POLYGONS[name]

    @property
    def poses(self):
        return judged(self.x0)

    def boxes(self):
        """[P][4] x0, x1, y0, y1 of every pose's box (classify's clamp)"""
        box = box_of(self.name, self.w.res)
        _, fx, fy = fr.cells(self.w.res, self.w.xmin, self.w.ymin, self.w.xs, self.w.ys, self.poses)
        return np.stack([np.maximum(fx - box, 0), np.minimum(fx + box, self.w.xs - 1), np.maximum(fy - box, 0),
                         np.minimum(fy + box, self.w.ys - 1)], 1).astype(np.int64)

    def window_x0(self):
        """[P] wx0 of the robots' windows (the start pose's cell, the reserved reach)"""
        box = box_of(self.name, self.w.res)
        _, fx, _ = fr.cells(self.w.res, self.w.xmin, self.w.ymin, self.w.xs, self.w.ys, self.x0)
        return np.maximum(fx - (self.W + box), 0).astype(np.int64)

    def sq_at_pose(self):
        """[P] the distance field at the poses' own cells (every pose of a scene has one)"""
        has, fx, fy = fr.cells(self.w.res, self.w.xmin, self.w.ymin, self.w.xs, self.w.ys, self.poses)
        assert has.all()
        oi, oj = np.nonzero(fr.cr.occupied(self.w.data, self.w.threshold))
        return np.array([((oi - int(y)) ** 2 + (oj - int(x)) ** 2).min() for x, y in zip(fx, fy)], dtype=np.int64)

    def sparse_sq(self):
        """a field that holds sq_at_pose at the poses' cells and -2 elsewhere: all `footprint_restatement.filtered` reads"""
        _, fx, fy = fr.cells(self.w.res, self.w.xmin, self.w.ymin, self.w.xs, self.w.ys, self.poses)
        sq = np.full((self.w.ys, self.w.xs), -2, dtype=np.int64)
        sq[fy.astype(int), fx.astype(int)] = self.sq_at_pose()
        return sq

    def ambiguous(self):
        sq_hit, sq_free, _ = fr.thresholds(*radii(self.name), self.w.res)
        s = self.sq_at_pose()
        return (s > sq_hit) & (s <= sq_free)


def _world(xs, ys, res):
    """an empty grid whose origin is no round number"""
    return pr.World(np.zeros((ys, xs), dtype=np.int8), res, -0.5 * xs * res + 0.0123 * res, -0.5 * ys * res - 0.0071 * res)


def _centre(w, i, j):
    return np.float64(j) * w.res + w.res / 2.0 + w.xmin, np.float64(i) * w.res + w.res / 2.0 + w.ymin


def _rot(th, b):
    c, s = math.cos(th), math.sin(th)
    return c * b[0] - s * b[1], s * b[0] + c * b[1]


def _wrap(th):
    return math.atan2(math.sin(th), math.cos(th))


# ---- A, B: one cell ----------------------------------------------------------------------------------------------------------------

def pulls(res):
    return (1e-6, 1e-3, 0.3 * res)


def vertex_point(verts, k, m, outward):
    """vertex k moved along the ray from the origin so that the adjacent half-planes' larger value is +m / -m"""
    _, _, h = fr.planes(verts)[:3]
    ha, hb = h[k - 1], h[k]
    s = m / max(ha, hb) if outward else -m / min(ha, hb)
    return verts[k][0] * (1.0 + s), verts[k][1] * (1.0 + s)


def edge_point(verts, k, t, m, outward):
    """the point at t along edge k moved along its normal by +m / -m"""
    nx, ny, _ = fr.planes(verts)[:3]
    a, b = verts[k], verts[(k + 1) % len(verts)]
    d = m if outward else -m
    return a[0] + t * (b[0] - a[0]) + d * nx[k], a[1] + t * (b[1] - a[1]) + d * ny[k]


def pose_for(w, cell, b, th):
    """the start pose with heading th from which the JUDGED pose (th through the wrap, which moves it by an ulp or two) has
    the centre of `cell` at the body point b"""
    cx, cy = _centre(w, *cell)
    rx, ry = _rot(judged([[0.0, 0.0, th]])[0, 2], b)
    return [cx - rx, cy - ry, th]


def single_cell_world(res, names):
    """one occupied cell in the middle of a grid that holds every probing pose's cell; at most 720 x 720, where the boxes of
    the poses farthest from the cell are clipped"""
    box = max(box_of(n, res) for n in names)
    side = min(720, 2 * (2 * box + 2 + 9) + 1)
    w = _world(side, side, res)
    cell = (side // 2, side // 2)
    w.data[cell] = 100
    return w, cell


def _keep(family, tag, name, w, cell, cands, W):
    """the candidates [(x0, outward)] whose 50-digit value has the intended sign with |.| >= MARGIN and whose pose has a cell
    `classify` calls ambiguous"""
    verts = POLYGONS[name]
    x0, hit, margin = [], [], []
    for x, outward in cands:
        p = judged([x])[0]
        if not (np.array_equal(p[:2], np.asarray(x[:2], dtype=np.float64)) and fr.cells(w.res, w.xmin, w.ymin, w.xs, w.ys, p[None])[0][0]):
            continue
        v = exact_signed(w.res, w.xmin, w.ymin, cell[0], cell[1], verts, p)
        if (v > 0) != outward or abs(v) < MARGIN:
            continue
        x0.append(x)
        hit.append(not outward)
        margin.append(float(abs(v)))
    sc = EdgeScene(family, tag, name, w, np.array(x0).reshape(-1, 3), hit, margin, W)
    amb = sc.ambiguous()
    return EdgeScene(family, tag, name, w, sc.x0[amb], sc.hit[amb], sc.margin[amb], W)


def family_a(res, name, w=None, cell=None, W=W_DEFAULT):
    if w is None:
        w, cell = single_cell_world(res, names_at(res))
    verts = POLYGONS[name]
    rng = np.random.default_rng([1, NAMES.index(name), int(res * 1e6)])
    cands = []
    for k in range(len(verts)):
        for m in pulls(res):
            for outward in (False, True):
                cands.append((pose_for(w, cell, vertex_point(verts, k, m, outward), rng.uniform(-3.1, 3.1)), outward))
                cands.append((pose_for(w, cell, edge_point(verts, k, rng.uniform(0.05, 0.95), m, outward), rng.uniform(-3.1, 3.1)), outward))
    return _keep("A", "A-%s-%g" % (name, res), name, w, cell, cands, W)


def family_b(res, name, w=None, cell=None, W=W_DEFAULT):
    """edge k (one per polygon) at a_k = cos(th + atan2(ny_k, nx_k)) = eps, as the top and as the bottom edge of the polygon;
    the cell near either end of the edge and at a random point of it"""
    if w is None:
        w, cell = single_cell_world(res, names_at(res))
    verts = POLYGONS[name]
    rng = np.random.default_rng([2, NAMES.index(name), int(res * 1e6)])
    nx, ny, _ = fr.planes(verts)[:3]
    k = int(rng.integers(0, len(verts)))
    phi = math.atan2(ny[k], nx[k])
    cands = []
    for q, eps in enumerate(EPS_PARALLEL):
        for side in (1.0, -1.0):
            th = _wrap(side * math.acos(eps) - phi)
            for m in pulls(res):
                for outward in (False, True):
                    for t in ((0.03, 0.97)[q % 2], rng.uniform(0.05, 0.95)):
                        cands.append((pose_for(w, cell, edge_point(verts, k, t, m, outward), th), outward))
    sc = _keep("B", "B-%s-%g" % (name, res), name, w, cell, cands, W)
    sc.info = {"edge": k}
    return sc


def a_of_edge(sc):
    """[P] a_k of the scene's edge at every pose, in doubles"""
    nx, ny, _ = fr.planes(sc.verts)[:3]
    k = sc.info["edge"]
    th = sc.poses[:, 2]
    return nx[k] * np.cos(th) - ny[k] * np.sin(th)


# ---- C: the hollow block -----------------------------------------------------------------------------------------------------------

def hollow(family, tag, name, res, m, rng, xs, ys, cell, W, positions=("first", "last", "top", "bottom", "narrow")):
    """[EdgeScene]: the pose in `cell` = (fy, fx) of an xs x ys grid, every cell of its box occupied except those with
    exact_signed <= m (free), then one scene more per position with one cell of exact_signed <= -m occupied (hit)"""
    verts = POLYGONS[name]
    w = _world(xs, ys, res)
    fy, fx = cell
    pose = None
    for _ in range(50):
        x = [w.xmin + (fx + rng.uniform(0.05, 0.95)) * res, w.ymin + (fy + rng.uniform(0.05, 0.95)) * res, rng.uniform(-3.1, 3.1)]
        p = judged([x])[0]
        _, gx, gy = fr.cells(res, w.xmin, w.ymin, xs, ys, p[None])
        if np.array_equal(p[:2], np.asarray(x[:2])) and gx[0] == fx and gy[0] == fy:
            pose = x
            break
    assert pose is not None
    box = box_of(name, res)
    y0, y1, x0, x1 = max(fy - box, 0), min(fy + box, ys - 1), max(fx - box, 0), min(fx + box, xs - 1)
    ii, jj = [a.ravel() for a in np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")]
    v = signed_many(w, verts, p, ii, jj, at=(m, -m, 0.0))
    occ = v > m
    w.data[ii[occ], jj[occ]] = 100
    margin = float(np.abs(v[occ]).min())
    info = {"occupied": int(occ.sum()), "box": (x0, x1, y0, y1)}
    scenes = [EdgeScene(family, tag + "-free", name, w, [pose], [False], [margin], W, info)]
    deep = v <= -m
    if not deep.any():
        return scenes
    # (the added cell farther from the pose's than sqrt(sq_hit) cells: the field alone must not call the pose a hit)
    far = (ii - fy) ** 2 + (jj - fx) ** 2 > fr.thresholds(*radii(name), res)[0]
    ends = {int(r): (int(jj[deep & (ii == r)].min()), int(jj[deep & (ii == r)].max())) for r in np.unique(ii[deep])}
    ok = lambda r, j: bool(far[(ii == r) & (jj == j)][0])
    rows = [r for r in sorted(ends) if ok(r, ends[r][0]) and ok(r, ends[r][1])]
    picks = {}
    if rows:
        mid = rows[len(rows) // 2 if len(rows) < 3 else int(rng.integers(1, len(rows) - 1))]
        picks = {"first": (mid, ends[mid][0]), "last": (mid, ends[mid][1]), "top": (rows[-1], ends[rows[-1]][0]),
                 "bottom": (rows[0], ends[rows[0]][1])}
        if rows[-1] != max(ends) or rows[0] != min(ends):
            del picks["top"], picks["bottom"]
    inside = v <= 0.0
    one = [r for r in rows if (inside & (ii == r)).sum() == 1]
    if one:
        r = one[len(one) // 2]
        picks["narrow"] = (r, ends[r][0])
    for pos in positions:
        if pos not in picks:
            continue
        i, j = picks[pos]
        w2 = pr.World(w.data.copy(), res, w.xmin, w.ymin)
        w2.data[i, j] = 100
        d = float(abs(v[(ii == i) & (jj == j)][0]))
        scenes.append(EdgeScene(family, "%s-%s" % (tag, pos), name, w2, [pose], [True], [min(margin, d)], W,
                                dict(info, cell=(i, j), position=pos)))
    return scenes


def hollow_names(res):
    """the polygons of family C: below 0.01 m a block has 0.4 to 0.6 million cells, and two polygons (one where no window fits)
    keep the reference quick"""
    return names_at(res) if res >= 0.01 else ("rect",) if res == RES_NO_WINDOW else ("rect", "gon16")


def family_c(res, name):
    box = box_of(name, res)
    W = W_DEFAULT
    side = 2 * (box + W + 2) + 1
    rng = np.random.default_rng([3, NAMES.index(name), int(res * 1e6)])
    out = []
    for m in (1e-6, 0.3 * res):
        out += hollow("C", "C-%s-%g-m%g" % (name, res, m), name, res, m, rng, side, side, (side // 2, side // 2), W)
    return out


# ---- D: seams and clips ------------------------------------------------------------------------------------------------------------

SEAM_NAMES = ("rect", "oct")          # (their vertices share one radius: several probes of one cell from one pose's cell)
SEAM_RES = (0.1, 0.01)


def _seam_single(name, res, rng, xs, ys, cell, W, tag, turn=0.0):
    """family A's vertex probes of ONE cell from poses that all lie in `cell` = (fy, fx): the heading of vertex k's probe turns
    the vertex to where vertex 0's was"""
    verts = POLYGONS[name]
    w = _world(xs, ys, res)
    fy, fx = cell
    px, py = w.xmin + (fx + 0.5) * res, w.ymin + (fy + 0.5) * res
    th0 = _wrap(turn + rng.uniform(0.2, 1.3) - math.atan2(verts[0][1], verts[0][0]))          # vertex 0 towards the grid's inside
    rx, ry = _rot(th0, verts[0])
    j, i = int(math.floor((px + rx - w.xmin) / res)), int(math.floor((py + ry - w.ymin) / res))
    if not (0 <= i < ys and 0 <= j < xs):
        return None
    w.data[i, j] = 100
    cands = []
    for k in range(len(verts)):
        th = _wrap(th0 + math.atan2(verts[0][1], verts[0][0]) - math.atan2(verts[k][1], verts[k][0]))
        for m in (1e-6, 1e-3):
            for outward in (False, True):
                cands.append((pose_for(w, (i, j), vertex_point(verts, k, m, outward), th), outward))
    sc = _keep("D", tag, name, w, (i, j), cands, W)
    _, gx, gy = fr.cells(res, w.xmin, w.ymin, xs, ys, sc.poses)
    here = (gx == fx) & (gy == fy)
    return EdgeScene("D", tag, name, w, sc.x0[here], sc.hit[here], sc.margin[here], W)


def family_d(res, name):
    """lower left: the pose's cell at column box + c0 and row box - d, d = 0..3, with W = max(c0, 2): wx0 = wy0 = 0, the box's
    first column in the window is c0, its clipped height 2 box + 1 - d.  Upper right: box and window clipped from above"""
    box = box_of(name, res)
    rng = np.random.default_rng([4, NAMES.index(name), int(res * 1e6)])
    out = []
    for q, c0 in enumerate(C0_LIST):
        W, d = max(c0, 2), q % 4
        fx, fy = box + c0, box - d
        xs, ys = fx + box + W + 3, fy + box + W + 3
        tag = "D-%s-%g-c%d" % (name, res, c0)
        out += hollow("D", tag, name, res, 1e-6, rng, xs, ys, (fy, fx), W, positions=("first", "last", "top", "bottom"))
        s = _seam_single(name, res, rng, xs, ys, (fy, fx), W, tag + "-cell")
        if s is not None and len(s.x0):
            out.append(s)
    for q in range(4):             # upper right: the pose's cell box - q - 1 cells from the last column and box - 3 + q from the last row
        W = 9
        xs, ys = 2 * box + W + 12, 2 * box + W + 9
        fx, fy = xs - 1 - (box - q - 1), ys - 1 - (box - 3 + q)
        tag = "D-%s-%g-ur%d" % (name, res, q)
        out += hollow("D", tag, name, res, 1e-6, rng, xs, ys, (fy, fx), W, positions=("first", "last", "top", "bottom"))
        s = _seam_single(name, res, rng, xs, ys, (fy, fx), W, tag + "-cell", turn=math.pi)
        if s is not None and len(s.x0):
            out.append(s)
    return out


# ---- E: the fan --------------------------------------------------------------------------------------------------------------------

FAN_N = (64, 128, 200)
FAN_NAMES = ("rect", "tri", "needle", "gon16")
FAN_RES = (0.1, 0.01)
FAN_ROT = 30.0               # rad/s: +-3 rad in the one step of 0.1 s


class Fan:
    """one position, N headings: dwa (ns = (1, 1, N)), World, x0 [3], the Robot (samples and poses), free bool [N], margin [N]"""

    def __init__(self, name, res, N, w, x0):
        self.name, self.verts, self.N, self.w, self.x0 = name, POLYGONS[name], N, w, np.asarray(x0, dtype=np.float64)
        self.dwa = dwa_cfg(res, W=2, ns=(1, 1, N), rot=FAN_ROT)
        self.dwa = pr.with_(self.dwa, max_vel_x=0.0, acc_lim_th=FAN_ROT)          # zero linear window: a reach of 1 cell
        self.robot = pr.Robot(self.dwa, self.x0, np.zeros(3))
        self.poses = self.robot.poses.reshape(N, 3)
        hit, self.margin = fr.brute(w.res, w.xmin, w.ymin, w.data, w.threshold, self.verts, self.poses)
        self.free = ~hit
        self.tag = "E-%s-%g-N%d" % (name, res, N)

    def sq_at_pose(self):
        """the distance field at the cell all N poses share"""
        _, fx, fy = fr.cells(self.w.res, self.w.xmin, self.w.ymin, self.w.xs, self.w.ys, self.poses)
        assert (fx == fx[0]).all() and (fy == fy[0]).all()
        oi, oj = np.nonzero(self.w.data)
        return int(((oi - int(fy[0])) ** 2 + (oj - int(fx[0])) ** 2).min())

    def ambiguous(self):
        """`classify` sends every lane to the exact test: sq_hit < sq <= sq_free"""
        sq_hit, sq_free, _ = fr.thresholds(*radii(self.name), self.w.res)
        return sq_hit < self.sq_at_pose() <= sq_free


@functools.lru_cache(maxsize=None)
def fan(name, res, N):
    """two or three cells in the annulus r_in .. r_out around the pose; the first seed at which every heading is decided and
    both verdicts occur among them"""
    r_in, r_out = radii(name)
    box = box_of(name, res)
    side = 2 * (box + 3) + 1
    for seed in range(40):
        rng = np.random.default_rng([5, NAMES.index(name), int(res * 1e6), N, seed])
        w = _world(side, side, res)
        c = side // 2
        x0 = [w.xmin + (c + rng.uniform(0.05, 0.95)) * res, w.ymin + (c + rng.uniform(0.05, 0.95)) * res, rng.uniform(-0.1, 0.1)]
        for _ in range(int(rng.integers(2, 4))):
            r, a = rng.uniform(r_in + 0.25 * (r_out - r_in), r_out), rng.uniform(-np.pi, np.pi)
            j, i = int(math.floor((x0[0] + r * math.cos(a) - w.xmin) / res)), int(math.floor((x0[1] + r * math.sin(a) - w.ymin) / res))
            w.data[i, j] = 100
        f = Fan(name, res, N, w, x0)
        if (f.margin >= 100 * fr.DECIDED).all() and 3 <= f.free.sum() <= N - 3 and f.ambiguous():
            return f
    raise AssertionError("no decided fan for %s at %g, N = %d" % (name, res, N))


# ---- the lists the two test modules run --------------------------------------------------------------------------------------------

def families(family, res):
    """[EdgeScene] of a family at a resolution (A - D)"""
    if family in ("A", "B"):
        names = names_at(res)
        w, cell = single_cell_world(res, names)
        return [(family_a if family == "A" else family_b)(res, n, w, cell) for n in names]
    if family == "C":
        return [s for n in hollow_names(res) for s in family_c(res, n)]
    if family == "D":
        return [s for n in SEAM_NAMES for s in family_d(res, n)]
    raise ValueError(family)


CASES = [(f, r) for f in ("A", "B", "C") for r in RES] + [("D", r) for r in SEAM_RES]


# ---- the body layer: the same probes where a robot's stamp is the obstacle ---------------------------------------------------------

BODY_RES = (0.1, 0.05, 0.01)
BODY_NAMES = ("rect", "tri", "oct")


def with_far_robot(sc):
    """(World, poses [2][3], mask [2]) for a single-cell scene: the grid widened to the right, robot 1 stamped there -- more
    than 3 box + W cells from every probing pose's cell, outside every window and every near-map neighbourhood -- and robot 0,
    whose poses the probes are, not stamped"""
    box = box_of(sc.name, sc.w.res)
    pad = 4 * box + sc.W + 8
    data = np.pad(sc.w.data, ((0, 0), (0, pad)))
    w = pr.World(data, sc.w.res, sc.w.xmin, sc.w.ymin)
    far = [w.xmin + (w.xs - box - 2 + 0.37) * w.res, w.ymin + (w.ys // 2 + 0.41) * w.res, 0.7]
    return w, np.array([sc.x0[0], far]), np.array([0, 1], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def stamp_probes(res, name):
    """(World -- empty --, layer poses [2][3], mask, x0 [P][3], hit [P], margin [P]): robot 1 stamped in the middle of an empty
    grid, and poses of robot 0 that bring a vertex, pulled inward / outward by family A's three pulls, to the centre of the
    stamp's extreme cell in one of twelve directions.  Family A's edge probes are left out: an edge laid along a stamp of many
    cells has other cells of the stamp inside the polygon, and no single cell decides.  The verdicts are exact_verdicts' on
    the grid that holds the stamp; kept are the poses with a margin of MARGIN"""
    from tests import body_layer_restatement as br
    verts = POLYGONS[name]
    box = box_of(name, res)
    side = 6 * box + 2 * W_DEFAULT + 9
    w = _world(side, side, res)
    rng = np.random.default_rng([6, NAMES.index(name), int(res * 1e6)])
    c = side // 2
    stamp_pose = [w.xmin + (c + rng.uniform(0.05, 0.95)) * res, w.ymin + (c + rng.uniform(0.05, 0.95)) * res, rng.uniform(-3.1, 3.1)]
    body, body_margin = br.cover(w, verts, stamp_pose)
    assert body_margin >= fr.DECIDED
    bi, bj = np.nonzero(body)
    grid = pr.World(body.astype(np.int8) * 100, res, w.xmin, w.ymin)
    x0 = []
    for q in range(12):
        a = 2.0 * math.pi * (q + rng.uniform(0.1, 0.9)) / 12.0
        far = int(np.argmax(bj * math.cos(a) + bi * math.sin(a)))
        for k in range(len(verts)):
            th = _wrap(a + math.pi - math.atan2(verts[k][1], verts[k][0]))          # vertex k points against direction a
            for m in pulls(res):
                for outward in (False, True):
                    x0.append(pose_for(w, (int(bi[far]), int(bj[far])), vertex_point(verts, k, m, outward), th))
    x0 = np.array(x0)
    hit, margin, _ = exact_verdicts(grid, verts, judged(x0), nearest=4)          # (of the stamp's cells one is near the boundary)
    keep = margin >= MARGIN
    return w, np.array([x0[0], stamp_pose]), np.array([0, 1], dtype=np.int32), x0[keep], hit[keep], margin[keep]

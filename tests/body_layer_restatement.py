"""The body layer (eea_body_layer_* / eea_body_collision_check_batch / eea_body_validate_control_batch /
eea_body_dwa_control_batch / eea_tick_batch_bodies: csrc/body_layer_kernel.hip) restated in numpy on top of
tests/footprint_restatement.py and tests/footprint_plan_restatement.py, for tests/test_body_layer.py (CPU) and
tests/test_gpu_body_layer.py.

Robot j is STAMPED when it is active, its pose is finite and its box touches the grid; its body is the set of in-grid cells
whose centre lies in the closed polygon placed at its pose.  The verdict of a pose of robot i is the footprint's verdict on
robot i's OWN GRID: the grid with every cell of every other stamped robot's body set to 100.  Everything below is that
sentence: own_grid, then footprint_restatement.brute / footprint_plan_restatement.validate / dwa_control on it."""
import functools
import math

import numpy as np

from tests import footprint_plan_restatement as pr
from tests import footprint_restatement as fr

SNAP = 5


def box_of(w, verts):
    pl = fr.planes(verts)
    return fr.thresholds(pl[3], pl[4], w.res)[2]


def cells_of(w, poses):
    """(fx [P], fy [P]): floor((p - min) / res) as doubles, no wrap; NaN for a pose that is not finite"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.floor((poses[:, 0] - np.float64(w.xmin)) / np.float64(w.res))
        fy = np.floor((poses[:, 1] - np.float64(w.ymin)) / np.float64(w.res))
    return fx, fy


def stamped(w, verts, poses, mask=None):
    """bool [B]: active, finite, and the box touches the grid (classify's first test, as doubles)"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    box = float(box_of(w, verts))
    fx, fy = cells_of(w, poses)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(poses).all(1) & (fx + box >= 0.0) & (fx - box <= w.xs - 1.0) & (fy + box >= 0.0) & (fy - box <= w.ys - 1.0)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    return ok


def cover(w, verts, pose):
    """(body bool [ys][xs], margin): the in-grid cells whose centre lies in the closed polygon placed at `pose` (finite), and
    the smallest distance-like margin |max_k (n_k . b - h_k)| of any in-grid centre to the polygon's boundary"""
    ii, jj = np.divmod(np.arange(w.ys * w.xs), w.xs)
    worst, inside = fr._signed(w.res, w.xmin, w.ymin, fr.planes(verts), np.asarray(pose, dtype=np.float64).reshape(1, 3), ii, jj)
    return inside[0].reshape(w.ys, w.xs), float(np.abs(worst[0]).min())


class Layer:
    """what an update leaves: flags [B], covers (list of bool maps, None for a robot that is not stamped), margins [B] (inf for
    those), cover int32 [ys][xs], near int32 [ys + 2 box][xs + 2 box], snapshot [B][5] (numpy's sine and cosine)"""

    def __init__(self, w, verts, poses, mask=None):
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
        self.w, self.verts, self.poses = w, verts, poses
        self.flags = stamped(w, verts, poses, mask)
        self.covers, self.margins = [], np.full(len(poses), np.inf)
        self.cover = np.zeros((w.ys, w.xs), dtype=np.int32)
        for j in range(len(poses)):
            if self.flags[j]:
                body, self.margins[j] = cover(w, verts, poses[j])
                self.covers.append(body)
                self.cover += body
            else:
                self.covers.append(None)
        self.box = box_of(w, verts)
        self.near = near(w, verts, poses, self.flags)
        self.snapshot = np.zeros((len(poses), SNAP))
        for j in np.nonzero(self.flags)[0]:
            self.snapshot[j] = [poses[j, 0], poses[j, 1], np.sin(poses[j, 2]), np.cos(poses[j, 2]), 1.0]

    def decided(self):
        """bool [B]: a stamped robot is decided when no in-grid centre lies within DECIDED of its polygon's boundary"""
        return self.margins >= fr.DECIDED


def near(w, verts, poses, flags):
    """int32 [ys + 2 box][xs + 2 box] over the cells [-box, size + box): the stamped robots whose cell lies within Chebyshev
    distance Rn = 2 box of the cell"""
    box = box_of(w, verts)
    rn = 2 * box
    out = np.zeros((w.ys + 2 * box, w.xs + 2 * box), dtype=np.int32)
    fx, fy = cells_of(w, poses)
    for j in np.nonzero(flags)[0]:
        cx, cy = int(fx[j]) + box, int(fy[j]) + box
        out[max(cy - rn, 0):cy + rn + 1, max(cx - rn, 0):cx + rn + 1] += 1
    return out


def near_minus_self(layer, fx, fy, i):
    """near at the cell (fx, fy) -- inside the near map -- without robot i (-1: nobody)"""
    box = layer.box
    n = int(layer.near[int(fy) + box, int(fx) + box])
    if i >= 0 and layer.flags[i]:
        sx, sy = cells_of(layer.w, layer.poses[i:i + 1])
        if abs(fx - sx[0]) <= 2 * box and abs(fy - sy[0]) <= 2 * box:
            n -= 1
    return n


def own_grid(w, covers, i):
    """the World of robot i (-1: nobody's): w with the bodies of every other stamped robot at 100"""
    data = w.data.copy()
    for j, body in enumerate(covers):
        if body is not None and j != i:
            data[body] = 100
    return pr.World(data, w.res, w.xmin, w.ymin, w.threshold)


def check(layer, poses, self_index=None, static=True):
    """(hit bool [P], margin [P]) of the poses, pose q robot self_index[q]'s (None / -1: nobody's); static False: robots only"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    idx = np.full(len(poses), -1) if self_index is None else np.asarray(self_index)
    hit, margin = np.zeros(len(poses), dtype=bool), np.full(len(poses), np.inf)
    base = layer.w if static else pr.World(np.zeros_like(layer.w.data), layer.w.res, layer.w.xmin, layer.w.ymin, layer.w.threshold)
    for i in np.unique(idx):
        sel = idx == i
        hit[sel], margin[sel] = pr.verdicts(own_grid(base, layer.covers, int(i)), layer.verts, poses[sel])
    return hit, margin


def validate(layer, x0, u, dt, horizon, self_index):
    """(valid int32 [P], decided bool [P])"""
    valid, decided = np.zeros(len(x0), dtype=np.int32), np.zeros(len(x0), dtype=bool)
    for q in range(len(x0)):
        v, d = pr.validate(own_grid(layer.w, layer.covers, int(self_index[q])), layer.verts, x0[q:q + 1], u[q:q + 1], dt, horizon)
        valid[q], decided[q] = v[0], d[0]
    return valid, decided


def dwa_control(layer, dwa, robot, i, vref=None, xt=None, dt_ref=0.0):
    """footprint_plan_restatement.Answer of `robot` (a pr.Robot) as robot i of the layer"""
    return pr.dwa_control(own_grid(layer.w, layer.covers, int(i)), layer.verts, dwa, robot, vref=vref, xt=xt, dt_ref=dt_ref)


# ---- the greedy fleet of the study scene -----------------------------------------------------------------------------------------

MAX_FLEET = 40
VAL_DT, VAL_HORIZON = 0.1, 0.5          # "5 steps of vref"


@functools.lru_cache(maxsize=None)
def greedy_fleet(name):
    """(indices into the study's x0, Layer of those robots): taken in order, each free on the static grid and its body
    sharing no cell with an earlier one's, at most MAX_FLEET"""
    w, x0, _, _, _, _ = pr.study()
    verts = fr.FOOTPRINTS[name]
    free = ~pr.verdicts(w, verts, x0)[0]
    taken, union = [], np.zeros((w.ys, w.xs), dtype=bool)
    for q in range(pr.N_STUDY):
        if len(taken) == MAX_FLEET:
            break
        if not free[q] or not stamped(w, verts, x0[q:q + 1])[0]:
            continue
        body = cover(w, verts, x0[q])[0]
        if (body & union).any():
            continue
        taken.append(q)
        union |= body
    idx = np.array(taken)
    return idx, Layer(w, verts, x0[idx])


@functools.lru_cache(maxsize=None)
def fleet_answers(name, mode="vref"):
    """per robot of the greedy fleet: (plain Answer, layer Answer) of the dynamic window, mode "vref" or "traj" (the plain
    answer only in the twist-error mode: None in the other, whose free sets are the same)"""
    w, x0, vb, vref, xt, robots = pr.study()
    idx, layer = greedy_fleet(name)
    out = []
    for i, q in enumerate(idx):
        kw = dict(vref=vref[q]) if mode == "vref" else dict(xt=xt[q], dt_ref=pr.DT_REF)
        plain = pr.dwa_control(w, layer.verts, pr.DWA_OMNI, robots[q], **kw) if mode == "vref" else None
        out.append((plain, dwa_control(layer, pr.DWA_OMNI, robots[q], i, **kw)))
    return out


@functools.lru_cache(maxsize=None)
def fleet_validate(name):
    """(plain valid, layer valid, decided) of validate_control of the study's vref over 5 steps, per robot of the greedy fleet"""
    w, x0, _, vref, _, _ = pr.study()
    idx, layer = greedy_fleet(name)
    plain, dec0 = pr.validate(w, layer.verts, x0[idx], vref[idx], VAL_DT, VAL_HORIZON)
    with_, dec1 = validate(layer, x0[idx], vref[idx], VAL_DT, VAL_HORIZON, np.arange(len(idx)))
    return plain, with_, dec0 & dec1


def study_row(name):
    """(robots, validate verdicts changed, window free sets changed, undecided robots, smallest stamp margin)"""
    idx, layer = greedy_fleet(name)
    plain, with_, vdec = fleet_validate(name)
    ans = fleet_answers(name)
    changed = sum(not np.array_equal(a.free, b.free) for a, b in ans)
    und = sum(not (a.decided and b.decided and vdec[i] and layer.decided()[i]) for i, (a, b) in enumerate(ans))
    return len(idx), int((plain != with_).sum()), changed, und, float(layer.margins.min())


def window_mix(name):
    """(windows that lose every free sample they had, that keep all they had, that lose some but keep at least one)"""
    lose_all = keep = some = 0
    for a, b in fleet_answers(name):
        if np.array_equal(a.free, b.free):
            keep += 1
        elif not b.free.any():
            lose_all += 1
        else:
            some += 1
    return lose_all, keep, some

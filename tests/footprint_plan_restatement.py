"""Footprint planning (eea_footprint_validate_control_batch / eea_footprint_dwa_control_batch / eea_tick_batch_footprint:
csrc/footprint_plan_kernel.hip) restated on the host, for tests/test_footprint_plan.py (CPU) and
tests/test_gpu_footprint_plan.py.

Defined by composition: the window and the sample values as the oracle forms them (repeated +=, dynamic_window.cpp:92-235),
every rollout through oracle.pyoracle.integrate_twist plus the wrap (numerics.hpp:312-330), the verdict and the margin of every
pose from footprint_restatement.brute, the costs in the reference's order (dynamic_window.cpp:237-286), the first strict minimum
in loop order.  A sample is DECIDED when every step up to and including its first hit has a margin of at least
footprint_restatement.DECIDED; a robot is decided when all its samples are."""
import functools
import math

import numpy as np

from oracle import pyoracle as po
from tests import footprint_restatement as fr

DBL_MAX = 1.7976931348623157e308
COLL = (0.7, 1.0, 0.2, 0.8)          # test_gpu_dwa_parity's radii and threshold (the footprint reads the threshold only)
# dt, horizon, acc_dt, acc_lim x/y/th, max/min vx, max/min vy, max/min w, samples: the field order of capi.DwaCfg
DWA_OMNI = (0.1, 1.0, 0.2, 1.0, 1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 2.0, -2.0, 3, 8, 5)
DWA_CART = (0.1, 2.0, 0.2, 2.5, 0.0, 1.0, 1.0, -1.0, 0.0, 0.0, 2.0, -2.0, 3, 1, 5)
FIELDS = ("dt", "horizon", "acc_dt", "acc_lim_x", "acc_lim_y", "acc_lim_th", "max_vel_x", "min_vel_x", "max_vel_y", "min_vel_y",
          "max_rot_vel", "min_rot_vel", "vx_samples", "vy_samples", "vth_samples")


def with_(dwa, ns=None, **kw):
    """the DWA tuple with other sample counts / fields"""
    d = dict(zip(FIELDS, dwa))
    d.update(kw)
    if ns is not None:
        d["vx_samples"], d["vy_samples"], d["vth_samples"] = ns
    return tuple(d[n] for n in FIELDS)


class World:
    """a grid: data int8 [ys][xs] at `res` metres per cell from (xmin, ymin); threshold = occupied_threshold"""

    def __init__(self, data, res, xmin, ymin, threshold=COLL[3]):
        self.data, self.res, self.xmin, self.ymin, self.threshold = np.ascontiguousarray(data, dtype=np.int8), res, xmin, ymin, threshold
        self.ys, self.xs = self.data.shape


def world(seed):
    """the world of test_gpu_dwa_parity._world(seed): 80 x 60 at 0.1 m; returns (World, the generator behind it)"""
    rng = np.random.default_rng(seed)
    xs, ys = 80, 60
    data = np.zeros((ys, xs), dtype=np.int8)
    data[20:26, 30:38] = 100
    data[45:48, 10:30] = 100
    data[rng.integers(0, ys, 20), rng.integers(0, xs, 20)] = 100
    data[5:9, 60:70] = -1
    return World(data, 0.1, -2.0, -1.0), rng


def steps_of(dwa):
    return po.steps(dwa[1], dwa[0])


def window(dwa, vb):
    """(lower [3], upper [3], delta [3], ns [3]) of dynamic_window.cpp:191-235; a sample count of 0 is raised to 1"""
    acc = np.array(dwa[3:6]) * dwa[2]
    vmax, vmin = np.array([dwa[6], dwa[8], dwa[10]]), np.array([dwa[7], dwa[9], dwa[11]])
    vb = np.asarray(vb, dtype=np.float64)
    lower, upper = np.fmax(vb - acc, vmin), np.fmin(vb + acc, vmax)
    ns = [int(n) if n else 1 for n in dwa[12:15]]
    delta = np.array([(upper[a] - lower[a]) / float(ns[a] - 1) if ns[a] > 1 else 0.0 for a in range(3)])
    return lower, upper, delta, ns


def samples(dwa, vb):
    """[nsamp][3] in the reference's loop order (vx outermost), every value by repeated +="""
    lower, _, delta, ns = window(dwa, vb)
    axes = []
    for a in range(3):
        v, vals = np.float64(lower[a]), []
        for _ in range(ns[a]):
            vals.append(v)
            v = v + np.float64(delta[a])
        axes.append(vals)
    return np.array([[vx, vy, w] for vx in axes[0] for vy in axes[1] for w in axes[2]], dtype=np.float64).reshape(-1, 3)


def reach(dwa, vb, res):
    """the robot's own reach in cells: ceil(steps * |dt| * sqrt(mx^2 + my^2) / res) + 1, mx / my the largest |lower|, |upper|"""
    lower, upper, _, _ = window(dwa, vb)
    mx, my = max(abs(lower[0]), abs(upper[0])), max(abs(lower[1]), abs(upper[1]))
    return math.ceil(steps_of(dwa) * abs(dwa[0]) * math.sqrt(mx * mx + my * my) / res) + 1.0


def limits_reach(dwa, res):
    """the same from vmin / vmax: what a launch reserves its window for"""
    mx, my = max(abs(dwa[6]), abs(dwa[7])), max(abs(dwa[8]), abs(dwa[9]))
    return math.ceil(steps_of(dwa) * abs(dwa[0]) * math.sqrt(mx * mx + my * my) / res) + 1.0


def rollout(x0, u, dt, steps):
    """[steps][3]: validate_control's poses (integrate_twist, the heading wrapped after every step)"""
    out = np.empty((steps, 3))
    x = np.asarray(x0, dtype=np.float64).copy()
    for i in range(steps):
        x = po.integrate_twist(x, u, dt)
        x[2] = po.normalize_angle_PI(x[2])
        out[i] = x
    return out


def verdicts(w, verts, poses):
    """(hit bool [n], margin [n]) of footprint_restatement.brute, in chunks"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    hit, margin = np.zeros(len(poses), dtype=bool), np.full(len(poses), np.inf)
    for a in range(0, len(poses), 4096):
        hit[a:a + 4096], margin[a:a + 4096] = fr.brute(w.res, w.xmin, w.ymin, w.data, w.threshold, verts, poses[a:a + 4096])
    return hit, margin


def first_hits(hit, margin):
    """per trajectory of hit / margin [n][steps]: (first colliding step or -1, decided)"""
    n, steps = hit.shape
    first = np.where(hit.any(1), hit.argmax(1), -1) if steps else np.full(n, -1)
    upto = np.where(first < 0, steps, first + 1)
    ok = margin >= fr.DECIDED
    decided = np.array([ok[q, :upto[q]].all() for q in range(n)], dtype=bool)
    return first, decided


def validate(w, verts, x0, u, dt, horizon):
    """(valid int [P], decided bool [P]) of validate_control for the polygon"""
    steps = po.steps(horizon, dt)
    P = len(x0)
    poses = np.array([rollout(x0[q], u[q], dt, steps) for q in range(P)]).reshape(P, steps, 3)
    hit, margin = verdicts(w, verts, poses)
    first, decided = first_hits(hit.reshape(P, steps), margin.reshape(P, steps))
    return (first < 0).astype(np.int32), decided


class Robot:
    """one robot's dynamic window: u [nsamp][3], poses [nsamp][steps][3] -- the part no footprint changes"""

    def __init__(self, dwa, x0, vb):
        self.u = samples(dwa, vb)
        self.steps = steps_of(dwa)
        self.poses = np.array([rollout(x0, s, dwa[0], self.steps) for s in self.u]).reshape(len(self.u), self.steps, 3)


def traj_cost(dwa, poses, first, xt, dt_ref):
    """the trajectory objective of one sample (dynamic_window.cpp:258-286), xt [n_ref][3]; DBL_MAX after a hit"""
    if first >= 0:
        return DBL_MAX
    n_ref = len(xt)
    tf = float(n_ref) * dt_ref
    t, cost = 0.0, 0.0
    for p in poses:
        j = int(round_half_away(float(n_ref - 1) * t / tf))
        dx, dy = xt[j, 0] - p[0], xt[j, 1] - p[1]
        cost += math.sqrt(dx * dx + dy * dy)
        cost += abs(po.normalize_angle_PI(po.normalize_angle_PI(xt[j, 2]) - p[2]))
        t += dwa[0]
    return cost


def round_half_away(v):
    """C's round()"""
    return math.floor(v + 0.5) if v >= 0.0 else math.ceil(v - 0.5)


def twist_cost(u, first, vref):
    if first >= 0:
        return DBL_MAX
    e0, e1, e2 = vref[0] - u[0], vref[1] - u[1], vref[2] - u[2]
    return (e0 * e0 + e2 * e2) + e1 * e1


class Answer:
    """what DynamicWindow::control gives for the polygon: found, u_opt, the minimum and every sample's cost, which samples are
    free, whether the robot is decided, and the samples themselves"""

    def __init__(self, found, u_opt, cost, costs, free, decided, samples):
        self.found, self.u_opt, self.cost, self.costs, self.free, self.decided = found, u_opt, cost, costs, free, decided
        self.samples = samples          # [nsamp][3], in loop order


def dwa_control(w, verts, dwa, robot, vref=None, xt=None, dt_ref=0.0):
    n, steps = len(robot.u), robot.steps
    hit, margin = verdicts(w, verts, robot.poses)
    first, decided = first_hits(hit.reshape(n, steps), margin.reshape(n, steps))
    if xt is not None:
        costs = np.array([traj_cost(dwa, robot.poses[s], first[s], xt, dt_ref) for s in range(n)])
    else:
        costs = np.array([twist_cost(robot.u[s], first[s], vref) for s in range(n)])
    best, arg = DBL_MAX, -1
    for s in range(n):           # the first strict minimum in loop order
        if costs[s] < best:
            best, arg = costs[s], s
    found = not abs(best - DBL_MAX) < 1.0e-12
    u_opt = robot.u[arg].copy() if arg >= 0 else np.zeros(3)
    return Answer(int(found), u_opt, best, costs, first < 0, bool(decided.all()), robot.u)


# ---- the study scene: world(3), DWA_OMNI, 256 robots drawn as test_gpu_dwa_parity draws them --------------------------------

N_STUDY, N_REF, DT_REF = 256, 50, 0.1


@functools.lru_cache(maxsize=None)
def study():
    """(World, x0 [256][3], vb, vref, xt [256][50][3], [Robot]): computed once per process"""
    w, rng = world(3)
    P = N_STUDY
    x0 = np.stack([rng.uniform(-1.5, 5.5, P), rng.uniform(-0.5, 4.5, P), rng.uniform(-np.pi, np.pi, P)], 1)
    vb = np.stack([rng.uniform(-1, 1, P), rng.uniform(-1, 1, P), rng.uniform(-2, 2, P)], 1)
    vref = np.stack([rng.uniform(-1, 1, P), rng.uniform(-1, 1, P), rng.uniform(-2, 2, P)], 1)
    xt = np.empty((P, N_REF, 3))
    for i in range(P):      # reference trajectories: constant-twist arcs from the start pose, as test_dwa_traj_mode's
        x, tw = x0[i].copy(), np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-2, 2)])
        for t in range(N_REF):
            x = po.integrate_twist(x, tw, DT_REF)
            xt[i, t] = x
    robots = [Robot(DWA_OMNI, x0[q], vb[q]) for q in range(P)]
    return w, x0, vb, vref, xt, robots


@functools.lru_cache(maxsize=None)
def study_answers(name, mode):
    """[Answer] of the study's robots for the footprint `name`, mode "vref" or "traj" """
    w, x0, vb, vref, xt, robots = study()
    verts = fr.FOOTPRINTS[name]
    if mode == "vref":
        return [dwa_control(w, verts, DWA_OMNI, robots[q], vref=vref[q]) for q in range(N_STUDY)]
    return [dwa_control(w, verts, DWA_OMNI, robots[q], xt=xt[q], dt_ref=DT_REF) for q in range(N_STUDY)]


def mix(answers):
    """(undecided robots, no free sample, every sample free, mixed)"""
    und = sum(not a.decided for a in answers)
    none = sum(not a.free.any() for a in answers)
    every = sum(bool(a.free.all()) for a in answers)
    return und, none, every, len(answers) - none - every

"""The fleet layer (include/ergodic_amd.h: eea_fleet_layer_*, eea_tick_batch_fleet) restated for the tests: the offset set F
cell by cell, the counts and the cell table in numpy, the per-robot grids on which the CPU oracle is the checker, the small
oracle loop of a fleet tick with a collision tuple of its own, and the scenario the CPU and the GPU test share."""
import math

import numpy as np

from tests import sense_restatement as sr

NOT_STAMPED = -2 ** 31
RES = 0.05
COLL_S = (0.2, 0.4, 0.1, 0.8)     # small robots: boundary 0.2 m, search 0.4 m, obstacle threshold 0.1 m


def radii(coll, res):
    """(r_bnd, r_col, r_max) in cells, the library's formula (csrc/entry_util.hpp collision_params, collision.cpp:130-133)"""
    return (int(math.floor(coll[0] / res)), int(math.floor((coll[0] + coll[2]) / res)), int(math.floor(coll[1] / res)))


def ring_offsets(r_bnd, r_col, r_max):
    """S: the offsets (cell - centre) the ring search r_bnd .. r_max visits (collision.cpp:166-214) within r_col (:239)"""
    pts = set()
    for r0 in range(r_bnd, r_max + 1):
        x, y, err = -r0, 0, 2 - 2 * r0
        while x < 0:
            pts |= {(-x, y), (-y, -x), (x, -y), (y, x)}
            r = err
            if r <= y:
                y += 1
                err += 2 * y + 1
            if r > x or err > y:
                x += 1
                err += 2 * x + 1
    return {p for p in pts if p[0] * p[0] + p[1] * p[1] <= r_col * r_col}


def disc(body):
    return {(dx, dy) for dx in range(-body, body + 1) for dy in range(-body, body + 1) if dx * dx + dy * dy <= body * body}


def offset_set(r_bnd, r_col, r_max, body):
    """F = { o + d : o in S, d.d <= body^2 } as a set of (dx, dy)"""
    return {(o[0] + d[0], o[1] + d[1]) for o in ring_offsets(r_bnd, r_col, r_max) for d in disc(body)}


def cells_of(g, poses, mask=None):
    """[B][2] (x, y) of every robot, NOT_STAMPED twice for a robot that is masked or whose cell is outside the grid"""
    out = np.full((len(poses), 2), NOT_STAMPED, dtype=np.int64)
    for b, p in enumerate(poses):
        if mask is not None and mask[b] == 0:
            continue
        i, j = sr.world2grid(g, p[0], p[1])
        if j < g.xsize and i < g.ysize:
            out[b] = (j, i)
    return out


def counts(g, F, reach, cells):
    """count[(cy + R') , (cx + R')] = the stamped robots j with (cx, cy) - cell_j in F, over the padded centres"""
    out = np.zeros((g.ysize + 2 * reach, g.xsize + 2 * reach), dtype=np.int32)
    off = np.array(sorted(F), dtype=np.int64).reshape(-1, 2)
    for (x, y) in cells:
        if x == NOT_STAMPED:
            continue
        np.add.at(out, (y + off[:, 1] + reach, x + off[:, 0] + reach), 1)
    return out


def verdicts(g, data, S, F, cells, poses, owner):
    """eea_fleet_collision_check_batch by the rule, pose by pose: with c the pose's cell (the wrapped indices of a pose outside
    the grid taken as signed ints), 1 iff an occupied cell o of data [ysize][xsize] has o - c in S, or a stamped robot j other
    than owner (-1: nobody) has c - cell_j in F"""
    signed = lambda v: v - (1 << 32) if v >= (1 << 31) else v
    occupied = [(x, y) for y, x in zip(*np.nonzero(np.vectorize(lambda v: sr.blocks(v, g.occupied_threshold))(data)))]
    out = np.zeros(len(poses), dtype=np.int32)
    for q, (p, b) in enumerate(zip(poses, owner)):
        i, j = sr.world2grid(g, p[0], p[1])
        cx, cy = signed(j), signed(i)
        static = any((x - cx, y - cy) in S for (x, y) in occupied)
        robots = any(r != b and x != NOT_STAMPED and (cx - x, cy - y) in F for r, (x, y) in enumerate(cells))
        out[q] = 1 if static or robots else 0
    return out


def robot_grid(data, cells, b, body):
    """the grid of robot b: a copy of data [ysize][xsize] with every cell within d.d <= body^2 of each OTHER stamped robot's
    cell set to 100 (discs are clipped to the grid here: the tests keep the robots at least `body` cells inside)"""
    out = np.array(data, dtype=np.int8, copy=True)
    ys, xs = out.shape
    for j, (x, y) in enumerate(cells):
        if j == b or x == NOT_STAMPED:
            continue
        for (dx, dy) in disc(body):
            if 0 <= x + dx < xs and 0 <= y + dy < ys:
                out[y + dy, x + dx] = 100
    return out


# ---- the fleet tick on the oracle ------------------------------------------------------------------
BOUNDS = (-1.0, 11.0, -1.0, 5.0)      # 240 x 120 cells at 0.05
MEANS, SIGMAS = [[5.0, 2.0]], [[0.8, 0.8]]
OBSTACLE = (4.85, 1.55, 5.1, 1.8)     # one static block between the two groups
TICKS, VAL_DT, VAL_HORIZON, DT = 8, 0.1, 0.5, 0.1


def model_limits(model):
    if model == "omni":
        return np.diag([1.0, 1.0, 2.0]), np.array([1.0, 1.0, 2.0])
    return np.diag([1.0, 0.0, 2.0]), np.array([1.0, 0.0, 2.0])


def plain_grid(po):
    """(GridMap, data [ysize][xsize]) of the scenario: free space and one block"""
    x0, x1, y0, y1 = BOUNDS
    nx, ny = po.lib().eo_axis_length(x0, x1, RES), po.lib().eo_axis_length(y0, y1, RES)
    data = np.zeros((ny, nx), dtype=np.int8)
    cx, cy = x0 + (np.arange(nx) + 0.5) * RES, y0 + (np.arange(ny) + 0.5) * RES
    data[np.ix_((cy >= OBSTACLE[1]) & (cy <= OBSTACLE[3]), (cx >= OBSTACLE[0]) & (cx <= OBSTACLE[2]))] = 100
    return grid_map(po, data), data


def grid_map(po, data):
    x0, x1, y0, y1 = BOUNDS
    return po.GridMap(x0, x1, y0, y1, RES, np.ascontiguousarray(data).reshape(-1))


GAP = {"omni": 1.6, "simple_cart": 1.0}     # between the groups: they meet within the 8 ticks (the cart is the slower one)


def start_poses(model):
    """12 robots: six on the left facing +x, six on the right facing -x, 0.6 m apart within a group (outside each other's F,
    whose reach is 0.5 m); the target and the block lie between the groups"""
    ys = 0.35 + 0.6 * np.arange(6)
    left = np.stack([np.full(6, 5.0 - GAP[model] / 2), ys, np.zeros(6)], 1)
    right = np.stack([np.full(6, 5.0 + GAP[model] / 2), ys + 0.1, np.full(6, math.pi - 1e-3)], 1)
    return np.concatenate([left, right], 0)


class FleetOracle:
    """The loop body of Exploration<ModelT>::control (reference exploration.hpp:197-292) on the CPU oracle, as
    tests/test_host_mirror.py restates it, with the collision tuple and the target of this scenario; `grid` is set by the
    caller every tick (the robot's own grid)."""

    def __init__(self, po, model, dwa):
        self.po, self.model, self.dwa = po, model, dwa
        Rinv, lim = model_limits(model)
        om = {"omni": po.MODEL_OMNI, "simple_cart": po.MODEL_SIMPLE_CART}[model]
        self.ec = po.ErgodicControl(om, 0.1, 5.0, 0.1, 1.0, 10, Rinv, -lim, lim)
        self.ec.set_target(MEANS, SIGMAS)
        self.grid, self.memory, self.follow, self.i, self.u = None, [], False, 0, np.zeros(3)
        self.dwa_steps = po.steps(dwa[1], dwa[0])

    def tick(self, pose, vb):
        po = self.po
        self.memory.append(np.array(pose))
        source = "ergodic"
        if self.follow:
            self.i += 1
            self.follow = self.i != self.dwa_steps
            source = "dwa-follow"
        if not self.follow:
            self.u = self.ec.control(BOUNDS, pose, np.array(self.memory).T)
            source = "ergodic"
        self.u_checked = self.u.copy()      # the twist validate_control sees
        if not po.validate_control(COLL_S, self.grid, pose, self.u, VAL_DT, VAL_HORIZON):
            if self.follow:
                _, self.u, _ = po.dwa_control(self.dwa, COLL_S, self.grid, pose, vb, vref=self.u)
                self.follow = False
                source = "dwa-replan"
            else:
                ok, self.u, _ = po.dwa_control(self.dwa, COLL_S, self.grid, pose, vb, xt_ref=self.ec.opt_traj(), dt_ref=0.1)
                self.follow = ok
                if ok:
                    self.i = 0
                source = "dwa-reference"
        return self.u.copy(), source

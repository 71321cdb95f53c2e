#!/usr/bin/env python3
"""What planning with a polygon base costs (eea_footprint_dwa_control_batch / eea_footprint_validate_control_batch /
eea_tick_batch_footprint: csrc/footprint_plan_kernel.hip) beside the disc's calls of the same run (eea_dwa_control_batch /
eea_validate_control_batch / eea_tick_batch).

With device events around windows of calls on one stream (warm-up first, the legs alternating), on the 240 x 120 demo map
(0.05 m cells, the three blocks of tests/test_gpu_fleet_tick.py, the robot of host/config/explore_omni.yaml), the 0.9 m x 0.5 m
rectangular base and the omni window (3 x 8 x 5 samples x 20 steps):
  the dynamic window at P = 4096 and 65536, both modes, with and without d_sq, beside the disc's;
  validate_control (5 steps) at the same P, with and without d_sq, beside the disc's;
  the tick at B = 4096 (robots moved by eea_integrate_twist_batch after every tick, the field built once) beside eea_tick_batch.
The share of the pose-steps the field decides and of the robots on the memory path are counted on the host.  The ratios are
those of this run.
usage: tools/footprint_dwa_cost.py [--out FILE] [--windows 5] [--calls 20]"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ergodic_exploration_amd import capi  # noqa: E402
from tools.footprint_cost import BOUNDS, COLL, NX, NY, RECT, RES, demo_map, stats, window  # noqa: E402

DWA = (0.1, 2.0, 0.2, 2.5, 2.5, 1.0, 1.0, -1.0, 1.0, -1.0, 2.0, -2.0, 3, 8, 5)      # host/config/explore_omni.yaml
SIZES = (4096, 65536)
B_TICK = 4096
VAL_DT, VAL_HORIZON = 0.1, 0.5


def reach_cells(mx, my, steps):
    return np.ceil(steps * abs(DWA[0]) * np.sqrt(mx * mx + my * my) / RES) + 1.0


def pose_steps(x0, vb, sq, r_in, r_out):
    """(decided by the field, ambiguous, without a cell) over every step of every sample of the robots x0 / vb, the rollouts in
    numpy (counts only: numpy's sine and cosine, no early exit at a hit)"""
    acc = np.array(DWA[3:6]) * DWA[2]
    vmax, vmin = np.array([DWA[6], DWA[8], DWA[10]]), np.array([DWA[7], DWA[9], DWA[11]])
    lo, up = np.fmax(vb - acc, vmin), np.fmin(vb + acc, vmax)
    ns = DWA[12:15]
    ax = [lo[:, a, None] + (up[:, a, None] - lo[:, a, None]) * (np.arange(ns[a]) / max(ns[a] - 1, 1))[None, :] for a in range(3)]
    u0 = np.broadcast_to(ax[0][:, :, None, None], (len(x0),) + tuple(ns)).reshape(len(x0), -1)
    u1 = np.broadcast_to(ax[1][:, None, :, None], (len(x0),) + tuple(ns)).reshape(len(x0), -1)
    u2 = np.broadcast_to(ax[2][:, None, None, :], (len(x0),) + tuple(ns)).reshape(len(x0), -1)
    dt, steps = DWA[0], int(abs(DWA[1] / DWA[0]))
    w = np.where(np.abs(u2) < 1e-12, 1.0, u2 * dt)
    s, c = np.sin(w), np.cos(w)
    straight = np.abs(u2) < 1e-12
    d0 = np.where(straight, u0 * dt, (u0 * dt * s + u1 * dt * (c - 1.0)) / w)
    d1 = np.where(straight, u1 * dt, (u1 * dt * s + u0 * dt * (1.0 - c)) / w)
    x, y, th = (np.repeat(x0[:, k, None], u0.shape[1], 1) for k in range(3))
    a = r_in / RES - 0.7072 - 1e-6
    sq_hit = int(math.floor(a)) ** 2 if a >= 0 else -1
    sq_free = int(math.ceil(r_out / RES + 0.7072 + 1e-6)) ** 2
    decided = ambiguous = no_cell = 0
    for _ in range(steps):
        x, y, th = x + (np.cos(th) * d0 - np.sin(th) * d1), y + (np.sin(th) * d0 + np.cos(th) * d1), th + np.where(straight, 0.0, u2 * dt)
        fx, fy = np.floor((x - BOUNDS[0]) / RES), np.floor((y - BOUNDS[2]) / RES)
        has = (fx >= 0) & (fx <= NX - 1) & (fy >= 0) & (fy <= NY - 1)
        v = sq[fy[has].astype(int), fx[has].astype(int)]
        dec = int(((v < 0) | (v > sq_free) | (v <= sq_hit)).sum())
        decided += dec
        ambiguous += int(has.sum()) - dec
        no_cell += int((~has).sum())
    return decided, ambiguous, no_cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "footprint_dwa.txt"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("footprint_dwa_cost.py measures on the GPU: none found")
    warm = 3
    cfg, dcfg = capi.make_collision_cfg(BOUNDS[0], BOUNDS[2], RES, NX, NY, *COLL), capi.DwaCfg(*DWA)
    fp = capi.Footprint.of(RECT)
    r_in, r_out = capi.footprint_radii(fp)
    data = demo_map()
    grid = torch.as_tensor(data).cuda()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rng = np.random.default_rng(7)
    P_max, n_ref = max(SIZES), 50
    x0_np = np.stack([rng.uniform(-0.5, 10.5, P_max), rng.uniform(-0.5, 4.5, P_max), rng.uniform(-np.pi, np.pi, P_max)], 1)
    vb_np = np.stack([rng.uniform(-1, 1, P_max), rng.uniform(-1, 1, P_max), rng.uniform(-2, 2, P_max)], 1)
    vref_np = np.stack([rng.uniform(-1, 1, P_max), rng.uniform(-1, 1, P_max), rng.uniform(-2, 2, P_max)], 1)
    x0, vb, vref = (torch.as_tensor(a).cuda() for a in (x0_np, vb_np, vref_np))
    # reference trajectories: straight lines from the start pose along the reference twist, 50 columns every 0.1 s
    xt = (x0[:, None, :] + torch.arange(1, n_ref + 1, device="cuda", dtype=torch.float64)[None, :, None] * (0.1 * vref[:, None, :])).contiguous()
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    sq = i32(NY, NX)
    outs = {k: (f64(P_max, 3), i32(P_max)) for k in ("fv", "xv", "dv", "ft", "xt", "dt")}
    val = {k: i32(P_max) for k in ("f", "x", "d")}

    # the same window with velocity limits of 30 m/s: the limits' reach needs more LDS than there is, no window is reserved and
    # every robot takes its cells from memory through the cooperative resolve.  The odometry is kept 0.5 m/s (1 rad/s) inside
    # the real limits for this pair of legs, so that both clip no window and roll out the same samples
    wide = list(DWA)
    wide[6:10] = 30.0, -30.0, 30.0, -30.0
    dcfg_wide = capi.DwaCfg(*wide)
    vb_in = (vb * 0.5).contiguous()
    outs["fm"], outs["fw"] = (f64(P_max, 3), i32(P_max)), (f64(P_max, 3), i32(P_max))

    def dwa(key, P, disc=False, field=False, traj=False, d=None, odom=None):
        u, f = outs[key]
        d, odom = dcfg if d is None else d, vb if odom is None else odom
        kw = dict(xt_ref=xt[:P], dt_ref=0.1) if traj else dict(vref=vref[:P])
        if disc:
            return lambda: capi.dwa_control_batch(cfg, d, grid, x0[:P], odom[:P], u[:P], f[:P], stream=s, **kw)
        return lambda: capi.footprint_dwa_control_batch(cfg, d, fp, grid, x0[:P], odom[:P], u[:P], f[:P], sq=sq if field else None,
                                                        stream=s, **kw)

    legs = []
    for P in SIZES:
        for traj, mode in ((False, "twist"), (True, "traj")):
            k = "t" if traj else "v"
            legs += [("footprint window, %s, field, P = %d" % (mode, P), dwa("f" + k, P, field=True, traj=traj)),
                     ("footprint window, %s, no field, P = %d" % (mode, P), dwa("x" + k, P, traj=traj)),
                     ("disc window, %s, P = %d" % (mode, P), dwa("d" + k, P, disc=True, traj=traj))]
        legs += [("LDS window, slow odometry, twist, field, P = %d" % P, dwa("fw", P, field=True, odom=vb_in)),
                 ("memory path, slow odometry, twist, field, P = %d" % P, dwa("fm", P, field=True, d=dcfg_wide, odom=vb_in))]
        legs += [("footprint validate, field, P = %d" % P, lambda P=P: capi.footprint_validate_control_batch(
                     cfg, fp, grid, x0[:P], vref[:P], VAL_DT, VAL_HORIZON, val["f"][:P], sq=sq, stream=s)),
                 ("footprint validate, no field, P = %d" % P, lambda P=P: capi.footprint_validate_control_batch(
                     cfg, fp, grid, x0[:P], vref[:P], VAL_DT, VAL_HORIZON, val["x"][:P], stream=s)),
                 ("disc validate, P = %d" % P, lambda P=P: capi.validate_control_batch(cfg, grid, x0[:P], vref[:P], VAL_DT, VAL_HORIZON,
                                                                                     val["d"][:P], stream=s))]

    # the tick: two fleets from the same start, each moved by its own twists
    lim = np.array([1.0, 1.0, 2.0])
    eng = capi.Engine(capi.make_config(capi.MODEL_OMNI, 0.1, 5.0, 0.1, 1.0, 10, np.diag([1.0, 1.0, 2.0]), -lim, lim))
    eng.set_target_gaussians([[2.5, 2.5], [8.5, 2.5]], [[1.5, 1.5], [1.5, 1.5]])
    eng.config_domain(BOUNDS)
    T, B = eng.T, B_TICK
    start = torch.as_tensor(np.stack([rng.uniform(0.2, 9.5, B), rng.uniform(-0.2, 4.2, B), rng.uniform(-0.6, 0.6, B)], 1)).cuda()

    class Fleet:
        def __init__(self):
            self.pose, self.ut, self.u, self.traj, self.vb = start.clone(), f64(B, T, 3), f64(B, 3), f64(B, T, 3), f64(B, 3)
            self.follow, self.count, self.valid, self.skip, self.source = i32(B), i32(B), i32(B), i32(B), i32(B)

    fleets = {"footprint": Fleet(), "disc": Fleet()}

    def tick(kind):
        f = fleets[kind]

        def run():
            if kind == "footprint":
                eng.tick_batch_footprint(fp, B, f.pose, f.ut, f.follow, f.count, f.u, f.vb, grid, f.traj, f.valid, f.skip, cfg, dcfg,
                                         VAL_DT, VAL_HORIZON, sq=sq, source=f.source, stream=s)
            else:
                eng.tick_batch(B, f.pose, f.ut, f.follow, f.count, f.u, f.vb, grid, f.traj, f.valid, f.skip, cfg, dcfg, VAL_DT,
                               VAL_HORIZON, source=f.source, stream=s, grid_epoch=1)
            capi.integrate_twist_batch(f.pose, f.u, 0.1, stream=s)      # the robots move; odometry = the commanded twist
            f.vb.copy_(f.u)
        return run
    legs += [("footprint tick + move, B = %d" % B, tick("footprint")), ("disc tick + move, B = %d" % B, tick("disc"))]

    us = {name: [] for name, _ in legs}
    with torch.cuda.stream(stream):
        capi.distance_field(cfg, grid, sq, stream=s)            # the filter's field, built once
        for name, fn in legs:
            window(stream, fn, warm)
        stream.synchronize()
        for _ in range(args.windows):
            for name, fn in legs:
                us[name].append(window(stream, fn, args.calls))
        stream.synchronize()
    same = all(bool(torch.equal(outs["f" + k][i], outs["x" + k][i])) for k in "vt" for i in (0, 1)) and bool(torch.equal(val["f"], val["x"]))
    same_paths = all(bool(torch.equal(outs["fw"][i], outs["fm"][i])) for i in (0, 1))
    sq_np = sq.cpu().numpy()
    med = {name: float(np.median(v)) for name, v in us.items()}
    box = math.ceil(r_out / RES) + 1
    steps = int(abs(DWA[1] / DWA[0]))
    lim_reach = float(reach_cells(max(abs(DWA[6]), abs(DWA[7])), max(abs(DWA[8]), abs(DWA[9])), steps))
    side = int(2 * (lim_reach + box) + 1)
    lines = ["footprint planning: cost per call (tools/footprint_dwa_cost.py)",
             "%s; demo map %d x %d cells of %.2f m (%d occupied); base 0.9 m x 0.5 m (r_in %.3f m, r_out %.3f m, box %d cells); the disc: "
             "robot %s" % (torch.cuda.get_device_name(0), NX, NY, RES, int((data >= 80).sum()), r_in, r_out, box, COLL),
             "window 3 x 8 x 5 samples x %d steps of %.1f s; the limits' reach %d cells: an LDS window of %d x %d bits, %d B behind %d B "
             "of costs" % (steps, DWA[0], lim_reach, side, side, side * ((side + 63) // 64) * 8, 8 * 120),
             "device events, %d windows x %d calls per leg after %d warm-up calls, legs alternating; median [min .. max] us per call"
             % (args.windows, args.calls, warm),
             "with and without the field the answers are the same bits: %s; from the LDS window and from memory: %s" % (same, same_paths)]
    acc = np.array(DWA[3:6]) * DWA[2]
    for P in SIZES:
        lo = np.fmax(vb_np[:P] - acc, [DWA[7], DWA[9], DWA[11]])
        up = np.fmin(vb_np[:P] + acc, [DWA[6], DWA[8], DWA[10]])
        own = reach_cells(np.maximum(np.abs(lo[:, 0]), np.abs(up[:, 0])), np.maximum(np.abs(lo[:, 1]), np.abs(up[:, 1])), steps)
        n = min(P, 4096)
        dec, amb, nc = pose_steps(x0_np[:n], vb_np[:n], sq_np, r_in, r_out)
        tot = dec + amb + nc
        lines.append("the %d robots: %d find a twist (twist mode; the disc: %d), %d valid (the disc: %d); %.1f %% on the memory path; of "
                     "the pose-steps of the first %d robots (no early exit counted) the field decides %.1f %%, %.1f %% are ambiguous, "
                     "%.1f %% have no cell" % (P, int(outs["fv"][1][:P].sum().item()), int(outs["dv"][1][:P].sum().item()),
                                               int(val["f"][:P].sum().item()), int(val["d"][:P].sum().item()),
                                               100.0 * float((own > lim_reach).mean()), n, 100.0 * dec / tot, 100.0 * amb / tot,
                                               100.0 * nc / tot))
    for kind, f in fleets.items():
        src = np.bincount(f.source.cpu().numpy().clip(0, 3), minlength=4)
        lines.append("the %s fleet after its ticks: sources of the last tick ergodic %d, follow %d, window %d, replan %d" % ((kind,) + tuple(src)))
    lines.append("")
    for name, _ in legs:
        lines.append("  %-52s %s" % (name, stats(us[name])))
    lines += ["", "ratios of this run (medians):"]
    for P in SIZES:
        for mode in ("twist", "traj"):
            f_, x_, d_ = (med["%s, %s, %sP = %d" % (a, mode, b, P)] for a, b in (("footprint window", "field, "), ("footprint window", "no field, "), ("disc window", "")))
            lines.append("  window, %s, P = %d: field / no field %.2f; field / disc %.2f; no field / disc %.2f" % (mode, P, f_ / x_, f_ / d_, x_ / d_))
        f_, x_, d_ = med["footprint validate, field, P = %d" % P], med["footprint validate, no field, P = %d" % P], med["disc validate, P = %d" % P]
        lines.append("  validate, P = %d: field / no field %.2f; field / disc %.2f" % (P, f_ / x_, f_ / d_))
        lines.append("  P = %d, slow odometry: LDS window / memory path %.2f" % (P, med["LDS window, slow odometry, twist, field, P = %d" % P] /
                                                                            med["memory path, slow odometry, twist, field, P = %d" % P]))
    lines.append("  tick + move, B = %d: footprint / disc %.2f" % (B, med["footprint tick + move, B = %d" % B] / med["disc tick + move, B = %d" % B]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    eng.close()
    capi.release_collision_caches()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the footprint check costs (eea_footprint_check_batch / eea_footprint_traj_first: csrc/footprint_kernel.hip) with and
without the distance field as its filter, beside the disc's calls on the same poses (eea_collision_check_batch: the ring search;
eea_distance_query_batch / eea_distance_traj_min: one lookup in the field).

With device events around windows of calls on one stream (warm-up first, the legs alternating), on the 240 x 120 demo map
(0.05 m cells, the three blocks of tests/test_gpu_fleet_tick.py, the robot of host/config/explore_omni.yaml) and the 0.9 m x
0.5 m rectangular base:
  the check at P = 4096 and 65536 with and without d_sq, beside the query and the disc's collision check at the same poses;
  eea_footprint_traj_first at B = 4096, T = 200 with and without d_sq, beside eea_distance_traj_min.
The shares of the poses the field decides are counted on the host from the field itself.  The ratios are those of this run.
usage: tools/footprint_cost.py [--out FILE] [--windows 5] [--calls 20]"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ergodic_exploration_amd import capi  # noqa: E402

COLL = (0.7, 1.0, 0.2, 0.8)                                       # host/config/explore_omni.yaml
BOUNDS = (-1.0, 11.0, -1.0, 5.0)
RES, NX, NY = 0.05, 240, 120
OBSTACLES = [(2.4, 0.2, 3.0, 2.6), (6.0, 2.0, 6.5, 4.6), (8.8, -0.4, 9.4, 1.2)]
RECT = [(0.45, -0.25), (0.45, 0.25), (-0.45, 0.25), (-0.45, -0.25)]
SIZES = (4096, 65536)
B_TRAJ, T_TRAJ = 4096, 200


def demo_map():
    data = np.zeros((NY, NX), dtype=np.int8)
    cx, cy = BOUNDS[0] + (np.arange(NX) + 0.5) * RES, BOUNDS[2] + (np.arange(NY) + 0.5) * RES
    for (x0, y0, x1, y1) in OBSTACLES:
        data[np.ix_((cy >= y0) & (cy <= y1), (cx >= x0) & (cx <= x1))] = 100
    return data


def window(stream, fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(n):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def stats(v):
    return "%10.1f  [%.1f .. %.1f]" % (float(np.median(v)), min(v), max(v))


def shares(sq, poses, r_in, r_out):
    """(sure hits, surely free, ambiguous, without a cell) of poses [.][3] by the header's thresholds, from the field sq"""
    a = r_in / RES - 0.7072 - 1e-6
    sq_hit = int(math.floor(a)) ** 2 if a >= 0 else -1
    sq_free = int(math.ceil(r_out / RES + 0.7072 + 1e-6)) ** 2
    fx, fy = np.floor((poses[:, 0] - BOUNDS[0]) / RES), np.floor((poses[:, 1] - BOUNDS[2]) / RES)
    has = (fx >= 0) & (fx <= NX - 1) & (fy >= 0) & (fy <= NY - 1)
    s = sq[fy[has].astype(int), fx[has].astype(int)]
    hit, free = int(((s >= 0) & (s <= sq_hit)).sum()), int(((s < 0) | (s > sq_free)).sum())
    return hit, free, int(has.sum()) - hit - free, int((~has).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "footprint.txt"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("footprint_cost.py measures on the GPU: none found")
    warm = 3
    cfg = capi.make_collision_cfg(BOUNDS[0], BOUNDS[2], RES, NX, NY, *COLL)
    fp = capi.Footprint.of(RECT)
    r_in, r_out = capi.footprint_radii(fp)
    data = demo_map()
    grid = torch.as_tensor(data).cuda()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rng = np.random.default_rng(7)
    P_max = max(SIZES)
    poses_np = np.stack([rng.uniform(-0.5, 10.5, P_max), rng.uniform(-0.5, 4.5, P_max), rng.uniform(-np.pi, np.pi, P_max)], 1)
    poses = torch.as_tensor(poses_np).cuda()
    walk = np.cumsum(rng.normal(0.0, 0.05, (B_TRAJ, T_TRAJ, 3)), axis=1)
    traj_np = np.stack([rng.uniform(0.0, 10.0, B_TRAJ), rng.uniform(0.0, 4.0, B_TRAJ), rng.uniform(-np.pi, np.pi, B_TRAJ)], 1)[:, None, :] + walk
    traj = torch.as_tensor(np.ascontiguousarray(traj_np)).cuda()
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    sq, near = i32(NY, NX), i32(NY, NX)
    hit_f, hit_x, hit_disc = i32(P_max), i32(P_max), i32(P_max)
    out, dmin = i32(P_max, 4), f64(P_max)
    step_f, step_x = i32(B_TRAJ), i32(B_TRAJ)
    t_out, t_step, t_dmin = i32(B_TRAJ, 4), i32(B_TRAJ), f64(B_TRAJ)

    legs = []
    for P in SIZES:
        legs += [("footprint check, field, P = %d" % P, lambda P=P: capi.footprint_check_batch(cfg, fp, grid, poses[:P], hit_f[:P], sq, stream=s)),
                 ("footprint check, no field, P = %d" % P, lambda P=P: capi.footprint_check_batch(cfg, fp, grid, poses[:P], hit_x[:P], stream=s)),
                 ("distance query, P = %d" % P, lambda P=P: capi.distance_query_batch(cfg, sq, near, poses[:P], out[:P], dmin[:P], stream=s)),
                 ("disc collision check, P = %d" % P, lambda P=P: capi.collision_check_batch(cfg, grid, poses[:P], hit_disc[:P], stream=s))]
    shape = "B = %d, T = %d" % (B_TRAJ, T_TRAJ)
    legs += [("footprint traj_first, field, " + shape, lambda: capi.footprint_traj_first(cfg, fp, grid, traj, step_f, sq, stream=s)),
             ("footprint traj_first, no field, " + shape, lambda: capi.footprint_traj_first(cfg, fp, grid, traj, step_x, stream=s)),
             ("distance traj_min, " + shape, lambda: capi.distance_traj_min(cfg, sq, near, traj, t_out, t_step, t_dmin, stream=s))]
    us = {name: [] for name, _ in legs}
    with torch.cuda.stream(stream):
        capi.distance_field(cfg, grid, sq, near, stream=s)            # the filter's field
        for name, fn in legs:
            window(stream, fn, warm)
        stream.synchronize()
        for _ in range(args.windows):
            for name, fn in legs:
                us[name].append(window(stream, fn, args.calls))
        stream.synchronize()
    same = bool(torch.equal(hit_f, hit_x)) and bool(torch.equal(step_f, step_x))
    sq_np = sq.cpu().numpy()
    med = {name: float(np.median(v)) for name, v in us.items()}
    lines = ["footprint collision: cost per call (tools/footprint_cost.py)",
             "%s; demo map %d x %d cells of %.2f m (%d occupied); base 0.9 m x 0.5 m (r_in %.3f m, r_out %.3f m: boxes of up to %d x %d "
             "cells); the disc: robot %s" % (torch.cuda.get_device_name(0), NX, NY, RES, int((data >= 80).sum()), r_in, r_out,
                                             2 * (math.ceil(r_out / RES) + 1) + 1, 2 * (math.ceil(r_out / RES) + 1) + 1, COLL),
             "device events, %d windows x %d calls per leg after %d warm-up calls, legs alternating; median [min .. max] us per call"
             % (args.windows, args.calls, warm),
             "legs of 7 - 8 us (the distance query, traj_min) are at the cadence of back-to-back launches from this process, the "
             "same at every P: they bound those kernels' times from above, and the footprint legs' ratios to them are lower bounds",
             "with and without the field the answers are the same: %s" % same]
    for P in SIZES:
        h, f, a, n = shares(sq_np, poses_np[:P], r_in, r_out)
        lines.append("the %d poses: %d collide (the disc: %d); by the field %d sure hits, %d surely free, %d ambiguous (%.1f %%), %d without "
                     "a cell" % (P, int(hit_f[:P].sum().item()), int(hit_disc[:P].sum().item()), h, f, a, 100.0 * a / P, n))
    h, f, a, n = shares(sq_np, traj_np.reshape(-1, 3), r_in, r_out)
    steps = B_TRAJ * T_TRAJ
    lines += ["the %d trajectories: %d collide somewhere, %d at step 0; of their %d steps %.1f %% sure hits, %.1f %% surely free, %.1f %% "
              "ambiguous, %.1f %% without a cell" % (B_TRAJ, int((step_f >= 0).sum().item()), int((step_f == 0).sum().item()), steps,
                                                     100.0 * h / steps, 100.0 * f / steps, 100.0 * a / steps, 100.0 * n / steps), ""]
    for name, _ in legs:
        lines.append("  %-52s %s" % (name, stats(us[name])))
    lines += ["", "ratios of this run (medians):"]
    for P in SIZES:
        lines.append("  P = %d: field / no field %.2f; field / distance query %.2f; field / disc collision check %.2f"
                     % (P, med["footprint check, field, P = %d" % P] / med["footprint check, no field, P = %d" % P],
                        med["footprint check, field, P = %d" % P] / med["distance query, P = %d" % P],
                        med["footprint check, field, P = %d" % P] / med["disc collision check, P = %d" % P]))
    lines.append("  traj_first: field / no field %.2f; field / distance traj_min %.2f"
                 % (med["footprint traj_first, field, " + shape] / med["footprint traj_first, no field, " + shape],
                    med["footprint traj_first, field, " + shape] / med["distance traj_min, " + shape]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    capi.release_collision_caches()


if __name__ == "__main__":
    main()

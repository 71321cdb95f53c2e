#!/usr/bin/env python3
"""What the distance field costs (eea_distance_field / eea_distance_query_batch / eea_distance_traj_min:
csrc/distance_kernel.hip) beside the clearance calls of the reference's ring search (eea_clearance_field /
eea_clearance_batch: csrc/clearance_kernel.hip).

With device events around windows of calls on one stream (warm-up first, the legs alternating):
  the build (both planes) on the 240 x 120 demo map (0.05 m cells, the three blocks of tests/test_gpu_fleet_tick.py, the robot
  of host/config/explore_omni.yaml), beside eea_clearance_field (both outputs) on the same map and parameters;
  the build on the 1024 x 1024 grid of BASELINE config 5 (seed 2024: 10 % occupied in 32-cell blocks), and on two adversarial
  grids of that size: one occupied cell in a corner (every lane of the row pass walks to it: the cubic case) and no occupied
  cell (answered after the column pass);
  the query (all three outputs) at P = 64 ... 32768 on the demo map, beside eea_clearance_batch at the same poses;
  eea_distance_traj_min (all three outputs) at B = 4096, T = 200.
The ratios are those of this run.  usage: tools/distance_cost.py [--out FILE] [--windows 5] [--calls 20]"""
import argparse
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
SIZES = (64, 512, 4096, 32768)
BIG = 1024
B_TRAJ, T_TRAJ = 4096, 200


def demo_map():
    data = np.zeros((NY, NX), dtype=np.int8)
    cx, cy = BOUNDS[0] + (np.arange(NX) + 0.5) * RES, BOUNDS[2] + (np.arange(NY) + 0.5) * RES
    for (x0, y0, x1, y1) in OBSTACLES:
        data[np.ix_((cy >= y0) & (cy <= y1), (cx >= x0) & (cx <= x1))] = 100
    return data


def occupancy(nx, ny, seed=2024, block=32):
    """BASELINE config 5's grid (the construction of tests/test_gpu_phik_parity.py)"""
    rng = np.random.default_rng(seed)
    blocks = rng.choice(np.array([0, 100, -1], dtype=np.int8), size=(ny // block + 1, nx // block + 1), p=[0.7, 0.1, 0.2])
    return np.ascontiguousarray(np.kron(blocks, np.ones((block, block), dtype=np.int8))[:ny, :nx])


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_field.txt"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("distance_cost.py measures on the GPU: none found")
    warm = 3
    cfg = capi.make_collision_cfg(BOUNDS[0], BOUNDS[2], RES, NX, NY, *COLL)
    big_cfg = capi.make_collision_cfg(0.0, 0.0, 0.1, BIG, BIG, *COLL)
    data = demo_map()
    grid = torch.as_tensor(data).cuda()
    config5 = occupancy(BIG, BIG)
    corner = np.zeros((BIG, BIG), dtype=np.int8)
    corner[0, 0] = 100
    bigs = {"config 5": torch.as_tensor(config5).cuda(), "one cell in a corner": torch.as_tensor(corner).cuda(),
            "no occupied cell": torch.zeros((BIG, BIG), dtype=torch.int8, device="cuda")}
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rng = np.random.default_rng(7)
    P_max = max(SIZES)
    poses = torch.as_tensor(np.stack([rng.uniform(-0.5, 10.5, P_max), rng.uniform(-0.5, 4.5, P_max), np.zeros(P_max)], 1)).cuda()
    walk = np.cumsum(rng.normal(0.0, 0.05, (B_TRAJ, T_TRAJ, 2)), axis=1)
    traj_np = np.zeros((B_TRAJ, T_TRAJ, 3))
    traj_np[:, :, :2] = np.stack([rng.uniform(0.0, 10.0, B_TRAJ), rng.uniform(0.0, 4.0, B_TRAJ)], 1)[:, None, :] + walk
    traj = torch.as_tensor(traj_np).cuda()
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    sq, near = i32(NY, NX), i32(NY, NX)
    big_sq, big_near = i32(BIG, BIG), i32(BIG, BIG)
    out, dmin, disp = i32(P_max, 4), f64(P_max), f64(P_max, 2)
    ring_out, ring_dmin, ring_disp = i32(P_max, 4), f64(P_max), f64(P_max, 2)
    field, fmin = i32(NY, NX, 4), f64(NY, NX)
    t_out, t_step, t_dmin = i32(B_TRAJ, 4), i32(B_TRAJ), f64(B_TRAJ)

    legs = [("build 240 x 120 demo map", lambda: capi.distance_field(cfg, grid, sq, near, stream=s)),
            ("clearance_field 240 x 120", lambda: capi.clearance_field(cfg, grid, field, fmin, stream=s))]
    for name, g in bigs.items():
        legs.append(("build 1024 x 1024, %s" % name, lambda g=g: capi.distance_field(big_cfg, g, big_sq, big_near, stream=s)))
    for P in SIZES:
        legs += [("query P = %d" % P, lambda P=P: capi.distance_query_batch(cfg, sq, near, poses[:P], out[:P], dmin[:P], disp[:P], stream=s)),
                 ("clearance_batch P = %d" % P,
                  lambda P=P: capi.clearance_batch(cfg, grid, poses[:P], ring_out[:P], ring_dmin[:P], ring_disp[:P], stream=s))]
    legs.append(("traj_min B = %d, T = %d" % (B_TRAJ, T_TRAJ),
                 lambda: capi.distance_traj_min(cfg, sq, near, traj, t_out, t_step, t_dmin, stream=s)))
    us = {name: [] for name, _ in legs}
    with torch.cuda.stream(stream):
        capi.distance_field(cfg, grid, sq, near, stream=s)            # the queries' field
        for name, fn in legs:
            window(stream, fn, warm)
        stream.synchronize()
        for _ in range(args.windows):
            for name, fn in legs:
                us[name].append(window(stream, fn, args.calls))
        stream.synchronize()
        # what the calls answered
        capi.distance_field(cfg, grid, sq, near, stream=s)
        capi.distance_query_batch(cfg, sq, near, poses, out, dmin, disp, stream=s)
        capi.clearance_batch(cfg, grid, poses, ring_out, ring_dmin, ring_disp, stream=s)
        capi.distance_traj_min(cfg, sq, near, traj, t_out, t_step, t_dmin, stream=s)
        capi.distance_field(big_cfg, bigs["one cell in a corner"], big_sq, big_near, stream=s)
        stream.synchronize()
    classes = [int((out[:, 0] == m).sum().item()) for m in range(4)]
    ring_classes = [int((ring_out[:, 0] == m).sum().item()) for m in range(3)]
    t_classes = [int((t_out[:, 0] == m).sum().item()) for m in range(4)]
    ii, jj = torch.meshgrid(torch.arange(BIG, device="cuda"), torch.arange(BIG, device="cuda"), indexing="ij")
    corner_ok = bool(torch.equal(big_sq.long(), ii * ii + jj * jj)) and bool((big_near == 0).all())
    med = {name: float(np.median(v)) for name, v in us.items()}
    lines = ["distance field: cost per call (tools/distance_cost.py)",
             "%s; demo map %d x %d cells of %.2f m (%d occupied), robot %s; 1024 x 1024 grids of 0.1 m: BASELINE config 5 (seed 2024, "
             "%d occupied), one cell in a corner, none" % (torch.cuda.get_device_name(0), NX, NY, RES, int((data >= 80).sum()), COLL,
                                                            int((config5 >= 80).sum())),
             "device events, %d windows x %d calls per leg after %d warm-up calls, legs alternating; median [min .. max] us per call"
             % (args.windows, args.calls, warm),
             "the %d poses through the field: %d crash, %d obstacle, %d none, %d off the grid; by the ring search: %d crash, %d obstacle, "
             "%d none" % ((P_max,) + tuple(classes) + tuple(ring_classes)),
             "the %d trajectories' worst steps: %d crash, %d obstacle, %d none, %d off the grid; the corner grid's field is the closed "
             "form: %s" % ((B_TRAJ,) + tuple(t_classes) + (corner_ok,)), ""]
    for name, _ in legs:
        lines.append("  %-44s %s" % (name, stats(us[name])))
    cells = BIG * BIG
    lines += ["", "ratios of this run (medians):",
              "  build / clearance_field on the demo map: %.2f" % (med["build 240 x 120 demo map"] / med["clearance_field 240 x 120"])]
    for P in SIZES:
        lines.append("  query / clearance_batch at P = %d: %.2f" % (P, med["query P = %d" % P] / med["clearance_batch P = %d" % P]))
    for name in bigs:
        t = med["build 1024 x 1024, %s" % name]
        lines.append("  build 1024 x 1024, %s: %.3g ns per cell" % (name, t * 1e3 / cells))
    t = med["traj_min B = %d, T = %d" % (B_TRAJ, T_TRAJ)]
    lines.append("  traj_min: %.3g ns per step (%d steps, 24 bytes of pose each: %.0f GB/s)"
                 % (t * 1e3 / (B_TRAJ * T_TRAJ), B_TRAJ * T_TRAJ, B_TRAJ * T_TRAJ * 24 / (t * 1e-6) / 1e9))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    capi.release_collision_caches()


if __name__ == "__main__":
    main()

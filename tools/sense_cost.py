#!/usr/bin/env python3
"""What the fleet's range sensor costs (eea_sense_reveal_batch, eea_grid_census: csrc/sense_kernel.hip), and what it is
compared with.

4096 robots on the 1024 x 1024 occupancy grid of BASELINE config 5 (seed 2024: 70 % free, 10 % occupied, 20 % unknown in
32-cell blocks, 0.1 m cells), used as the ground truth, at R = 10, 50 and 127 cells (127: the largest range whose window is
marched in LDS; pass --ranges for others, above 127 the rays march in global memory).  Per range, with device events around
windows of calls on one stream (warm-up first, the legs alternating):
  the reveal (with and without the ranges output), the census of the known grid;
against
  (a) eea_tick_batch of the same fleet on the same grid, timed in the same run (K = 10, T = 50, the inflated collision map
      cached: the loop's other per-tick cost);
  (b) the host route the reveal replaces: poses read back, a numpy ray cast of the whole fleet (vectorised over robots and
      rays, one numpy pass per step -- a C++ host would cast faster), the known grid uploaded; host clock, once.
The device's known grid and ranges must equal the numpy cast's, bit for bit, or the run fails.
usage: tools/sense_cost.py [--out FILE] [--ranges 10,50,127]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ergodic_exploration_amd import capi  # noqa: E402
from tests import sense_restatement as sr  # noqa: E402

COLL = (0.7, 1.0, 0.2, 0.8)
DWA_OMNI = (0.1, 2.0, 0.2, 2.5, 2.5, 1.0, 1.0, -1.0, 1.0, -1.0, 2.0, -2.0, 3, 8, 5)   # host/config/explore_omni.yaml


def occupancy(nx, ny, seed=2024, block=32):
    """BASELINE config 5's grid (the construction of tests/test_gpu_phik_parity.py)"""
    rng = np.random.default_rng(seed)
    blocks = rng.choice(np.array([0, 100, -1], dtype=np.int8), size=(ny // block + 1, nx // block + 1), p=[0.7, 0.1, 0.2])
    return np.ascontiguousarray(np.kron(blocks, np.ones((block, block), dtype=np.int8))[:ny, :nx])


def host_cast(g, R, truth, known, poses):
    """tests/sense_restatement.py's reveal for a whole fleet at once: one numpy pass per step over [P][8R] rays"""
    P = poses.shape[0]
    cell = np.array([sr.world2grid(g, x, y) for x, y, _ in poses], dtype=np.int64)     # (i0, j0)
    on_grid = (cell[:, 0] <= g.ysize - 1) & (cell[:, 1] <= g.xsize - 1)
    i0, j0 = cell[:, 0][:, None], cell[:, 1][:, None]
    t = np.array([sr.ray_target(q, R) for q in range(8 * R)], dtype=np.int64)
    ax, ay, sx, sy = np.abs(t[:, 0])[None, :], np.abs(t[:, 1])[None, :], np.sign(t[:, 0])[None, :], np.sign(t[:, 1])[None, :]
    ranges = np.full((P, 8 * R), -1, dtype=np.int32)
    alive = np.repeat(on_grid[:, None], 8 * R, axis=1)
    own = cell[on_grid]
    known[own[:, 0], own[:, 1]] = truth[own[:, 0], own[:, 1]]
    blocking = ~(truth.astype(np.float64) / 100.0 < g.occupied_threshold)
    for s in range(1, R + 1):
        dx, dy = sx * ((2 * s * ax + R) // (2 * R)), sy * ((2 * s * ay + R) // (2 * R))
        i, j = i0 + dy, j0 + dx
        alive &= (dx * dx + dy * dy <= R * R) & (i >= 0) & (i < g.ysize) & (j >= 0) & (j < g.xsize)
        ii, jj = i[alive], j[alive]
        known[ii, jj] = truth[ii, jj]
        hit = np.zeros_like(alive)
        hit[alive] = blocking[ii, jj]
        ranges[hit] = s
        alive &= ~hit
    return ranges


def window(stream, fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(n):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sense.txt"))
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--ranges", default="10,50,127")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sense_cost.py measures on the GPU: none found")
    B, warm = args.robots, 3
    nx = ny = 1024
    res = 0.1
    g = sr.Geometry(0.0, 0.0, res, nx, ny, COLL[3])
    truth = occupancy(nx, ny)
    ccfg = capi.make_collision_cfg(0.0, 0.0, res, nx, ny, *COLL)
    dcfg = capi.DwaCfg(*DWA_OMNI)
    lim = np.array([1.0, 1.0, 2.0])
    eng = capi.Engine(capi.make_config(capi.MODEL_OMNI, 0.1, 5.0, res, 1.0, 10, np.diag([1.0, 1.0, 2.0]), -lim, lim))
    lx, ly = (nx - 1) * res, (ny - 1) * res
    T = eng.T
    rng = np.random.default_rng(7)
    poses = np.stack([rng.uniform(0.0, nx * res, B), rng.uniform(0.0, ny * res, B), rng.uniform(-3.0, 3.0, B)], 1)
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device="cuda")
    d_pose, d_vb, d_truth = torch.as_tensor(poses).cuda(), z(B, 3), torch.as_tensor(truth).cuda()
    d_known = torch.full((ny, nx), -1, dtype=torch.int8, device="cuda")
    d_counts = z(3, dt=torch.int64)
    d_ut, d_follow, d_count, d_u, d_traj = z(B, T, 3), z(B, dt=torch.int32), z(B, dt=torch.int32), z(B, 3), z(B, T, 3)
    d_valid, d_skip = z(B, dt=torch.int32), z(B, dt=torch.int32)
    eng.set_target_occupancy(nx, ny, d_truth, lx, ly)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def tick():
        eng.tick_batch(B, d_pose, d_ut, d_follow, d_count, d_u, d_vb, d_truth, d_traj, d_valid, d_skip, ccfg, dcfg, 0.1, 0.5,
                       stream=s, grid_epoch=1)

    def fresh_tick():
        for x in (d_ut, d_follow, d_count, d_u):
            x.zero_()
        tick()

    lines = ["range sensing of a fleet: cost per call of eea_sense_reveal_batch / eea_grid_census (tools/sense_cost.py)",
             "%s, %d robots, %d x %d ground-truth grid (BASELINE config 5, seed 2024)" % (torch.cuda.get_device_name(0), B, nx, ny),
             "device events, %d windows x %d calls per leg after %d warm-up calls, legs alternating; median [min .. max] us per call"
             % (args.windows, args.calls, warm),
             "(a) = eea_tick_batch of the same fleet on the same grid (K = 10, T = %d, collision map cached), same run" % T,
             "(b) = the host route: poses read back + numpy ray cast of the fleet + upload of the known grid, host clock, once", ""]
    ok = True
    for R in [int(v) for v in args.ranges.split(",")]:
        d_ranges = torch.full((B, 8 * R), -7, dtype=torch.int32, device="cuda")
        legs = [("reveal + ranges", lambda: capi.sense_reveal_batch(ccfg, R, d_truth, d_known, d_pose, d_ranges, stream=s)),
                ("reveal", lambda: capi.sense_reveal_batch(ccfg, R, d_truth, d_known, d_pose, stream=s)),
                ("census", lambda: capi.grid_census(ccfg, d_known, d_counts, stream=s)),
                ("(a) tick", tick)]
        us = {name: [] for name, _ in legs}
        with torch.cuda.stream(stream):
            d_known.fill_(-1)
            fresh_tick()
            for _, fn in legs:
                window(stream, fn, warm)
            for _ in range(args.windows):
                for name, fn in legs:
                    us[name].append(window(stream, fn, args.calls))
            stream.synchronize()
            # (b), and the check of the device's result at this size
            t0 = time.perf_counter()
            h_pose = d_pose.cpu().numpy()
            t1 = time.perf_counter()
            h_known = np.full((ny, nx), -1, dtype=np.int8)
            h_ranges = host_cast(g, R, truth, h_known, h_pose)
            t2 = time.perf_counter()
            d_up = torch.as_tensor(h_known).cuda()
            stream.synchronize()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            same = bool((d_up == d_known).all().item()) and np.array_equal(d_ranges.cpu().numpy(), h_ranges)
            counts = d_counts.cpu().numpy()
        ok = ok and same and tuple(int(c) for c in counts) == sr.census(g, h_known)
        visits = 8 * R * R * B
        lines.append("R = %d (%d rays per robot, %.1f M cell visits at most, %s): known cells after the call %d of %d; device == numpy cast: %s"
                     % (R, 8 * R, visits / 1e6, "LDS window of %d B" % ((2 * R + 1) ** 2) if R <= 127 else "global memory",
                        int(counts[1] + counts[2]), nx * ny, "yes" if same else "NO"))
        for name, _ in legs:
            med = float(np.median(us[name]))
            lines.append("  %-18s %9.1f  [%.1f .. %.1f]" % (name, med, min(us[name]), max(us[name])))
        lines.append("  %-18s %9.1f  = read-back %.1f + numpy cast %.1f + upload %.1f"
                     % ("(b) host route", (t3 - t0) * 1e6, (t1 - t0) * 1e6, (t2 - t1) * 1e6, (t3 - t2) * 1e6))
        lines.append("  reveal + census = %.2f x the tick" % ((np.median(us["reveal"]) + np.median(us["census"])) / np.median(us["(a) tick"])))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    eng.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

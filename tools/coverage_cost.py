#!/usr/bin/env python3
"""What the coverage of a fleet's history costs (eea_replay_history_records + eea_ck_records_sum + eea_records_metric,
csrc/coverage_kernel.hip), and what it is compared with.

fp64, K = 10, 4096 robots, three fills of the stores: every count 1200, every count 4096, counts ragged uniformly in
[0, 4096].  Per fill, with device events around windows of calls on one stream (warm-up first, the legs alternating):
  history_records alone, records_sum alone, records_metric (per robot + fleet) alone, and ReplayMemory.coverage() as a whole;
against
  (a) the time the STORED POSES' bytes alone need at the HBM rate the phi_k kernel reaches (5.8 TB/s, profiles/HISTORY.md:
      `roofline_phik`) -- sum n_b x 24 bytes: what a kernel that only had to stream the store could not beat;
  (b) the only route without these entries: eea_replay_read (a device-wide wait and a copy) + eea_basis_traj_coeff (host
      pointers) per robot, host clock over 64 robots, scaled to the fleet.
usage: tools/coverage_cost.py [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ergodic_exploration_amd import capi  # noqa: E402

PHIK_HBM_RATE = 5.8e12   # bytes / s: the phi_k streaming kernel on this chip (profiles/HISTORY.md, roofline_phik)
BOUNDS = (-1.0, 11.0, -1.0, 5.0)


def fill(mem, counts, stream):
    """appends uniform poses until robot b holds counts[b] of them (masks built on the device)"""
    d_counts = torch.as_tensor(counts.astype(np.int32)).cuda()
    gen = torch.Generator(device="cuda").manual_seed(7)
    lo = torch.tensor([BOUNDS[0] - 1.0, BOUNDS[2] - 1.0, -3.0], dtype=torch.float64, device="cuda")
    span = torch.tensor([BOUNDS[1] - BOUNDS[0] + 2.0, BOUNDS[3] - BOUNDS[2] + 2.0, 6.0], dtype=torch.float64, device="cuda")
    for t in range(int(counts.max())):
        pose = lo + span * torch.rand((mem.B, 3), dtype=torch.float64, device="cuda", generator=gen)
        mask = (d_counts > t).to(torch.int32)
        mem.append(pose, mask, stream=stream)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coverage.txt"))
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("coverage_cost.py measures on the GPU: none found")
    B, K, cap, warm = args.robots, 10, 4096, 5
    lim = np.array([1.0, 1.0, 2.0])
    eng = capi.Engine(capi.make_config(capi.MODEL_OMNI, 0.1, 5.0, 0.1, 1.0, K, np.diag([1.0, 1.0, 2.0]), -lim, lim))
    eng.set_target_gaussians([[2.5, 2.5], [8.5, 2.5]], [[1.5, 1.5], [1.5, 1.5]])
    eng.config_domain(BOUNDS)
    L = eng.ck_record_len
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rng = np.random.default_rng(11)
    fills = [("every count 1200", np.full(B, 1200)), ("every count 4096", np.full(B, cap)),
             ("counts uniform in [0, 4096]", rng.integers(0, cap + 1, B))]
    lines = ["coverage of a fleet's history: cost per call (tools/coverage_cost.py)",
             "%s, fp64, K = %d, %d robots, store capacity %d poses per robot" % (torch.cuda.get_device_name(0), K, B, cap),
             "device events, %d windows x %d calls per leg after %d warm-up calls, legs alternating; median [min .. max] us per call"
             % (args.windows, args.calls, warm),
             "(a) = the stored poses' bytes (sum n_b x 24) at %.1f TB/s, the phi_k kernel's HBM rate; (b) = eea_replay_read +"
             % (PHIK_HBM_RATE / 1e12),
             "eea_basis_traj_coeff per robot, host clock over 64 robots, scaled to the fleet", ""]
    for title, counts in fills:
        mem = capi.ReplayMemory(B, cap, 100, seed=1)
        fill(mem, counts, None)
        got, dropped = mem.counts()
        assert dropped == 0 and np.array_equal(got, counts.astype(np.uint32))
        rec = torch.empty((B, L), dtype=torch.float64, device="cuda")
        fleet, eps, eps_fleet = (torch.empty(n, dtype=torch.float64, device="cuda") for n in (L, B, 1))

        def history():
            mem.history_records(eng, rec, stream=s)

        def rsum():
            eng.ck_records_sum(B, rec, fleet, stream=s)

        def metric():
            capi.records_metric(eng, rec, eps, stream=s)
            capi.records_metric(eng, fleet, eps_fleet, stream=s)

        def whole():
            mem.coverage(eng, stream=s)

        def window(fn, n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(n):
                fn()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b) * 1e3 / n

        legs = [("history_records", history), ("records_sum", rsum), ("records_metric (robots + fleet)", metric), ("coverage() as a whole", whole)]
        us = {name: [] for name, _ in legs}
        with torch.cuda.stream(stream):
            for _, fn in legs:
                window(fn, warm)
            for _ in range(args.windows):
                for name, fn in legs:
                    us[name].append(window(fn, args.calls))
        stream.synchronize()
        # (b): the route of a caller without the entries, per robot: a device-wide wait + copy, then host pointers in
        lx, ly = BOUNDS[1] - BOUNDS[0], BOUNDS[3] - BOUNDS[2]
        robots = [b for b in range(B) if counts[b] > 0][:64]
        t0 = time.perf_counter()
        for b in robots:
            p = mem.read(b, 0, int(counts[b]))
            xy = np.ascontiguousarray((p[:, :2] - np.array([BOUNDS[0], BOUNDS[2]])).T)
            capi.basis_traj_coeff(lx, ly, K, xy)
        per_robot = (time.perf_counter() - t0) / len(robots) * 1e6
        poses = int(counts.sum())
        floor = poses * 24 / PHIK_HBM_RATE * 1e6
        med = {k: float(np.median(v)) for k, v in us.items()}
        lines.append("%s: %d poses = %.1f MB" % (title, poses, poses * 24 / 1e6))
        for name, _ in legs:
            lines.append("  %-34s %9.1f  [%.1f .. %.1f]" % (name, med[name], min(us[name]), max(us[name])))
        h = med["history_records"]
        lines += ["  (a) the poses' bytes at the phi_k rate  %9.1f us; history_records is %.2f x that (%.2f TB/s of poses, %.1f G poses/s)"
                  % (floor, h / floor, poses * 24 / (h * 1e-6) / 1e12, poses / (h * 1e-6) / 1e9),
                  "  (b) read + traj_coeff per robot        %9.1f us (mean of %d robots) = %.0f ms for the fleet: %.0f x coverage()"
                  % (per_robot, len(robots), per_robot * B / 1e3, per_robot * B / med["coverage() as a whole"]), ""]
        mem.close()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    eng.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the clearance queries cost (eea_clearance_batch / eea_clearance_field: csrc/clearance_kernel.hip) beside the plain
collision check (eea_collision_check_batch).

The demo map (240 x 120 cells of 0.05 m, the three blocks of tests/test_gpu_fleet_tick.py) with the robot of
host/config/explore_omni.yaml: the search visits 744 cells per pose (12 passes of a wavefront), the key map covers
280 x 160 centres.  With device events around windows of calls on one stream (warm-up first, the legs alternating):
  eea_clearance_batch in the ring form (one wavefront per pose) and in the map form (fill + scatter + one load per pose) at
  P = 64, 512, 4096, 32768, all three outputs written;
  the map form at P = 1: the build of the key map alone, but for a one-block query -- and the same on an empty grid, where
  the scatter finds no cell: the fill of the buffer and the three launches, i.e. what every build pays before its keys;
  eea_clearance_field (both outputs) in either form;
  eea_collision_check_batch at the same P in its two forms, so that what the extra information costs can be seen.
The last lines restate the figures as the constants of the dispatch's cost model (use_key_map in csrc/clearance_kernel.hip).
usage: tools/clearance_cost.py [--out FILE] [--windows 5] [--calls 20]"""
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
N_OFF, REACH = 744, 20


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
    return "%9.1f  [%.1f .. %.1f]" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clearance.txt"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("clearance_cost.py measures on the GPU: none found")
    warm = 3
    cfg = capi.make_collision_cfg(BOUNDS[0], BOUNDS[2], RES, NX, NY, *COLL)
    data = demo_map()
    grid = torch.as_tensor(data).cuda()
    empty = torch.zeros_like(grid)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rng = np.random.default_rng(7)
    P_max = max(SIZES)
    poses = torch.as_tensor(np.stack([rng.uniform(-0.5, 10.5, P_max), rng.uniform(-0.5, 4.5, P_max), np.zeros(P_max)], 1)).cuda()
    out = torch.zeros((P_max, 4), dtype=torch.int32, device="cuda")
    dmin, disp = torch.zeros(P_max, dtype=torch.float64, device="cuda"), torch.zeros((P_max, 2), dtype=torch.float64, device="cuda")
    hit = torch.zeros(P_max, dtype=torch.int32, device="cuda")
    field = torch.zeros((NY, NX, 4), dtype=torch.int32, device="cuda")
    fmin = torch.zeros((NY, NX), dtype=torch.float64, device="cuda")

    def forced(impl, fn):
        def call():
            capi.set_option(capi.OPT_COLLISION_IMPL, impl)
            fn()
        return call

    legs = []
    for P in (1,) + SIZES:
        clear = lambda P=P: capi.clearance_batch(cfg, grid, poses[:P], out[:P], dmin[:P], disp[:P], stream=s)
        check = lambda P=P: capi.collision_check_batch(cfg, grid, poses[:P], hit[:P], stream=s)
        if P == 1:
            bare = lambda: capi.clearance_batch(cfg, empty, poses[:1], out[:1], dmin[:1], disp[:1], stream=s)
            legs += [("clearance map  P = 1 (build)", forced(2, clear)), ("  ... on an empty grid (fill)", forced(2, bare))]
            continue
        legs += [("clearance ring P = %d" % P, forced(1, clear)), ("clearance map  P = %d" % P, forced(2, clear)),
                 ("collision ring P = %d" % P, forced(1, check)), ("collision map  P = %d" % P, forced(2, check))]
    fld = lambda: capi.clearance_field(cfg, grid, field, fmin, stream=s)
    legs += [("field map  (%d cells)" % (NX * NY), forced(2, fld)), ("field ring (%d cells)" % (NX * NY), forced(1, fld))]
    us = {name: [] for name, _ in legs}
    try:
        with torch.cuda.stream(stream):
            for name, fn in legs:
                window(stream, fn, warm)
            stream.synchronize()
            for _ in range(args.windows):
                for name, fn in legs:
                    us[name].append(window(stream, fn, args.calls))
            stream.synchronize()
            # what the calls answered: the forms agree, and the classes of the timed poses
            capi.set_option(capi.OPT_COLLISION_IMPL, 1)
            capi.clearance_batch(cfg, grid, poses, out, dmin, disp, stream=s)
            stream.synchronize()
            ring = (out.clone(), dmin.clone(), disp.clone())
            capi.set_option(capi.OPT_COLLISION_IMPL, 2)
            capi.clearance_batch(cfg, grid, poses, out, dmin, disp, stream=s)
            stream.synchronize()
            agree = all(torch.equal(a, b) for a, b in zip(ring, (out, dmin, disp)))
    finally:
        capi.set_option(capi.OPT_COLLISION_IMPL, 0)
    classes = [int((out[:, 0] == m).sum().item()) for m in (0, 1, 2)]
    med = {name: float(np.median(v)) for name, v in us.items()}
    lines = ["clearance queries: cost per call (tools/clearance_cost.py)",
             "%s, demo map %d x %d cells of %.2f m (%d occupied), robot %s: %d offsets per pose, key map of %d x %d centres"
             % (torch.cuda.get_device_name(0), NX, NY, RES, int((data >= 80).sum()), COLL, N_OFF, NX + 2 * REACH, NY + 2 * REACH),
             "device events, %d windows x %d calls per leg after %d warm-up calls, legs alternating; median [min .. max] us per call"
             % (args.windows, args.calls, warm),
             "the %d poses: %d crash, %d obstacle, %d none; ring form and map form agree bit for bit: %s"
             % (P_max, classes[0], classes[1], classes[2], agree), ""]
    for name, _ in legs:
        lines.append("  %-32s %s" % (name, stats(us[name])))
    passes = (N_OFF + 63) // 64
    lo, hi = SIZES[0], SIZES[-1]
    build = med["clearance map  P = 1 (build)"]
    lines += ["", "as constants of the cost model (use_key_map, csrc/clearance_kernel.hip):",
              "  ring: fixed %.1f us (P = %d), %.3g us per pose and pass of 64 offsets (P = %d against %d, %d passes)"
              % (med["clearance ring P = %d" % lo], lo, (med["clearance ring P = %d" % hi] - med["clearance ring P = %d" % lo]) / ((hi - lo) * passes),
                 hi, lo, passes),
              "  map:  build %.1f us = %.3g us per centre of the key map with %d occupied cells; %.3g us per pose (P = %d against %d)"
              % (build, build / ((NX + 2 * REACH) * (NY + 2 * REACH)), int((data >= 80).sum()),
                 (med["clearance map  P = %d" % hi] - med["clearance map  P = %d" % lo]) / (hi - lo), hi, lo)]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    capi.release_collision_caches()


if __name__ == "__main__":
    main()

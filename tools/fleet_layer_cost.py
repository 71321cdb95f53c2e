#!/usr/bin/env python3
"""What the fleet layer costs (eea_fleet_layer_update, eea_tick_batch_fleet: csrc/fleet_layer_kernel.hip and the layer
instances of csrc/collision_kernel.hip), and that eea_tick_batch itself costs what it did.

4096 robots on the demo map (240 x 120 cells of 0.05 m, the three blocks of tests/test_gpu_fleet_tick.py) with the robot of
host/config/explore_omni.yaml (r_bnd 13, r_col 17, r_max 20 cells) and body = r_bnd: reach 30, |F| = 2789 cells in 61 row spans.
With device events around windows of calls on one stream (warm-up first, the legs alternating):
  the update (clear + stamp + row scan);
  eea_tick_batch, eea_tick_batch_fleet with the layer of the fleet's poses, eea_tick_batch_fleet with an empty layer (every
  robot masked: the cost of the lookups alone) -- K = 10, T = 50, the inflated collision map cached, every tick from the same
  zeroed state, so every leg does the same work in every call.
4096 robots of 0.65 m on 12 m x 6 m stand in each other's bodies: with the layer no twist validates and no dynamic window
finds a way, which the counts printed with the timings show; --spread N thins the fleet to every N-th robot active in the
layer (the tick still runs all 4096).
--against VARIANT: eea_tick_batch of this library and of lib/libergodic_amd<VARIANT>.so (the parent commit's sources built with
`make VARIANT=<VARIANT>`), each in processes of its own, alternating, ROUNDS times: the medians per process and their spread.
usage: tools/fleet_layer_cost.py [--out FILE] [--against _parent] [--rounds 5] [--spread 64]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ergodic_exploration_amd import capi  # noqa: E402

COLL = (0.7, 1.0, 0.2, 0.8)
DWA_OMNI = (0.1, 2.0, 0.2, 2.5, 2.5, 1.0, 1.0, -1.0, 1.0, -1.0, 2.0, -2.0, 3, 8, 5)   # host/config/explore_omni.yaml
BOUNDS = (-1.0, 11.0, -1.0, 5.0)
RES, NX, NY = 0.05, 240, 120
OBSTACLES = [(2.4, 0.2, 3.0, 2.6), (6.0, 2.0, 6.5, 4.6), (8.8, -0.4, 9.4, 1.2)]


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


class Fleet:
    def __init__(self, B):
        lim = np.array([1.0, 1.0, 2.0])
        self.eng = capi.Engine(capi.make_config(capi.MODEL_OMNI, 0.1, 5.0, 0.1, 1.0, 10, np.diag([1.0, 1.0, 2.0]), -lim, lim))
        self.eng.set_target_gaussians([[2.5, 2.5], [8.5, 2.5]], [[1.5, 1.5], [1.5, 1.5]])
        self.eng.config_domain(BOUNDS)
        self.B, self.T = B, self.eng.T
        rng = np.random.default_rng(7)
        poses = np.stack([rng.uniform(0.0, 10.0, B), rng.uniform(0.0, 4.0, B), rng.uniform(-3.0, 3.0, B)], 1)
        z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device="cuda")
        self.pose, self.vb, self.grid = torch.as_tensor(poses).cuda(), z(B, 3), torch.as_tensor(demo_map()).cuda()
        self.ut, self.follow, self.count, self.u, self.traj = z(B, self.T, 3), z(B, dt=torch.int32), z(B, dt=torch.int32), z(B, 3), z(B, self.T, 3)
        self.valid, self.skip, self.source = z(B, dt=torch.int32), z(B, dt=torch.int32), z(B, dt=torch.int32)
        self.ccfg, self.dcfg = capi.make_collision_cfg(BOUNDS[0], BOUNDS[2], RES, NX, NY, *COLL), capi.DwaCfg(*DWA_OMNI)
        self.stream = torch.cuda.Stream()

    def tick(self, layer=None):
        """one tick from the zeroed state: the same work in every call"""
        for x in (self.ut, self.follow, self.count, self.u):
            x.zero_()
        args = (self.B, self.pose, self.ut, self.follow, self.count, self.u, self.vb, self.grid, self.traj, self.valid, self.skip,
                self.ccfg, self.dcfg, 0.1, 0.5)
        kw = dict(source=self.source, stream=self.stream.cuda_stream, grid_epoch=1)
        if layer is None:
            self.eng.tick_batch(*args, **kw)
        else:
            self.eng.tick_batch_fleet(layer, *args, **kw)


def stats(v):
    return "%9.1f  [%.1f .. %.1f]" % (float(np.median(v)), min(v), max(v))


def tick_only(args):
    """the child of --against: eea_tick_batch alone, one JSON line"""
    f = Fleet(args.robots)
    with torch.cuda.stream(f.stream):
        window(f.stream, f.tick, 3)
        us = [window(f.stream, f.tick, args.calls) for _ in range(args.windows)]
    f.eng.close()
    print(json.dumps({"variant": os.environ.get("EEA_LIB_VARIANT", ""), "median_us": float(np.median(us)), "min_us": min(us), "max_us": max(us)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fleet_layer.txt"))
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed window")
    ap.add_argument("--spread", type=int, default=64, help="a second layer with every N-th robot active")
    ap.add_argument("--against", default=None, help="library variant of the parent commit, e.g. _parent")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tick-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fleet_layer_cost.py measures on the GPU: none found")
    if args.tick_only:
        return tick_only(args)
    B, warm = args.robots, 3
    f = Fleet(B)
    s = f.stream.cuda_stream
    r_bnd = int(np.floor(COLL[0] / RES))
    full, thin, empty = (capi.FleetLayer(f.ccfg, r_bnd, B) for _ in range(3))
    thin_mask = torch.zeros(B, dtype=torch.int32, device="cuda")
    thin_mask[::args.spread] = 1
    none_mask = torch.zeros(B, dtype=torch.int32, device="cuda")
    legs = [("update", lambda: full.update(f.pose, stream=s)),
            ("tick", lambda: f.tick()),
            ("tick + empty layer", lambda: f.tick(empty)),
            ("tick + layer, 1 in %d" % args.spread, lambda: f.tick(thin)),
            ("tick + layer, all", lambda: f.tick(full))]
    us, valid = {name: [] for name, _ in legs}, {}
    with torch.cuda.stream(f.stream):
        full.update(f.pose, stream=s)
        thin.update(f.pose, mask=thin_mask, stream=s)
        empty.update(f.pose, mask=none_mask, stream=s)
        for name, fn in legs:
            window(f.stream, fn, warm)
            f.stream.synchronize()
            valid[name] = (int(f.valid.sum().item()), int((f.source == 2).sum().item()), int((f.u.abs().sum(1) > 0).sum().item()))
        for _ in range(args.windows):
            for name, fn in legs:
                us[name].append(window(f.stream, fn, args.calls))
        f.stream.synchronize()
    count, cell = full.read()
    lines = ["fleet layer: cost per call (tools/fleet_layer_cost.py)",
             "%s, %d robots, demo map %d x %d cells of %.2f m, robot %s, body %d cells: reach %d, layer of %d x %d centres"
             % (torch.cuda.get_device_name(0), B, NX, NY, RES, COLL, r_bnd, full.reach, full.shape[1], full.shape[0]),
             "device events, %d windows x %d calls per leg after %d warm-up calls, legs alternating; median [min .. max] us per call"
             % (args.windows, args.calls, warm),
             "every tick starts from the zeroed state (K = 10, T = %d, inflated collision map cached)" % f.T,
             "stamped robots %d, largest count %d" % (int((cell[:, 0] != capi.FleetLayer.NOT_STAMPED).sum()), int(count.max())), ""]
    for name, _ in legs:
        extra = "" if name == "update" else "   valid twists %d, dynamic windows %d, moving robots %d of %d" % (valid[name] + (B,))
        lines.append("  %-24s %s%s" % (name, stats(us[name]), extra))
    base = float(np.median(us["tick"]))
    lines.append("")
    lines.append("  per tick, update + (tick with the layer - tick): empty %+.1f us, 1 in %d %+.1f us, all %+.1f us"
                 % (np.median(us["update"]) + np.median(us["tick + empty layer"]) - base, args.spread,
                    np.median(us["update"]) + np.median(us[legs[3][0]]) - base,
                    np.median(us["update"]) + np.median(us["tick + layer, all"]) - base))
    for l in (full, thin, empty):
        l.close()
    f.eng.close()
    if args.against is not None:
        lines += ["", "eea_tick_batch alone, this library against lib/libergodic_amd%s.so: %d processes each, alternating;"
                  % (args.against, args.rounds), "median [min .. max] us per call of each process's %d windows x %d calls"
                  % (args.windows, args.calls)]
        res = {"": [], args.against: []}
        for _ in range(args.rounds):
            for variant in ("", args.against):
                env = dict(os.environ, EEA_LIB_VARIANT=variant)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tick-only", "--robots", str(B), "--windows",
                                      str(args.windows), "--calls", str(args.calls)], env=env, capture_output=True, text=True,
                                     timeout=300)
                if out.returncode != 0:
                    sys.exit("the tick-only child failed (variant %r): %s" % (variant, out.stderr[-2000:]))
                res[variant].append(json.loads(out.stdout.strip().splitlines()[-1]))
        for variant, name in (("", "this library"), (args.against, "parent (%s)" % args.against)):
            med = [r["median_us"] for r in res[variant]]
            lines.append("  %-24s %s   per process: %s" % (name, stats(med), " ".join("%.1f" % m for m in med)))
        a, b = np.median([r["median_us"] for r in res[""]]), np.median([r["median_us"] for r in res[args.against]])
        lines.append("  this / parent = %.4f; the parent's own processes spread over %.2f %% of their median"
                     % (a / b, 100.0 * (max(r["median_us"] for r in res[args.against]) - min(r["median_us"] for r in res[args.against])) / b))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()

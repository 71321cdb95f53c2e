#!/usr/bin/env python3
"""What the pooled replay memory (eea_replay_pool_sample, csrc/replay_kernel.hip) costs per call, beside the robot's own
memory (eea_replay_sample) at the same shapes in the same run, and what sharing the past does to the fleet's ergodic metric.

4096 robots, fp64.  Stores filled to: 1200 poses each, 4096 each (400 MB of store), and uniform in [0, 4096]; 16 and 100 columns;
the pool with and without the robot's own poses.  Device events around windows of calls on one stream (warm-up first, the legs
alternating); a pooled call is TWO launches (the offsets scan, the sampler) and is timed as the pair.
At the end a closed loop of 4096 robots x 120 ticks (Omni, K = 10, T = 50: eea_control_batch + eea_integrate_twist_batch) runs
two ways with 100 columns per robot in both: 100 own columns; 50 own + 50 pooled (without the robot's own poses, accumulated).
The fleet's eea_records_metric of both histories is printed: information for DESIGN.md, not a pass / fail bar.
usage: tools/pool_cost.py [--out FILE]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ergodic_exploration_amd import capi  # noqa: E402


def fill(mem, counts, B, gen):
    """appends until robot b holds counts[b] poses (poses uniform on the demo map, drawn on the device)"""
    d_counts = torch.as_tensor(counts, dtype=torch.int32).cuda()
    scale = torch.tensor([9.0, 4.0, 1.0], dtype=torch.float64, device="cuda")
    for t in range(int(counts.max())):
        pose = torch.rand((B, 3), dtype=torch.float64, device="cuda", generator=gen) * scale
        mem.append(pose, (d_counts > t).to(torch.int32))
    got, dropped = mem.counts()
    assert got.tolist() == counts.tolist() and dropped == 0


def window(stream, fn, n):
    """microseconds per call of fn over n calls on the stream, by device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(n):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def closed_loop(B, ticks, own, pooled, stream, lines):
    """the fleet's metric after `ticks` ticks of a loop whose robots get `own` own and `pooled` pooled columns"""
    lim = np.array([1.0, 1.0, 2.0])
    eng = capi.Engine(capi.make_config(capi.MODEL_OMNI, 0.1, 5.0, 0.1, 1.0, 10, np.diag([1.0, 1.0, 2.0]), -lim, lim))
    eng.set_target_gaussians([[2.5, 2.5], [8.5, 2.5]], [[1.5, 1.5], [1.5, 1.5]])
    eng.config_domain((-1.0, 11.0, -1.0, 5.0))
    rng = np.random.default_rng(2)
    poses = np.stack([rng.uniform(0.2, 9.5, B), rng.uniform(-0.2, 4.2, B), rng.uniform(-0.6, 0.6, B)], 1)
    d_pose = torch.as_tensor(poses).cuda()
    d_ut = torch.zeros((B, eng.T, 3), dtype=torch.float64, device="cuda")
    d_u0 = torch.zeros((B, 3), dtype=torch.float64, device="cuda")
    stride = own + pooled
    d_cols = torch.zeros((B, stride, 3), dtype=torch.float64, device="cuda")
    d_n = torch.zeros((B,), dtype=torch.int32, device="cuda")
    mem = capi.ReplayMemory(B, ticks + 8, own, seed=1)
    s = stream.cuda_stream
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for t in range(ticks):
            mem.append_sample(d_pose, t, d_cols, d_n, stream=s)
            if pooled:
                mem.sample_pool(t, pooled, d_cols, d_n, exclude_self=True, accumulate=True, stream=s)
            eng.control_batch(B, d_pose, d_ut, d_u0, mem_cols=d_cols, n_mem=d_n, mem_stride=stride, stream=s)
            capi.integrate_twist_batch(d_pose, d_u0, 0.1, stream=s)
        eps, eps_fleet = mem.coverage(eng, stream=s)
    stream.synchronize()
    lines.append("  %3d own + %3d pooled columns: fleet metric %.6e, per-robot metric median %.6e, columns in the last tick %d .. %d"
                 % (own, pooled, float(eps_fleet.cpu()[0]), float(eps.median().cpu()), int(d_n.min().cpu()), int(d_n.max().cpu())))
    mem.close()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_pool.txt"))
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200, help="calls per timed window")
    ap.add_argument("--ticks", type=int, default=120, help="ticks of the closed loops at the end")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pool_cost.py measures on the GPU: none found")
    B, cap, warm = args.robots, 4096, 20
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    cases = [("1200 each", np.full(B, 1200, dtype=np.uint32)), ("4096 each", np.full(B, 4096, dtype=np.uint32)),
             ("uniform in [0, 4096]", np.random.default_rng(1).integers(0, 4097, B).astype(np.uint32))]
    lines = ["pooled replay memory: cost per call (tools/pool_cost.py)",
             "%s, %d robots, fp64, capacity %d; device events, %d windows x %d calls per leg after %d warm-up calls, legs alternating"
             % (torch.cuda.get_device_name(0), B, cap, args.windows, args.calls, warm),
             "a pooled call = offsets scan + sampler (two launches, timed as the pair); median [min .. max] us per call", ""]
    for name, counts in cases:
        for n_cols in (16, 100):
            mem = capi.ReplayMemory(B, cap, n_cols, seed=1)
            fill(mem, counts, B, gen)
            d_cols = torch.zeros((B, n_cols, 3), dtype=torch.float64, device="cuda")
            d_n = torch.zeros((B,), dtype=torch.int32, device="cuda")
            draw = [0]

            def own():
                draw[0] += 1
                mem.sample(draw[0], d_cols, d_n, stream=s)

            def pool_all():
                draw[0] += 1
                mem.sample_pool(draw[0], n_cols, d_cols, d_n, exclude_self=False, stream=s)

            def pool_others():
                draw[0] += 1
                mem.sample_pool(draw[0], n_cols, d_cols, d_n, exclude_self=True, stream=s)

            legs = [("eea_replay_sample (own)", own), ("pool, all robots", pool_all), ("pool, without own", pool_others)]
            res = {k: [] for k, _ in legs}
            with torch.cuda.stream(stream):
                for _, fn in legs:
                    window(stream, fn, warm)
                for _ in range(args.windows):
                    for k, fn in legs:
                        res[k].append(window(stream, fn, args.calls))
            med = {k: float(np.median(v)) for k, v in res.items()}
            lines.append("counts %s, %d columns (%.2f MB of columns per call)" % (name, n_cols, B * n_cols * 24 / 1e6))
            for k, _ in legs:
                lines.append("  %-26s %8.1f  [%.1f .. %.1f]   x %.2f of the own-memory call"
                             % (k, med[k], min(res[k]), max(res[k]), med[k] / med["eea_replay_sample (own)"]))
            mem.close()
            del d_cols, d_n, mem
    lines += ["", "closed loop, %d robots x %d ticks (Omni K = 10, T = 50), 100 columns per robot in both runs:" % (B, args.ticks)]
    closed_loop(B, args.ticks, 100, 0, stream, lines)
    closed_loop(B, args.ticks, 50, 50, stream, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

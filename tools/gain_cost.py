#!/usr/bin/env python3
"""What the information-gain target costs (eea_sense_gain_field, eea_set_target_gain: csrc/gain_kernel.hip), and what it is
compared with.

The 1024 x 1024 occupancy grid of BASELINE config 5 (seed 2024: 70 % free, 10 % occupied, 20 % unknown in 32-cell blocks,
0.1 m cells) as the ground truth, partly revealed by 512 robots at R = 50 (eea_sense_reveal_batch); on that known grid, at
(range_cells, stride) = (10, 1), (50, 4) and (127, 8) -- the last one marches in global memory (its window passes 64 KB) --,
with device events around windows of calls on one stream (warm-up first, the legs alternating) and the host's clock around the
same windows:
  the field call; eea_set_target_gain (field -> values -> phi_k, K = 10, no host wait);
against
  eea_set_target_occupancy of the same known grid in the same run (the entropy() surrogate; it waits for its stream).
The device's field must equal tests/gain_restatement.py on a sub-window of candidates, bit for bit, or the run fails.
usage: tools/gain_cost.py [--out FILE] [--points 10:1,50:4,127:8]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ergodic_exploration_amd import capi  # noqa: E402
from tests import gain_restatement as gr  # noqa: E402
from tests import sense_restatement as sr  # noqa: E402

COLL = (0.7, 1.0, 0.2, 0.8)


def occupancy(nx, ny, seed=2024, block=32):
    """BASELINE config 5's grid (the construction of tests/test_gpu_phik_parity.py)"""
    rng = np.random.default_rng(seed)
    blocks = rng.choice(np.array([0, 100, -1], dtype=np.int8), size=(ny // block + 1, nx // block + 1), p=[0.7, 0.1, 0.2])
    return np.ascontiguousarray(np.kron(blocks, np.ones((block, block), dtype=np.int8))[:ny, :nx])


def window(stream, fn, n):
    """(device us per call, host us per call until the last call has returned)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    t1 = time.perf_counter()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n, (t1 - t0) * 1e6 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gain.txt"))
    ap.add_argument("--points", default="10:1,50:4,127:8")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5, help="calls per timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gain_cost.py measures on the GPU: none found")
    nx = ny = 1024
    res, K, P, warm = 0.1, 10, 512, 2
    g = sr.Geometry(0.0, 0.0, res, nx, ny, COLL[3])
    truth = occupancy(nx, ny)
    ccfg = capi.make_collision_cfg(0.0, 0.0, res, nx, ny, *COLL)
    lim = np.array([1.0, 1.0, 2.0])
    eng = capi.Engine(capi.make_config(capi.MODEL_OMNI, 0.1, 5.0, res, 1.0, K, np.diag([1.0, 1.0, 2.0]), -lim, lim))
    lx, ly = (nx - 1) * res, (ny - 1) * res
    rng = np.random.default_rng(7)
    poses = np.stack([rng.uniform(0.0, nx * res, P), rng.uniform(0.0, ny * res, P), rng.uniform(-3.0, 3.0, P)], 1)
    d_truth = torch.as_tensor(truth).cuda()
    d_known = torch.full((ny, nx), -1, dtype=torch.int8, device="cuda")
    d_counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    d_gain = torch.zeros((ny, nx), dtype=torch.int32, device="cuda")
    capi.sense_reveal_batch(ccfg, 50, d_truth, d_known, torch.as_tensor(poses).cuda())
    capi.grid_census(ccfg, d_known, d_counts)
    torch.cuda.synchronize()
    known = d_known.cpu().numpy()
    counts = d_counts.cpu().numpy()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    lines = ["information-gain target: cost per call of eea_sense_gain_field / eea_set_target_gain (tools/gain_cost.py)",
             "%s, %d x %d known grid (BASELINE config 5, seed 2024, revealed by %d robots at R = 50: %d of %d cells unknown), K = %d"
             % (torch.cuda.get_device_name(0), nx, ny, P, int(counts[0]), nx * ny, K),
             "device events and the host's clock, %d windows x %d calls per leg after %d warm-up calls, legs alternating;"
             % (args.windows, args.calls, warm),
             "median [min .. max] us per call on the device | median us per call on the host until the call returns", ""]
    ok = True
    for R, stride in [tuple(int(v) for v in pt.split(":")) for pt in args.points.split(",")]:
        legs = [("gain field", lambda: capi.sense_gain_field(ccfg, R, stride, d_known, d_gain, stream=s)),
                ("set_target_gain", lambda: eng.set_target_gain(ccfg, R, stride, d_known, lx, ly, floor=0.5, stream=s)),
                ("set_target_occupancy", lambda: eng.set_target_occupancy(nx, ny, d_known, lx, ly, stream=s))]
        us = {name: [] for name, _ in legs}
        with torch.cuda.stream(stream):
            for _, fn in legs:
                window(stream, fn, warm)
            for _ in range(args.windows):
                for name, fn in legs:
                    us[name].append(window(stream, fn, args.calls))
            capi.sense_gain_field(ccfg, R, stride, d_known, d_gain, stream=s)
            stream.synchronize()
        # the check at this size: the candidates of a sub-window around the grid's centre, against the restatement
        side = {1: 24, 4: 24, 8: 24}.get(stride, 3 * stride)
        lo = (nx // 2 // stride) * stride
        rows = cols = range(lo, lo + side)
        want = gr.gain_field(g, R, stride, known, rows, cols)
        got = d_gain.cpu().numpy().view(np.uint32)
        same = np.array_equal(got[lo:lo + side, lo:lo + side], want[lo:lo + side, lo:lo + side])
        off = np.ones((ny, nx), dtype=bool)
        off[::stride, ::stride] = False
        same = same and bool((got[off] == 0).all())
        ok = ok and same
        W, H = 31 * stride + 1 + 2 * R, 7 * stride + 1 + 2 * R
        lines.append("R = %d, stride %d (%d candidates, %d rays each, %s): max gain %d, candidates with gain > 0: %d; device == "
                     "restatement on %d x %d cells: %s"
                     % (R, stride, ((nx - 1) // stride + 1) * ((ny - 1) // stride + 1), 8 * R,
                        "LDS window of %d B per tile of 32 x 8 candidates" % (W * H) if W * H <= 65536 else "global memory",
                        int(got.max()), int((got > 0).sum()), side, side, "yes" if same else "NO"))
        for name, _ in legs:
            dev, host = [u[0] for u in us[name]], [u[1] for u in us[name]]
            lines.append("  %-22s %10.1f  [%.1f .. %.1f] | %9.1f" % (name, float(np.median(dev)), min(dev), max(dev), float(np.median(host))))
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

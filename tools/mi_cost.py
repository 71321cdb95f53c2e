#!/usr/bin/env python3
"""What the mutual-information target costs (eea_sense_mi_field, eea_set_target_mi: csrc/mi_kernel.hip) beside the gain count it
refines (eea_sense_gain_field, eea_set_target_gain: csrc/gain_kernel.hip).

The grid, seed, reveal and (range_cells, stride) legs of tools/gain_cost.py (profiles/gain.txt): the 1024 x 1024 occupancy grid
of BASELINE config 5 (seed 2024) as the ground truth, partly revealed by 512 robots at R = 50; on that known grid at (10, 1),
(50, 4) and (127, 8) -- the last one marches in global memory --, with device events around windows of calls on one stream
(warm-up first, the legs alternating in the same run) and the host's clock around the same windows:
  the MI field beside the gain field; eea_set_target_mi beside eea_set_target_gain (field -> values -> phi_k, K = 10).
The figure to read is the ratio MI field / gain field per leg.  The device's MI field must equal tests/mi_restatement.py fed the
library's table on a 24 x 24 window of candidates, bit for bit, or the run fails.
usage: tools/mi_cost.py [--out FILE] [--points 10:1,50:4,127:8] [--p-unknown 0.5]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ergodic_exploration_amd import capi  # noqa: E402
from gain_cost import COLL, occupancy, window  # noqa: E402
from tests import mi_restatement as mr  # noqa: E402
from tests import sense_restatement as sr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mi.txt"))
    ap.add_argument("--points", default="10:1,50:4,127:8")
    ap.add_argument("--p-unknown", type=float, default=0.5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5, help="calls per timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mi_cost.py measures on the GPU: none found")
    nx = ny = 1024
    res, K, P, warm, p_unknown = 0.1, 10, 512, 2, args.p_unknown
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
    d_mi = torch.zeros((ny, nx), dtype=torch.float64, device="cuda")
    capi.sense_reveal_batch(ccfg, 50, d_truth, d_known, torch.as_tensor(poses).cuda())
    capi.grid_census(ccfg, d_known, d_counts)
    torch.cuda.synchronize()
    known = d_known.cpu().numpy()
    counts = d_counts.cpu().numpy()
    h, pass_ = capi.sense_mi_table(ccfg, p_unknown)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    lines = ["mutual-information target: cost per call of eea_sense_mi_field / eea_set_target_mi beside the gain count's entries "
             "(tools/mi_cost.py)",
             "%s, %d x %d known grid (BASELINE config 5, seed 2024, revealed by %d robots at R = 50: %d of %d cells unknown), K = %d, "
             "p_unknown = %g" % (torch.cuda.get_device_name(0), nx, ny, P, int(counts[0]), nx * ny, K, p_unknown),
             "device events and the host's clock, %d windows x %d calls per leg after %d warm-up calls, legs alternating;"
             % (args.windows, args.calls, warm),
             "median [min .. max] us per call on the device | median us per call on the host until the call returns", ""]
    ok = True
    for R, stride in [tuple(int(v) for v in pt.split(":")) for pt in args.points.split(",")]:
        legs = [("mi field", lambda: capi.sense_mi_field(ccfg, R, stride, d_known, d_mi, p_unknown=p_unknown, stream=s)),
                ("gain field", lambda: capi.sense_gain_field(ccfg, R, stride, d_known, d_gain, stream=s)),
                ("set_target_mi", lambda: eng.set_target_mi(ccfg, R, stride, d_known, lx, ly, p_unknown=p_unknown, floor=0.5,
                                                            stream=s)),
                ("set_target_gain", lambda: eng.set_target_gain(ccfg, R, stride, d_known, lx, ly, floor=0.5, stream=s))]
        us = {name: [] for name, _ in legs}
        with torch.cuda.stream(stream):
            for _, fn in legs:
                window(stream, fn, warm)
            for _ in range(args.windows):
                for name, fn in legs:
                    us[name].append(window(stream, fn, args.calls))
            capi.sense_mi_field(ccfg, R, stride, d_known, d_mi, p_unknown=p_unknown, stream=s)
            stream.synchronize()
        # the check at this size: the candidates of a 24 x 24 window around the grid's centre, against the restatement
        side = 24 if 24 % stride == 0 else 3 * stride
        lo = (nx // 2 // stride) * stride
        rows = cols = range(lo, lo + side)
        want = mr.mi_field(g, R, stride, known, h, pass_, rows, cols)
        got = d_mi.cpu().numpy()
        same = np.array_equal(got[lo:lo + side, lo:lo + side].view(np.uint64), want[lo:lo + side, lo:lo + side].view(np.uint64))
        off = np.ones((ny, nx), dtype=bool)
        off[::stride, ::stride] = False
        same = same and bool((got[off].view(np.uint64) == 0).all())
        ok = ok and same
        W, H = 31 * stride + 1 + 2 * R, 7 * stride + 1 + 2 * R
        med = {name: float(np.median([u[0] for u in us[name]])) for name, _ in legs}
        lines.append("R = %d, stride %d (%d candidates, %d rays each, %s): max mi %.4f nat, candidates with mi > 0: %d; device == "
                     "restatement on %d x %d cells: %s"
                     % (R, stride, ((nx - 1) // stride + 1) * ((ny - 1) // stride + 1), 8 * R,
                        "LDS window of %d B + 1648 B of table per tile of 32 x 8 candidates" % (W * H)
                        if W * H + 1648 <= 65536 else "global memory",
                        float(got.max()), int((got > 0).sum()), side, side, "yes" if same else "NO"))
        for name, _ in legs:
            dev, host = [u[0] for u in us[name]], [u[1] for u in us[name]]
            lines.append("  %-22s %10.1f  [%.1f .. %.1f] | %9.1f" % (name, med[name], min(dev), max(dev), float(np.median(host))))
        lines.append("  mi field / gain field = %.2f, set_target_mi / set_target_gain = %.2f"
                     % (med["mi field"] / med["gain field"], med["set_target_mi"] / med["set_target_gain"]))
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

#!/usr/bin/env python3
"""What the evidence grid costs (eea_sense_observe_batch, eea_evidence_publish: csrc/evidence_kernel.hip) beside the calls it
stands next to (eea_sense_reveal_batch, eea_grid_census: csrc/sense_kernel.hip).

The grid and seed of tools/gain_cost.py (profiles/gain.txt): the 1024 x 1024 occupancy grid of BASELINE config 5 (seed 2024) as
the ground truth, 4096 robots scattered over it, at R = 10, 50 and 127, with device events around windows of calls on one
stream (warm-up first, the legs alternating in the same run) and the host's clock around the same windows:
  a noisy observe (thr_miss = 2^30, thr_false = 2^32 / 20, a new scan number per call) beside the reveal with the same poses;
  the publication with and without its counts beside the census of the published grid.
The figure to read is the ratio observe / reveal per R.  Before the timing, per R: the ideal sensor's ranges must equal the
reveal's bit for bit and its evidence must be non-zero exactly where the reveal wrote, and the published grid must equal the
table lookup in numpy with the census' counts, or the run fails.
usage: tools/evidence_cost.py [--out FILE] [--ranges 10,50,127]"""
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
from tests import evidence_restatement as er  # noqa: E402
from tests import sense_restatement as sr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evidence.txt"))
    ap.add_argument("--ranges", default="10,50,127")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5, help="calls per timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("evidence_cost.py measures on the GPU: none found")
    nx = ny = 1024
    res, P, warm = 0.1, 4096, 2
    g = sr.Geometry(0.0, 0.0, res, nx, ny, COLL[3])
    truth = occupancy(nx, ny)
    ccfg = capi.make_collision_cfg(0.0, 0.0, res, nx, ny, *COLL)
    ideal = er.Evidence(25, 7, 1024, er.QUANTUM, 0, 0, 2024, 0)
    noisy = ideal._replace(thr_miss=1 << 30, thr_false=(1 << 32) // 20)
    e_ideal, e_noisy = capi.EvidenceCfg(*ideal), capi.EvidenceCfg(*noisy)
    table = capi.evidence_table(e_noisy)
    rng = np.random.default_rng(7)
    poses = np.stack([rng.uniform(0.0, nx * res, P), rng.uniform(0.0, ny * res, P), rng.uniform(-3.0, 3.0, P)], 1)
    d_pose = torch.as_tensor(poses).cuda()
    d_truth = torch.as_tensor(truth).cuda()
    d_known = torch.full((ny, nx), -1, dtype=torch.int8, device="cuda")
    d_evid = torch.zeros((ny, nx), dtype=torch.int32, device="cuda")
    d_counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    d_census = torch.zeros(3, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    lines = ["evidence grid: cost per call of eea_sense_observe_batch / eea_evidence_publish beside eea_sense_reveal_batch / "
             "eea_grid_census (tools/evidence_cost.py)",
             "%s, %d x %d truth grid (BASELINE config 5, seed 2024), %d robots, noisy sensor thr_miss = 2^30, thr_false = 2^32 / 20"
             % (torch.cuda.get_device_name(0), nx, ny, P),
             "device events and the host's clock, %d windows x %d calls per leg after %d warm-up calls, legs alternating;"
             % (args.windows, args.calls, warm),
             "median [min .. max] us per call on the device | median us per call on the host until the call returns", ""]
    ok = True
    scan = [0]

    def observe(R):
        scan[0] += 1
        capi.sense_observe_batch(ccfg, e_noisy, R, scan[0], d_truth, d_evid, d_pose, stream=s)

    for R in [int(v) for v in args.ranges.split(",")]:
        # the checks at this size, device against device and against numpy
        d_r1 = torch.full((P, 8 * R), -7, dtype=torch.int32, device="cuda")
        d_r2 = torch.full((P, 8 * R), -8, dtype=torch.int32, device="cuda")
        with torch.cuda.stream(stream):
            d_known.fill_(-1)
            d_evid.zero_()
            capi.sense_reveal_batch(ccfg, R, d_truth, d_known, d_pose, d_r1, stream=s)
            capi.sense_observe_batch(ccfg, e_ideal, R, 0, d_truth, d_evid, d_pose, d_r2, stream=s)
            stream.synchronize()
            same = bool(torch.equal(d_r1, d_r2))
            revealed = d_known.cpu().numpy() != -1
            evid0 = d_evid.cpu().numpy()
            # (a truth cell of -1 stays -1 in the reveal: count the cells it wrote through the evidence of free space instead)
            same = same and bool(((evid0 != 0) >= revealed).all()) and bool(((evid0 != 0) & ~revealed <= (truth == -1)).all())
            touched = int((evid0 != 0).sum())
            for k in range(3):
                capi.sense_observe_batch(ccfg, e_noisy, R, 100 + k, d_truth, d_evid, d_pose, stream=s)
            capi.evidence_publish(ccfg, e_noisy, d_evid, d_known, d_counts, stream=s)
            capi.grid_census(ccfg, d_known, d_census, stream=s)
            stream.synchronize()
            evid = d_evid.cpu().numpy()
            known = d_known.cpu().numpy()
            same = same and np.array_equal(known, er.publish(noisy, evid, table))
            same = same and tuple(int(v) for v in d_counts.cpu().numpy()) == tuple(int(v) for v in d_census.cpu().numpy()) \
                == sr.census(g, known)
        ok = ok and same
        legs = [("observe (noisy)", lambda: observe(R)),
                ("reveal", lambda: capi.sense_reveal_batch(ccfg, R, d_truth, d_known, d_pose, stream=s)),
                ("publish + counts", lambda: capi.evidence_publish(ccfg, e_noisy, d_evid, d_known, d_counts, stream=s)),
                ("publish", lambda: capi.evidence_publish(ccfg, e_noisy, d_evid, d_known, stream=s)),
                ("census", lambda: capi.grid_census(ccfg, d_known, d_census, stream=s))]
        us = {name: [] for name, _ in legs}
        with torch.cuda.stream(stream):
            for _, fn in legs:
                window(stream, fn, warm)
            for _ in range(args.windows):
                for name, fn in legs:
                    us[name].append(window(stream, fn, args.calls))
            stream.synchronize()
        W = 2 * R + 1
        med = {name: float(np.median([u[0] for u in us[name]])) for name, _ in legs}
        lines.append("R = %d (%d rays, window of %d B of LDS per robot; cells with evidence after one ideal scan: %d; one scan = "
                     "at most %d Philox calls): device == reveal / numpy: %s"
                     % (R, 8 * R, W * W, touched, P * W * ((W + 3) // 4 + 1), "yes" if same else "NO"))
        for name, _ in legs:
            dev, host = [u[0] for u in us[name]], [u[1] for u in us[name]]
            lines.append("  %-22s %10.1f  [%.1f .. %.1f] | %9.1f" % (name, med[name], min(dev), max(dev), float(np.median(host))))
        lines.append("  observe / reveal = %.2f, publish + counts / census = %.2f, publish / census = %.2f"
                     % (med["observe (noisy)"] / med["reveal"], med["publish + counts"] / med["census"], med["publish"] / med["census"]))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

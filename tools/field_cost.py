#!/usr/bin/env python3
"""What a coverage field costs (eea_records_field, csrc/field_kernel.hip), and what it is compared with.

Cases: 4096 records on the shipped 121 x 61 grid at K = 10 and K = 20, and one record on 1024 x 1024 at K = 30 (the row-tiled
grid of BASELINE config 5); fp64 and fp32 engines; the three kinds.  Per case, with device events around windows of calls on
one stream (warm-up first, the legs alternating):
  records_field of each kind;
against
  (a) the time the OUTPUT's bytes alone need at 5.8 TB/s -- the HBM rate the phi_k streaming kernel reaches on this chip
      (profiles/HISTORY.md: `roofline_phik`).  That is a READ rate: the write rate of this part has not been measured in this
      project, so the ratio printed is "x the output's bytes at the phi_k read rate", not a fraction of a peak;
  (b) the same product as two torch.matmul calls on precomputed tables on the device: W = A CY^T ([n][K][ny]), then
      F = W^T CX ([n][ny][nx]), the coefficients a_m given (the division, phi_k and lamda_k are left out of (b)).
usage: tools/field_cost.py [--out FILE]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ergodic_exploration_amd import capi  # noqa: E402

PHIK_HBM_RATE = 5.8e12   # bytes / s, a read rate: the phi_k streaming kernel on this chip (profiles/HISTORY.md, roofline_phik)
KIND_NAMES = {capi.FIELD_DENSITY: "density", capi.FIELD_DEFICIT: "deficit", capi.FIELD_POTENTIAL: "potential"}
# (records, K, nx, ny, bounds of the domain at resolution 0.1)
CASES = [(4096, 10, 121, 61, (-1.0, 11.0, -1.0, 5.0)), (4096, 20, 121, 61, (-1.0, 11.0, -1.0, 5.0)),
         (1, 30, 1024, 1024, (0.0, 102.3, 0.0, 102.3))]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field.txt"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("field_cost.py measures on the GPU: none found")
    warm = 5
    lim = np.array([1.0, 1.0, 2.0])
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    lines = ["coverage fields: cost per call of eea_records_field (tools/field_cost.py)", torch.cuda.get_device_name(0),
             "device events, %d windows x %d calls per leg after %d warm-up calls, legs alternating; median [min .. max] us per call"
             % (args.windows, args.calls, warm),
             "(a) = the output's bytes at %.1f TB/s, the phi_k kernel's HBM READ rate (the write rate of this part has not been"
             % (PHIK_HBM_RATE / 1e12),
             "measured in this project: the ratio is against that read rate, not a fraction of a peak); (b) = two torch.matmul calls",
             "on precomputed tables and given coefficients", ""]
    for n, K, nx, ny, bounds in CASES:
        for prec, dt, size in ((capi.PREC_F64, torch.float64, 8), (capi.PREC_F32, torch.float32, 4)):
            eng = capi.Engine(capi.make_config(capi.MODEL_OMNI, 0.1, 5.0, 0.1, 1.0, K, np.diag([1.0, 1.0, 2.0]), -lim, lim,
                                               precision=prec))
            eng.set_target_gaussians([[0.2 * bounds[1], 0.4 * bounds[3]], [0.7 * bounds[1], 0.4 * bounds[3]]],
                                     [[0.12 * bounds[1]] * 2, [0.12 * bounds[1]] * 2])
            eng.config_domain(bounds)
            assert eng.target_grid_size == (nx, ny), eng.target_grid_size
            gen = torch.Generator(device="cuda").manual_seed(5)
            rec = torch.rand((n, eng.ck_record_len), dtype=dt, device="cuda", generator=gen) * 2 - 1
            rec[:, K * K] = 1.0
            out = torch.empty((n, ny, nx), dtype=dt, device="cuda")
            # (b): tables and coefficients precomputed; the two products only
            A = rec[:, :K * K].reshape(n, K, K).transpose(1, 2).contiguous()       # [n][k1][k2]
            k = torch.arange(K, dtype=dt, device="cuda")[:, None]
            lx, ly = bounds[1] - bounds[0], bounds[3] - bounds[2]
            CX = torch.cos(k * (np.pi / lx) * (0.1 * torch.arange(nx, dtype=dt, device="cuda"))[None, :])    # [k1][nx]
            CY = torch.cos(k * (np.pi / ly) * (0.1 * torch.arange(ny, dtype=dt, device="cuda"))[None, :])    # [k2][ny]

            def matmul():
                W = torch.matmul(A, CY)                               # [n][k1][ny]
                torch.matmul(W.transpose(1, 2), CX, out=out)          # [n][ny][nx]

            legs = [(KIND_NAMES[kind], (lambda kind=kind: capi.records_field(eng, kind, rec, out, nx, ny, stream=s))) for kind in KIND_NAMES]
            legs.append(("(b) two torch.matmul", matmul))
            us = {name: [] for name, _ in legs}
            with torch.cuda.stream(stream):
                for _, fn in legs:
                    window(stream, fn, warm)
                for _ in range(args.windows):
                    for name, fn in legs:
                        us[name].append(window(stream, fn, args.calls))
            stream.synchronize()
            nbytes = n * nx * ny * size
            floor = nbytes / PHIK_HBM_RATE * 1e6
            lines.append("%d record(s) x %d x %d, K = %d, %s: %.1f MB of output, %.2f Gflop; (a) %.1f us"
                         % (n, nx, ny, K, "fp64" if size == 8 else "fp32", nbytes / 1e6, 2e-9 * n * K * ny * (K + nx), floor))
            for name, _ in legs:
                med = float(np.median(us[name]))
                lines.append("  %-22s %9.1f  [%.1f .. %.1f]   %.2f x the output's bytes at the phi_k read rate (%.2f TB/s written)"
                             % (name, med, min(us[name]), max(us[name]), med / floor, nbytes / (med * 1e-6) / 1e12))
            lines.append("")
            eng.close()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

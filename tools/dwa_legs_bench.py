#!/usr/bin/env python3
"""The dynamic-window legs of bench_legs.tick_legs alone, on the inflated map, with more repetitions: the same 240 x 120 grid,
3 x 8 x 5 window x 20 steps, poses (seed 99) and timing (HIP events on the launch stream), three timed blocks of 400 calls
(P = 4096) / 60 calls (P = 65536) per leg, and the sum of u_opt as a checksum.  One line per P.
Both legs run dwa_control_kernel<true, false>: dwa_vref towards a reference twist, dwa_traj along a trajectory.
usage: [EEA_LIB_VARIANT=_x] tools/dwa_legs_bench.py -- run it in fresh processes, alternating the libraries to compare
(profiles/collision_refactor.txt, run 2: parent new new parent, three times)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from ergodic_exploration_amd import capi
COLL = (0.7, 1.0, 0.2, 0.8)
DWA = (0.1, 2.0, 0.2, 2.5, 2.5, 1.0, 1.0, -1.0, 1.0, -1.0, 2.0, -2.0, 3, 8, 5)
xs, ys, res, x0, y0 = 240, 120, 0.05, -1.0, -1.0
data = np.zeros((ys, xs), dtype=np.int8)
cx, cy = x0 + (np.arange(xs) + 0.5) * res, y0 + (np.arange(ys) + 0.5) * res
for (a, b, c, d) in [(2.4, 0.2, 3.0, 2.6), (6.0, 2.0, 6.5, 4.6), (8.8, -0.4, 9.4, 1.2)]:
    data[np.ix_((cy >= b) & (cy <= d), (cx >= a) & (cx <= c))] = 100
ccfg = capi.make_collision_cfg(x0, y0, res, xs, ys, *COLL)
dcfg = capi.DwaCfg(*DWA)
d_grid = torch.as_tensor(data).cuda()
st = torch.cuda.Stream()
sp = st.cuda_stream
rng = np.random.default_rng(99)

def timed(fn, n):
    torch.cuda.synchronize()
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(st)
    for _ in range(n):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n

tag = os.environ.get("EEA_LIB_VARIANT", "") or "new"
capi.set_option(capi.OPT_COLLISION_IMPL, 2)
for P in (4096, 65536):
    x = torch.as_tensor(np.stack([rng.uniform(-0.5, 10.5, P), rng.uniform(-0.5, 4.5, P), rng.uniform(-3, 3, P)], 1)).cuda()
    u = torch.as_tensor(np.stack([rng.uniform(-1, 1, P), rng.uniform(-1, 1, P), rng.uniform(-2, 2, P)], 1)).cuda()
    hit = torch.empty((P,), dtype=torch.int32, device="cuda")
    uo = torch.empty((P, 3), dtype=torch.float64, device="cuda")
    xt = x[:, None, :].repeat(1, 50, 1).contiguous()
    n = 400 if P == 4096 else 60
    vref = [timed(lambda: capi.dwa_control_batch(ccfg, dcfg, d_grid, x, u, uo, hit, vref=u, stream=sp), n) for _ in range(3)]
    cs = float(uo.sum().item())
    traj = [timed(lambda: capi.dwa_control_batch(ccfg, dcfg, d_grid, x, u, uo, hit, xt_ref=xt, dt_ref=0.1, stream=sp), n) for _ in range(3)]
    print("[%s] inflated map P=%5d  dwa_vref %s  dwa_traj %s us  (checksums %r %r)" % (
        tag, P, " ".join("%.2f" % v for v in vref), " ".join("%.2f" % v for v in traj), cs, float(uo.sum().item())))
capi.set_option(capi.OPT_COLLISION_IMPL, 0)

#!/usr/bin/env python3
"""What the body layer costs (eea_body_layer_update / eea_body_collision_check_batch / eea_tick_batch_bodies:
csrc/body_layer_kernel.hip, csrc/footprint_plan_kernel.hip) beside eea_fleet_layer_update and eea_tick_batch_footprint of the
same run.

With device events around windows of calls on one stream (warm-up first, the legs alternating), on the 240 x 120 demo map
(0.05 m cells) with the 0.9 m x 0.5 m base and the omni window of tools/footprint_dwa_cost.py:
  the update alone at B = 4096 and for the sparse fleet, beside eea_fleet_layer_update at B = 4096;
  eea_tick_batch_footprint + move at B = 4096;
  eea_tick_batch_bodies + move at B = 4096 with every robot masked (the price of the lookups; one tick from the same state is
  asserted to give the footprint tick's bits first);
  update + eea_tick_batch_bodies + move for a sparse fleet that can move (20 robots, bodies apart at the start) and for 4096
  robots, each beside eea_tick_batch_footprint + move of the same fleet;
  the check entry at P = 65536 on the sparse fleet's layer with and without EEA_BODY_LAYER_NO_FILTER, beside
  eea_footprint_check_batch.
The ratios are those of this run.
usage: tools/body_layer_cost.py [--out FILE] [--windows 5] [--calls 20]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ergodic_exploration_amd import capi  # noqa: E402
from tools.footprint_cost import BOUNDS, COLL, NX, NY, RECT, RES, demo_map, stats, window  # noqa: E402
from tools.footprint_dwa_cost import DWA, VAL_DT, VAL_HORIZON  # noqa: E402

B_BIG, B_SPARSE, P_CHECK = 4096, 20, 65536


def sparse_start(rng, data, n):
    """n poses on free floor, at least 1.1 m apart (two 0.9 m x 0.5 m bases, r_out 0.515 m, cannot touch)"""
    out = []
    for _ in range(100000):
        if len(out) == n:
            break
        p = np.array([rng.uniform(-0.4, 10.4), rng.uniform(-0.4, 4.4), rng.uniform(-np.pi, np.pi)])
        j, i = int((p[0] - BOUNDS[0]) / RES), int((p[1] - BOUNDS[2]) / RES)
        if data[max(i - 12, 0):i + 13, max(j - 12, 0):j + 13].any():
            continue
        if all(np.hypot(p[0] - q[0], p[1] - q[1]) >= 1.1 for q in out):
            out.append(p)
    assert len(out) == n, "the floor does not hold %d robots 1.1 m apart" % n
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "body_layer.txt"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("body_layer_cost.py measures on the GPU: none found")
    warm = 3
    cfg, dcfg = capi.make_collision_cfg(BOUNDS[0], BOUNDS[2], RES, NX, NY, *COLL), capi.DwaCfg(*DWA)
    fp = capi.Footprint.of(RECT)
    data = demo_map()
    grid = torch.as_tensor(data).cuda()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rng = np.random.default_rng(7)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    sq = i32(NY, NX)
    lim = np.array([1.0, 1.0, 2.0])
    eng = capi.Engine(capi.make_config(capi.MODEL_OMNI, 0.1, 5.0, 0.1, 1.0, 10, np.diag([1.0, 1.0, 2.0]), -lim, lim))
    eng.set_target_gaussians([[2.5, 2.5], [8.5, 2.5]], [[1.5, 1.5], [1.5, 1.5]])
    eng.config_domain(BOUNDS)
    T = eng.T
    starts = {B_BIG: np.stack([rng.uniform(0.2, 9.5, B_BIG), rng.uniform(-0.2, 4.2, B_BIG), rng.uniform(-0.6, 0.6, B_BIG)], 1),
              B_SPARSE: sparse_start(rng, data, B_SPARSE)}

    class Fleet:
        def __init__(self, B, layer=None, masked=False):
            self.B, self.layer, self.masked = B, layer, masked
            self.start = torch.as_tensor(starts[B]).cuda()
            self.pose, self.ut, self.u, self.traj, self.vb = self.start.clone(), f64(B, T, 3), f64(B, 3), f64(B, T, 3), f64(B, 3)
            self.follow, self.count, self.valid, self.skip, self.source = i32(B), i32(B), i32(B), i32(B), i32(B)
            self.mask = i32(B)
            self.differ = 0

        def tick(self, move=True):
            a = (self.B, self.pose, self.ut, self.follow, self.count, self.u, self.vb, grid, self.traj, self.valid, self.skip, cfg, dcfg,
                 VAL_DT, VAL_HORIZON)
            if self.layer is None:
                eng.tick_batch_footprint(fp, *a, sq=sq, source=self.source, stream=s)
            else:
                if not self.masked:
                    self.layer.update(self.pose, stream=s)
                eng.tick_batch_bodies(self.layer, *a, sq=sq, source=self.source, stream=s)
            if move:
                capi.integrate_twist_batch(self.pose, self.u, 0.1, stream=s)      # the robots move; odometry = the commanded twist
                self.vb.copy_(self.u)

    layers = {k: capi.BodyLayer(cfg, fp, B) for k, B in (("masked", B_BIG), ("big", B_BIG), ("sparse", B_SPARSE), ("update", B_BIG),
                                                            ("check", B_SPARSE))}
    nofilter = capi.BodyLayer(cfg, fp, B_SPARSE, flags=capi.BODY_LAYER_NO_FILTER)
    disc_layer = capi.FleetLayer(cfg, 13, B_BIG)
    fleets = {"footprint tick + move, B = %d" % B_BIG: Fleet(B_BIG),
              "bodies tick + move, every robot masked, B = %d" % B_BIG: Fleet(B_BIG, layers["masked"], masked=True),
              "update + bodies tick + move, B = %d" % B_BIG: Fleet(B_BIG, layers["big"]),
              "footprint tick + move, B = %d" % B_SPARSE: Fleet(B_SPARSE),
              "update + bodies tick + move, B = %d" % B_SPARSE: Fleet(B_SPARSE, layers["sparse"])}
    big_pose, sparse_pose = torch.as_tensor(starts[B_BIG]).cuda(), torch.as_tensor(starts[B_SPARSE]).cuda()
    poses = torch.as_tensor(np.stack([rng.uniform(-0.5, 10.5, P_CHECK), rng.uniform(-0.5, 4.5, P_CHECK),
                                      rng.uniform(-np.pi, np.pi, P_CHECK)], 1)).cuda()
    hits = {k: i32(P_CHECK) for k in ("filter", "nofilter", "plain")}
    legs = [("body layer update, B = %d" % B_BIG, lambda: layers["update"].update(big_pose, stream=s)),
            ("fleet layer update, B = %d" % B_BIG, lambda: disc_layer.update(big_pose, stream=s)),
            ("body layer update, B = %d" % B_SPARSE, lambda: nofilter.update(sparse_pose, stream=s))]
    legs += [(name, f.tick) for name, f in fleets.items()]
    legs += [("body check, P = %d" % P_CHECK, lambda: layers["check"].check(grid, poses, hits["filter"], sq=sq, stream=s)),
             ("body check, no filter, P = %d" % P_CHECK, lambda: nofilter.check(grid, poses, hits["nofilter"], sq=sq, stream=s)),
             ("footprint check, P = %d" % P_CHECK, lambda: capi.footprint_check_batch(cfg, fp, grid, poses, hits["plain"], sq=sq, stream=s))]

    us = {name: [] for name, _ in legs}
    with torch.cuda.stream(stream):
        capi.distance_field(cfg, grid, sq, stream=s)
        layers["check"].update(sparse_pose, stream=s)          # the check legs: the sparse fleet where it starts, in both layers
        nofilter.update(sparse_pose, stream=s)
        # the price of the lookups is a price for the same answers: one tick from the same state, bit for bit
        layers["masked"].update(big_pose, fleets["bodies tick + move, every robot masked, B = %d" % B_BIG].mask, stream=s)
        a, b = Fleet(B_BIG), Fleet(B_BIG, layers["masked"], masked=True)
        a.tick(move=False)
        b.tick(move=False)
        stream.synchronize()
        for x, y in ((a.valid, b.valid), (a.follow, b.follow), (a.source, b.source), (a.u.view(torch.int64), b.u.view(torch.int64))):
            assert bool(torch.equal(x, y)), "the masked layer changed a verdict"
        for name, fn in legs:
            window(stream, fn, warm)
        stream.synchronize()
        for _ in range(args.windows):
            for name, fn in legs:
                us[name].append(window(stream, fn, args.calls))
        stream.synchronize()
    assert bool(torch.equal(hits["filter"], hits["nofilter"])), "the near filter changed a verdict"
    med = {name: float(np.median(v)) for name, v in us.items()}
    cover, near, snap = layers["update"].read()
    s_cover, s_near, _ = layers["check"].read()
    lines = ["body layer: cost per call (tools/body_layer_cost.py)",
             "%s; demo map %d x %d cells of %.2f m; base 0.9 m x 0.5 m (box %d cells, near over %d x %d cells, Rn %d); the disc layer: "
             "robot %s, body 13 cells" % (torch.cuda.get_device_name(0), NX, NY, RES, layers["update"].box, near.shape[1], near.shape[0],
                                          2 * layers["update"].box, COLL),
             "device events, %d windows x %d calls per leg after %d warm-up calls, legs alternating; median [min .. max] us per call"
             % (args.windows, args.calls, warm),
             "one tick with every robot masked gives the footprint tick's bits: True; with and without the near filter the check's "
             "answers are the same bits: True",
             "the %d robots of the update legs: %d stamped, largest cover %d, largest near %d; the sparse layer of the check legs: largest "
             "cover %d, near is 0 on %.1f %% of its cells" % (B_BIG, int(snap[:, 4].sum()), int(cover.max()), int(near.max()),
                                                            int(s_cover.max()), 100.0 * float((s_near == 0).mean())),
             "check: %d of %d poses hit with the layer, %d without" % (int(hits["filter"].sum().item()), P_CHECK, int(hits["plain"].sum().item()))]
    for name, f in fleets.items():
        src = np.bincount(f.source.cpu().numpy().clip(0, 3), minlength=4)
        lines.append("%s: sources of the last tick ergodic %d, follow %d, window %d, replan %d" % ((name,) + tuple(src)))
    lines.append("")
    for name, _ in legs:
        lines.append("  %-52s %s" % (name, stats(us[name])))
    r = lambda a, b: med[a] / med[b]
    lines += ["", "ratios of this run (medians):",
              "  update, B = %d: body / fleet layer %.2f" % (B_BIG, r("body layer update, B = %d" % B_BIG, "fleet layer update, B = %d" % B_BIG)),
              "  tick + move, B = %d: masked bodies / footprint %.2f; update + bodies / footprint %.2f" % (
                  B_BIG, r("bodies tick + move, every robot masked, B = %d" % B_BIG, "footprint tick + move, B = %d" % B_BIG),
                  r("update + bodies tick + move, B = %d" % B_BIG, "footprint tick + move, B = %d" % B_BIG)),
              "  tick + move, B = %d: update + bodies / footprint %.2f" % (
                  B_SPARSE, r("update + bodies tick + move, B = %d" % B_SPARSE, "footprint tick + move, B = %d" % B_SPARSE)),
              "  check, P = %d: filter / no filter %.2f; filter / footprint check %.2f" % (
                  P_CHECK, r("body check, P = %d" % P_CHECK, "body check, no filter, P = %d" % P_CHECK),
                  r("body check, P = %d" % P_CHECK, "footprint check, P = %d" % P_CHECK))]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    for l in list(layers.values()) + [nofilter, disc_layer]:
        l.close()
    eng.close()
    capi.release_collision_caches()


if __name__ == "__main__":
    main()

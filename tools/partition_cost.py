#!/usr/bin/env python3
"""What the geodesic partition costs (eea_geodesic_partition, eea_partition_goals, eea_partition_path_batch:
csrc/partition_kernel.hip), beside the calls it extends.

One 1024 x 1024 map at 0.1 m cells: the occupancy grid of BASELINE config 5 partly revealed by 512 robots at R = 50 (the known
grid of tools/geodesic_cost.py; unknown cells block).  With device events around windows of calls on one stream (warm-up first,
the legs alternating in one process) and the host's clock around the same windows:
  the waiting partition build (max_rounds = 0) beside eea_geodesic_field of the same scene, from 64 and from 4096 sources;
  eea_partition_goals at 4096 labels and at ONE label (which owns everything the others did), for the gain field (kind 0) and
  the mutual-information field (kind 1), stride 1, weights (1, 0.125): if the one-label leg is far above the 4096-label one,
  the reduction inside the wavefront is not doing its job;
  eea_partition_path_batch of 4096 robots x 64 steps, each to its own goal, beside eea_geodesic_path_batch from those goal
  cells down the same field.
Every partition must have eea_geodesic_field's cost plane bit for bit, owners -1 exactly where the cost is, every accepted source
owning its own cell unless a smaller label shares it, and areas that add up to the reached cells -- or the run fails.
usage: tools/partition_cost.py [--out FILE]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partition.txt"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("partition_cost.py measures on the GPU: none found")
    nx = ny = 1024
    res, P, warm, n_steps = 0.1, 512, 1, 64
    ccfg = capi.make_collision_cfg(0.0, 0.0, res, nx, ny, *COLL)
    rng = np.random.default_rng(7)
    poses = np.stack([rng.uniform(0.0, nx * res, P), rng.uniform(0.0, ny * res, P), rng.uniform(-3.0, 3.0, P)], 1)
    d_truth = torch.as_tensor(occupancy(nx, ny)).cuda()
    d_known = torch.full((ny, nx), -1, dtype=torch.int8, device="cuda")
    capi.sense_reveal_batch(ccfg, 50, d_truth, d_known, torch.as_tensor(poses).cuda())
    torch.cuda.synchronize()
    known = d_known.cpu().numpy()
    free = np.argwhere(known == 0)
    many = free[rng.choice(len(free), size=4096, replace=False)]
    robots = lambda cs: torch.as_tensor(np.stack([(cs[:, 1] + 0.5) * res, (cs[:, 0] + 0.5) * res, np.zeros(len(cs))], 1)).cuda()
    d_many, d_few = robots(many), robots(many[:64])
    plane = lambda: torch.empty((ny, nx), dtype=torch.int32, device="cuda")
    d_geo, d_owner, d_plain, d_one_owner = plane(), plane(), plane(), plane()
    d_ws = torch.empty(capi.partition_ws_bytes(ccfg), dtype=torch.uint8, device="cuda")
    d_gws = torch.empty(capi.geodesic_ws_bytes(ccfg), dtype=torch.uint8, device="cuda")
    d_state = torch.zeros(4, dtype=torch.int32, device="cuda")
    d_gain = torch.zeros((ny, nx), dtype=torch.int32, device="cuda")
    d_mi = torch.zeros((ny, nx), dtype=torch.float64, device="cuda")
    d_cell, d_score = torch.empty(4096, dtype=torch.int32, device="cuda"), torch.empty(4096, dtype=torch.float64, device="cuda")
    d_area = torch.empty(4096, dtype=torch.int32, device="cuda")
    d_path = torch.empty((4096, n_steps, 3), dtype=torch.float64, device="cuda")
    d_len = torch.empty(4096, dtype=torch.int32, device="cuda")
    d_plen = torch.empty(4096, dtype=torch.int32, device="cuda")
    UB = capi.GEODESIC_UNKNOWN_BLOCKS
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def build(src):
        capi.geodesic_partition(ccfg, d_known, d_geo, d_owner, d_ws, d_state, pose=src, flags=UB, stream=s)

    def plain(src):
        capi.geodesic_field(ccfg, d_known, d_plain, d_gws, d_state, pose=src, flags=UB, stream=s)

    def goals(kind, owner, n):
        capi.partition_goals(ccfg, kind, d_gain if kind == 0 else d_mi, 1, d_known, d_geo, owner, d_cell[:n], d_score[:n], d_area[:n],
                             w_field=1.0, w_cost=0.125, stream=s)

    ok, facts = True, []
    with torch.cuda.stream(stream):
        capi.sense_gain_field(ccfg, 10, 1, d_known, d_gain, stream=s)
        capi.sense_mi_field(ccfg, 10, 1, d_known, d_mi, p_unknown=0.5, stream=s)
        for name, src in (("64 sources", d_few), ("4096 sources", d_many)):
            build(src)
            stream.synchronize()
            st = d_state.cpu().numpy().view(np.uint32).copy()
            plain(src)
            stream.synchronize()
            goals(0, d_owner, src.shape[0])
            stream.synchronize()
            cost, owner, area = d_geo.cpu().numpy(), d_owner.cpu().numpy(), d_area.cpu().numpy()[:src.shape[0]]
            at = many[:src.shape[0]]
            same = bool(np.array_equal(cost, d_plain.cpu().numpy()) and np.array_equal(owner == -1, cost == -1)
                        and (owner[at[:, 0], at[:, 1]] == np.arange(len(at))).all() and (cost[at[:, 0], at[:, 1]] == 0).all()
                        and int(area.sum()) == int((owner >= 0).sum()) and st[0] == 1 and st[2] == len(at))
            ok = ok and same
            facts.append("%-14s %4d rounds changed something, %7d cells reached, largest region %6d cells, %4d goals; checks: %s"
                         % (name, int(st[1]), int((cost >= 0).sum()), int(area.max()), int((d_cell[:len(at)] >= 0).sum().item()),
                            "pass" if same else "FAIL"))
        # d_geo / d_owner hold the partition of the 4096 robots; one label that owns all of it
        d_one_owner.copy_(torch.where(d_owner >= 0, torch.zeros_like(d_owner), d_owner))
        goals(0, d_owner, 4096)
        stream.synchronize()
        # the geodesic walk beside the partition's: from each robot's goal cell down the same field (the same way, backwards, by
        # the cost-only rule); a robot without a goal stands on its own cell in both
        gc = d_cell.cpu().numpy()
        at = np.where(gc[:, None] >= 0, np.stack([gc // nx, gc % nx], 1), many)
        d_from_goal = robots(at)
        legs = [("partition build, 64 sources", lambda: build(d_few), args.calls),
                ("geodesic_field, 64 sources", lambda: plain(d_few), args.calls),
                ("partition build, 4096 sources", lambda: build(d_many), args.calls),
                ("geodesic_field, 4096 sources", lambda: plain(d_many), args.calls),
                ("goals, gain, 4096 labels", lambda: goals(0, d_owner, 4096), args.calls),
                ("goals, gain, 1 label", lambda: goals(0, d_one_owner, 1), args.calls),
                ("goals, MI, 4096 labels", lambda: goals(1, d_owner, 4096), args.calls),
                ("goals, MI, 1 label", lambda: goals(1, d_one_owner, 1), args.calls),
                ("partition paths 4096 x 64", lambda: capi.partition_path_batch(ccfg, d_geo, d_owner, d_many, d_cell, d_path, d_plen,
                                                                                stream=s), args.calls),
                ("geodesic paths 4096 x 64", lambda: capi.geodesic_path_batch(ccfg, d_geo, d_from_goal, d_path, d_len, stream=s),
                 args.calls)]
        us = {name: [] for name, _, _ in legs}
        for _, fn, n in legs:
            window(stream, fn, warm)
        for _ in range(args.windows):
            for name, fn, n in legs:
                if name.startswith("goals, gain, 4096") or name.startswith("partition paths"):
                    # (the build legs left the planes of 4096 sources; the one-label legs overwrote the goals)
                    goals(0, d_owner, 4096)
                us[name].append(window(stream, fn, n))
        stream.synchronize()
    plen = d_plen.cpu().numpy()
    lines = ["geodesic partition: cost per call of eea_geodesic_partition / eea_partition_goals / eea_partition_path_batch "
             "(tools/partition_cost.py)",
             "%s, %d x %d cells, tiles of %d x %d; known grid: BASELINE config 5, seed 2024, revealed by %d robots at R = 50 "
             "(%d cells unknown, unknown blocks)"
             % (torch.cuda.get_device_name(0), nx, ny, capi.GEODESIC_TILE_X, capi.GEODESIC_TILE_Y, P, int((known < 0).sum())),
             "device events and the host's clock, %d windows x %d calls per leg after %d warm-up call, legs alternating in one process;"
             % (args.windows, args.calls, warm),
             "median [min .. max] us per call on the device | median us per call on the host until the call returns", ""]
    lines += facts
    lines.append("paths: %d of 4096 robots have a goal and a way, %d walks of the full %d steps"
                 % (int((plen >= 0).sum()), int((plen == n_steps).sum()), n_steps))
    lines.append("")
    for name, _, _ in legs:
        dev, host = [u[0] for u in us[name]], [u[1] for u in us[name]]
        lines.append("  %-32s %11.1f  [%.1f .. %.1f] | %11.1f" % (name, float(np.median(dev)), min(dev), max(dev), float(np.median(host))))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

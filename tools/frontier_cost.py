#!/usr/bin/env python3
"""What the frontier regions cost (eea_frontier_regions, eea_frontier_goals: csrc/frontier_kernel.hip), beside one plain read
of the same bytes and beside the call whose goals they stand next to.

The scene of tools/partition_cost.py: one 1024 x 1024 map at 0.1 m cells, the occupancy grid of BASELINE config 5 partly
revealed by 512 robots at R = 50, partitioned from 4096 sources (unknown cells block).  With device events around windows of
calls on one stream (warm-up first, the legs alternating in one process) and the host's clock around the same windows:
  eea_frontier_regions of the known grid with d_geo / d_owner and without;
  eea_grid_census of the same grid: one plain read pass over the same bytes;
  EEA_FRONTIER_OF_MASK on a checkerboard of the same size (the most unions, and ONE region that owns every member) and on
  isolated cells, one in every 2 x 2 block (the most regions): if the one-region leg is far above the many-region leg per
  member cell, the combine inside the wavefront is not doing its job;
  eea_frontier_goals at 4096 robots beside eea_partition_goals at 4096 labels.
Every labelling must obey, by a torch-side check: root <= cell and root[root] == root on the members, -1 on both planes
elsewhere, the records' sizes add up to d_state[2], and the ranks ascend with the roots -- or the run fails.
usage: tools/frontier_cost.py [--out FILE]"""
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

RECORD_BYTES = 56


def invariants(d_root, d_region, d_rec, d_state, max_regions):
    """the torch-side check of one labelling; (ok, regions, members, largest region)"""
    root, region = d_root.reshape(-1).long(), d_region.reshape(-1).long()
    state = d_state.cpu().numpy().view(np.uint32)
    n, kept, members = int(state[0]), int(state[1]), int(state[2])
    cell = torch.arange(root.numel(), device=root.device)
    m = root >= 0
    ok = bool(((region >= 0) == m).all()) and int(m.sum()) == members and state[3] == 0 and kept == min(n, max_regions)
    ok = ok and bool((root[m] <= cell[m]).all()) and bool((root[root[m]] == root[m]).all())
    roots = cell[m & (root == cell)]                                         # ascending
    ok = ok and roots.numel() == n and bool((region[roots] == torch.arange(n, device=root.device)).all())
    ok = ok and bool((region[m] == region[root[m]]).all())
    rec = d_rec.cpu().numpy()[:kept * RECORD_BYTES].view(np.dtype([("sums", "<u8", 2), ("entry", "<i4", 2), ("root", "<i4"), ("size", "<u4"),
                                                                   ("box", "<i4", 4), ("owner", "<i4"), ("reserved", "<i4")]))
    sizes = rec["size"].astype(np.int64)
    ok = ok and int(sizes.sum()) == int((m & (region < kept)).sum()) and (kept < n or int(sizes.sum()) == members)
    ok = ok and np.array_equal(rec["root"], roots[:kept].cpu().numpy())
    return ok, n, members, int(sizes.max()) if kept else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier.txt"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5, help="calls per timed window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frontier_cost.py measures on the GPU: none found")
    nx = ny = 1024
    res, P, warm, robots_n = 0.1, 512, 1, 4096
    max_regions = nx * ny // 4
    ccfg = capi.make_collision_cfg(0.0, 0.0, res, nx, ny, *COLL)
    rng = np.random.default_rng(7)
    poses = np.stack([rng.uniform(0.0, nx * res, P), rng.uniform(0.0, ny * res, P), rng.uniform(-3.0, 3.0, P)], 1)
    d_truth = torch.as_tensor(occupancy(nx, ny)).cuda()
    d_known = torch.full((ny, nx), -1, dtype=torch.int8, device="cuda")
    capi.sense_reveal_batch(ccfg, 50, d_truth, d_known, torch.as_tensor(poses).cuda())
    torch.cuda.synchronize()
    known = d_known.cpu().numpy()
    free = np.argwhere(known == 0)
    many = free[rng.choice(len(free), size=robots_n, replace=False)]
    d_many = torch.as_tensor(np.stack([(many[:, 1] + 0.5) * res, (many[:, 0] + 0.5) * res, np.zeros(len(many))], 1)).cuda()
    i, j = np.indices((ny, nx))
    d_checker = torch.as_tensor(((i + j) % 2 == 0).astype(np.int8)).cuda()
    d_isolated = torch.as_tensor(((i % 2 == 0) & (j % 2 == 0)).astype(np.int8)).cuda()
    plane = lambda: torch.empty((ny, nx), dtype=torch.int32, device="cuda")
    d_geo, d_owner, d_root, d_region = plane(), plane(), plane(), plane()
    d_pws = torch.empty(capi.partition_ws_bytes(ccfg), dtype=torch.uint8, device="cuda")
    d_ws = torch.empty(capi.frontier_ws_bytes(ccfg), dtype=torch.uint8, device="cuda")
    d_rec = torch.empty(max_regions * RECORD_BYTES, dtype=torch.uint8, device="cuda")
    d_state, d_pstate = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    d_counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    d_gain = torch.zeros((ny, nx), dtype=torch.int32, device="cuda")
    d_cell, d_greg = torch.empty(robots_n, dtype=torch.int32, device="cuda"), torch.empty(robots_n, dtype=torch.int32, device="cuda")
    d_score, d_area = torch.empty(robots_n, dtype=torch.float64, device="cuda"), torch.empty(robots_n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def label(kind, grid, planes):
        capi.frontier_regions(ccfg, kind, grid, d_root, d_region, d_ws, d_state, regions=d_rec, max_regions=max_regions,
                              geo=d_geo if planes else None, owner=d_owner if planes else None, stream=s)

    scenes = [("frontier, d_geo / d_owner", capi.FRONTIER_OF_GRID, d_known, True), ("frontier, no planes", capi.FRONTIER_OF_GRID, d_known, False),
              ("mask, checkerboard", capi.FRONTIER_OF_MASK, d_checker, False), ("mask, isolated cells", capi.FRONTIER_OF_MASK, d_isolated, False)]
    ok, facts, members_of = True, [], {}
    with torch.cuda.stream(stream):
        capi.geodesic_partition(ccfg, d_known, d_geo, d_owner, d_pws, d_pstate, pose=d_many, flags=capi.GEODESIC_UNKNOWN_BLOCKS, stream=s)
        capi.sense_gain_field(ccfg, 10, 1, d_known, d_gain, stream=s)
        stream.synchronize()
        for name, kind, grid, planes in scenes:
            label(kind, grid, planes)
            stream.synchronize()
            good, n, members, largest = invariants(d_root, d_region, d_rec, d_state, max_regions)
            ok = ok and good
            members_of[name] = members
            facts.append("%-28s %7d regions, %7d member cells, largest region %7d cells; checks: %s"
                         % (name, n, members, largest, "pass" if good else "FAIL"))

        def goals():
            capi.frontier_goals(d_rec, d_state, max_regions, d_cell, d_greg, d_score, min_size=2, w_size=1.0, w_cost=0.125, stream=s)

        def cell_goals():
            capi.partition_goals(ccfg, 0, d_gain, 1, d_known, d_geo, d_owner, d_cell, d_score, d_area, w_field=1.0, w_cost=0.125, stream=s)

        legs = [(name, (lambda k=kind, g=grid, p=planes: label(k, g, p))) for name, kind, grid, planes in scenes]
        legs.insert(2, ("grid_census (one read pass)", lambda: capi.grid_census(ccfg, d_known, d_counts, stream=s)))
        legs += [("frontier_goals, 4096 robots", goals), ("partition_goals, 4096 labels", cell_goals)]
        us = {name: [] for name, _ in legs}
        for name, fn in legs:
            if name.startswith("frontier_goals"):
                label(*scenes[0][1:])                                        # (the mask legs overwrote the records)
            window(stream, fn, warm)
        for _ in range(args.windows):
            for name, fn in legs:
                if name.startswith("frontier_goals"):
                    label(*scenes[0][1:])
                us[name].append(window(stream, fn, args.calls))
        stream.synchronize()
        goals()
        stream.synchronize()
        with_goal = int((d_cell >= 0).sum().item())
    lines = ["frontier regions: cost per call of eea_frontier_regions / eea_frontier_goals (tools/frontier_cost.py)",
             "%s, %d x %d cells, tiles of %d x %d; known grid: BASELINE config 5, seed 2024, revealed by %d robots at R = 50 "
             "(%d cells unknown), partition from %d sources (unknown blocks); room for %d records"
             % (torch.cuda.get_device_name(0), nx, ny, capi.GEODESIC_TILE_X, capi.GEODESIC_TILE_Y, P, int((known < 0).sum()), robots_n,
                max_regions),
             "device events and the host's clock, %d windows x %d calls per leg after %d warm-up call, legs alternating in one process;"
             % (args.windows, args.calls, warm),
             "median [min .. max] us per call on the device | median us per call on the host until the call returns", ""]
    lines += facts
    lines.append("goals: %d of %d robots own the entry of a region of at least 2 cells" % (with_goal, robots_n))
    lines.append("")
    med = {}
    for name, _ in legs:
        dev, host = [u[0] for u in us[name]], [u[1] for u in us[name]]
        med[name] = float(np.median(dev))
        lines.append("  %-30s %11.1f  [%.1f .. %.1f] | %11.1f" % (name, med[name], min(dev), max(dev), float(np.median(host))))
    one, lots = "mask, checkerboard", "mask, isolated cells"
    per_one, per_lots = med[one] * 1e3 / members_of[one], med[lots] * 1e3 / members_of[lots]
    lines += ["", "per member cell: one region (checkerboard) %.3f ns, one region per member (isolated cells) %.3f ns: ratio %.2f"
              % (per_one, per_lots, per_one / per_lots)]
    if per_one > 4.0 * per_lots:
        lines.append("THE ONE-REGION LEG IS FAR ABOVE THE MANY-REGION LEG PER MEMBER CELL: the combine inside the wavefront is not doing its job")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

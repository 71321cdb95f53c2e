#!/usr/bin/env python3
"""What the goal paths cost (eea_geodesic_goto_batch: csrc/goto_kernel.hip), beside the only route a goal from elsewhere had to a
path before it -- one whole-grid eea_geodesic_field per goal plus eea_geodesic_path_batch, existing code that this tool only
calls -- and beside one frontier auction round, for scale.

The scene of tools/frontier_cost.py and tools/auction_cost.py: one 1024 x 1024 map at 0.1 m cells, the occupancy grid of BASELINE
config 5 partly revealed by 512 robots at R = 50, 4096 robots on known free cells (unknown cells block), the frontier labelled
once; the goals are the goal cells of one eea_frontier_auction round (-1 for a robot it left without one: status NO_GOAL).  With
device events around windows of calls on one stream (warm-up first, the legs alternating in one process) and the host's clock
around the same windows:
  (a) eea_geodesic_goto_batch for the 4096 robots at margin 8, 16 and 32, with the four counts;
  (b) eea_geodesic_field(cells = [g]) + eea_geodesic_path_batch for 16 sampled robots that have a goal, in the budgeted form
      with the smallest of 32, 64, ... tile rounds that ends every one of the 16 builds final; per goal, and x 4096;
  (c) one eea_frontier_auction round in the budgeted form;
  (d) by window size: 4096 robots on an all-free grid of the same size whose goals lie (31, 31) and (127, 127) cells away at
      margin 0 -- windows of exactly 32 x 32 and 128 x 128 cells, every robot's path the diagonal.
Before any timing, by a torch-side check: the four counts add up to the robots and are the statuses'; cost >= 0 exactly for status
OK; an OK robot's cost is at least the auction's cost to the same cell (the auction's graph holds the window's) and, at margin 32,
at least the whole-grid field's for the sampled robots and equal to it for most; the free-grid legs cost 7 x 31 and 7 x 127 -- or
the run fails.
With --ab-lib FILE (a build of the same sources with EXTRA=-DEEA_GOTO_PRUNE=0 VARIANT=_noprune) the legs (a) and (d) are timed
through that library too, alternating with the product's in the same windows, and its answers must be the product's bit for bit.
usage: tools/goto_cost.py [--out FILE] [--ab-lib FILE] [--resources "$(tools/goto_cost.py --print-resources)"]"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ergodic_exploration_amd import capi  # noqa: E402
from auction_cost import CELLS_PER_ROBOT, MIN_SIZE, N_STEPS, Scene  # noqa: E402
from gain_cost import window  # noqa: E402

MARGINS = (8, 16, 32)
SAMPLED = 16
LDS_PER_CU = 160 * 1024


def resources():
    """the kernel's registers and LDS from the code object of the build, or a reason"""
    import kernel_resources as kr
    obj = os.path.join(os.path.dirname(capi.LIB_PATH), "..", "csrc", "build", "goto_kernel.o")
    if not os.path.exists(obj):
        return "goto_kernel: no object file beside the library (built elsewhere): resources not read"
    for k in kr.kernels(obj):
        name = subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.strip()
        if "vgpr_count" in k and "goto_kernel(" in name:
            static = int(k["group_segment_fixed_size"])
            out = "goto_kernel: %s VGPRs, %s SGPRs, scratch %s B, static LDS %d B; dynamic LDS 4 B per cell of the largest window:" % (
                k["vgpr_count"], k["sgpr_count"], k["private_segment_fixed_size"], static)
            for cells in (1024, 4096, 16384):
                lds = static + 4 * cells
                out += " %d cells %d B (%d workgroups per CU by LDS, at most 8 by wavefronts)" % (cells, lds, min(8, LDS_PER_CU // lds))
            return out
    return "goto_kernel: not found in the object file"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "goto.txt"))
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed window")
    ap.add_argument("--print-resources", action="store_true", help="print the kernel's resources from the build's object file and exit (no GPU)")
    ap.add_argument("--resources", default=None, help="that line, for a run where the object file is not beside the library")
    args = ap.parse_args()
    if args.print_resources:
        print(resources())
        return
    if not torch.cuda.is_available():
        sys.exit("goto_cost.py measures on the GPU: none found")
    sc = Scene()
    P, nx, ny, s = sc.robots_n, sc.nx, sc.ny, sc.s
    ints = lambda n: torch.empty(n, dtype=torch.int32, device="cuda")
    d_cost, d_status, d_len, d_state = ints(P), ints(P), ints(P), torch.zeros(4, dtype=torch.int32, device="cuda")
    d_path = torch.empty((P, N_STEPS, 3), dtype=torch.float64, device="cuda")
    d_free = torch.zeros((ny, nx), dtype=torch.int8, device="cuda")
    d_geo1 = torch.empty((ny, nx), dtype=torch.int32, device="cuda")
    d_gws = torch.empty(capi.geodesic_ws_bytes(sc.ccfg), dtype=torch.uint8, device="cuda")
    d_gstate = torch.zeros(4, dtype=torch.int32, device="cuda")
    d_path1, d_len1 = torch.empty((1, N_STEPS, 3), dtype=torch.float64, device="cuda"), ints(1)
    alt = None
    if args.ab_lib:
        alt = C.CDLL(os.path.abspath(args.ab_lib))
        alt.eea_geodesic_goto_batch.argtypes = capi.lib().eea_geodesic_goto_batch.argtypes
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def goto(grid, pose, goal, margin, flags, lib=None):
        if lib is None:
            capi.geodesic_goto_batch(sc.ccfg, grid, pose, goal, d_cost, d_status, d_state, path=d_path, length=d_len, flags=flags,
                                     margin=margin, stream=s)
        else:
            st = lib.eea_geodesic_goto_batch(0, C.byref(sc.ccfg), ptr(grid), None, 0, flags, ptr(pose), ptr(goal), None, P, margin, N_STEPS,
                                             ptr(d_cost), ptr(d_status), ptr(d_path), ptr(d_len), ptr(d_state), C.c_void_p(s))
            assert st == 0, st

    def answer():
        return [t.clone() for t in (d_cost, d_status, d_len, d_path, d_state)]

    ok, facts = True, []
    with torch.cuda.stream(sc.stream):
        sc.partition(0)
        sc.label()
        sc.stream.synchronize()
        a_budget = sc.smallest_budget(lambda b: sc.auction(1, b), sc.d_astate)
        d_goal, auction_cost = sc.d_cell.clone(), sc.d_cost.clone()
        have = d_goal >= 0
        facts.append("auction round: %d of %d robots have a goal (budget %d tile rounds)" % (int(have.sum()), P, a_budget))
        # the robots' cells (they stand on cell centres)
        ci, cj = (sc.d_many[:, 1] / sc.res).floor().long(), (sc.d_many[:, 0] / sc.res).floor().long()
        gi, gj = torch.div(d_goal.long(), nx, rounding_mode="floor"), d_goal.long() % nx
        # (d): goals a fixed offset away on the free grid, from cells that leave room for it
        rng = np.random.default_rng(11)
        free_legs = {}
        for side in (32, 128):
            at = rng.integers(0, nx - side, size=(P, 2))
            pose = torch.as_tensor(np.stack([(at[:, 1] + 0.5) * sc.res, (at[:, 0] + 0.5) * sc.res, np.zeros(P)], 1)).cuda()
            goal = torch.as_tensor(((at[:, 0] + side - 1) * nx + at[:, 1] + side - 1).astype(np.int32)).cuda()
            free_legs[side] = (pose, goal)
        # ---- the checks, before any timing ----
        answers = {}
        for m in MARGINS:
            goto(sc.d_known, sc.d_many, d_goal, m, capi.GEODESIC_UNKNOWN_BLOCKS)
            sc.stream.synchronize()
            answers[m] = answer()
            st = d_state.cpu().numpy().view(np.uint32)
            counts = [int((d_status == k).sum()) for k in range(5)]
            good = int(st.sum()) == P and st.tolist() == [counts[0], counts[3], counts[4], counts[1] + counts[2]]
            good = good and bool(((d_cost >= 0) == (d_status == 0)).all()) and bool(((d_status == 2) == ~have).all())
            okm = d_status == 0
            good = good and bool((d_cost[okm] >= auction_cost[okm]).all()) and bool(((d_len[okm] >= 0) & (d_len[okm] <= N_STEPS)).all())
            h = (torch.maximum(ci, gi) + m).clamp(max=ny - 1) - (torch.minimum(ci, gi) - m).clamp(min=0) + 1
            w = (torch.maximum(cj, gj) + m).clamp(max=nx - 1) - (torch.minimum(cj, gj) - m).clamp(min=0) + 1
            cells = (h * w)[have].double()
            ok = ok and good
            facts.append("margin %2d: OK %4d, WINDOW %4d, CUT_OFF %4d, no robot / no goal %4d; of the OK robots %4d at the auction's cost; "
                         "window cells of the robots with a goal: median %d, mean %d, max %d; checks: %s"
                         % (m, st[0], st[1], st[2], st[3], int((d_cost[okm] == auction_cost[okm]).sum()), int(cells.median()), int(cells.mean()),
                            int(cells.max()), "pass" if good else "FAIL"))
        for side, (pose, goal) in free_legs.items():
            goto(d_free, pose, goal, 0, 0)
            sc.stream.synchronize()
            answers[-side] = answer()
            good = bool((d_status == 0).all()) and bool((d_cost == 7 * (side - 1)).all()) and d_state.cpu().numpy().tolist() == [P, 0, 0, 0]
            ok = ok and good
            facts.append("free grid, windows of %3d x %3d cells: every cost %d; checks: %s" % (side, side, 7 * (side - 1), "pass" if good else "FAIL"))
        if alt is not None:
            same = True
            for m in MARGINS:
                goto(sc.d_known, sc.d_many, d_goal, m, capi.GEODESIC_UNKNOWN_BLOCKS, alt)
                sc.stream.synchronize()
                same = same and all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(answer(), answers[m]))
            for side, (pose, goal) in free_legs.items():
                goto(d_free, pose, goal, 0, 0, alt)
                sc.stream.synchronize()
                same = same and all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(answer(), answers[-side]))
            ok = ok and same
            facts.append("the library without the pruning gives the same bits: %s" % ("pass" if same else "FAIL"))
        # (b): 16 sampled robots with a goal
        picks = torch.nonzero(have).reshape(-1)[torch.as_tensor(rng.choice(int(have.sum()), size=SAMPLED, replace=False)).cuda()].tolist()
        one_goal = [d_goal[q:q + 1].clone() for q in picks]
        one_pose = [sc.d_many[q:q + 1].clone() for q in picks]

        def route(k, budget):
            capi.geodesic_field(sc.ccfg, sc.d_known, d_geo1, d_gws, d_gstate, cells=one_goal[k], flags=capi.GEODESIC_UNKNOWN_BLOCKS,
                                max_rounds=budget, stream=s)
            capi.geodesic_path_batch(sc.ccfg, d_geo1, one_pose[k], d_path1, d_len1, stream=s)

        g_budget = 32
        while g_budget < 1 << 14:
            final = True
            for k in range(SAMPLED):
                route(k, g_budget)
                sc.stream.synchronize()
                final = final and int(d_gstate[0].item()) == 1
            if final:
                break
            g_budget *= 2
        equal = 0
        for k, q in enumerate(picks):
            route(k, g_budget)
            sc.stream.synchronize()
            whole = int(d_geo1[int(ci[q]), int(cj[q])].item())
            mine, status = int(answers[32][0][q].item()), int(answers[32][1][q].item())
            good = whole >= 0 and (mine >= whole if status == 0 else status in (3, 4))
            if status == 0 and mine == whole:
                equal += 1 if torch.equal(answers[32][3][q], d_path1[0]) else 0
            ok = ok and good
        facts.append("the %d sampled robots against the whole-grid field (budget %d tile rounds): %d with the same cost and the same path "
                     "at margin 32; checks: %s" % (SAMPLED, g_budget, equal, "pass" if ok else "FAIL"))
        ok = ok and equal >= SAMPLED // 2

        def all_routes():
            for k in range(SAMPLED):
                route(k, g_budget)

        # ---- the timing ----
        legs = []
        for m in MARGINS:
            legs.append(("(a) goto_batch, margin %d" % m, (lambda m=m: goto(sc.d_known, sc.d_many, d_goal, m, capi.GEODESIC_UNKNOWN_BLOCKS))))
            if alt is not None:
                legs.append(("    ... without the pruning", (lambda m=m: goto(sc.d_known, sc.d_many, d_goal, m, capi.GEODESIC_UNKNOWN_BLOCKS, alt))))
        legs.append(("(b) field + path, %d goals" % SAMPLED, all_routes))
        legs.append(("(c) auction, one round", lambda: sc.auction(1, a_budget)))
        for side, (pose, goal) in free_legs.items():
            legs.append(("(d) goto_batch, %d x %d windows" % (side, side), (lambda p=pose, g=goal: goto(d_free, p, g, 0, 0))))
            if alt is not None:
                legs.append(("    ... without the pruning ", (lambda p=pose, g=goal: goto(d_free, p, g, 0, 0, alt))))
        names = ["%s#%d" % (n, k) for k, (n, _) in enumerate(legs)]
        us = {n: [] for n in names}
        for _, fn in legs:
            window(sc.stream, fn, 1)
        for _ in range(args.windows):
            for n, (_, fn) in zip(names, legs):
                us[n].append(window(sc.stream, fn, args.calls))
        sc.stream.synchronize()
    lines = ["goal paths: cost per call of eea_geodesic_goto_batch (tools/goto_cost.py)",
             "%s, %d x %d cells; known grid: BASELINE config 5, seed 2024, revealed by %d robots at R = 50 (%d cells unknown), %d robots on "
             "known free cells, unknown cells block; goals: the goal cells of one eea_frontier_auction round (min_size %d, %d cells per "
             "robot); n_steps %d" % (torch.cuda.get_device_name(0), nx, ny, sc.P, sc.unknown, P, MIN_SIZE, CELLS_PER_ROBOT, N_STEPS),
             "device events and the host's clock, %d windows x %d calls per leg after 1 warm-up call, legs alternating in one process;"
             % (args.windows, args.calls),
             "median [min .. max] us per call on the device | median us per call on the host until the call returns", "",
             args.resources or resources(), ""]
    lines += facts
    lines.append("")
    med = {}
    for n, (label, _) in zip(names, legs):
        dev, host = [u[0] for u in us[n]], [u[1] for u in us[n]]
        med[n] = float(np.median(dev))
        lines.append("  %-36s %11.1f  [%.1f .. %.1f] | %11.1f" % (label, med[n], min(dev), max(dev), float(np.median(host))))
    by_label = {label: med[n] for n, (label, _) in zip(names, legs)}
    per_goal = by_label["(b) field + path, %d goals" % SAMPLED] / SAMPLED
    lines += ["", "(b) per goal: %.1f us; x %d goals: %.0f us" % (per_goal, P, per_goal * P)]
    n_goal = int(have.sum())
    for m in MARGINS:
        t = by_label["(a) goto_batch, margin %d" % m]
        lines.append("(a) margin %2d: %.1f us per call = %.3f us per robot with a goal; (a) / (b x %d) = %.5f; (a) / (b x the %d robots with a goal) "
                     "= %.5f" % (m, t, t / max(n_goal, 1), P, t / (per_goal * P), n_goal, t / (per_goal * max(n_goal, 1))))
    for side in free_legs:
        t = by_label["(d) goto_batch, %d x %d windows" % (side, side)]
        lines.append("(d) %3d x %3d windows: %.1f us per call of %d robots = %.3f us per robot" % (side, side, t, P, t / P))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

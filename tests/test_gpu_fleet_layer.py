"""The fleet layer on the device (include/ergodic_amd.h: eea_fleet_layer_*, eea_fleet_collision_check_batch,
eea_tick_batch_fleet; csrc/fleet_layer_kernel.hip and the layer instances of csrc/collision_kernel.hip): the robots of a fleet
as obstacles to one another.

Checkers: the counts and the cell table against the numpy restatement of the rule (tests/fleet_layer_restatement.py),
exactly; the collision verdicts against the CPU oracle's collisionCheck on a grid of its own per robot (the other robots'
bodies as occupied cells), bit for bit, through the inflated map and the ring search; the fleet tick against independent
oracle loops on per-robot grids rebuilt every tick, with the assertions of tests/test_gpu_fleet_tick.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pyoracle as po
from ergodic_exploration_amd import capi
from tests import fleet_layer_restatement as fr
from tests.test_host_mirror import DWA

pytestmark = pytest.mark.gpu

SOURCES = ["ergodic", "dwa-follow", "dwa-reference", "dwa-replan"]
R_BND, R_COL, R_MAX = fr.radii(fr.COLL_S, fr.RES)


def dev(a, t=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=t).cuda()


def _cfg(xmin, ymin, xsize, ysize):
    return capi.make_collision_cfg(xmin, ymin, fr.RES, xsize, ysize, *fr.COLL_S)


def _centre(xmin, ymin, x, y):
    """a pose in the middle of cell (x, y)"""
    return [xmin + (x + 0.5) * fr.RES, ymin + (y + 0.5) * fr.RES, 0.0]


@pytest.mark.parametrize("body", [R_BND, 0])
def test_counts_and_cells_equal_the_restatement(body):
    """150 x 40 cells, reach 10 (body 4) or 6: a padded row of 170 / 162 centres -- three passes of the row scan, the last
    one partial -- and 70 robots, more than one wavefront of stamps: masked ones, two in one cell, robots in every corner and
    on the edges (their spans reach the first and the last column of the map), robots outside the grid on every side
    (negative coordinates wrap and fail the bounds).  A second update with moved robots leaves no stale count."""
    xmin, ymin, xs, ys, B = -1.0, -0.5, 150, 40, 70
    g = fr.sr.Geometry(xmin, ymin, fr.RES, xs, ys, fr.COLL_S[3])
    reach = R_COL + body
    F = fr.offset_set(R_BND, R_COL, R_MAX, body)
    rng = np.random.default_rng(3)
    poses = np.stack([rng.uniform(xmin, xmin + xs * fr.RES, B), rng.uniform(ymin, ymin + ys * fr.RES, B), rng.uniform(-3, 3, B)], 1)
    for k, (x, y) in enumerate([(0, 0), (xs - 1, 0), (0, ys - 1), (xs - 1, ys - 1), (75, 0), (0, 20), (xs - 1, 21), (76, ys - 1)]):
        poses[k] = _centre(xmin, ymin, x, y)
    poses[8] = poses[9] = _centre(xmin, ymin, 40, 17)                   # two robots in one cell
    poses[10, :2] = (xmin - 0.01, 0.3)                                  # outside: negative cell indices wrap
    poses[11, :2] = (1.0, ymin - 2.0)
    poses[12, :2] = (xmin + xs * fr.RES + 0.07, 0.3)                    # outside, beyond the upper edges
    poses[13, :2] = (1.0, ymin + ys * fr.RES + 0.3)
    poses[14, :2] = (xmin + xs * fr.RES, ymin + ys * fr.RES)            # exactly on the upper edges: the last cell
    mask = np.ones(B, dtype=np.int32)
    mask[[3, 20, 21, 30, 64, 69]] = 0
    layer = capi.FleetLayer(_cfg(xmin, ymin, xs, ys), body, B)
    try:
        assert layer.reach == reach and layer.shape == (ys + 2 * reach, xs + 2 * reach)
        assert layer.shape[1] > 128 and layer.shape[1] % 64 != 0
        count, cell = layer.read()                                      # before the first update: nobody is an obstacle
        assert not count.any() and (cell == fr.NOT_STAMPED).all()
        moved = poses.copy()
        moved[:, :2] += rng.uniform(-0.4, 0.4, (B, 2))
        for p, m in ((poses, mask), (moved, None), (poses, np.zeros(B, dtype=np.int32))):
            layer.update(dev(p), None if m is None else dev(m, torch.int32))
            count, cell = layer.read()
            want_cell = fr.cells_of(g, p, m)
            assert np.array_equal(cell, want_cell)
            assert np.array_equal(count, fr.counts(g, F, reach, want_cell))
        first = fr.cells_of(g, poses, mask)
        assert (first[[3, 10, 11, 12, 13, 30]] == fr.NOT_STAMPED).all() and tuple(first[14]) == (xs - 1, ys - 1)
        assert tuple(first[8]) == tuple(first[9]) == (40, 17) and (first[:8] != fr.NOT_STAMPED).sum() == 14
        # two stamped robots in one cell: both ends of every span meet on the same words -- each of them counts twice over F
        layer.update(dev(poses), dev(mask, torch.int32))
        count, _ = layer.read()
        want = fr.counts(g, F, reach, first)
        assert np.array_equal(count, want)
        lone = first.copy()
        lone[9] = fr.NOT_STAMPED
        assert (want - fr.counts(g, F, reach, lone)).sum() == len(F)
        for (dx, dy) in [(0, 0), (R_COL + body, 0), (0, -R_BND), (-R_COL, 0)]:
            assert ((dx, dy) in F) <= (count[17 + dy + reach, 40 + dx + reach] >= 2), (dx, dy)
        assert (R_COL + body, 0) in F and ((0, 0) in F) == (body >= R_BND)
    finally:
        layer.close()


@pytest.fixture(scope="module")
def check_scene():
    """13 robots on 64 x 48 cells with two static blocks -- two of them in one cell, one masked, one outside the grid --,
    every stamped robot at least `body` = 4 cells inside; the poses: the centre
    of every cell of the window of reach + 2 cells around every robot (windows spill over the grid's edges: wrapped cells).
    The oracle's verdicts are computed once: on the robot's own grid (the pose is the robot's) and on the grid that holds
    every robot's body (the pose is nobody's)."""
    xmin, ymin, xs, ys, body = -0.7, -0.3, 64, 48, R_BND
    reach = R_COL + body
    data = np.zeros((ys, xs), dtype=np.int8)
    data[20:24, 30:33] = 100
    data[40:42, 5:20] = 90
    data[10, 50] = 70                                                    # below the threshold of 0.8: free
    cells = np.array([(4, 4), (59, 43), (4, 43), (59, 4), (30, 12), (36, 14), (31, 30), (12, 25), (13, 25), (50, 24),
                      (36, 14), (45, 36), (-3, 20)])
    robots = np.array([_centre(xmin, ymin, x, y) for (x, y) in cells])
    mask = np.ones(len(cells), dtype=np.int32)
    mask[11] = 0                      # robot 11 is masked and robot 12 stands outside the grid: no obstacles, but poses of theirs
    geom = fr.sr.Geometry(xmin, ymin, fr.RES, xs, ys, fr.COLL_S[3])
    stamped = fr.cells_of(geom, robots, mask)
    assert (stamped[[11, 12]] == fr.NOT_STAMPED).all() and np.array_equal(stamped[:11], cells[:11])
    assert tuple(stamped[5]) == tuple(stamped[10])      # two robots in one cell: each sees the other's body, not its own
    pose, owner = [], []
    for b, (x, y) in enumerate(cells):
        for dy in range(-reach - 2, reach + 3):
            for dx in range(-reach - 2, reach + 3):
                pose.append(_centre(xmin, ymin, x + dx, y + dy))
                owner.append(b)
    pose, owner = np.array(pose), np.array(owner, dtype=np.int32)
    grid_of = lambda d: po.GridMap(xmin, xmin + xs * fr.RES, ymin, ymin + ys * fr.RES, fr.RES, d.reshape(-1))
    own_grids = [grid_of(fr.robot_grid(data, stamped, b, body)) for b in range(len(cells))]
    all_grid = grid_of(fr.robot_grid(data, stamped, -1, body))
    want_own = np.array([po.collision_check(fr.COLL_S, own_grids[b], p)[0] for p, b in zip(pose, owner)], dtype=np.int32)
    want_all = np.array([po.collision_check(fr.COLL_S, all_grid, p)[0] for p in pose], dtype=np.int32)
    want_static = np.array([po.collision_check(fr.COLL_S, grid_of(data), p)[0] for p in pose], dtype=np.int32)
    assert 0 < want_own.sum() < want_all.sum() < len(pose) and (want_own != want_static).any()
    # the poses of the robots that are no obstacles see every body, as nobody's poses do
    assert np.array_equal(want_own[owner >= 11], want_all[owner >= 11]) and want_own[owner == 11].any()
    # at the shared cell a robot of the pair is hit by its twin (body >= r_bnd: (0, 0) in F)
    assert want_own[(owner == 5) & (pose[:, 0] == robots[5, 0]) & (pose[:, 1] == robots[5, 1])].tolist() == [1]
    return dict(cfg=_cfg(xmin, ymin, xs, ys), body=body, data=data, robots=robots, mask=mask, pose=pose, owner=owner, want_own=want_own,
                want_all=want_all, want_static=want_static)


@pytest.mark.parametrize("impl", [1, 2])
def test_collision_check_equals_the_oracle_on_per_robot_grids(check_scene, impl):
    s = check_scene
    layer = capi.FleetLayer(s["cfg"], s["body"], len(s["robots"]))
    try:
        capi.set_option(capi.OPT_COLLISION_IMPL, impl)
        layer.update(dev(s["robots"]), dev(s["mask"], torch.int32))
        d_grid, d_pose = dev(s["data"], torch.int8), dev(s["pose"])
        hit = torch.full((len(s["pose"]),), -7, dtype=torch.int32, device="cuda")
        layer.collision_check(d_grid, d_pose, hit, self_index=dev(s["owner"], torch.int32))
        assert np.array_equal(hit.cpu().numpy(), s["want_own"])
        for nobody in (None, torch.full((len(s["pose"]),), -1, dtype=torch.int32, device="cuda")):
            hit.fill_(-7)
            layer.collision_check(d_grid, d_pose, hit, self_index=nobody)
            assert np.array_equal(hit.cpu().numpy(), s["want_all"])
        # robots only: the static blocks drop out -- what is left are the verdicts of an empty grid with the bodies
        hit.fill_(-7)
        layer.collision_check(None, d_pose, hit, self_index=dev(s["owner"], torch.int32))
        got = hit.cpu().numpy()
        assert ((got == 1) <= (s["want_own"] == 1)).all() and np.array_equal(got | s["want_static"], s["want_own"])
    finally:
        capi.set_option(capi.OPT_COLLISION_IMPL, 0)
        layer.close()


@pytest.mark.parametrize("body", [R_BND, 0])
def test_a_lone_robot_sees_the_static_verdict_only(check_scene, body):
    """with d_self = itself the layer changes nothing; as nobody's pose the robot's own cell is hit iff (0, 0) in F"""
    s = check_scene
    layer = capi.FleetLayer(s["cfg"], body, 1)
    try:
        layer.update(dev(s["robots"][4:5]))
        sel = s["owner"] == 4
        pose = np.concatenate([s["robots"][4:5], s["pose"][sel]])
        d_pose = dev(pose)
        hit = torch.full((len(pose),), -7, dtype=torch.int32, device="cuda")
        layer.collision_check(dev(s["data"], torch.int8), d_pose, hit, self_index=torch.zeros(len(pose), dtype=torch.int32, device="cuda"))
        got = hit.cpu().numpy()
        assert got[0] == 0 and np.array_equal(got[1:], s["want_static"][sel])
        layer.collision_check(None, d_pose, hit, self_index=None)
        got = hit.cpu().numpy()
        assert ((0, 0) in fr.offset_set(R_BND, R_COL, R_MAX, body)) == (body >= R_BND) == bool(got[0])
        assert got.sum() > 1
    finally:
        layer.close()


def _engine(model):
    em = {"omni": capi.MODEL_OMNI, "simple_cart": capi.MODEL_SIMPLE_CART}[model]
    Rinv, lim = fr.model_limits(model)
    eng = capi.Engine(capi.make_config(em, 0.1, 5.0, 0.1, 1.0, 10, Rinv, -lim, lim))
    eng.set_target_gaussians(fr.MEANS, fr.SIGMAS)
    eng.config_domain(fr.BOUNDS)
    return eng


class _TickState:
    def __init__(self, B, T, fill=0):
        z = lambda *s, dt=torch.float64, v=0: torch.full(s, v, dtype=dt, device="cuda")
        self.ut, self.u = z(B, T, 3), z(B, 3)
        self.follow, self.count = z(B, dt=torch.int32), z(B, dt=torch.int32)
        self.traj = z(B, T, 3, v=fill)
        self.valid, self.skip = z(B, dt=torch.int32, v=fill), z(B, dt=torch.int32, v=fill)
        self.source, self.status = z(B, dt=torch.int32, v=-1), z(B, dt=torch.int32, v=-1)

    def tensors(self):
        return dict(ut=self.ut, u=self.u, follow=self.follow, count=self.count, traj=self.traj, valid=self.valid, skip=self.skip,
                    source=self.source, status=self.status)

    def tick(self, eng, layer, B, pose, vb, grid, ccfg, dcfg, mem=None, n_mem=None, mem_stride=0):
        args = (B, pose, self.ut, self.follow, self.count, self.u, vb, grid, self.traj, self.valid, self.skip, ccfg, dcfg,
                fr.VAL_DT, fr.VAL_HORIZON)
        kw = dict(source=self.source, mem_cols=mem, n_mem=n_mem, mem_stride=mem_stride, status=self.status)
        if layer is None:
            eng.tick_batch(*args, **kw)
        else:
            eng.tick_batch_fleet(layer, *args, **kw)


@pytest.mark.parametrize("model,impl", [("omni", 0), ("simple_cart", 0), ("omni", 1)])
def test_fleet_tick_equals_oracle_loops_on_per_robot_grids(model, impl):
    """12 small robots, two groups driving at each other past one block, 8 ticks of a closed loop: update and tick go to one
    stream with no wait between them.  Every robot is an independent oracle loop on a grid of its own, rebuilt every tick
    from the other robots' cells.  As in tests/test_gpu_fleet_tick.py: the source, follow / count and validate_control's
    verdict are identical; twists <= 1e-9 where control() produced them, bitwise where the dynamic window chose them (a
    differing choice must be a tie of the oracle's own objective).  The layer has to bite: at least 3 (tick, robot) pairs
    whose verdict on the plain grid is another one.  impl 0: the library's choice of the static part (the inflated map at this
    many rollout poses), 1: the ring search."""
    _, data = fr.plain_grid(po)
    plain = fr.grid_map(po, data)
    ys, xs = data.shape
    g = fr.sr.Geometry(fr.BOUNDS[0], fr.BOUNDS[2], fr.RES, xs, ys, fr.COLL_S[3])
    ccfg, dcfg = _cfg(fr.BOUNDS[0], fr.BOUNDS[2], xs, ys), capi.DwaCfg(*DWA[model])
    poses = fr.start_poses(model)
    B, body = len(poses), R_BND
    eng = _engine(model)
    layer = capi.FleetLayer(ccfg, body, B)
    try:
        capi.set_option(capi.OPT_COLLISION_IMPL, impl)
        T = eng.T
        st = _TickState(B, T)
        ors = [fr.FleetOracle(po, model, DWA[model]) for _ in range(B)]
        d_grid = dev(data, torch.int8)
        mem, vb = np.zeros((B, fr.TICKS, 3)), np.zeros((B, 3))
        seen, bites = set(), []
        for t in range(fr.TICKS):
            mem[:, t] = poses
            ut_before = st.ut.cpu().numpy()
            d_pose = dev(poses)
            layer.update(d_pose)                      # (the same stream as the tick, no wait in between)
            st.tick(eng, layer, B, d_pose, dev(vb), d_grid, ccfg, dcfg, mem=dev(mem[:, :t + 1]),
                    n_mem=torch.full((B,), t + 1, dtype=torch.int32, device="cuda"), mem_stride=t + 1)
            torch.cuda.synchronize()
            u, src, follow, count = st.u.cpu().numpy(), st.source.cpu().numpy(), st.follow.cpu().numpy(), st.count.cpu().numpy()
            valid, ut_after = st.valid.cpu().numpy(), st.ut.cpu().numpy()
            cells = fr.cells_of(g, poses)
            assert np.array_equal(layer.read()[1], cells)
            for b, o in enumerate(ors):
                o.grid = fr.grid_map(po, fr.robot_grid(data, cells, b, body))
                if t == 0:      # no robot starts in collision
                    assert po.validate_control(fr.COLL_S, o.grid, poses[b], np.zeros(3), fr.VAL_DT, fr.VAL_HORIZON), b
                o.memory = list(mem[b, :t])           # (tick() appends the pose itself)
                o.ec.ut = ut_before[b].T              # the oracle starts every tick from the engine's warm start
                uo, so = o.tick(poses[b], vb[b])
                assert SOURCES[src[b]] == so, (t, b, SOURCES[src[b]], so)
                assert bool(follow[b]) == o.follow and (not o.follow or int(count[b]) == o.i), (t, b, follow[b], count[b], o.follow, o.i)
                assert bool(valid[b]) == (so in ("ergodic", "dwa-follow")), (t, b, valid[b], so)
                if bool(valid[b]) != po.validate_control(fr.COLL_S, plain, poses[b], o.u_checked, fr.VAL_DT, fr.VAL_HORIZON):
                    bites.append((t, b))
                if so in ("ergodic", "dwa-follow"):
                    assert np.abs(u[b] - uo).max() <= 1e-9, (t, b, so, u[b], uo)
                elif not np.array_equal(u[b], uo):
                    if so == "dwa-replan":
                        raise AssertionError((t, b, so, u[b], uo))   # (control-error cost from identical doubles: bitwise)
                    xt = o.ec.opt_traj()
                    ca = po.dwa_objective_traj(DWA[model], fr.COLL_S, o.grid, poses[b], u[b], xt, 0.1)
                    cb = po.dwa_objective_traj(DWA[model], fr.COLL_S, o.grid, poses[b], uo, xt, 0.1)
                    assert abs(ca - cb) <= 1e-9 * max(1.0, abs(cb)), (t, b, u[b], uo, ca, cb)
                if so == "dwa-follow":
                    assert np.array_equal(ut_after[b], ut_before[b])
                seen.add(so)
            assert (st.status.cpu().numpy()[src == 0] == 0).all()
            for b in range(B):
                poses[b] = po.integrate_twist(poses[b], u[b], fr.DT)
            vb = u.copy()
        assert seen >= {"ergodic", "dwa-reference"}, seen
        assert len(bites) >= 3, bites
    finally:
        capi.set_option(capi.OPT_COLLISION_IMPL, 0)
        layer.close()
        eng.close()


def _scenario_inputs(model, B=None):
    _, data = fr.plain_grid(po)
    ys, xs = data.shape
    poses = fr.start_poses(model)
    if B is not None:
        poses = poses[:B]
    rng = np.random.default_rng(5)
    return dict(ccfg=_cfg(fr.BOUNDS[0], fr.BOUNDS[2], xs, ys), dcfg=capi.DwaCfg(*DWA[model]), grid=dev(data, torch.int8),
                pose=dev(poses), vb=dev(rng.uniform(-0.3, 0.3, poses.shape)), B=len(poses))


@pytest.mark.parametrize("model", ["omni", "simple_cart"])
def test_an_empty_layer_changes_nothing(model):
    """a layer whose mask is all zero: eea_tick_batch_fleet gives bitwise the outputs and the state of eea_tick_batch, over
    three ticks from the same start (some robots head for the block: the dynamic window runs too)"""
    s = _scenario_inputs(model)
    B = s["B"]
    layer = capi.FleetLayer(s["ccfg"], R_BND, B)
    results = []
    try:
        layer.update(s["pose"], mask=torch.zeros(B, dtype=torch.int32, device="cuda"))
        for with_layer in (False, True):
            eng = _engine(model)
            st = _TickState(B, eng.T)
            for _ in range(3):
                st.tick(eng, layer if with_layer else None, B, s["pose"], s["vb"], s["grid"], s["ccfg"], s["dcfg"])
            torch.cuda.synchronize()
            results.append({k: v.cpu().numpy().copy() for k, v in st.tensors().items()})
            eng.close()
        for k in results[0]:
            assert np.array_equal(results[0][k], results[1][k]), k
        # (the robots in front of the block took a dynamic-window twist in the first tick and follow it, the others ran control())
        assert set(results[0]["source"].tolist()) >= {0, 1}
    finally:
        layer.close()


def test_a_mismatched_configuration_or_fleet_size_is_refused_with_the_state_untouched():
    s = _scenario_inputs("omni")
    B = s["B"]
    eng = _engine("omni")
    layer = capi.FleetLayer(s["ccfg"], R_BND, B)
    try:
        layer.update(s["pose"])
        st = _TickState(B, eng.T, fill=-7)
        st.follow[::2] = 1
        st.count[::2] = 3
        st.u.copy_(s["vb"])
        before = {k: v.clone() for k, v in st.tensors().items()}
        ys, xs = 120, 240
        others = [capi.make_collision_cfg(fr.BOUNDS[0], fr.BOUNDS[2], fr.RES, xs, ys, 0.25, 0.4, 0.1, 0.8),   # another r_bnd
                  capi.make_collision_cfg(fr.BOUNDS[0], fr.BOUNDS[2], fr.RES, xs, ys - 1, *fr.COLL_S),       # another grid
                  capi.make_collision_cfg(fr.BOUNDS[0], fr.BOUNDS[2], fr.RES, xs, ys, 0.2, 0.4, 0.1, 0.7)]   # another threshold
        for ccfg, b in [(c, B) for c in others] + [(s["ccfg"], B - 1)]:
            with pytest.raises(capi.EngineError) as ei:
                st.tick(eng, layer, b, s["pose"], s["vb"], s["grid"], ccfg, s["dcfg"])
            assert ei.value.status == capi.ERR_INVALID_ARGUMENT and "fleet layer" in str(ei.value)
        with pytest.raises(capi.EngineError) as ei:
            eng.tick_batch_fleet(None, B, s["pose"], st.ut, st.follow, st.count, st.u, s["vb"], s["grid"], st.traj, st.valid,
                                 st.skip, s["ccfg"], s["dcfg"], fr.VAL_DT, fr.VAL_HORIZON)      # no layer at all
        assert ei.value.status == capi.ERR_INVALID_ARGUMENT
        torch.cuda.synchronize()
        for k, v in st.tensors().items():
            assert torch.equal(v, before[k]), k
        # the same call with the layer's own configuration is taken
        st.tick(eng, layer, B, s["pose"], s["vb"], s["grid"], s["ccfg"], s["dcfg"])
        torch.cuda.synchronize()
        assert (st.valid >= 0).all() and (st.source >= 0).all() and st.count[0].item() == 4
    finally:
        layer.close()
        eng.close()


COLL = (0.7, 1.0, 0.2, 0.8)      # the radii of tests/test_hit_map_table.py, at 0.1 m: 6, 8 and 10 cells


@pytest.fixture(scope="module")
def release_scene():
    """24 x 16 cells at 0.1 m with four occupied cells, three robots of body 1 (the third masked), 64 poses: around the two
    stamped robots the cells one short of the layer's reach, on its rim and one past it -- half of them outside the grid,
    where the indices wrap --, the robots' own cells, and cells up to 11 outside the grid on every side.  The wanted verdicts
    come from the rule (tests/fleet_layer_restatement.py), once."""
    xmin, ymin, res, xs, ys, body = -0.4, -0.3, 0.1, 24, 16, 1
    r_bnd, r_col, r_max = fr.radii(COLL, res)
    reach = r_col + body
    g = fr.sr.Geometry(xmin, ymin, res, xs, ys, COLL[3])
    data = np.zeros((ys, xs), dtype=np.int8)
    data[3, 3], data[12, 20], data[2, 12], data[15, 0] = 100, 100, 80, 90
    data[8, 8] = 79                                                      # below the threshold: free
    centre = lambda x, y: [xmin + (x + 0.5) * res, ymin + (y + 0.5) * res, 0.0]
    robot_cells = [(6, 5), (17, 10), (12, 8)]
    robots, mask = np.array([centre(x, y) for (x, y) in robot_cells]), np.array([1, 1, 0], dtype=np.int32)
    cells = [(x + dx, y + dy) for (x, y) in robot_cells[:2] for d in (reach - 1, reach, reach + 1)
             for (dx, dy) in ((d, 0), (-d, 0), (0, d), (0, -d))] + robot_cells
    rng = np.random.default_rng(11)
    while len(cells) < 64:
        cells.append((int(rng.integers(-11, xs + 11)), int(rng.integers(-11, ys + 11))))
    pose = np.array([centre(x, y) for (x, y) in cells])
    owner = (np.arange(64, dtype=np.int32) % 4) - 1                      # nobody's, robot 0's, 1's, 2's
    stamped = fr.cells_of(g, robots, mask)
    assert np.array_equal(stamped[:2], robot_cells[:2]) and (stamped[2] == fr.NOT_STAMPED).all()
    S, F = fr.ring_offsets(r_bnd, r_col, r_max), fr.offset_set(r_bnd, r_col, r_max, body)
    want = fr.verdicts(g, data, S, F, stamped, pose, owner)
    outside = np.array([not (j < xs and i < ys) for (i, j) in (fr.sr.world2grid(g, p[0], p[1]) for p in pose)])   # (unsigned)
    assert 0 < want.sum() < 64 and want[outside].any() and not want[outside].all() and outside.sum() >= 16
    # the layer bites, and so does a pose's own robot
    nobody = np.full(64, -1, dtype=np.int32)
    assert (want != fr.verdicts(g, data, S, F, np.full((3, 2), fr.NOT_STAMPED), pose, owner)).any()
    assert (want != fr.verdicts(g, data, S, F, stamped, pose, nobody)).any()
    return dict(cfg=capi.make_collision_cfg(xmin, ymin, res, xs, ys, *COLL), body=body, data=data, robots=robots, mask=mask,
                pose=pose, owner=owner, want=want)


@pytest.mark.parametrize("impl", [1, 2])
def test_a_live_layer_survives_a_cache_release(release_scene, impl):
    """release_collision_caches() with a layer alive frees the tables nobody holds and leaves the layer's span table where it
    is: the layer, a second one made from the same parameters afterwards (a hit on the kept table), that one after the first
    is gone, and a third one made after everything was released (a fresh table) all answer as the rule does.  The static part
    goes through the ring search (impl 1) or the inflated map (2), whose offsets and buffers every release frees."""
    s = release_scene
    d_grid, d_pose, d_owner = dev(s["data"], torch.int8), dev(s["pose"]), dev(s["owner"], torch.int32)
    d_robots, d_mask = dev(s["robots"]), dev(s["mask"], torch.int32)
    layers = []

    def create():
        layers.append(capi.FleetLayer(s["cfg"], s["body"], len(s["robots"])))
        layers[-1].update(d_robots, d_mask)
        return layers[-1]

    def answers(layer):
        hit = torch.full((len(s["pose"]),), -7, dtype=torch.int32, device="cuda")
        layer.collision_check(d_grid, d_pose, hit, self_index=d_owner)
        return hit.cpu().numpy()

    try:
        capi.set_option(capi.OPT_COLLISION_IMPL, impl)
        a = create()
        assert np.array_equal(answers(a), s["want"])
        capi.release_collision_caches()                   # a is alive
        b = create()
        assert np.array_equal(answers(a), s["want"]) and np.array_equal(answers(b), s["want"])
        a.close()
        capi.release_collision_caches()
        assert np.array_equal(answers(b), s["want"])
        b.close()
        capi.release_collision_caches()
        c = create()
        assert np.array_equal(answers(c), s["want"])
    finally:
        capi.set_option(capi.OPT_COLLISION_IMPL, 0)
        for layer in layers:
            layer.close()
        capi.release_collision_caches()

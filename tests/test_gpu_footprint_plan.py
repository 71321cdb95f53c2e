"""Footprint planning on the device (eea_footprint_validate_control_batch / eea_footprint_dwa_control_batch /
eea_tick_batch_footprint: csrc/footprint_plan_kernel.hip).

1. free space: bitwise the disc's kernels (everything but the collision test is held to the oracle-pinned kernels);
2. against tests/footprint_plan_restatement.py on the robots it calls decided (no occupied centre within 1e-9 m of the polygon's
   boundary at any step that matters): validate's verdict, found and u_opt bitwise in the twist-error mode, found and u_opt or
   a tie of the restatement's own cost in the trajectory mode;
3. with d_sq == without, bitwise, over ALL robots;
4. the two entries agree;
5. the shapes at which the kernel takes another path;
6. the corridor a 0.9 m x 0.5 m base passes and its circumscribed disc does not, and the rotation its inscribed disc allows;
7. refusals behind a device; 8. the tick against the same loop written with the public pieces."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ergodic_exploration_amd import capi
from tests import clearance_restatement as cr
from tests import footprint_plan_restatement as pr
from tests import footprint_restatement as fr

pytestmark = pytest.mark.gpu

P_STUDY = 128
NAMES = ("rect", "tri", "offc")


def dev(a, t=None):
    if a is None:
        return None
    x = torch.as_tensor(np.ascontiguousarray(a))
    return (x if t is None else x.to(t)).cuda()


class Scene:
    """a World on the device, its collision cfg (radii: those of the disc it is compared with) and its distance field"""

    def __init__(self, w, coll=pr.COLL):
        self.w = w
        self.ccfg = capi.make_collision_cfg(w.xmin, w.ymin, w.res, w.xs, w.ys, *coll)
        self.d_grid = dev(w.data)
        self.d_sq = torch.empty((w.ys, w.xs), dtype=torch.int32, device="cuda")
        capi.distance_field(self.ccfg, self.d_grid, self.d_sq)

    def outputs(self, P):
        return (torch.full((P, 3), float("nan"), dtype=torch.float64, device="cuda"),
                torch.full((P,), -1, dtype=torch.int32, device="cuda"))

    def dwa(self, dwa, verts, x0, vb, vref=None, xt=None, dt_ref=0.0, with_sq=False, out=None):
        d_u, d_f = self.outputs(len(x0)) if out is None else out
        capi.footprint_dwa_control_batch(self.ccfg, capi.DwaCfg(*dwa), capi.Footprint.of(verts), self.d_grid, dev(x0), dev(vb), d_u,
                                         d_f, sq=self.d_sq if with_sq else None, vref=dev(vref), xt_ref=dev(xt), dt_ref=dt_ref)
        torch.cuda.synchronize()
        return d_u.cpu().numpy(), d_f.cpu().numpy()

    def dwa_both(self, dwa, verts, x0, vb, **kw):
        """with and without the field: the same bits over all robots (3.); returns them once"""
        u, f = self.dwa(dwa, verts, x0, vb, with_sq=False, **kw)
        u2, f2 = self.dwa(dwa, verts, x0, vb, with_sq=True, **kw)
        assert np.array_equal(f, f2) and np.array_equal(u.view(np.uint64), u2.view(np.uint64))
        return u, f

    def validate(self, verts, x0, u, dt, horizon, with_sq=False):
        d_v = torch.full((len(x0),), -1, dtype=torch.int32, device="cuda")
        capi.footprint_validate_control_batch(self.ccfg, capi.Footprint.of(verts), self.d_grid, dev(x0), dev(u), dt, horizon, d_v,
                                              sq=self.d_sq if with_sq else None)
        torch.cuda.synchronize()
        return d_v.cpu().numpy()

    def validate_both(self, verts, x0, u, dt, horizon):
        v = self.validate(verts, x0, u, dt, horizon, False)
        assert np.array_equal(v, self.validate(verts, x0, u, dt, horizon, True))
        return v

    def disc_dwa(self, dwa, x0, vb, vref=None, xt=None, dt_ref=0.0):
        d_u, d_f = self.outputs(len(x0))
        capi.dwa_control_batch(self.ccfg, capi.DwaCfg(*dwa), self.d_grid, dev(x0), dev(vb), d_u, d_f, vref=dev(vref), xt_ref=dev(xt),
                               dt_ref=dt_ref)
        torch.cuda.synchronize()
        return d_u.cpu().numpy(), d_f.cpu().numpy()

    def disc_validate(self, x0, u, dt, horizon):
        d_v = torch.full((len(x0),), -1, dtype=torch.int32, device="cuda")
        capi.validate_control_batch(self.ccfg, self.d_grid, dev(x0), dev(u), dt, horizon, d_v)
        torch.cuda.synchronize()
        return d_v.cpu().numpy()


def _arcs(rng, x0, n_ref, dt_ref):
    from oracle import pyoracle as po
    xt = np.empty((len(x0), n_ref, 3))
    for i in range(len(x0)):
        x, tw = x0[i].copy(), np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-2, 2)])
        for t in range(n_ref):
            x = po.integrate_twist(x, tw, dt_ref)
            xt[i, t] = x
    return xt


def _check(sc, verts, dwa, x0, vb, u, f, vref=None, xt=None, dt_ref=0.0):
    """2. for the robots the restatement decides; returns (decided robots, found among them, [Answer])"""
    answers, n_dec, n_found = [], 0, 0
    for q in range(len(x0)):
        a = pr.dwa_control(sc.w, verts, dwa, pr.Robot(dwa, x0[q], vb[q]), vref=None if vref is None else vref[q],
                           xt=None if xt is None else xt[q], dt_ref=dt_ref)
        answers.append(a)
        if a.decided:
            _check_one(a, q, u[q], f[q], traj=xt is not None)
            n_dec += 1
            n_found += a.found
    return n_dec, n_found, answers


def _check_one(a, q, u, f, traj):
    assert int(f) == a.found, (q, f, a.found)
    if np.array_equal(u, a.u_opt):
        return
    assert traj, (q, u, a.u_opt)          # the twist-error cost has no trigonometry: bitwise
    # another choice is legitimate only as a tie of the restatement's own cost (test_dwa_traj_mode's rule), and it is a free sample
    s = [k for k in range(len(a.costs)) if np.array_equal(u, a.samples[k])]
    assert len(s) >= 1, (q, u)
    assert a.free[s[0]] and abs(a.costs[s[0]] - a.cost) <= 1e-12 * max(1.0, abs(a.cost)), (q, u, a.u_opt, a.costs[s[0]], a.cost)


# ---- 1. free space ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("dwa", [pr.DWA_OMNI, pr.DWA_CART])
def test_free_space_is_the_discs_kernel_bitwise(dwa, far):
    """no occupied cell; or occupied cells only in the columns 0..4 (x < -1.5 m) with every robot at x >= 2.5 m: 4 m away,
    more than the reach (2 m: 20 steps of 0.1 s at 1 m/s) + r_out (0.6 m) + the disc's search radius (1 m)"""
    rng = np.random.default_rng(21)
    data = np.zeros((60, 80), dtype=np.int8)
    if far:
        data[:, :5] = 100
    sc = Scene(pr.World(data, 0.1, -2.0, -1.0))
    P = 96
    x0 = np.stack([rng.uniform(2.5, 5.5, P), rng.uniform(-0.5, 4.5, P), rng.uniform(-np.pi, np.pi, P)], 1)
    vb = np.stack([rng.uniform(-1, 1, P), rng.uniform(-1, 1, P) * (dwa[8] != 0), rng.uniform(-2, 2, P)], 1)
    vref = np.stack([rng.uniform(-1, 1, P), rng.uniform(-1, 1, P) * (dwa[8] != 0), rng.uniform(-2, 2, P)], 1)
    xt = _arcs(rng, x0, 30, 0.1)
    for name in ("rect", "tri"):
        verts = fr.FOOTPRINTS[name]
        for kw in (dict(vref=vref), dict(xt=xt, dt_ref=0.1)):
            u, f = sc.dwa_both(dwa, verts, x0, vb, **kw)
            ud, fd = sc.disc_dwa(dwa, x0, vb, **kw)
            assert np.array_equal(f, fd) and (f == 1).all()
            assert np.array_equal(u.view(np.uint64), ud.view(np.uint64))
        v = sc.validate_both(verts, x0, vref, dwa[0], dwa[1])
        assert np.array_equal(v, sc.disc_validate(x0, vref, dwa[0], dwa[1])) and (v == 1).all()


# ---- 2. - 4. the study scene -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_dwa_against_the_restatement(name):
    w, x0, vb, vref, xt, _ = pr.study()
    x0, vb, vref, xt = x0[:P_STUDY], vb[:P_STUDY], vref[:P_STUDY], xt[:P_STUDY]
    verts = fr.FOOTPRINTS[name]
    sc = Scene(w)
    for mode in ("vref", "traj"):
        kw = dict(vref=vref) if mode == "vref" else dict(xt=xt, dt_ref=pr.DT_REF)
        u, f = sc.dwa_both(pr.DWA_OMNI, verts, x0, vb, **kw)
        answers = pr.study_answers(name, mode)[:P_STUDY]
        n_dec = 0
        for q, a in enumerate(answers):
            if a.decided:
                _check_one(a, q, u[q], f[q], traj=mode == "traj")
                n_dec += 1
        assert n_dec >= P_STUDY - (2 * P_STUDY) // 100
        found = sum(a.found for a in answers)
        und, none, every, mixed = pr.mix(answers)
        assert 0 < found < P_STUDY and none > 0 and every > 0 and mixed > 0
        if mode == "vref":
            # 4. the two entries agree: the chosen twist is valid, a twist the restatement rejects with margin is not
            ok = sc.validate_both(verts, x0, u, pr.DWA_OMNI[0], pr.DWA_OMNI[1])
            bad_q, bad_u = [], []
            for q, a in enumerate(answers):
                if a.decided and a.found:
                    assert ok[q] == 1, q
                if a.decided and not a.free.all():
                    bad_q.append(q)
                    bad_u.append(a.samples[int(np.argmin(a.free))])
            assert len(bad_q) > 20
            assert (sc.validate_both(verts, x0[bad_q], np.array(bad_u), pr.DWA_OMNI[0], pr.DWA_OMNI[1]) == 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_validate_against_the_restatement(name):
    w, x0, _, vref, _, _ = pr.study()
    x0, u = x0[:P_STUDY], vref[:P_STUDY]
    verts = fr.FOOTPRINTS[name]
    v = Scene(w).validate_both(verts, x0, u, 0.1, 1.0)
    ref, decided = pr.validate(w, verts, x0, u, 0.1, 1.0)
    assert decided.sum() >= P_STUDY - (2 * P_STUDY) // 100
    assert np.array_equal(v[decided], ref[decided]) and 0 < ref.sum() < P_STUDY


# ---- 5. shapes -------------------------------------------------------------------------------------------------------------------

def _robots(rng, P):
    x0 = np.stack([rng.uniform(-1.5, 5.5, P), rng.uniform(-0.5, 4.5, P), rng.uniform(-np.pi, np.pi, P)], 1)
    tw = lambda: np.stack([rng.uniform(-1, 1, P), rng.uniform(-1, 1, P), rng.uniform(-2, 2, P)], 1)
    return x0, tw(), tw()


def _both_modes(sc, verts, dwa, x0, vb, vref, rng, min_decided=None):
    """5.: against the restatement on the decided robots, with / without d_sq bitwise; returns the twist-error mode's answers"""
    u, f = sc.dwa_both(dwa, verts, x0, vb, vref=vref)
    n_dec, n_found, answers = _check(sc, verts, dwa, x0, vb, u, f, vref=vref)
    assert n_dec >= (len(x0) - 1 if min_decided is None else min_decided)
    xt = _arcs(rng, x0, 25, 0.1)
    u, f = sc.dwa_both(dwa, verts, x0, vb, xt=xt, dt_ref=0.1)
    _check(sc, verts, dwa, x0, vb, u, f, xt=xt, dt_ref=0.1)
    return n_found, answers


@pytest.mark.parametrize("ns", [(1, 1, 1), (4, 4, 4), (5, 13, 1), (8, 4, 4), (3, 43, 1), (7, 11, 13)])
def test_sample_counts(ns):
    """1, 64 | 65, 128 | 129, 1001 samples: one wavefront | 128 threads | the strided sample loop"""
    w, rng = pr.world(7)
    P = 10
    x0, vb, vref = _robots(rng, P)
    n_found, _ = _both_modes(Scene(w), fr.FOOTPRINTS["rect"], pr.with_(pr.DWA_OMNI, ns=ns), x0, vb, vref, rng)
    assert 0 < n_found < P


@pytest.mark.parametrize("horizon,steps", [(0.05, 0), (0.1, 1)])
def test_rollouts_of_no_and_one_step(horizon, steps):
    w, rng = pr.world(7)
    P = 24
    dwa = pr.with_(pr.DWA_OMNI, horizon=horizon)
    assert pr.steps_of(dwa) == steps
    x0, vb, vref = _robots(rng, P)
    sc = Scene(w)
    n_found, _ = _both_modes(sc, fr.FOOTPRINTS["tri"], dwa, x0, vb, vref, rng)
    assert n_found == P if steps == 0 else 0 < n_found < P
    v = sc.validate_both(fr.FOOTPRINTS["tri"], x0, vref, 0.1, horizon)
    ref, decided = pr.validate(w, fr.FOOTPRINTS["tri"], x0, vref, 0.1, horizon)
    assert np.array_equal(v[decided], ref[decided]) and decided.sum() >= P - 1


@pytest.mark.parametrize("P", [1, 63, 64, 65, 257])
def test_validate_batch_sizes(P):
    """one robot, a wavefront less one, a full one, one more; more than one workgroup"""
    w, rng = pr.world(7)
    x0, u, _ = _robots(rng, P)
    v = Scene(w).validate_both(fr.FOOTPRINTS["offc"], x0, u, 0.1, 0.6)
    ref, decided = pr.validate(w, fr.FOOTPRINTS["offc"], x0, u, 0.1, 0.6)
    assert np.array_equal(v[decided], ref[decided]) and decided.sum() >= P - max(1, P // 50)


def test_edge_poses():
    """a robot in every grid corner, straddling every edge, one window off the grid, at 1e9 m, and with NaN / +-inf components"""
    w, rng = pr.world(7)
    x_hi, y_hi = w.xmin + w.xs * w.res, w.ymin + w.ys * w.res
    off = (pr.limits_reach(pr.DWA_OMNI, w.res) + 8) * w.res
    nan, inf = float("nan"), float("inf")
    xy = [(w.xmin + 0.05, w.ymin + 0.05), (x_hi - 0.05, w.ymin + 0.05), (w.xmin + 0.05, y_hi - 0.05), (x_hi - 0.05, y_hi - 0.05),
          (w.xmin - 0.02, 2.0), (x_hi + 0.02, 2.0), (1.0, w.ymin - 0.02), (1.0, y_hi + 0.02), (w.xmin, 1.0), (x_hi, 1.0),
          (w.xmin - off, 2.0), (x_hi + off, 2.0), (1.0, w.ymin - off), (1.0, y_hi + off), (w.xmin - off - 0.3, y_hi + off + 0.3),
          (1e9, 2.0), (-1e9, -1e9), (1.0, 1e9)]
    x0 = np.array([[x, y, th] for (x, y), th in zip(xy, rng.uniform(-np.pi, np.pi, len(xy)))] +
                  [[nan, 2.0, 0.3], [1.0, nan, 0.3], [1.0, 2.0, nan], [inf, 2.0, 0.3], [1.0, -inf, 0.3], [1.0, 2.0, inf], [nan, nan, nan]])
    P = len(x0)
    _, vb, vref = _robots(rng, P)
    sc = Scene(w)
    for name in ("rect", "offc"):
        n_found, _ = _both_modes(sc, fr.FOOTPRINTS[name], pr.DWA_OMNI, x0, vb, vref, rng, min_decided=P - 2)
        assert n_found > 0
        v = sc.validate_both(fr.FOOTPRINTS[name], x0, vref, 0.1, 1.0)
        ref, decided = pr.validate(w, fr.FOOTPRINTS[name], x0, vref, 0.1, 1.0)
        assert np.array_equal(v[decided], ref[decided])


def test_odometry_outside_the_limits_leaves_the_window_path():
    """vb at twice the limits: lower = 1.8 > vmax, the robot's reach (27 cells) is above the one the launch reserved (16);
    and windows clipped to lower > upper from either side.  Half the robots stay on the window path"""
    w, rng = pr.world(7)
    P = 24
    x0, vb, vref = _robots(rng, P)
    vb[0:6] = [2.0, 2.0, 4.0]
    vb[6:10] = [3.0, -3.0, 0.0]
    vb[10:14] = [-3.0, 0.5, 5.0]
    lim = pr.limits_reach(pr.DWA_OMNI, w.res)
    own = np.array([pr.reach(pr.DWA_OMNI, vb[q], w.res) for q in range(P)])
    assert (own[:14] > lim).all() and (own[14:] <= lim).all() and lim == 16.0 and own[0] == 27.0
    lo, up, _, _ = pr.window(pr.DWA_OMNI, vb[6])
    assert (lo > up)[:2].all()
    n_found, _ = _both_modes(Scene(w), fr.FOOTPRINTS["rect"], pr.DWA_OMNI, x0, vb, vref, rng)
    assert 0 < n_found < P


def test_a_window_that_cannot_fit_the_lds():
    """velocity limits of 30 m/s: the limits' reach is 426 cells, a window of 867 x 867 bits is 97 KB -- the launch reserves none
    and every robot takes its cells from memory (the robots' own windows stay small: the acceleration limits)"""
    w, rng = pr.world(7)
    dwa = pr.with_(pr.DWA_OMNI, max_vel_x=30.0, min_vel_x=-30.0, max_vel_y=30.0, min_vel_y=-30.0)
    side = 2 * (pr.limits_reach(dwa, w.res) + 7) + 1
    assert side * ((side + 63) // 64) * 8 + 8 * 120 > 64 * 1024
    P = 24
    x0, vb, vref = _robots(rng, P)
    n_found, _ = _both_modes(Scene(w), fr.FOOTPRINTS["rect"], dwa, x0, vb, vref, rng)
    assert 0 < n_found < P


@pytest.mark.parametrize("kind", ["one_cell", "full"])
def test_smallest_and_full_grids(kind):
    rng = np.random.default_rng(9)
    P = 16 if kind == "one_cell" else 5          # (the restatement tests every occupied cell against every pose)
    if kind == "one_cell":
        w = pr.World(np.full((1, 1), 100, dtype=np.int8), 0.1, 0.0, 0.0)
        x0 = np.stack([rng.uniform(-1.5, 1.5, P), rng.uniform(-1.5, 1.5, P), rng.uniform(-np.pi, np.pi, P)], 1)
    else:
        w = pr.World(np.full((60, 80), 100, dtype=np.int8), 0.1, -2.0, -1.0)
        x0 = _robots(rng, P)[0]
    _, vb, vref = _robots(rng, P)
    sc = Scene(w)
    n_found, _ = _both_modes(sc, fr.FOOTPRINTS["rect"], pr.DWA_OMNI, x0, vb, vref, rng, min_decided=P - 2)
    if kind == "full":
        u, f = sc.dwa(pr.DWA_OMNI, fr.FOOTPRINTS["rect"], x0, vb, vref=vref)
        assert n_found == 0 and (f == 0).all() and np.array_equal(u, np.zeros((P, 3))) and not np.signbit(u).any()
    else:
        assert 0 < n_found


# ---- 6. fact scenes --------------------------------------------------------------------------------------------------------------

def test_the_corridor():
    """`rect` at the centre of the 0.7 m corridor, heading along it: the footprint's window finds a twist whose rollout the
    restatement calls free where the 0.51 m disc's finds none; a pure rotation that brings the base across the corridor is
    invalid where the 0.25 m disc's validate_control accepts it"""
    w = pr.World(fr.fact_scene(fr.CORRIDOR), cr.RES41, cr.XMIN41, cr.YMIN41)
    verts = fr.FOOTPRINTS["rect"]
    x0 = np.array([[fr.CORRIDOR_POSE[0], fr.CORRIDOR_POSE[1], 0.0]])
    vb, vref = np.zeros((1, 3)), np.array([[0.3, 0.0, 0.0]])
    big = Scene(w, coll=(0.51, 1.0, 0.0, 0.8))
    u, f = big.dwa_both(pr.DWA_OMNI, verts, x0, vb, vref=vref)
    a = pr.dwa_control(w, verts, pr.DWA_OMNI, pr.Robot(pr.DWA_OMNI, x0[0], vb[0]), vref=vref[0])
    assert a.decided and a.found == 1 and f[0] == 1 and np.array_equal(u[0], a.u_opt)
    hit, margin = pr.verdicts(w, verts, pr.rollout(x0[0], u[0], pr.DWA_OMNI[0], pr.steps_of(pr.DWA_OMNI)))
    assert not hit.any() and (margin >= fr.DECIDED).all()
    ud, fd = big.disc_dwa(pr.DWA_OMNI, x0, vb, vref=vref)
    assert fd[0] == 0 and np.array_equal(ud[0], np.zeros(3))
    small = Scene(w, coll=(0.25, 1.0, 0.0, 0.8))
    spin = np.array([[0.0, 0.0, 1.0]])
    ref, decided = pr.validate(w, verts, x0, spin, 0.1, 2.0)
    assert decided[0] and ref[0] == 0
    assert small.validate_both(verts, x0, spin, 0.1, 2.0)[0] == 0 and small.disc_validate(x0, spin, 0.1, 2.0)[0] == 1


# ---- 7. refusals behind a device ---------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_alone():
    w, rng = pr.world(11)
    sc = Scene(w)
    P = 8
    x0, vb, vref = _robots(rng, P)
    verts = fr.FOOTPRINTS["rect"]
    long_ = pr.with_(pr.DWA_OMNI, horizon=2.0)
    arcs = _arcs(rng, x0, 20, 0.1)
    cases = [(capi.ERR_INVALID_ARGUMENT, long_, dict(xt=np.ascontiguousarray(arcs[:, :18]), dt_ref=0.1)),     # n_ref too short
             (capi.ERR_INVALID_ARGUMENT, long_, dict(xt=arcs, dt_ref=0.0)),
             (capi.ERR_UNSUPPORTED, pr.with_(pr.DWA_OMNI, ns=(17, 17, 29)), dict(vref=vref))]               # 8381 samples
    for status, dwa, kw in cases:
        out = sc.outputs(P)
        with pytest.raises(capi.EngineError) as ei:
            sc.dwa(dwa, verts, x0, vb, out=out, **kw)
        assert ei.value.status == status, ei.value
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[0]).all()) and bool((out[1] == -1).all())
    u, f = sc.dwa(long_, verts, x0, vb, xt=np.ascontiguousarray(arcs[:, :19]), dt_ref=0.1)       # 19 columns serve 20 steps
    assert not np.isnan(u).any() and ((f == 0) | (f == 1)).all()


# ---- 8. the tick -------------------------------------------------------------------------------------------------------------------

def test_tick_is_the_loop_of_the_public_pieces():
    """64 robots x 12 ticks of eea_tick_batch_footprint, the robots moved by eea_integrate_twist_batch, a wall appearing at
    tick 5 (d_sq rebuilt): bitwise the same loop written with the follower bookkeeping of step 1 on the host,
    eea_control_batch with d_skip, eea_rollout_batch, eea_footprint_validate_control_batch and
    eea_footprint_dwa_control_batch in the robot's mode.  eea_tick_batch on the same inputs gives before and after what it
    gave."""
    from tests.test_host_mirror import COLL, DWA, _grid_with
    B, ticks, wall_tick, dt = 64, 12, 5, 0.1
    obstacles = [(2.4, 0.2, 3.0, 2.6), (6.0, 2.0, 6.5, 4.6), (8.8, -0.4, 9.4, 1.2)]
    wall = (4.2, -0.6, 4.5, 4.4)
    grid_a, bounds = _grid_with(obstacles)
    grid_b, _ = _grid_with(obstacles + [wall])
    xs, ys, res = grid_a.xsize, grid_a.ysize, 0.05
    worlds = [pr.World(np.asarray(g.data, dtype=np.int8).reshape(ys, xs), res, bounds[0], bounds[2]) for g in (grid_a, grid_b)]
    scenes = [Scene(wd, coll=COLL) for wd in worlds]
    ccfg, dwa = scenes[0].ccfg, DWA["omni"]
    dcfg, fp = capi.DwaCfg(*dwa), capi.Footprint.of(fr.FOOTPRINTS["rect"])
    dwa_steps = pr.steps_of(dwa)
    lim = np.array([1.0, 1.0, 2.0])
    eng = capi.Engine(capi.make_config(capi.MODEL_OMNI, 0.1, 5.0, 0.1, 1.0, 10, np.diag([1.0, 1.0, 2.0]), -lim, lim))
    eng.set_target_gaussians([[2.5, 2.5], [8.5, 2.5]], [[1.5, 1.5], [1.5, 1.5]])
    eng.config_domain(bounds)
    T = eng.T
    rng = np.random.default_rng(4)
    poses = np.stack([rng.uniform(0.2, 9.5, B), rng.uniform(-0.2, 4.2, B), rng.uniform(-0.6, 0.6, B)], 1)
    poses[:16, 0], poses[:16, 1], poses[:16, 2] = rng.uniform(1.0, 1.6, 16), rng.uniform(0.6, 2.2, 16), rng.uniform(-0.2, 0.2, 16)
    poses[16:28, 0], poses[16:28, 1] = rng.uniform(3.3, 3.7, 12), rng.uniform(0.0, 4.0, 12)
    start = pr.validate(worlds[1], fr.FOOTPRINTS["rect"], poses, np.zeros((B, 3)), 0.1, 0.1)[0]
    poses[start == 0, :2] = [0.0, -0.5]          # (no robot starts inside a collision: open floor left of the first obstacle)
    zeros = lambda shape, t: torch.zeros(shape, dtype=t, device="cuda")

    class State:
        def __init__(self):
            self.ut, self.u, self.traj = zeros((B, T, 3), torch.float64), zeros((B, 3), torch.float64), zeros((B, T, 3), torch.float64)
            self.follow, self.count = zeros((B,), torch.int32), zeros((B,), torch.int32)
            self.valid, self.skip = torch.full((B,), -1, dtype=torch.int32, device="cuda"), zeros((B,), torch.int32)
            self.source, self.status = torch.full((B,), -1, dtype=torch.int32, device="cuda"), zeros((B,), torch.int32)

    def disc_tick():
        s = State()
        eng.tick_batch(B, dev(poses), s.ut, s.follow, s.count, s.u, zeros((B, 3), torch.float64), scenes[0].d_grid, s.traj, s.valid,
                       s.skip, ccfg, dcfg, 0.1, 0.5, source=s.source, status=s.status)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in (s.u, s.follow, s.count, s.valid, s.source, s.ut)]

    disc_before = disc_tick()
    a, b = State(), State()
    d_pose, d_vb = dev(poses), zeros((B, 3), torch.float64)
    seen = set()
    for t in range(ticks):
        sc = scenes[0] if t < wall_tick else scenes[1]
        eng.tick_batch_footprint(fp, B, d_pose, a.ut, a.follow, a.count, a.u, d_vb, sc.d_grid, a.traj, a.valid, a.skip, ccfg, dcfg,
                                 0.1, 0.5, sq=sc.d_sq, source=a.source, status=a.status)
        # the same with the public pieces
        follow, count = b.follow.cpu().numpy().copy(), b.count.cpu().numpy().copy()
        for r in range(B):                                         # step 1 (exploration.hpp:223-228)
            if follow[r]:
                count[r] += 1
                follow[r] = 1 if count[r] != dwa_steps else 0
        b.skip = dev(follow)
        eng.control_batch(B, d_pose, b.ut, b.u, skip=b.skip, status=b.status)          # step 2
        eng.rollout_batch(B, d_pose, b.ut, b.traj)
        capi.footprint_validate_control_batch(ccfg, fp, sc.d_grid, d_pose, b.u, 0.1, 0.5, b.valid, sq=sc.d_sq)      # step 3
        u_f, f_f = sc.outputs(B)
        u_t, f_t = sc.outputs(B)
        capi.footprint_dwa_control_batch(ccfg, dcfg, fp, sc.d_grid, d_pose, d_vb, u_f, f_f, sq=sc.d_sq, vref=b.u)    # step 4
        capi.footprint_dwa_control_batch(ccfg, dcfg, fp, sc.d_grid, d_pose, d_vb, u_t, f_t, sq=sc.d_sq, xt_ref=b.traj, dt_ref=0.1)
        torch.cuda.synchronize()
        valid, u = b.valid.cpu().numpy(), b.u.cpu().numpy().copy()
        u_f, u_t, f_t = u_f.cpu().numpy(), u_t.cpu().numpy(), f_t.cpu().numpy()
        source = np.empty(B, dtype=np.int32)
        for r in range(B):
            if valid[r]:
                source[r] = 1 if follow[r] else 0
            elif follow[r]:
                u[r], follow[r], source[r] = u_f[r], 0, 3
            else:
                u[r], follow[r], source[r] = u_t[r], f_t[r], 2
                if f_t[r]:
                    count[r] = 0
        b.u, b.follow, b.count = dev(u), dev(follow), dev(count)
        got = [x.cpu().numpy() for x in (a.u, a.follow, a.count, a.valid, a.source)]
        for name, x, y in zip(("u", "follow_dwa", "dwa_count", "valid", "source"), got, (u, follow, count, valid, source)):
            assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                                  y.view(np.uint64) if y.dtype == np.float64 else y), (t, name, np.nonzero((x != y).reshape(B, -1).any(1))[0])
        seen |= set(int(v) for v in source)
        capi.integrate_twist_batch(d_pose, a.u, dt)       # the robots move, odometry reports the commanded twist
        d_vb = a.u.clone()
        torch.cuda.synchronize()
    assert seen == {0, 1, 2, 3}, seen
    for x, y in zip(disc_before, disc_tick()):
        assert np.array_equal(x, y, equal_nan=True)
    eng.close()


# ---- 9. the host mirror ------------------------------------------------------------------------------------------------------------

def test_host_mirror_prints_the_restatements_answers():
    """host/build/footprint_plan_tests (Footprint::validateControl, DynamicWindow::control for a polygon base, each with and
    without a DistanceField) runs once; what it prints against the restatement on the same grid and robots"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "ergodic_exploration_amd", "host", "build", "footprint_plan_tests")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.splitlines()]
    assert lines[0][0] == "grid" and (int(lines[0][1]), int(lines[0][2])) == (50, 40)
    res, ox, oy = (float(v) for v in lines[0][3:6])
    data = np.zeros((40, 50), dtype=np.int8)
    data[10:14, 20:26] = 100
    data[30, 5], data[31, 7], data[25, 40], data[3, 44], data[38, 30] = 80, 79, 100, 100, 100
    data[5:8, 2] = -1
    w = pr.World(data, res, ox, oy, 0.8)
    robots = np.array([[float(v) for v in l[2:11]] for l in lines if l[0] == "robot"])
    P = len(robots)
    assert P == 48
    x0, vb, tw = robots[:, 0:3], robots[:, 3:6], robots[:, 6:9]
    xt = np.array([[[x0[q, c] + float(t + 1) * (0.1 * tw[q, c]) for c in range(3)] for t in range(25)] for q in range(P)])
    for fi, name in enumerate(("rect", "offc")):
        verts = fr.FOOTPRINTS[name]
        rows = {kind: [l for l in lines if l[0] == kind and int(l[1]) == fi] for kind in ("validate", "vref", "traj")}
        assert all(len(v) == P and [int(l[2]) for l in v] == list(range(P)) for v in rows.values())
        ref, decided = pr.validate(w, verts, x0, tw, 0.1, 1.0)
        got = np.array([[int(l[3]), int(l[4])] for l in rows["validate"]])
        assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[decided, 0], ref[decided])
        assert decided.sum() >= P - 1 and 0 < ref.sum() < P
        for mode in ("vref", "traj"):
            n_found = 0
            for q, l in enumerate(rows[mode]):
                assert l[3:7] == l[7:11], (mode, q, l)              # through the field: the same answer
                a = pr.dwa_control(w, verts, pr.DWA_OMNI, pr.Robot(pr.DWA_OMNI, x0[q], vb[q]), vref=tw[q] if mode == "vref" else None,
                                   xt=xt[q] if mode == "traj" else None, dt_ref=0.1)
                if a.decided:
                    _check_one(a, q, np.array([float(v) for v in l[4:7]]), int(l[3]), traj=mode == "traj")
                    n_found += a.found
            assert 0 < n_found < P


def test_tick_refusals_leave_the_state_alone():
    """eea_tick_batch_footprint refuses a missing or malformed footprint, a grid it cannot index and a window past the
    reference before step 1: follow_dwa, dwa_count, u and valid keep their values; B == 0 is EEA_OK"""
    from tests.test_host_mirror import COLL, DWA
    B = 8
    lim = np.array([1.0, 1.0, 2.0])
    eng = capi.Engine(capi.make_config(capi.MODEL_OMNI, 0.1, 5.0, 0.1, 1.0, 10, np.diag([1.0, 1.0, 2.0]), -lim, lim))
    eng.set_target_gaussians([[2.5, 2.5], [8.5, 2.5]], [[1.5, 1.5], [1.5, 1.5]])
    eng.config_domain((-1.0, 11.0, -1.0, 5.0))
    T = eng.T
    good = capi.make_collision_cfg(-1.0, -1.0, 0.05, 240, 120, *COLL)
    rect = capi.Footprint.of(fr.FOOTPRINTS["rect"])
    i32 = lambda v: torch.full((B,), v, dtype=torch.int32, device="cuda")
    f64 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device="cuda")
    pose, ut, u, vb, traj = f64(B, 3), torch.zeros((B, T, 3), dtype=torch.float64, device="cuda"), f64(B, 3), f64(B, 3), f64(B, T, 3)
    follow, count, valid, skip = i32(1), i32(3), i32(-1), i32(-1)
    grid = torch.zeros((120, 240), dtype=torch.int8, device="cuda")

    def tick(fp=rect, cfg=good, dwa=DWA["omni"], n=B):
        eng.tick_batch_footprint(fp, n, pose, ut, follow, count, u, vb, grid, traj, valid, skip, cfg, capi.DwaCfg(*dwa), 0.1, 0.5)

    r_out = capi.footprint_radii(rect)[1]
    cases = [(capi.ERR_INVALID_ARGUMENT, dict(fp=None)),
             (capi.ERR_INVALID_ARGUMENT, dict(fp=capi.Footprint.of(fr.FOOTPRINTS["rect"][::-1]))),
             (capi.ERR_INVALID_ARGUMENT, dict(cfg=capi.make_collision_cfg(-1.0, -1.0, 0.0, 240, 120, *COLL))),
             (capi.ERR_UNSUPPORTED, dict(cfg=capi.make_collision_cfg(-1.0, -1.0, r_out / 1024.5, 240, 120, *COLL))),
             (capi.ERR_UNSUPPORTED, dict(dwa=pr.with_(DWA["omni"], ns=(17, 17, 29)))),
             (capi.ERR_INVALID_ARGUMENT, dict(dwa=pr.with_(DWA["omni"], horizon=6.0)))]      # 60 steps past the 50 columns of optTraj
    for status, kw in cases:
        with pytest.raises(capi.EngineError) as ei:
            tick(**kw)
        assert ei.value.status == status, (kw, ei.value)
    tick(n=0)
    torch.cuda.synchronize()
    assert bool((follow == 1).all()) and bool((count == 3).all()) and bool((valid == -1).all()) and bool((skip == -1).all())
    assert bool((u == 7.0).all())
    eng.close()

"""Parity of the batched DynamicWindow::control kernel (both overloads) against the CPU oracle.
The sample grid, the window and the control-error cost are computed from identical doubles on
both sides (the kernel is built without FMA contraction), so the chosen twist must be bitwise
equal; only the pose rollout goes through the device sincos, so a robot whose rollout passes
within an ulp of a cell edge, or two samples whose trajectory costs tie to the last bit, could
legitimately differ -- none are allowed in the `vref` mode, a handful in the `traj` mode.

Below the two yaml windows: the sample counts at which the kernel takes another path (one wavefront up to 64 samples, 128
threads up to 128, the strided loop beyond, 8192 = all 64 KiB of LDS, 8193+ refused), windows the velocity limits clip to
`lower > upper`, rollouts of no steps, a map without a free sample, EXACT cost ties (the first minimum in the reference's loop
order must win, within one stride of the sample loop and across strides), and the reference trajectory's edges: one column,
the longest rollout a reference can serve, headings on the +-pi seam -- and the refusal of a rollout that would read past its
reference (eea_dwa_control_batch, ergodic_amd.h).  test_both_implementations_forced (test_gpu_collision_parity.py) re-runs
this file with the ring search and with the inflated map pinned."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pyoracle as po
from ergodic_exploration_amd import capi

pytestmark = pytest.mark.gpu

COLL = (0.7, 1.0, 0.2, 0.8)
# dt, horizon, acc_dt, acc_lim x/y/th, max/min vx, max/min vy, max/min w, samples (omni yaml: 3 x 8 x 5)
DWA_OMNI = (0.1, 1.0, 0.2, 1.0, 1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 2.0, -2.0, 3, 8, 5)
DWA_CART = (0.1, 2.0, 0.2, 2.5, 0.0, 1.0, 1.0, -1.0, 0.0, 0.0, 2.0, -2.0, 3, 1, 5)


def _world(seed):
    rng = np.random.default_rng(seed)
    xs, ys, res = 80, 60, 0.1
    data = np.zeros((ys, xs), dtype=np.int8)
    data[20:26, 30:38] = 100
    data[45:48, 10:30] = 100
    data[rng.integers(0, ys, 20), rng.integers(0, xs, 20)] = 100
    data[5:9, 60:70] = -1
    g = po.GridMap(-2.0, -2.0 + xs * res, -1.0, -1.0 + ys * res, res, data.reshape(-1))
    cfg = capi.make_collision_cfg(-2.0, -1.0, res, xs, ys, *COLL)
    return g, cfg, data, rng


@pytest.mark.parametrize("dwa", [DWA_OMNI, DWA_CART])
def test_dwa_vref_mode_bitwise(dwa):
    g, ccfg, data, rng = _world(3)
    P = 600
    x0 = np.stack([rng.uniform(-1.5, 5.5, P), rng.uniform(-0.5, 4.5, P), rng.uniform(-np.pi, np.pi, P)], 1)
    vb = np.stack([rng.uniform(-1, 1, P), rng.uniform(-1, 1, P) * (dwa[8] != 0), rng.uniform(-2, 2, P)], 1)
    vref = np.stack([rng.uniform(-1, 1, P), rng.uniform(-1, 1, P) * (dwa[8] != 0), rng.uniform(-2, 2, P)], 1)
    d_u = torch.empty((P, 3), dtype=torch.float64, device="cuda")
    d_f = torch.full((P,), -1, dtype=torch.int32, device="cuda")
    capi.dwa_control_batch(ccfg, capi.DwaCfg(*dwa), torch.as_tensor(data).cuda(), torch.as_tensor(x0).cuda(),
                           torch.as_tensor(vb).cuda(), d_u, d_f, vref=torch.as_tensor(vref).cuda())
    torch.cuda.synchronize()
    u, f = d_u.cpu().numpy(), d_f.cpu().numpy()
    n_found = 0
    for i in range(P):
        ok, uo, _ = po.dwa_control(dwa, COLL, g, x0[i], vb[i], vref=vref[i])
        assert bool(f[i]) == ok, i
        assert np.array_equal(u[i], uo), (i, u[i], uo)
        n_found += ok
    assert 0 < n_found < P  # both outcomes exercised ("DWA Failed" and a valid twist)


def test_dwa_traj_mode():
    g, ccfg, data, rng = _world(5)
    P, n_ref, dt_ref = 300, 50, 0.1
    x0 = np.stack([rng.uniform(-1.5, 5.5, P), rng.uniform(-0.5, 4.5, P), rng.uniform(-np.pi, np.pi, P)], 1)
    vb = np.stack([rng.uniform(-1, 1, P), rng.uniform(-1, 1, P), rng.uniform(-2, 2, P)], 1)
    # reference trajectories: constant-twist arcs from the start pose
    xt = np.empty((P, n_ref, 3))
    for i in range(P):
        x = x0[i].copy()
        tw = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-2, 2)])
        for t in range(n_ref):
            x = po.integrate_twist(x, tw, dt_ref)
            xt[i, t] = x
    d_u = torch.empty((P, 3), dtype=torch.float64, device="cuda")
    d_f = torch.full((P,), -1, dtype=torch.int32, device="cuda")
    capi.dwa_control_batch(ccfg, capi.DwaCfg(*DWA_OMNI), torch.as_tensor(data).cuda(), torch.as_tensor(x0).cuda(),
                           torch.as_tensor(vb).cuda(), d_u, d_f, xt_ref=torch.as_tensor(xt).cuda(), dt_ref=dt_ref)
    torch.cuda.synchronize()
    u, f = d_u.cpu().numpy(), d_f.cpu().numpy()
    differ = 0
    for i in range(P):
        ok, uo, cost = po.dwa_control(DWA_OMNI, COLL, g, x0[i], vb[i], xt_ref=xt[i].T, dt_ref=dt_ref)
        assert bool(f[i]) == ok, i
        if not np.array_equal(u[i], uo):
            # a different choice is legitimate only as a floating-point tie: the oracle's own cost of the
            # kernel's twist must equal its minimum (the kernel's rollout goes through the device sincos)
            differ += 1
            c_gpu = po.dwa_objective_traj(DWA_OMNI, COLL, g, x0[i], u[i], xt[i].T, dt_ref)
            assert abs(c_gpu - cost) <= 1e-12 * max(1.0, abs(cost)), (i, u[i], uo, c_gpu, cost)
    assert differ <= 2, differ


# ---- window shapes, ties, the reference trajectory's edges ------------------------------------------------------------

def _with(dwa, ns=None, **kw):
    """the DWA tuple with other sample counts / fields (field order of capi.DwaCfg)"""
    d = dict(zip([n for n, _ in capi.DwaCfg._fields_], dwa))
    d.update(kw)
    if ns is not None:
        d["vx_samples"], d["vy_samples"], d["vth_samples"] = ns
    return tuple(d[n] for n, _ in capi.DwaCfg._fields_)


def _outputs(P):
    """u pre-filled with NaN and found with -1, so that a skipped write (or a write that should not happen) shows"""
    return (torch.full((P, 3), float("nan"), dtype=torch.float64, device="cuda"),
            torch.full((P,), -1, dtype=torch.int32, device="cuda"))


def _gpu(ccfg, dwa, data, x0, vb, vref=None, xt=None, dt_ref=0.0, out=None):
    """eea_dwa_control_batch on host arrays -> (u, found) as host arrays"""
    d_u, d_f = _outputs(len(x0)) if out is None else out
    dev = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()
    capi.dwa_control_batch(ccfg, capi.DwaCfg(*dwa), dev(data), dev(x0), dev(vb), d_u, d_f, vref=dev(vref), xt_ref=dev(xt),
                           dt_ref=dt_ref)
    torch.cuda.synchronize()
    return d_u.cpu().numpy(), d_f.cpu().numpy()


def _refused(status, P, *args, **kw):
    """the call raises EngineError(status) and writes neither u nor found"""
    out = _outputs(P)
    with pytest.raises(capi.EngineError) as ei:
        _gpu(*args, out=out, **kw)
    assert ei.value.status == status, ei.value
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[0]).all()) and bool((out[1] == -1).all())


def _poses(rng, P):
    return np.stack([rng.uniform(-1.5, 5.5, P), rng.uniform(-0.5, 4.5, P), rng.uniform(-np.pi, np.pi, P)], 1)


def _twists(rng, P):
    return np.stack([rng.uniform(-1, 1, P), rng.uniform(-1, 1, P), rng.uniform(-2, 2, P)], 1)


def _check_vref_bitwise(dwa, g, x0, vb, vref, u, f):
    n_found = 0
    for i in range(len(x0)):
        ok, uo, _ = po.dwa_control(dwa, COLL, g, x0[i], vb[i], vref=vref[i])
        assert int(f[i]) == int(ok), (i, f[i], ok)
        assert np.array_equal(u[i], uo), (i, u[i], uo)
        n_found += ok
    return n_found


@pytest.mark.parametrize("ns", [(1, 1, 1), (4, 4, 4), (5, 13, 1), (8, 4, 4), (3, 43, 1), (7, 11, 13), (0, 0, 5)])
def test_dwa_window_shapes_bitwise(ns):
    """1, 64 | 65, 128 | 129, 1001 samples: one wavefront | 128 threads | the strided sample loop; a count of 0 is raised to 1"""
    g, ccfg, data, rng = _world(7)
    P = 40
    dwa = _with(DWA_OMNI, ns=ns)
    x0, vb, vref = _poses(rng, P), _twists(rng, P), _twists(rng, P)
    u, f = _gpu(ccfg, dwa, data, x0, vb, vref=vref)
    assert 0 < _check_vref_bitwise(dwa, g, x0, vb, vref, u, f) < P


def test_dwa_8192_samples_fill_the_lds():
    """32 x 16 x 16 = 8192 samples: exactly the 64 KiB of dynamic LDS the launcher accepts"""
    g, ccfg, data, rng = _world(7)
    dwa = _with(DWA_OMNI, ns=(32, 16, 16))
    x0 = _poses(rng, 4)
    x0[0, :2] = 0.35, 1.3      # 0.65 m left of the block data[20:26, 30:38]: in collision wherever a 0.2 m/s window takes it
    x0[1, :2] = 3.0, 3.5       # open floor
    vb, vref = np.zeros((4, 3)), _twists(rng, 4)
    u, f = _gpu(ccfg, dwa, data, x0, vb, vref=vref)
    assert 0 < _check_vref_bitwise(dwa, g, x0, vb, vref, u, f) < 4


def test_dwa_more_than_8192_samples_is_refused():
    g, ccfg, data, rng = _world(7)
    x0, vb, vref = _poses(rng, 4), _twists(rng, 4), _twists(rng, 4)
    _refused(capi.ERR_UNSUPPORTED, 4, ccfg, _with(DWA_OMNI, ns=(17, 17, 29)), data, x0, vb, vref=vref)   # 8381 samples


def test_dwa_window_clipped_to_lower_above_upper():
    """odometry outside the velocity limits: lower = max(vb - a dt, vmin) > upper = min(vb + a dt, vmax), delta < 0"""
    g, ccfg, data, rng = _world(7)
    P = 40
    x0, vref = _poses(rng, P), _twists(rng, P)
    vb = np.tile([3.0, -3.0, 0.0], (P, 1))
    vb[P // 2:] = [-3.0, 0.5, 5.0]       # clipped from the other side; the heading axis clipped too
    lo = np.maximum(vb - 0.2, [-1.0, -1.0, -2.0])
    hi = np.minimum(vb + 0.2, [1.0, 1.0, 2.0])
    assert (lo[0] > hi[0])[:2].all() and (lo[-1] > hi[-1])[[0, 2]].all()     # the premise
    u, f = _gpu(ccfg, DWA_OMNI, data, x0, vb, vref=vref)
    assert 0 < _check_vref_bitwise(DWA_OMNI, g, x0, vb, vref, u, f) < P


def test_dwa_rollout_of_no_steps():
    """horizon < dt: no rollout step, so no collision test -- vref mode is the plain arg-min over the window, in traj mode
    every cost is 0 and the first sample (the window's lower corner) wins"""
    g, ccfg, data, rng = _world(7)
    P = 40
    dwa = _with(DWA_OMNI, horizon=0.05)
    assert po.steps(dwa[1], dwa[0]) == 0
    x0, vb, vref = _poses(rng, P), _twists(rng, P), _twists(rng, P)
    u, f = _gpu(ccfg, dwa, data, x0, vb, vref=vref)
    assert _check_vref_bitwise(dwa, g, x0, vb, vref, u, f) == P
    xt = np.tile(x0[:, None, :], (1, 3, 1))
    u, f = _gpu(ccfg, dwa, data, x0, vb, xt=xt, dt_ref=0.1)
    for i in range(P):
        ok, uo, cost = po.dwa_control(dwa, COLL, g, x0[i], vb[i], xt_ref=xt[i].T, dt_ref=0.1)
        assert ok and cost == 0.0 and f[i] == 1 and np.array_equal(u[i], uo), (i, u[i], uo)
        assert np.array_equal(uo, np.maximum(vb[i] - 0.2, [-1.0, -1.0, -2.0]))


def test_dwa_no_free_sample():
    """every cell occupied: found = 0 and u = (0, 0, 0) exactly (u_opt stays zero, dynamic_window.cpp:92-189)"""
    _, ccfg, data, rng = _world(7)
    full = np.full_like(data, 100)
    g = po.GridMap(-2.0, -2.0 + 80 * 0.1, -1.0, -1.0 + 60 * 0.1, 0.1, full.reshape(-1))
    P = 40
    x0, vb, vref = _poses(rng, P), _twists(rng, P), _twists(rng, P)
    u, f = _gpu(ccfg, DWA_OMNI, full, x0, vb, vref=vref)
    assert _check_vref_bitwise(DWA_OMNI, g, x0, vb, vref, u, f) == 0
    assert (f == 0).all() and np.array_equal(u, np.zeros((P, 3))) and not np.signbit(u).any()


def _free_world():
    xs, ys, res = 80, 60, 0.1
    data = np.zeros((ys, xs), dtype=np.int8)
    g = po.GridMap(-2.0, -2.0 + xs * res, -1.0, -1.0 + ys * res, res, data.reshape(-1))
    return g, capi.make_collision_cfg(-2.0, -1.0, res, xs, ys, *COLL), data


def _oracle_cost_of(dwa, g, x0, sample, vref):
    """the oracle's own cost of ONE sample of a robot at rest: a 1 x 1 x 1 window whose velocity limits pin the sample"""
    s = [float(v) for v in sample]
    one = _with(dwa, ns=(1, 1, 1), max_vel_x=s[0], min_vel_x=s[0], max_vel_y=s[1], min_vel_y=s[1], max_rot_vel=s[2],
                min_rot_vel=s[2])
    ok, u, cost = po.dwa_control(one, COLL, g, x0, np.zeros(3), vref=vref)
    assert ok and np.array_equal(u, s), (u, s)
    return cost


def test_dwa_exact_ties_take_the_first_sample_in_loop_order():
    """A robot at rest in free space: the control-error costs of mirrored samples are EQUAL doubles.  The reference keeps
    the first strict minimum of its vx / vy / vth loops (dynamic_window.cpp:92-189); an arg-min that scans in another order
    (a parallel reduction) would return another twist.  The premise -- the other sample's cost equals the minimum bitwise --
    is asserted with the oracle first."""
    g, ccfg, data = _free_world()
    x0, vb = np.array([[2.0, 2.0, 0.3]]), np.zeros((1, 3))
    # within one stride of the sample loop: 2 x 2 x 2, vref = 0 -- all eight costs are (0.04 + 0.04) + 0.04
    dwa, vref = _with(DWA_OMNI, ns=(2, 2, 2)), np.zeros((1, 3))
    ok, uo, cmin = po.dwa_control(dwa, COLL, g, x0[0], vb[0], vref=vref[0])
    assert ok and cmin == 0.12000000000000002 and np.array_equal(uo, [-0.2, -0.2, -0.2])
    for s in np.array(np.meshgrid([-0.2, 0.2], [-0.2, 0.2], [-0.2, 0.2])).reshape(3, -1).T:
        assert _oracle_cost_of(dwa, g, x0[0], s, vref[0]) == cmin, s
    u, f = _gpu(ccfg, dwa, data, x0, vb, vref=vref)
    assert f[0] == 1 and np.array_equal(u[0], uo), (u[0], uo)
    # across strides: 2 x 1 x 200, vref = (0, 0, w) with w the 78th value of the heading axis -- samples 77 and 277 tie
    dwa = _with(DWA_OMNI, ns=(2, 1, 200))
    lo, hi = max(0.0 - 1.0 * 0.2, -2.0), min(0.0 + 1.0 * 0.2, 2.0)
    delta, w = (hi - lo) / 199.0, lo
    for _ in range(77):
        w += delta
    vref = np.array([[0.0, 0.0, w]])
    ok, uo, cmin = po.dwa_control(dwa, COLL, g, x0[0], vb[0], vref=vref[0])
    assert ok and np.array_equal(uo, [-0.2, -0.2, w]) and abs(w + 0.0452) < 1e-4
    assert _oracle_cost_of(dwa, g, x0[0], [0.2, -0.2, w], vref[0]) == cmin     # sample 200 + 77
    u, f = _gpu(ccfg, dwa, data, x0, vb, vref=vref)
    assert f[0] == 1 and np.array_equal(u[0], uo) and u[0, 0] == -0.2, (u[0], uo)


def _arcs(rng, x0, n_ref, dt_ref):
    """reference trajectories: constant-twist arcs from the start poses, [P][n_ref][3]"""
    xt = np.empty((len(x0), n_ref, 3))
    for i in range(len(x0)):
        x, tw = x0[i].copy(), np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-2, 2)])
        for t in range(n_ref):
            x = po.integrate_twist(x, tw, dt_ref)
            xt[i, t] = x
    return xt


def _check_traj(dwa, g, x0, vb, xt, dt_ref, u, f):
    """the rule of test_dwa_traj_mode: a differing choice must be a tie of the oracle's own objective to 1e-12 relative, in
    at most 1 % of the robots"""
    P, differ, n_found = len(x0), 0, 0
    for i in range(P):
        ok, uo, cost = po.dwa_control(dwa, COLL, g, x0[i], vb[i], xt_ref=xt[i].T, dt_ref=dt_ref)
        assert int(f[i]) == int(ok), (i, f[i], ok)
        n_found += ok
        if not np.array_equal(u[i], uo):
            differ += 1
            c_gpu = po.dwa_objective_traj(dwa, COLL, g, x0[i], u[i], xt[i].T, dt_ref)
            assert abs(c_gpu - cost) <= 1e-12 * max(1.0, abs(cost)), (i, u[i], uo, c_gpu, cost)
    assert differ <= P // 100, differ
    return n_found


PI = float(np.pi)
SEAM = [PI, -PI, float(np.nextafter(PI, 0.0)), float(np.nextafter(-PI, 0.0)), 3.0 * PI, -3.0 * PI]


@pytest.mark.parametrize("case", ["one_column", "longest_rollout", "seam_headings"])
def test_dwa_traj_mode_edges(case):
    """n_ref = 1: the column index is always 0.  horizon 2.0 at dt = dt_ref = 0.1 on 19 columns: the last step reads column
    18 = n_ref - 1, the longest rollout this reference serves.  Reference headings at +-pi, one ulp inside and at +-3 pi: the
    double wrap of the heading cost (dynamic_window.cpp:280-282) on its seam.  (With these seeds no robot's two best costs
    of the oracle lie within 1e-9 relative of each other: a differing choice would not be an oracle-side tie.)"""
    g, ccfg, data, rng = _world(11)
    P = 100
    x0, vb = _poses(rng, P), _twists(rng, P)
    dwa, dt_ref = DWA_OMNI, 0.1
    if case == "one_column":
        xt = _arcs(rng, x0, 1, 0.5)
    elif case == "longest_rollout":
        dwa = _with(DWA_OMNI, horizon=2.0)
        xt = _arcs(rng, x0, 19, dt_ref)
    else:
        xt = _arcs(rng, x0, 12, dt_ref)
        xt[:, :, 2] = np.array(SEAM)[np.arange(P) % len(SEAM)][:, None]
    u, f = _gpu(ccfg, dwa, data, x0, vb, xt=xt, dt_ref=dt_ref)
    assert 0 < _check_traj(dwa, g, x0, vb, xt, dt_ref, u, f) < P


# ---- the reference index stays inside the reference --------------------------------------------------------------------

def test_dwa_reference_too_short_for_the_rollout_is_refused():
    """column round((n_ref - 1) t / (n_ref dt_ref)) of the reference is read at every rollout step (dynamic_window.cpp:277,
    where Armadillo's bounds check throws).  dt = dt_ref = 0.1, horizon 2.0: 20 and 19 columns serve it (largest index 18);
    on 18 columns the index reaches 18 = the first column of the NEXT robot -- refused before anything is launched, like
    dt_ref = 0 (a NaN index)."""
    g, ccfg, data, rng = _world(11)
    P = 40
    dwa = _with(DWA_OMNI, horizon=2.0)
    x0, vb = _poses(rng, P), _twists(rng, P)
    arcs = _arcs(rng, x0, 20, 0.1)
    for n_ref in (20, 19):
        xt = np.ascontiguousarray(arcs[:, :n_ref])
        u, f = _gpu(ccfg, dwa, data, x0, vb, xt=xt, dt_ref=0.1)
        assert 0 < _check_traj(dwa, g, x0, vb, xt, 0.1, u, f) < P
    for n_ref, dt_ref in ((18, 0.1), (20, 0.0), (20, -0.1), (20, float("nan"))):
        _refused(capi.ERR_INVALID_ARGUMENT, P, ccfg, dwa, data, x0, vb, xt=np.ascontiguousarray(arcs[:, :n_ref]), dt_ref=dt_ref)

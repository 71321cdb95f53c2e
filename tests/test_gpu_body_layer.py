"""The body layer on the device (eea_body_layer_* / eea_body_collision_check_batch / eea_body_validate_control_batch /
eea_body_dwa_control_batch / eea_tick_batch_bodies: csrc/body_layer_kernel.hip, csrc/footprint_plan_kernel.hip).

1. the maps and the snapshot table against tests/body_layer_restatement.py, exactly;
2. the check entry, 3. validate_control and the dynamic window against the restatement on what it calls decided;
   with d_sq == without d_sq == EEA_BODY_LAYER_NO_FILTER, bitwise, over ALL poses / robots, in every test;
4. the shapes at which the kernels take another path; 5. an empty layer is the plain footprint, bitwise;
6. the tick against the same loop written with the public pieces; its refusals."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ergodic_exploration_amd import capi
from tests import body_layer_restatement as br
from tests import footprint_plan_restatement as pr
from tests import footprint_restatement as fr
from tests.test_gpu_footprint_plan import Scene, _arcs, _check_one, dev

pytestmark = pytest.mark.gpu

NAMES = ("rect", "tri", "offc")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


class Bodies:
    """a Scene with two layers of one fleet on it, the second with EEA_BODY_LAYER_NO_FILTER; every call runs three ways (with
    d_sq, without, without any filter) and asserts the same bits over everything before it returns them once"""

    def __init__(self, w, verts, B, coll=pr.COLL):
        self.sc, self.w, self.verts, self.B = Scene(w, coll), w, verts, B
        fp = capi.Footprint.of(verts)
        self.layers = [capi.BodyLayer(self.sc.ccfg, fp, B), capi.BodyLayer(self.sc.ccfg, fp, B, flags=capi.BODY_LAYER_NO_FILTER)]
        self.ways = [(self.layers[0], self.sc.d_sq), (self.layers[0], None), (self.layers[1], self.sc.d_sq), (self.layers[1], None)]

    def update(self, poses, mask=None):
        for l in self.layers:
            l.update(dev(poses), dev(mask))

    def _same(self, outs):
        for o in outs[1:]:
            for x, y in zip(outs[0], o):
                assert np.array_equal(bits(x), bits(y))
        return outs[0]

    def check(self, poses, self_index=None, grid=True):
        outs = []
        for l, sq in self.ways:
            d_hit = torch.full((len(poses),), -1, dtype=torch.int32, device="cuda")
            l.check(self.sc.d_grid if grid else None, dev(poses), d_hit, sq=sq if grid else None, self_index=dev(self_index))
            torch.cuda.synchronize()
            outs.append((d_hit.cpu().numpy(),))
        return self._same(outs)[0]

    def validate(self, x0, u, dt, horizon, self_index):
        outs = []
        for l, sq in self.ways:
            d_v = torch.full((len(x0),), -1, dtype=torch.int32, device="cuda")
            l.validate(self.sc.d_grid, dev(x0), dev(u), dt, horizon, d_v, sq=sq, self_index=dev(self_index))
            torch.cuda.synchronize()
            outs.append((d_v.cpu().numpy(),))
        return self._same(outs)[0]

    def dwa(self, dwa, x0, vb, self_index, vref=None, xt=None, dt_ref=0.0):
        outs = []
        for l, sq in self.ways:
            d_u, d_f = self.sc.outputs(len(x0))
            l.dwa(capi.DwaCfg(*dwa), self.sc.d_grid, dev(x0), dev(vb), d_u, d_f, sq=sq, vref=dev(vref), xt_ref=dev(xt), dt_ref=dt_ref,
                  self_index=dev(self_index))
            torch.cuda.synchronize()
            outs.append((d_u.cpu().numpy(), d_f.cpu().numpy()))
        return self._same(outs)

    def close(self):
        for l in self.layers:
            l.close()


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


# ---- 1. the maps and the snapshot ------------------------------------------------------------------------------------------------

def _map_fleet(w, rng, B, box):
    """70 robots on a 150 x 40 grid: random ones, one in every corner, one across every edge, two coincident, one whose box
    misses the grid, NaN / +-inf / 1e9 components"""
    x_hi, y_hi = w.xmin + w.xs * w.res, w.ymin + w.ys * w.res
    nan, inf = float("nan"), float("inf")
    special = [(w.xmin + 0.031, w.ymin + 0.017), (x_hi - 0.023, w.ymin + 0.041), (w.xmin + 0.037, y_hi - 0.013), (x_hi - 0.011, y_hi - 0.029),
               (w.xmin - 0.213, 1.07), (x_hi + 0.187, 2.03), (3.11, w.ymin - 0.171), (7.07, y_hi + 0.233), (w.xmin - 0.613, y_hi + 0.577),
               (5.013, 1.507), (5.013, 1.507)]
    poses = np.stack([rng.uniform(w.xmin - 0.3, x_hi + 0.3, B), rng.uniform(w.ymin - 0.3, y_hi + 0.3, B), rng.uniform(-np.pi, np.pi, B)], 1)
    for k, (x, y) in enumerate(special):
        poses[k, :2] = x, y
    poses[10, 2] = poses[9, 2]                                   # coincident: the same pose twice
    poses[11] = [w.xmin - box * w.res - 0.35, 1.0, 0.4]          # the box misses the grid
    poses[12] = [x_hi + 2.0, y_hi + 2.0, 1.0]
    poses[13], poses[14], poses[15] = [nan, 1.0, 0.3], [2.0, nan, 0.3], [2.0, 1.0, nan]
    poses[16], poses[17], poses[18] = [inf, 1.0, 0.3], [2.0, -inf, 0.3], [2.0, 1.0, inf]
    poses[19], poses[20] = [1e9, 1.0, 0.3], [2.0, -1e9, 0.3]
    return poses


@pytest.mark.parametrize("name", NAMES)
def test_maps_and_snapshot_are_the_restatements(name):
    rng = np.random.default_rng(31)
    xs, ys, B = 150, 40, 70
    w = pr.World(np.zeros((ys, xs), dtype=np.int8), 0.1, -1.0, -0.5)
    w.data[rng.integers(0, ys, 40), rng.integers(0, xs, 40)] = 100          # (a body is stamped whatever the cells hold)
    verts = fr.FOOTPRINTS[name]
    ccfg = capi.make_collision_cfg(w.xmin, w.ymin, w.res, xs, ys, *pr.COLL)
    layer = capi.BodyLayer(ccfg, capi.Footprint.of(verts), B)
    box = br.box_of(w, verts)
    assert layer.box == box and layer.near_shape == (ys + 2 * box, xs + 2 * box)
    # before the first update: nothing
    cover, near, snap = layer.read()
    assert not cover.any() and not near.any() and not snap.any()
    poses = _map_fleet(w, rng, B, box)
    masks = [None, i32(rng.integers(0, 3, B) != 0), i32(np.ones(B))]
    masks[1][[0, 9]] = [0, 1]
    rounds = []
    stream = torch.cuda.current_stream().cuda_stream
    L = capi.lib()
    GUARD, n_c, n_n = 64, ys * xs, (ys + 2 * box) * (xs + 2 * box)
    for k in range(3):                                  # three updates on one stream, read after each
        p = poses.copy()
        if k:
            p[21:, :2] += rng.uniform(-0.4, 0.4, (B - 21, 2))
            p[:, 2] = np.where(np.isfinite(p[:, 2]), p[:, 2] + 0.37 * k, p[:, 2])
        layer.update(dev(p), dev(masks[k]), stream=stream)
        # the maps as read back sit between guard words
        h_c, h_n = np.full(n_c + 2 * GUARD, -77, dtype=np.int32), np.full(n_n + 2 * GUARD, -77, dtype=np.int32)
        h_s = np.full(B * 5 + 2 * GUARD, -77.0)
        capi.check(L.eea_body_layer_read(layer.h, C.c_void_p(h_c.ctypes.data + 4 * GUARD), C.c_void_p(h_n.ctypes.data + 4 * GUARD),
                                         C.c_void_p(h_s.ctypes.data + 8 * GUARD)))
        for h, n in ((h_c, n_c), (h_n, n_n), (h_s, 5 * B)):
            assert (h[:GUARD] == -77).all() and (h[GUARD + n:] == -77).all()
        rounds.append((p, masks[k], h_c[GUARD:GUARD + n_c].reshape(ys, xs), h_n[GUARD:GUARD + n_n].reshape(ys + 2 * box, xs + 2 * box),
                       h_s[GUARD:GUARD + 5 * B].reshape(B, 5)))
    for k, (p, mask, cover, near, snap) in enumerate(rounds):
        ref = br.Layer(w, verts, p, mask)
        assert ref.decided()[ref.flags].all()                      # a condition of the scene: every stamped robot is decided
        assert np.array_equal(snap[:, 4] != 0.0, ref.flags), k
        assert not ref.flags[11:21].any() and (k == 1 or ref.flags[:11].all())
        assert np.array_equal(cover, ref.cover), (k, np.argwhere(cover != ref.cover)[:5])
        assert np.array_equal(near, ref.near), (k, np.argwhere(near != ref.near)[:5])
        assert np.array_equal(snap[:, :2], ref.snapshot[:, :2]) and np.abs(snap[:, 2:4] - ref.snapshot[:, 2:4]).max() < 1e-15
        assert not snap[~ref.flags].any()
        assert cover.max() >= 2 and (k == 1 or cover[ref.covers[9]].min() >= 2)          # the coincident pair
        rim = np.ones((ys, xs), dtype=bool)
        rim[1:-1, 1:-1] = False
        assert k == 1 or sum(bool((ref.covers[j] & rim).any()) for j in range(9)) >= 4      # bodies that reach the grid's edge
    # an update after every robot is masked leaves both maps zero
    layer.update(dev(poses), dev(i32(np.zeros(B))), stream=stream)
    cover, near, snap = layer.read()
    assert not cover.any() and not near.any() and not snap.any()
    layer.close()


# ---- 2. the check entry ----------------------------------------------------------------------------------------------------------

def _fleet13(w, verts, rng):
    """13 robots on world(7): free on the static grid, bodies apart except one pair that overlaps; one masked"""
    cand = np.stack([rng.uniform(-1.5, 5.5, 200), rng.uniform(-0.5, 4.5, 200), rng.uniform(-np.pi, np.pi, 200)], 1)
    free = ~pr.verdicts(w, verts, cand)[0]
    taken, union = [], np.zeros((w.ys, w.xs), dtype=bool)
    for q in range(200):
        body = br.cover(w, verts, cand[q])[0]
        if free[q] and not (body & union).any():
            taken.append(q)
            union |= body
        if len(taken) == 12:
            break
    poses = np.concatenate([cand[taken], cand[taken[3]][None] + [0.21, 0.13, 0.5]])
    mask = i32(np.ones(13))
    mask[5] = 0
    return poses, mask


@pytest.mark.parametrize("name", NAMES)
def test_check_against_the_restatement(name):
    w, rng = pr.world(7)
    verts = fr.FOOTPRINTS[name]
    poses, mask = _fleet13(w, verts, rng)
    B = len(poses)
    bd = Bodies(w, verts, B)
    bd.update(poses, mask)
    ref = br.Layer(w, verts, poses, mask)
    assert ref.decided()[ref.flags].all() and ref.flags.sum() == B - 1 and ref.cover.max() == 2
    for P in (1, 63, 64, 65, 257):
        # poses near the robots (their own, nudged) and anywhere
        own = rng.integers(0, B, P)
        q = poses[own] + np.stack([rng.normal(0, 0.3, P), rng.normal(0, 0.3, P), rng.normal(0, 0.5, P)], 1)
        far = rng.uniform(0, 1, P) < 0.3
        q[far] = np.stack([rng.uniform(-2.5, 6.5, P), rng.uniform(-1.5, 5.5, P), rng.uniform(-np.pi, np.pi, P)], 1)[far]
        q[0] = poses[own[0]]                                      # a robot where it stands
        other = (own + 1 + rng.integers(0, B - 1, P)) % B
        for idx, grid in ((own, True), (other, True), (np.full(P, -1), True), (None, True), (own, False), (None, False)):
            hit = bd.check(q, None if idx is None else i32(idx), grid=grid)
            want, margin = br.check(ref, q, idx, static=grid)
            ok = margin >= fr.DECIDED
            assert ok.sum() >= P - P // 50 and ok[0]            # (pose 0 is a robot where it stands: the only pose of P = 1)
            assert np.array_equal(hit[ok], want[ok].astype(np.int32)), (P, grid, np.nonzero(hit[ok] != want[ok])[0][:5])
            assert set(np.unique(hit)) <= {0, 1}
        if P >= 63:
            mine, others = br.check(ref, q, own)[0], br.check(ref, q, other)[0]
            assert 0 < mine.sum() < P and (mine != others).any()
    # where it stands a robot is free as itself and a hit as anybody else, the overlapping pair a hit either way
    me = np.arange(B)
    stand = bd.check(poses, i32(me))
    solo = [j for j in range(B) if ref.flags[j] and (ref.cover[ref.covers[j]] == 1).all()]
    assert len(solo) >= 8 and not stand[solo].any() and stand[3] == 1 and stand[12] == 1
    assert bd.check(poses, None)[solo].all()
    bd.close()


# ---- 3. validate_control and the dynamic window on the study fleets --------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_window_and_validate_against_the_restatement(name):
    w, x0, vb, vref, xt, robots = pr.study()
    idx, ref = br.greedy_fleet(name)
    B = len(idx)
    verts = fr.FOOTPRINTS[name]
    bd = Bodies(w, verts, B)
    bd.update(x0[idx])
    me = i32(np.arange(B))
    cover, _, snap = bd.layers[0].read()
    assert np.array_equal(cover, ref.cover) and (snap[:, 4] == 1.0).all()
    # the window, twist-error mode: bitwise on the decided robots
    u, f = bd.dwa(pr.DWA_OMNI, x0[idx], vb[idx], me, vref=vref[idx])
    answers = br.fleet_answers(name)
    n_dec = changed = 0
    for i, (plain, a) in enumerate(answers):
        if a.decided:
            _check_one(a, i, u[i], f[i], traj=False)
            n_dec += 1
            changed += int(a.found != plain.found or not np.array_equal(a.u_opt, plain.u_opt))
    assert n_dec >= B - (2 * B) // 100 and changed >= 5 and 0 < sum(a.found for _, a in answers) < B
    # ... the layer is what changed them: the plain entry gives the plain answers
    up, fp_ = bd.sc.dwa_both(pr.DWA_OMNI, verts, x0[idx], vb[idx], vref=vref[idx])
    for i, (plain, _) in enumerate(answers):
        if plain.decided:
            _check_one(plain, i, up[i], fp_[i], traj=False)
    # trajectory mode, the whole fleet (test_dwa_traj_mode's tie rule)
    u, f = bd.dwa(pr.DWA_OMNI, x0[idx], vb[idx], me, xt=xt[idx], dt_ref=pr.DT_REF)
    n_dec = 0
    for i, (_, a) in enumerate(br.fleet_answers(name, "traj")):
        if a.decided:
            _check_one(a, i, u[i], f[i], traj=True)
            n_dec += 1
    assert n_dec >= B - (2 * B) // 100
    # validate_control of the study's vref over 5 steps
    plain, with_, decided = br.fleet_validate(name)
    v = bd.validate(x0[idx], vref[idx], br.VAL_DT, br.VAL_HORIZON, me)
    assert decided.sum() >= B - (2 * B) // 100 and np.array_equal(v[decided], with_[decided]) and (plain != with_).sum() >= 5
    # as nobody's poses every robot starts inside its own body; as each other's, inside that one's
    assert not bd.validate(x0[idx], np.zeros((B, 3)), 0.1, 0.1, i32(np.full(B, -1))).any()
    assert not bd.validate(x0[idx], np.zeros((B, 3)), 0.1, 0.1, i32(np.roll(me, 1))).any()
    assert bd.validate(x0[idx], np.zeros((B, 3)), 0.1, 0.1, me).all()
    bd.close()


# ---- 4. shapes -------------------------------------------------------------------------------------------------------------------

def _small_fleet(name="rect", n=16):
    """the first n robots of the study's greedy fleet, their restatement layer, and a Bodies updated with them"""
    w, x0, vb, vref, xt, robots = pr.study()
    idx, _ = br.greedy_fleet(name)
    idx = idx[:n]
    verts = fr.FOOTPRINTS[name]
    ref = br.Layer(w, verts, x0[idx])
    bd = Bodies(w, verts, n)
    bd.update(x0[idx])
    return bd, ref, x0[idx], vb[idx], vref[idx], xt[idx]


def _against(bd, ref, dwa, x0, vb, vref, me, xt=None, min_decided=None):
    u, f = bd.dwa(dwa, x0, vb, me, vref=vref if xt is None else None, xt=xt, dt_ref=0.1 if xt is not None else 0.0)
    n_dec = n_found = 0
    for i in range(len(x0)):
        a = br.dwa_control(ref, dwa, pr.Robot(dwa, x0[i], vb[i]), int(me[i]), vref=None if xt is not None else vref[i],
                           xt=None if xt is None else xt[i], dt_ref=0.1)
        if a.decided:
            _check_one(a, i, u[i], f[i], traj=xt is not None)
            n_dec += 1
            n_found += a.found
    assert n_dec >= (len(x0) - 1 if min_decided is None else min_decided)
    return u, f, n_found


@pytest.mark.parametrize("ns", [(1, 1, 1), (4, 4, 4), (5, 13, 1), (3, 43, 1)])
def test_sample_counts(ns):
    """1, 64 | 65 | 129 samples: one wavefront | 128 threads | the strided sample loop; both modes"""
    bd, ref, x0, vb, vref, xt = _small_fleet(n=12)
    me = i32(np.arange(12))
    dwa = pr.with_(pr.DWA_OMNI, ns=ns)
    _, f, n_found = _against(bd, ref, dwa, x0, vb, vref, me)
    assert ns == (1, 1, 1) or 0 < n_found < 12
    _against(bd, ref, dwa, x0, vb, vref, me, xt=np.ascontiguousarray(xt[:, :25]))
    bd.close()


@pytest.mark.parametrize("horizon,steps", [(0.05, 0), (0.1, 1)])
def test_rollouts_of_no_and_one_step(horizon, steps):
    bd, ref, x0, vb, vref, xt = _small_fleet("tri", n=12)
    me = i32(np.arange(12))
    dwa = pr.with_(pr.DWA_OMNI, horizon=horizon)
    assert pr.steps_of(dwa) == steps
    # (as robot (i + 1)'s poses, so that bodies are met at the first step)
    for idx in (me, i32(np.roll(me, 1))):
        _, f, n_found = _against(bd, ref, dwa, x0, vb, vref, idx)
        assert n_found == 12 if steps == 0 else (n_found > 0 if idx is me else n_found == 0)
        v = bd.validate(x0, vref, 0.1, horizon, idx)
        want, decided = br.validate(ref, x0, vref, 0.1, horizon, idx)
        assert np.array_equal(v[decided], want[decided]) and decided.sum() >= 11
    bd.close()


def test_window_path_and_memory_path():
    """the same robots through the LDS window and from memory -- a launch whose limits (30 m/s: a window of 97 KB) reserve no
    window; the odometry within 0.8 of the limits, so the limits bind nowhere and the samples are the same doubles -- give the
    same bits; a robot whose odometry is at twice the limits leaves the window path on its own"""
    bd, ref, x0, vb, vref, xt = _small_fleet(n=16)
    me = i32(np.arange(16))
    vb = np.clip(vb, [-0.8, -0.8, -1.8], [0.8, 0.8, 1.8])
    wide = pr.with_(pr.DWA_OMNI, max_vel_x=30.0, min_vel_x=-30.0, max_vel_y=30.0, min_vel_y=-30.0)
    side = 2 * (pr.limits_reach(wide, bd.w.res) + ref.box) + 1
    assert side * ((side + 63) // 64) * 8 + 8 * 120 > 64 * 1024
    for kw in (dict(), dict(xt=np.ascontiguousarray(xt[:, :25]))):
        u, f, n_found = _against(bd, ref, pr.DWA_OMNI, x0, vb, vref, me, **kw)
        u2, f2, _ = _against(bd, ref, wide, x0, vb, vref, me, **kw)
        assert np.array_equal(bits(u), bits(u2)) and np.array_equal(f, f2) and 0 < n_found < 16
    fast = vb.copy()
    fast[0:6] = [2.0, 2.0, 4.0]
    fast[6:8] = [3.0, -3.0, 0.0]
    own = np.array([pr.reach(pr.DWA_OMNI, fast[q], bd.w.res) for q in range(16)])
    assert (own[:8] > pr.limits_reach(pr.DWA_OMNI, bd.w.res)).all() and (own[8:] <= pr.limits_reach(pr.DWA_OMNI, bd.w.res)).all()
    _against(bd, ref, pr.DWA_OMNI, x0, fast, vref, me)
    bd.close()


def _window_holds_a_body(ref, dwa, poses):
    """per robot: does the window its workgroup stages (the cells within the limits' reach + box of its own) hold a cell of
    another robot's body?"""
    w = ref.w
    rw = int(pr.limits_reach(dwa, w.res)) + ref.box
    fx, fy = br.cells_of(w, poses)
    holds = []
    for i in range(len(poses)):
        others = ref.cover - (ref.covers[i] if ref.covers[i] is not None else 0)
        y0, x0 = max(int(fy[i]) - rw, 0), max(int(fx[i]) - rw, 0)
        holds.append(bool(others[y0:int(fy[i]) + rw + 1, x0:int(fx[i]) + rw + 1].any()))
    return holds


@pytest.mark.parametrize("name", NAMES)
def test_staging_flag_on_both_sides(name):
    """two robots a metre apart and one alone in the far corner of world(7): the first two stage body bits, the third's window
    holds none and the field alone decides its free poses"""
    w, rng = pr.world(7)
    verts = fr.FOOTPRINTS[name]
    poses = np.array([[2.53, 2.61, 0.4], [3.91, 2.93, -2.0], [-1.23, 0.07, 1.1]])
    ref = br.Layer(w, verts, poses)
    assert ref.flags.all() and ref.decided().all() and ref.cover.max() == 1 and not pr.verdicts(w, verts, poses)[0][[0, 2]].any()
    assert _window_holds_a_body(ref, pr.DWA_OMNI, poses) == [True, True, False]
    bd = Bodies(w, verts, 3)
    bd.update(poses)
    me = i32(np.arange(3))
    vb = np.array([[0.5, 0.1, 0.0], [0.5, -0.1, 0.3], [0.2, 0.2, -0.5]])
    vref = np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 0.5, 0.0]])
    _, f, n_found = _against(bd, ref, pr.DWA_OMNI, poses, vb, vref, me, min_decided=3)
    plain = [pr.dwa_control(w, verts, pr.DWA_OMNI, pr.Robot(pr.DWA_OMNI, poses[i], vb[i]), vref=vref[i]) for i in range(3)]
    mine = [br.dwa_control(ref, pr.DWA_OMNI, pr.Robot(pr.DWA_OMNI, poses[i], vb[i]), i, vref=vref[i]) for i in range(3)]
    assert not np.array_equal(plain[0].free, mine[0].free) and np.array_equal(plain[2].free, mine[2].free)
    _against(bd, ref, pr.DWA_OMNI, poses, vb, vref, i32([-1, 0, -1]), min_decided=3)
    bd.close()


def test_two_robots_nose_to_nose():
    """the fact scene of tests/test_body_layer.py on the device: two `rect` robots 1.0 m apart along x, facing each other.
    Forward at 1 m/s collides (at the second step), backward does not; as nobody's, a robot collides with "itself" where it
    stands; the window of robot 0 keeps its backward samples and loses every sample as nobody's"""
    from tests import clearance_restatement as cr
    w = pr.World(fr.fact_scene([]), cr.RES41, cr.XMIN41, cr.YMIN41)
    verts = fr.FOOTPRINTS["rect"]
    (ax, ay), (bx, by) = fr.centre41(15, 20), fr.centre41(25, 20)
    poses = np.array([[ax, ay, 0.0], [bx, by, np.pi]])
    ref = br.Layer(w, verts, poses)
    assert ref.flags.all() and ref.decided().all()
    bd = Bodies(w, verts, 2)
    bd.update(poses)
    cover, _, _ = bd.layers[0].read()
    assert np.array_equal(cover, ref.cover) and cover.sum() == 2 * 9 * 5
    me = i32([0, 1])
    fwd, back = np.array([[1.0, 0.0, 0.0]] * 2), np.array([[-1.0, 0.0, 0.0]] * 2)
    assert not bd.validate(poses, fwd, 0.1, 1.0, me).any() and bd.validate(poses, back, 0.1, 1.0, me).all()
    assert bd.validate(poses, fwd, 0.1, 0.1, me).all()                      # one step: still apart
    assert not bd.validate(poses, back, 0.1, 1.0, i32([-1, -1])).any()      # "itself", at step 0
    roll = pr.rollout(poses[0], fwd[0], 0.1, 10)
    hit = bd.check(roll, i32(np.zeros(10)))
    assert hit[0] == 0 and hit[1] == 1 and np.array_equal(hit, br.check(ref, roll, np.zeros(10, dtype=int))[0].astype(np.int32))
    assert not bd.check(poses, me).any() and bd.check(poses, me[::-1].copy()).all() and bd.check(poses, None).all()
    assert bd.check(poses, None, grid=False).all() and not bd.check(poses, me, grid=False).any()
    x0, vb, vref = poses[:1], np.zeros((1, 3)), np.array([[0.2, 0.0, 0.0]])
    u, f, _ = _against(bd, ref, pr.DWA_OMNI, x0, vb, vref, i32([0]), min_decided=1)
    assert f[0] == 1
    u, f, _ = _against(bd, ref, pr.DWA_OMNI, x0, vb, vref, i32([-1]), min_decided=1)
    assert f[0] == 0 and not u.any()
    bd.close()


@pytest.mark.parametrize("P", [1, 63, 64, 65, 257])
def test_validate_batch_sizes(P):
    bd, ref, x0, vb, vref, _ = _small_fleet("offc", n=16)
    rng = np.random.default_rng(P)
    own = rng.integers(0, 16, P)
    idx = np.where(rng.uniform(0, 1, P) < 0.7, own, rng.integers(-1, 16, P))
    u = np.stack([rng.uniform(-1, 1, P), rng.uniform(-1, 1, P), rng.uniform(-2, 2, P)], 1)
    v = bd.validate(x0[own], u, 0.1, 0.6, i32(idx))
    want, decided = br.validate(ref, x0[own], u, 0.1, 0.6, idx)
    assert np.array_equal(v[decided], want[decided]) and decided.sum() >= P - max(1, P // 50)
    assert P < 63 or 0 < want.sum() < P
    bd.close()


# ---- 5. the empty layer ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["never_updated", "all_masked"])
def test_an_empty_layer_is_the_plain_footprint(how):
    w, x0, vb, vref, xt, _ = pr.study()
    P = 96
    x0, vb, vref, xt = x0[:P], vb[:P], vref[:P], xt[:P]
    verts = fr.FOOTPRINTS["rect"]
    bd = Bodies(w, verts, P)
    if how == "all_masked":
        bd.update(x0)
        bd.update(x0, i32(np.zeros(P)))
    me = i32(np.arange(P))
    sc, fp = bd.sc, capi.Footprint.of(verts)
    for idx in (me, None):
        d_hit = torch.full((P,), -1, dtype=torch.int32, device="cuda")
        capi.footprint_check_batch(sc.ccfg, fp, sc.d_grid, dev(x0), d_hit, sq=sc.d_sq)
        torch.cuda.synchronize()
        assert np.array_equal(bd.check(x0, idx), d_hit.cpu().numpy())
        assert np.array_equal(bd.validate(x0, vref, 0.1, 1.0, idx), sc.validate_both(verts, x0, vref, 0.1, 1.0))
        for kw in (dict(vref=vref), dict(xt=xt, dt_ref=pr.DT_REF)):
            u, f = bd.dwa(pr.DWA_OMNI, x0, vb, idx, **kw)
            u0, f0 = sc.dwa_both(pr.DWA_OMNI, verts, x0, vb, **kw)
            assert np.array_equal(bits(u), bits(u0)) and np.array_equal(f, f0)
    assert not bd.check(x0, None, grid=False).any()
    bd.close()


# ---- 6. the tick -----------------------------------------------------------------------------------------------------------------

def _start_poses(worlds, verts, B):
    """B poses in the clusters of test_gpu_footprint_plan's tick scene, free on both grids, their bodies apart with a cell to
    spare"""
    rng = np.random.default_rng(4)
    n = 240
    ys, xs = worlds[0].data.shape
    cand = np.stack([rng.uniform(0.2, 9.5, n), rng.uniform(-0.2, 4.2, n), rng.uniform(-0.6, 0.6, n)], 1)
    cand[:60, 0], cand[:60, 1], cand[:60, 2] = rng.uniform(0.6, 2.0, 60), rng.uniform(0.2, 3.4, 60), rng.uniform(-0.2, 0.2, 60)
    cand[60:100, 0], cand[60:100, 1] = rng.uniform(3.2, 3.8, 40), rng.uniform(0.0, 4.0, 40)
    free = pr.validate(worlds[1], verts, cand, np.zeros((n, 3)), 0.1, 0.1)[0] == 1
    taken, union = [], np.zeros((ys, xs), dtype=bool)
    for q in range(n):
        body = br.cover(worlds[0], verts, cand[q])[0]
        grown = body.copy()
        grown[1:] |= body[:-1]
        grown[:-1] |= body[1:]
        grown[:, 1:] |= grown[:, :-1].copy()
        grown[:, :-1] |= grown[:, 1:].copy()
        if free[q] and not (grown & union).any():
            taken.append(q)
            union |= body
        if len(taken) == B:
            break
    assert len(taken) == B
    return cand[taken]


class _Tick:
    """the engine, the two grids (a wall appears at tick 5) and 24 robots whose bodies are apart at the start"""

    def __init__(self, B=24):
        from tests.test_host_mirror import COLL, DWA, _grid_with
        self.B, self.ticks, self.wall_tick, self.dt = B, 12, 5, 0.1
        obstacles = [(2.4, 0.2, 3.0, 2.6), (6.0, 2.0, 6.5, 4.6), (8.8, -0.4, 9.4, 1.2)]
        grid_a, bounds = _grid_with(obstacles)
        grid_b, _ = _grid_with(obstacles + [(4.2, -0.6, 4.5, 4.4)])
        xs, ys, res = grid_a.xsize, grid_a.ysize, 0.05
        self.worlds = [pr.World(np.asarray(g.data, dtype=np.int8).reshape(ys, xs), res, bounds[0], bounds[2]) for g in (grid_a, grid_b)]
        self.scenes = [Scene(wd, coll=COLL) for wd in self.worlds]
        self.ccfg, self.dwa = self.scenes[0].ccfg, DWA["omni"]
        self.dcfg, self.verts = capi.DwaCfg(*self.dwa), fr.FOOTPRINTS["rect"]
        self.fp = capi.Footprint.of(self.verts)
        lim = np.array([1.0, 1.0, 2.0])
        self.eng = capi.Engine(capi.make_config(capi.MODEL_OMNI, 0.1, 5.0, 0.1, 1.0, 10, np.diag([1.0, 1.0, 2.0]), -lim, lim))
        self.eng.set_target_gaussians([[2.5, 2.5], [8.5, 2.5]], [[1.5, 1.5], [1.5, 1.5]])
        self.eng.config_domain(bounds)
        self.T = self.eng.T
        self.poses = _start_poses(self.worlds, self.verts, B)

    def state(self):
        B, T = self.B, self.T
        zeros = lambda shape, t: torch.zeros(shape, dtype=t, device="cuda")

        class State:
            pass
        s = State()
        s.ut, s.u, s.traj = zeros((B, T, 3), torch.float64), zeros((B, 3), torch.float64), zeros((B, T, 3), torch.float64)
        s.follow, s.count = zeros((B,), torch.int32), zeros((B,), torch.int32)
        s.valid, s.skip = torch.full((B,), -1, dtype=torch.int32, device="cuda"), zeros((B,), torch.int32)
        s.source, s.status = torch.full((B,), -1, dtype=torch.int32, device="cuda"), zeros((B,), torch.int32)
        s.pose, s.vb = dev(self.poses), zeros((B, 3), torch.float64)
        return s

    def one_tick(self, kind, layer=None):
        """u, follow, count, valid, source, ut of ONE tick of the entry `kind` from the start state"""
        s, sc, B = self.state(), self.scenes[0], self.B
        args = (B, s.pose, s.ut, s.follow, s.count, s.u, s.vb, sc.d_grid, s.traj, s.valid, s.skip, self.ccfg, self.dcfg, 0.1, 0.5)
        if kind == "disc":
            self.eng.tick_batch(*args, source=s.source, status=s.status)
        elif kind == "fleet":
            self.eng.tick_batch_fleet(layer, *args, source=s.source, status=s.status)
        else:
            self.eng.tick_batch_footprint(self.fp, *args, sq=sc.d_sq, source=s.source, status=s.status)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in (s.u, s.follow, s.count, s.valid, s.source, s.ut)]

    def run(self, layer):
        """12 ticks on one stream without a host wait: update -> tick -> integrate; layer None: eea_tick_batch_footprint.
        Returns per tick the device copies (pose before the tick, u, follow, count, valid, source)"""
        s, out = self.state(), []
        stream = torch.cuda.current_stream().cuda_stream
        for t in range(self.ticks):
            sc = self.scenes[0] if t < self.wall_tick else self.scenes[1]
            before = s.pose.clone()
            args = (self.B, s.pose, s.ut, s.follow, s.count, s.u, s.vb, sc.d_grid, s.traj, s.valid, s.skip, self.ccfg, self.dcfg, 0.1, 0.5)
            if layer is not None:
                layer.update(s.pose, stream=stream)
                self.eng.tick_batch_bodies(layer, *args, sq=sc.d_sq, source=s.source, status=s.status, stream=stream)
            else:
                self.eng.tick_batch_footprint(self.fp, *args, sq=sc.d_sq, source=s.source, status=s.status, stream=stream)
            out.append([before] + [x.clone() for x in (s.u, s.follow, s.count, s.valid, s.source)])
            capi.integrate_twist_batch(s.pose, s.u, self.dt, stream=stream)
            s.vb.copy_(s.u)
        torch.cuda.synchronize()
        return [[x.cpu().numpy() for x in row] for row in out]


def test_tick_is_the_loop_of_the_public_pieces():
    tk = _Tick()
    B, eng = tk.B, tk.eng
    dwa_steps = pr.steps_of(tk.dwa)
    layer = capi.BodyLayer(tk.ccfg, tk.fp, B)
    fleet = capi.FleetLayer(tk.ccfg, 10, B)
    fleet.update(dev(tk.poses))
    before = [tk.one_tick(k, fleet) for k in ("disc", "fleet", "foot")]
    got = tk.run(layer)
    # the same with the public pieces
    b = tk.state()
    seen = set()
    for t in range(tk.ticks):
        sc = tk.scenes[0] if t < tk.wall_tick else tk.scenes[1]
        assert np.array_equal(bits(b.pose.cpu().numpy()), bits(got[t][0])), t
        layer.update(b.pose)
        follow, count = b.follow.cpu().numpy().copy(), b.count.cpu().numpy().copy()
        for r in range(B):                                         # step 1 (exploration.hpp:223-228)
            if follow[r]:
                count[r] += 1
                follow[r] = 1 if count[r] != dwa_steps else 0
        b.skip = dev(follow)
        eng.control_batch(B, b.pose, b.ut, b.u, skip=b.skip, status=b.status)          # step 2
        eng.rollout_batch(B, b.pose, b.ut, b.traj)
        me = dev(i32(np.arange(B)))
        layer.validate(sc.d_grid, b.pose, b.u, 0.1, 0.5, b.valid, sq=sc.d_sq, self_index=me)      # step 3
        u_f, f_f = sc.outputs(B)
        u_t, f_t = sc.outputs(B)
        layer.dwa(tk.dcfg, sc.d_grid, b.pose, b.vb, u_f, f_f, sq=sc.d_sq, vref=b.u, self_index=me)    # step 4
        layer.dwa(tk.dcfg, sc.d_grid, b.pose, b.vb, u_t, f_t, sq=sc.d_sq, xt_ref=b.traj, dt_ref=0.1, self_index=me)
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
        for name, x, y in zip(("u", "follow_dwa", "dwa_count", "valid", "source"), got[t][1:], (u, follow, count, valid, source)):
            assert np.array_equal(bits(x), bits(y)), (t, name, np.nonzero((x != y).reshape(B, -1).any(1))[0])
        seen |= set(int(v) for v in source)
        capi.integrate_twist_batch(b.pose, b.u, tk.dt)
        b.vb = b.u.clone()
        torch.cuda.synchronize()
    assert seen == {0, 1, 2, 3}, seen
    # the layer decides: verdicts differ from the same loop without it
    plain = tk.run(None)
    differ = sum(int((got[t][4] != plain[t][4]).sum()) for t in range(tk.ticks))
    assert differ >= 3, differ
    # the other ticks give before and after what they gave
    for k, want in zip(("disc", "fleet", "foot"), before):
        for x, y in zip(want, tk.one_tick(k, fleet)):
            assert np.array_equal(x, y, equal_nan=True), k
    layer.close()
    fleet.close()
    eng.close()


def test_tick_with_an_empty_layer_is_the_footprint_tick():
    tk = _Tick()
    layer = capi.BodyLayer(tk.ccfg, tk.fp, tk.B)
    s, p = tk.state(), tk.state()
    mask = dev(i32(np.zeros(tk.B)))
    for t in range(3):
        sc = tk.scenes[0]
        if t:
            layer.update(s.pose, mask)           # tick 0: never updated; then: every robot masked
        for st, with_layer in ((s, True), (p, False)):
            args = (tk.B, st.pose, st.ut, st.follow, st.count, st.u, st.vb, sc.d_grid, st.traj, st.valid, st.skip, tk.ccfg, tk.dcfg, 0.1, 0.5)
            if with_layer:
                tk.eng.tick_batch_bodies(layer, *args, sq=sc.d_sq, source=st.source, status=st.status)
            else:
                tk.eng.tick_batch_footprint(tk.fp, *args, sq=sc.d_sq, source=st.source, status=st.status)
            capi.integrate_twist_batch(st.pose, st.u, tk.dt)
            st.vb = st.u.clone()
        torch.cuda.synchronize()
        for name in ("u", "follow", "count", "valid", "source", "ut", "traj", "pose", "skip"):
            assert np.array_equal(bits(getattr(s, name).cpu().numpy()), bits(getattr(p, name).cpu().numpy())), (t, name)
    layer.close()
    tk.eng.close()


def test_tick_refusals_leave_the_state_alone():
    from tests.test_host_mirror import COLL, DWA
    B = 8
    lim = np.array([1.0, 1.0, 2.0])
    eng = capi.Engine(capi.make_config(capi.MODEL_OMNI, 0.1, 5.0, 0.1, 1.0, 10, np.diag([1.0, 1.0, 2.0]), -lim, lim))
    eng.set_target_gaussians([[2.5, 2.5], [8.5, 2.5]], [[1.5, 1.5], [1.5, 1.5]])
    eng.config_domain((-1.0, 11.0, -1.0, 5.0))
    T = eng.T
    good = capi.make_collision_cfg(-1.0, -1.0, 0.05, 240, 120, *COLL)
    rect = capi.Footprint.of(fr.FOOTPRINTS["rect"])
    layer = capi.BodyLayer(good, rect, B)
    fill = lambda v: torch.full((B,), v, dtype=torch.int32, device="cuda")
    f64 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device="cuda")
    pose, ut, u, vb, traj = f64(B, 3), torch.zeros((B, T, 3), dtype=torch.float64, device="cuda"), f64(B, 3), f64(B, 3), f64(B, T, 3)
    follow, count, valid, skip = fill(1), fill(3), fill(-1), fill(-1)
    grid = torch.zeros((120, 240), dtype=torch.int8, device="cuda")

    def tick(l=layer, cfg=good, dwa=DWA["omni"], n=B):
        eng.tick_batch_bodies(l, n, pose, ut, follow, count, u, vb, grid, traj, valid, skip, cfg, capi.DwaCfg(*dwa), 0.1, 0.5)

    INV, UNS = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED
    cases = [(INV, dict(l=None), b"null body layer"), (INV, dict(cfg=None), b""),
             (INV, dict(cfg=capi.make_collision_cfg(-1.0, -1.0, 0.0, 240, 120, *COLL)), b""),
             (INV, dict(cfg=capi.make_collision_cfg(-1.0, -1.0, 0.05, 240, 119, *COLL)), b"geometry"),
             (INV, dict(cfg=capi.make_collision_cfg(-1.0, -1.05, 0.05, 240, 120, *COLL)), b"geometry"),
             (INV, dict(cfg=capi.make_collision_cfg(-1.0, -1.0, 0.05, 240, 120, 0.7, 1.0, 0.2, 0.5)), b"occupied_threshold"),
             (INV, dict(n=B - 1), b"the tick's B"), (INV, dict(n=0), b"the tick's B"),
             (UNS, dict(dwa=pr.with_(DWA["omni"], ns=(17, 17, 29))), b"8192"),
             (INV, dict(dwa=pr.with_(DWA["omni"], horizon=6.0)), b"")]
    if torch.cuda.device_count() > 1:
        cases.append((INV, dict(l=capi.BodyLayer(good, rect, B, device=1)), b"another device"))
    for status, kw, text in cases:
        with pytest.raises(capi.EngineError) as ei:
            tick(**kw)
        assert ei.value.status == status and text in capi.lib().eea_last_error(), (kw, ei.value)
    # the radii are not the layer's business
    other_radii = capi.make_collision_cfg(-1.0, -1.0, 0.05, 240, 120, 0.3, 2.0, 0.1, 0.8)
    torch.cuda.synchronize()
    assert bool((follow == 1).all()) and bool((count == 3).all()) and bool((valid == -1).all()) and bool((skip == -1).all())
    assert bool((u == 7.0).all())
    tick(cfg=other_radii)
    torch.cuda.synchronize()
    assert bool(((valid == 0) | (valid == 1)).all())
    layer.close()
    eng.close()

"""The body layer (eea_body_layer_* / eea_body_collision_check_batch / eea_body_validate_control_batch /
eea_body_dwa_control_batch / eea_tick_batch_bodies) without a GPU: the entry points, every refusal that comes before the device
is touched (host buffers nothing may touch), and -- from tests/body_layer_restatement.py alone -- the study scenes the GPU test
uses, the soundness of the near filter, and two scenes whose answers are known by construction."""
import ctypes as C

import numpy as np
import pytest

from ergodic_exploration_amd import capi

from tests import body_layer_restatement as br
from tests import clearance_restatement as cr
from tests import footprint_plan_restatement as pr
from tests import footprint_restatement as fr

ENTRIES = {"eea_body_layer_create": 6, "eea_body_layer_destroy": 1, "eea_body_layer_update": 4, "eea_body_layer_read": 4,
           "eea_body_layer_box": 1, "eea_body_collision_check_batch": 8, "eea_body_validate_control_batch": 11,
           "eea_body_dwa_control_batch": 15, "eea_tick_batch_bodies": 9}


def test_entries_are_declared_exported_and_bound():
    raw = C.CDLL(capi.LIB_PATH)
    L = capi.lib()
    for name, n_args in ENTRIES.items():
        assert name in capi.declared_symbols() and hasattr(raw, name), name
        assert len(getattr(L, name).argtypes) == n_args, name
    for name in ("update", "read", "check", "validate", "dwa", "close"):
        assert callable(getattr(capi.BodyLayer, name)), name
    assert callable(capi.Engine.tick_batch_bodies)
    assert capi.BODY_LAYER_NO_FILTER == 1
    assert L.eea_abi_version() == 6
    assert L.eea_body_layer_box(None) == -1


def test_creation_refusals_come_before_the_device():
    L = capi.lib()
    xs, ys = 80, 60
    good = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, *pr.COLL)
    rect = capi.Footprint.of(fr.FOOTPRINTS["rect"])
    ref = lambda s: None if s is None else C.byref(s)
    SENTINEL = 0x1234

    def create(cfg=good, fp=rect, B=4, flags=0, out=True):
        h = C.c_void_p(SENTINEL)
        st = L.eea_body_layer_create(0, ref(cfg), ref(fp), B, flags, C.byref(h) if out else None)
        assert not out or h.value is None, "a refused creation hands out no layer"
        return st

    INV, UNS = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED
    named = lambda: L.eea_last_error().startswith(b"eea_body_layer_create")
    assert create(out=False) == INV and named()
    assert create(cfg=None) == INV and named() and create(fp=None) == INV and named()
    for what, verts in (("clockwise", fr.FOOTPRINTS["rect"][::-1]), ("n = 2", [(0.5, 0.0), (-0.5, 0.0)]),
                        ("origin outside", [(0.9, -0.2), (0.9, 0.2), (0.1, 0.2), (0.1, -0.2)]),
                        ("NaN vertex", [(0.6, 0.0), (float("nan"), 0.35), (-0.3, -0.35)])):
        assert create(fp=capi.Footprint.of(verts)) == INV and b"footprint" in L.eea_last_error() and named(), what
    for bad in (capi.make_collision_cfg(-2.0, -1.0, 0.1, 0, ys, *pr.COLL), capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, 0, *pr.COLL),
                capi.make_collision_cfg(-2.0, -1.0, 0.0, xs, ys, *pr.COLL), capi.make_collision_cfg(-2.0, -1.0, float("nan"), xs, ys, *pr.COLL)):
        assert create(cfg=bad) == INV and named()
    big = capi.make_collision_cfg(-2.0, -1.0, 0.1, 1 << 16, (1 << 15) + 1, *pr.COLL)
    assert create(cfg=big) == UNS and b"2^31" in L.eea_last_error() and named()
    # the grid fits, the near map (the grid and 2 * box = 14 cells more either way) does not
    edge = capi.make_collision_cfg(-2.0, -1.0, 0.1, 1 << 16, 1 << 15, *pr.COLL)
    assert create(cfg=edge) == UNS and b"near" in L.eea_last_error() and named()
    r_out = capi.footprint_radii(rect)[1]
    fine = capi.make_collision_cfg(-2.0, -1.0, r_out / 1024.5, xs, ys, *pr.COLL)
    assert create(cfg=fine) == UNS and b"1024" in L.eea_last_error() and named()
    assert create(B=0) == INV and b"at least one robot" in L.eea_last_error() and named()
    assert create(flags=2) == INV and b"flag" in L.eea_last_error() and named()
    assert create(flags=0x80000001) == INV and named()


def test_batch_refusals_come_before_the_device():
    """every refusal of the three batch entries, of update and of read is answered without a device (the layer is asked for
    last, so each is reached without one): the buffers are host arrays nothing may touch"""
    L = capi.lib()
    xs, ys, P = 80, 60, 4
    omni = capi.DwaCfg(*pr.DWA_OMNI)
    grid = np.zeros(xs * ys, dtype=np.int8)
    sq = np.full((ys, xs), 7, dtype=np.int32)
    x0, tw, xt = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros((P, 20, 3))
    self_ = np.full(P, -1, dtype=np.int32)
    hit, valid, found = (np.full(P, 7, dtype=np.int32) for _ in range(3))
    u_opt = np.full((P, 3), 7.0)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    ref = lambda s: None if s is None else C.byref(s)

    def chk(g=grid, s=sq, x=x0, i=self_, n=P, o=hit):
        return L.eea_body_collision_check_batch(None, p(g), p(s), p(x), p(i), n, p(o), None)

    def val(g=grid, s=sq, x=x0, u=tw, i=self_, n=P, o=valid, dt=0.1, horizon=1.0):
        return L.eea_body_validate_control_batch(None, p(g), p(s), p(x), p(u), p(i), dt, horizon, n, p(o), None)

    def dwa(d=omni, g=grid, s=sq, x=x0, vb=tw, vref=tw, tr=None, n_ref=0, dt_ref=0.0, i=self_, n=P, o=u_opt, f=found):
        return L.eea_body_dwa_control_batch(None, ref(d), p(g), p(s), p(x), p(vb), p(vref), p(tr), n_ref, dt_ref, p(i), n, p(o), p(f), None)

    INV, UNS = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED
    err = L.eea_last_error
    # required pointers (d_sq and d_self are not; d_grid is not for the check entry): "null argument", not yet the layer
    for call, entry in ((lambda: chk(x=None), b"eea_body_collision_check_batch"), (lambda: chk(o=None), b"eea_body_collision_check_batch"),
                        (lambda: val(g=None), b"eea_body_validate_control_batch"), (lambda: val(x=None), b"eea_body_validate_control_batch"),
                        (lambda: val(u=None), b"eea_body_validate_control_batch"), (lambda: val(o=None), b"eea_body_validate_control_batch"),
                        (lambda: dwa(d=None), b"eea_body_dwa_control_batch"), (lambda: dwa(g=None), b"eea_body_dwa_control_batch"),
                        (lambda: dwa(x=None), b"eea_body_dwa_control_batch"), (lambda: dwa(vb=None), b"eea_body_dwa_control_batch"),
                        (lambda: dwa(o=None), b"eea_body_dwa_control_batch"), (lambda: dwa(f=None), b"eea_body_dwa_control_batch")):
        assert call() == INV and err().startswith(entry) and b"null argument" in err(), err()
    # eea_dwa_control_batch's: both or neither reference, an empty one, more than 8192 samples, a rollout past its reference
    assert dwa(vref=None) == INV and b"either" in err() and dwa(tr=xt, n_ref=20, dt_ref=0.1) == INV and b"either" in err()
    assert dwa(vref=None, tr=xt, n_ref=0, dt_ref=0.1) == INV and b"empty" in err()
    assert dwa(d=capi.DwaCfg(*pr.with_(pr.DWA_OMNI, ns=(17, 17, 29)))) == UNS and b"8192" in err()
    long_ = capi.DwaCfg(*pr.with_(pr.DWA_OMNI, horizon=2.0))
    assert dwa(d=long_, vref=None, tr=xt, n_ref=18, dt_ref=0.1) == INV and b"reference" in err()
    assert err().startswith(b"eea_body_dwa_control_batch")
    # everything else in order: the layer is what is missing, P == 0 included
    for call in (chk, lambda: chk(g=None, s=None, i=None), lambda: chk(n=0), val, lambda: val(s=None, i=None), lambda: val(n=0), dwa,
                 lambda: dwa(s=None, i=None), lambda: dwa(n=0), lambda: dwa(d=long_, vref=None, tr=xt, n_ref=19, dt_ref=0.1)):
        assert call() == INV and b"null body layer" in err(), err()
    assert L.eea_body_layer_update(None, p(x0), None, None) == INV and err().startswith(b"eea_body_layer_update")
    assert L.eea_body_layer_read(None, None, None, None) == INV and err().startswith(b"eea_body_layer_read")
    L.eea_body_layer_destroy(None)
    assert (hit == 7).all() and (valid == 7).all() and (found == 7).all() and (u_opt == 7.0).all() and (sq == 7).all()


def test_tick_refusals_need_no_device():
    L = capi.lib()
    io, tick = capi.BatchIO(), capi.TickIO()
    good = capi.make_collision_cfg(-2.0, -1.0, 0.1, 80, 60, *pr.COLL)
    omni = capi.DwaCfg(*pr.DWA_OMNI)
    INV = capi.ERR_INVALID_ARGUMENT
    assert L.eea_tick_batch_bodies(None, 4, C.byref(io), C.byref(tick), C.byref(good), C.byref(omni), None, None, None) == INV
    assert b"null engine" in L.eea_last_error()


# ---- the study scenes ------------------------------------------------------------------------------------------------------------

# footprint: robots of the greedy fleet, validate_control verdicts changed (5 steps of vref), window free sets changed, undecided
STUDY = {"rect": (30, 11, 23, 0), "tri": (40, 20, 34, 0), "offc": (40, 21, 29, 0)}


@pytest.mark.parametrize("name", list(STUDY))
def test_study_scene(name):
    robots, verdicts, free_sets, und, margin = br.study_row(name)
    assert (robots, verdicts, free_sets, und) == STUDY[name]
    idx, layer = br.greedy_fleet(name)
    # the caps: conditions of the scene, not tolerances
    assert layer.flags.all() and layer.decided().all() and margin >= fr.DECIDED
    assert und <= (2 * robots) // 100
    assert layer.cover.max() == 1                 # the greedy rule: no two bodies share a cell
    # the outcomes are mixed: the layer changes what the planner decides, in both directions
    lose_all, keep, some = br.window_mix(name)
    assert 11 <= lose_all <= 24 and keep >= 4 and some >= 5 and lose_all + keep + some == robots
    # a robot is never its own obstacle: alone on the layer it answers as the plain footprint does
    w, x0, vb, vref, _, study_robots = pr.study()
    q = int(idx[0])
    alone = br.Layer(w, layer.verts, x0[q:q + 1])
    a = br.dwa_control(alone, pr.DWA_OMNI, study_robots[q], 0, vref=vref[q])
    b = pr.dwa_control(w, layer.verts, pr.DWA_OMNI, study_robots[q], vref=vref[q])
    assert np.array_equal(a.costs, b.costs) and a.found == b.found


# ---- the near filter -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rect", "tri", "offc"])
def test_near_proves_that_no_other_body_is_met(name):
    """wherever near - self == 0, no other body shares a cell with any polygon placed in that cell: brute force over 200
    headings on a 40 x 30 grid, the fleet's robots on and off the grid"""
    rng = np.random.default_rng(11)
    w = pr.World(np.zeros((30, 40), dtype=np.int8), 0.1, -1.0, -0.5)
    verts = fr.FOOTPRINTS[name]
    box = br.box_of(w, verts)
    B = 5
    poses = np.stack([rng.uniform(-1.6, 3.6, B), rng.uniform(-1.1, 3.1, B), rng.uniform(-np.pi, np.pi, B)], 1)
    layer = br.Layer(w, verts, poses)
    assert layer.flags.sum() >= 3
    proved = met = 0
    for th in rng.uniform(-np.pi, np.pi, 200):
        for _ in range(12):
            i = int(rng.integers(-1, B))
            q = np.array([rng.uniform(-1.0 - box * 0.1, 3.0 + box * 0.1), rng.uniform(-0.5 - box * 0.1, 2.5 + box * 0.1), th])
            if not br.stamped(w, verts, q[None])[0]:
                continue                                   # an empty box: nothing is looked up
            fx, fy = br.cells_of(w, q[None])
            body = br.cover(w, verts, q)[0]
            others = br.own_grid(pr.World(np.zeros_like(w.data), w.res, w.xmin, w.ymin), layer.covers, i).data != 0
            shares = bool((body & others).any())
            met += shares
            if br.near_minus_self(layer, fx[0], fy[0], i) == 0:
                proved += 1
                assert not shares, (q, i)
    assert proved > 200 and met > 50                 # both sides occur


# ---- two scenes whose answers are known --------------------------------------------------------------------------------------

def _world41(walls=()):
    return pr.World(fr.fact_scene(list(walls)), cr.RES41, cr.XMIN41, cr.YMIN41)


def test_two_robots_face_each_other():
    """two `rect` robots 1.0 m apart along x, nose to nose: 0.1 m between the 0.45 m half-lengths.  Forward at 1 m/s collides,
    backward does not; with nobody's body taken out a robot collides with "itself" where it stands"""
    w = _world41()
    verts = fr.FOOTPRINTS["rect"]
    (ax, ay), (bx, by) = fr.centre41(15, 20), fr.centre41(25, 20)
    poses = np.array([[ax, ay, 0.0], [bx, by, np.pi]])
    assert abs((bx - ax) - 1.0) < 1e-12
    layer = br.Layer(w, verts, poses)
    assert layer.flags.all() and layer.decided().all() and layer.cover.max() == 1
    assert layer.covers[0].sum() == 9 * 5 and layer.covers[1].sum() == 9 * 5          # centres within 0.45 m x 0.25 m
    fwd, back = np.array([[1.0, 0.0, 0.0]] * 2), np.array([[-1.0, 0.0, 0.0]] * 2)
    own = np.arange(2)
    valid, decided = br.validate(layer, poses, fwd, 0.1, 1.0, own)
    assert decided.all() and (valid == 0).all()
    valid, decided = br.validate(layer, poses, back, 0.1, 1.0, own)
    assert decided.all() and (valid == 1).all()
    # the first colliding step of the forward rollout: the noses' cells meet once the robot has moved 0.2 m
    roll = pr.rollout(poses[0], fwd[0], 0.1, 10)
    hit, margin = br.check(layer, roll, np.zeros(10, dtype=int))
    assert (margin >= fr.DECIDED).all() and hit.argmax() == 1 and not hit[0]
    # where they stand: free as themselves, a hit as each other and as nobody
    hit, margin = br.check(layer, poses, own)
    assert not hit.any() and (margin >= fr.DECIDED).all()
    assert br.check(layer, poses, own[::-1])[0].all() and br.check(layer, poses, None)[0].all()
    # ... and the dynamic window of robot 0: every forward sample that reaches the other is lost, the backward ones stay
    robot = pr.Robot(pr.DWA_OMNI, poses[0], np.zeros(3))
    plain = pr.dwa_control(w, verts, pr.DWA_OMNI, robot, vref=np.array([0.2, 0.0, 0.0]))
    with_ = br.dwa_control(layer, pr.DWA_OMNI, robot, 0, vref=np.array([0.2, 0.0, 0.0]))
    assert plain.free.all() and with_.free[robot.u[:, 0] < 0.0].all() and with_.found == 1
    # as nobody (-1) every sample starts inside its own body
    assert not br.dwa_control(layer, pr.DWA_OMNI, robot, -1, vref=np.zeros(3)).free.any()


def test_a_robot_alone_is_the_plain_footprint():
    w = _world41(fr.CORRIDOR)
    rng = np.random.default_rng(4)
    for name in ("rect", "tri", "offc"):
        verts = fr.FOOTPRINTS[name]
        x, y = fr.CORRIDOR_POSE
        layer = br.Layer(w, verts, np.array([[x, y, 0.3]]))
        assert layer.flags.all()
        poses = np.stack([rng.uniform(cr.XMIN41 - 1, cr.XMIN41 + 5.1, 300), rng.uniform(cr.YMIN41 - 1, cr.YMIN41 + 5.1, 300),
                          rng.uniform(-np.pi, np.pi, 300)], 1)
        mine, margin = br.check(layer, poses, np.zeros(300, dtype=int))
        plain, margin0 = pr.verdicts(w, verts, poses)
        assert np.array_equal(mine, plain) and np.array_equal(margin, margin0) and 0 < plain.sum() < 300
        # ... while to anybody else it is an obstacle
        assert br.check(layer, poses, None)[0].sum() >= plain.sum() and br.check(layer, layer.poses, None, static=False)[0][0]
        assert not br.check(layer, layer.poses, [0], static=False)[0][0]

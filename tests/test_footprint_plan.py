"""Footprint planning (eea_footprint_validate_control_batch / eea_footprint_dwa_control_batch / eea_tick_batch_footprint) without
a GPU: the entry points, every refusal that comes before the device is selected (host buffers nothing may touch), the reach
bound the LDS window of footprint_dwa_kernel rests on, and -- from tests/footprint_plan_restatement.py alone -- the cap on
undecided robots and the outcome mix of the scene the GPU test uses."""
import ctypes as C

import numpy as np
import pytest

from ergodic_exploration_amd import capi

from tests import footprint_plan_restatement as pr
from tests import footprint_restatement as fr

ENTRIES = {"eea_footprint_validate_control_batch": 12, "eea_footprint_dwa_control_batch": 16, "eea_tick_batch_footprint": 9}


def test_entries_are_declared_exported_and_bound():
    raw = C.CDLL(capi.LIB_PATH)
    L = capi.lib()
    for name, n_args in ENTRIES.items():
        assert name in capi.declared_symbols() and hasattr(raw, name), name
        assert len(getattr(L, name).argtypes) == n_args, name
    for name in ("footprint_validate_control_batch", "footprint_dwa_control_batch"):
        assert callable(getattr(capi, name)), name
    assert callable(capi.Engine.tick_batch_footprint)
    assert L.eea_abi_version() == 6


def test_argument_errors_come_before_the_device():
    """every refusal of the two batch entries is answered without a device: the buffers are host arrays nothing may touch;
    P == 0 is EEA_OK"""
    L = capi.lib()
    xs, ys, P = 80, 60, 4
    good = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, *pr.COLL)
    rect = capi.Footprint.of(fr.FOOTPRINTS["rect"])
    omni = capi.DwaCfg(*pr.DWA_OMNI)
    grid = np.zeros(xs * ys, dtype=np.int8)
    sq = np.full((ys, xs), 7, dtype=np.int32)
    x0, tw, xt = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros((P, 20, 3))
    valid, found, u_opt = np.full(P, 7, dtype=np.int32), np.full(P, 7, dtype=np.int32), np.full((P, 3), 7.0)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    ref = lambda s: None if s is None else C.byref(s)

    def val(cfg=good, fp=rect, g=grid, s=sq, x=x0, u=tw, n=P, o=valid, dt=0.1, horizon=1.0):
        return L.eea_footprint_validate_control_batch(0, ref(cfg), ref(fp), p(g), p(s), p(x), p(u), dt, horizon, n, p(o), None)

    def dwa(cfg=good, d=omni, fp=rect, g=grid, s=sq, x=x0, vb=tw, vref=tw, tr=None, n_ref=0, dt_ref=0.0, n=P, o=u_opt, f=found):
        return L.eea_footprint_dwa_control_batch(0, ref(cfg), ref(d), ref(fp), p(g), p(s), p(x), p(vb), p(vref), p(tr), n_ref, dt_ref,
                                                 n, p(o), p(f), None)

    INV, UNS = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED
    # required pointers (d_sq is not one)
    assert val(cfg=None) == INV and val(fp=None) == INV and val(g=None) == INV and val(x=None) == INV and val(u=None) == INV
    assert val(o=None) == INV
    assert dwa(cfg=None) == INV and dwa(d=None) == INV and dwa(fp=None) == INV and dwa(g=None) == INV and dwa(x=None) == INV
    assert dwa(vb=None) == INV and dwa(o=None) == INV and dwa(f=None) == INV
    # the footprint's own refusals, with the reason
    for what, verts in (("clockwise", fr.FOOTPRINTS["rect"][::-1]), ("n = 2", [(0.5, 0.0), (-0.5, 0.0)]),
                        ("origin outside", [(0.9, -0.2), (0.9, 0.2), (0.1, 0.2), (0.1, -0.2)]),
                        ("NaN vertex", [(0.6, 0.0), (float("nan"), 0.35), (-0.3, -0.35)])):
        bad = capi.Footprint.of(verts)
        assert val(fp=bad) == INV and b"footprint" in L.eea_last_error(), what
        assert dwa(fp=bad) == INV and b"footprint" in L.eea_last_error(), what
    # the grid's refusals; the radii and the threshold are neither read nor checked
    for bad in (capi.make_collision_cfg(-2.0, -1.0, 0.1, 0, ys, *pr.COLL), capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, 0, *pr.COLL),
                capi.make_collision_cfg(-2.0, -1.0, 0.0, xs, ys, *pr.COLL), capi.make_collision_cfg(-2.0, -1.0, float("nan"), xs, ys, *pr.COLL)):
        assert val(cfg=bad) == INV and dwa(cfg=bad) == INV
    big = capi.make_collision_cfg(-2.0, -1.0, 0.1, 1 << 16, (1 << 15) + 1, *pr.COLL)
    assert val(cfg=big) == UNS and dwa(cfg=big) == UNS and b"2^31" in L.eea_last_error()
    r_out = capi.footprint_radii(rect)[1]
    fine = capi.make_collision_cfg(-2.0, -1.0, r_out / 1024.5, xs, ys, *pr.COLL)
    assert val(cfg=fine) == UNS and dwa(cfg=fine) == UNS and b"1024" in L.eea_last_error()
    # eea_dwa_control_batch's: both or neither reference, an empty one, more than 8192 samples, a rollout past its reference
    assert dwa(vref=None) == INV and dwa(tr=xt, n_ref=20, dt_ref=0.1) == INV
    assert dwa(vref=None, tr=xt, n_ref=0, dt_ref=0.1) == INV
    assert dwa(d=capi.DwaCfg(*pr.with_(pr.DWA_OMNI, ns=(17, 17, 29)))) == UNS and b"8192" in L.eea_last_error()
    long_ = capi.DwaCfg(*pr.with_(pr.DWA_OMNI, horizon=2.0))
    assert dwa(d=long_, vref=None, tr=xt, n_ref=18, dt_ref=0.1) == INV and b"reference" in L.eea_last_error()
    assert dwa(d=long_, vref=None, tr=xt, n_ref=20, dt_ref=0.0) == INV
    # accepted without a device: nothing to do
    swapped = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 1.0, 0.7, 0.2, 100.5)
    assert val(n=0) == capi.OK and val(s=None, n=0) == capi.OK and val(cfg=swapped, n=0) == capi.OK
    assert dwa(n=0) == capi.OK and dwa(s=None, n=0) == capi.OK and dwa(cfg=swapped, n=0) == capi.OK
    assert dwa(d=long_, vref=None, tr=xt, n_ref=19, dt_ref=0.1, n=0) == capi.OK
    assert (valid == 7).all() and (found == 7).all() and (u_opt == 7.0).all() and (sq == 7).all()


def test_tick_refusals_need_no_device():
    """the arguments eea_tick_batch_footprint checks before it looks at the engine's state"""
    L = capi.lib()
    io, tick = capi.BatchIO(), capi.TickIO()
    good = capi.make_collision_cfg(-2.0, -1.0, 0.1, 80, 60, *pr.COLL)
    rect, omni = capi.Footprint.of(fr.FOOTPRINTS["rect"]), capi.DwaCfg(*pr.DWA_OMNI)
    INV = capi.ERR_INVALID_ARGUMENT
    assert L.eea_tick_batch_footprint(None, 4, C.byref(io), C.byref(tick), C.byref(good), C.byref(omni), C.byref(rect), None, None) == INV
    assert b"null engine" in L.eea_last_error()


# ---- the reach bound -------------------------------------------------------------------------------------------------------------

def _cells(w, xy):
    return np.floor((xy - np.array([w.xmin, w.ymin])) / w.res)


def test_no_sample_pose_leaves_the_reach():
    """no pose of any sample is more than the robot's own reach in cells from x0's cell: the study's robots, and robots whose
    odometry is at twice the limits (lower above vmax: their reach is larger than the one the limits give)"""
    w, x0, vb, _, _, robots = pr.study()
    lim = pr.limits_reach(pr.DWA_OMNI, w.res)
    for q in range(pr.N_STUDY):
        own = pr.reach(pr.DWA_OMNI, vb[q], w.res)
        assert own <= lim
        assert np.abs(_cells(w, robots[q].poses[..., :2]) - _cells(w, x0[q, :2])).max() <= own, q
    rng = np.random.default_rng(2)
    above = 0
    for q in range(24):
        fast = np.array([2.0, 2.0, 4.0]) * rng.choice([-1.0, 1.0], 3)
        own = pr.reach(pr.DWA_OMNI, fast, w.res)
        above += own > lim
        r = pr.Robot(pr.DWA_OMNI, x0[q], fast)
        assert np.abs(_cells(w, r.poses[..., :2]) - _cells(w, x0[q, :2])).max() <= own, q
    assert above == 24
    # the cart's window (no lateral velocity) and a finer grid
    for q in range(24):
        r = pr.Robot(pr.DWA_CART, x0[q], vb[q] * [1.0, 0.0, 1.0])
        fine = pr.World(w.data, 0.03, w.xmin, w.ymin)
        for wd in (w, fine):
            own = pr.reach(pr.DWA_CART, vb[q] * [1.0, 0.0, 1.0], wd.res)
            assert np.abs(_cells(wd, r.poses[..., :2]) - _cells(wd, x0[q, :2])).max() <= own, q


# ---- the cap and the mix ---------------------------------------------------------------------------------------------------------

# per footprint: undecided robots, robots with no free sample, with every sample free, mixed -- of the 256 robots of the study
# scene (world(3), DWA_OMNI: 120 samples of 10 steps), the sample values formed by repeated +=
MIX = {"rect": (0, 97, 59, 100), "offc": (0, 90, 59, 107), "tri": (0, 71, 77, 108)}


@pytest.mark.parametrize("name", list(MIX))
def test_cap_on_undecided_robots_and_the_outcome_mix(name):
    answers = pr.study_answers(name, "vref")
    und, none, every, mixed = pr.mix(answers)
    assert und <= (2 * pr.N_STUDY) // 100                 # the cap: a condition of the scene, not a tolerance
    assert (und, none, every, mixed) == MIX[name]
    first = answers[:128]                                 # the robots the GPU test uses
    assert sum(not a.decided for a in first) <= (2 * 128) // 100
    assert 0 < sum(a.found for a in first) < 128
    # the trajectory mode judges the same poses: the same samples are free
    w, _, _, _, xt, robots = pr.study()
    for q in range(16):
        b = pr.dwa_control(w, fr.FOOTPRINTS[name], pr.DWA_OMNI, robots[q], xt=xt[q], dt_ref=pr.DT_REF)
        assert np.array_equal(answers[q].free, b.free) and answers[q].decided == b.decided

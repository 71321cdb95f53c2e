"""The exact test of the footprint kernels at its edges, on the device: every scene of tests/footprint_edge_scenes.py, whose
verdicts a 50-digit reference decides (tests/test_footprint_edges.py holds the scenes to that), against

  the check entry (eea_footprint_check_batch: the cooperative resolve, cells from memory),
  validate_control (eea_footprint_validate_control_batch: resolve_together),
  the dynamic window (eea_footprint_dwa_control_batch) on the window path -- resolve_window: row_span, the masks, the word
  loop, the four-row read-ahead --, on the memory path (limits no window fits the LDS with), and with a few robots of the
  same launch whose odometry is at twice the limits, so that both paths share a launch,

each with and without the distance field, bitwise equal; and against the body layer's instances, where the occupied cells are
a second robot's stamp or the probing robot's own body has to come out of the window's bits.  One pose per robot is made
observable by a window of one sample, the zero twist, over one step: found == not hit.  The fan (one workgroup, N headings of
one body) is compared with footprint_plan_restatement.dwa_control bitwise.  Every comparison is of integers or of bits."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ergodic_exploration_amd import capi
from tests import body_layer_restatement as br
from tests import footprint_edge_scenes as es
from tests import footprint_plan_restatement as pr
from tests.test_gpu_body_layer import Bodies, i32
from tests.test_gpu_footprint_plan import Scene, dev

pytestmark = pytest.mark.gpu

ZERO_BITS = np.zeros(3, dtype=np.uint64)


class Devices:
    """the device side of the worlds of one test: a Scene per World object"""

    def __init__(self):
        self.by_world = {}

    def of(self, w):
        if id(w) not in self.by_world:
            self.by_world[id(w)] = (w, Scene(w))
        return self.by_world[id(w)][1]


def check_entry(sd, verts, poses):
    """eea_footprint_check_batch with and without the field: the same ints, returned once"""
    outs = []
    for sq in (None, sd.d_sq):
        d_hit = torch.full((len(poses),), -1, dtype=torch.int32, device="cuda")
        capi.footprint_check_batch(sd.ccfg, capi.Footprint.of(verts), sd.d_grid, dev(poses), d_hit, sq=sq)
        torch.cuda.synchronize()
        outs.append(d_hit.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    return outs[0]


def window_reaches(res):
    """the reaches the window path is run with: 2 cells (0.05 m/s at 0.1 m), and at the coarse resolutions 9 more, so that
    the box's first column in the window and with it the bits a lane reads vary"""
    return (2, 9) if res >= 0.01 else (es.W_DEFAULT,)


def found_of(sd, sc, W, x0=None, vb=None, dwa=None):
    x0 = sc.x0 if x0 is None else x0
    vb = np.zeros((len(x0), 3)) if vb is None else vb
    u, f = sd.dwa_both(es.dwa_cfg(sc.w.res, W) if dwa is None else dwa, sc.verts, x0, vb, vref=np.zeros((len(x0), 3)))
    return u, f


def plain_paths(sd, sc, counts, mixed=True):
    """one scene through the check entry, validate_control and the three launches of the dynamic window"""
    want = sc.hit.astype(np.int32)
    P = len(want)
    hit = check_entry(sd, sc.verts, sc.poses)
    assert np.array_equal(hit, want), (sc.tag, "check", np.nonzero(hit != want)[0][:8])
    v = sd.validate_both(sc.verts, sc.x0, np.zeros((P, 3)), es.DT, es.DT)
    assert np.array_equal(v, 1 - want), (sc.tag, "validate", np.nonzero(v != 1 - want)[0][:8])
    counts["check"] += P
    counts["validate"] += P
    Ws = sorted(set(window_reaches(sc.w.res) + (sc.W,))) if sc.family != "D" else [sc.W]
    for W in Ws + [es.W_MEMORY]:
        window = es.fits(sc.name, sc.w.res, W)
        assert window == (W != es.W_MEMORY and sc.w.res != es.RES_NO_WINDOW), (sc.tag, W)
        u, f = found_of(sd, sc, W)
        assert np.array_equal(f, 1 - want), (sc.tag, "window" if window else "memory", W, np.nonzero(f != 1 - want)[0][:8])
        assert (u.view(np.uint64) == ZERO_BITS).all()          # the one sample is the zero twist, found or not
        counts["window" if window else "memory"] += P
        if window:
            b = sc.boxes()
            counts["widest"] = max(counts["widest"], int((b[:, 1] - b[:, 0] + 1).max()))
            counts["cells"] = max(counts["cells"], es.radii(sc.name)[1] / sc.w.res)
    if mixed:
        mixed_launch(sd, sc, counts)


def mixed_launch(sd, sc, counts):
    """the scene's robots (at most 8 of them), each once with vb = 0 and once with vb at twice the limits: lower = 1.5 max_vel,
    the robot's own reach 8 cells against the 6 the launch reserved -- the second half of the workgroups takes its cells from
    memory beside the first half's windows.  Against footprint_plan_restatement.dwa_control where it is decided"""
    n = min(len(sc.x0), 8)
    pick = np.linspace(0, len(sc.x0) - 1, n).astype(int)
    dwa = es.dwa_cfg(sc.w.res, es.W_DEFAULT)
    dwa = pr.with_(dwa, acc_lim_x=0.5 * dwa[6])
    x0 = np.concatenate([sc.x0[pick], sc.x0[pick]])
    vb = np.zeros((2 * n, 3))
    vb[n:, 0] = 2.0 * dwa[6]
    lim = pr.limits_reach(dwa, sc.w.res)
    assert all(pr.reach(dwa, vb[q], sc.w.res) <= lim for q in range(n)) and all(pr.reach(dwa, vb[q], sc.w.res) > lim for q in range(n, 2 * n))
    u, f = found_of(sd, sc, None, x0=x0, vb=vb, dwa=dwa)
    assert np.array_equal(f[:n], 1 - sc.hit[pick].astype(np.int32)), (sc.tag, "mixed")
    for q in range(n, 2 * n):
        a = pr.dwa_control(sc.w, sc.verts, dwa, pr.Robot(dwa, x0[q], vb[q]), vref=np.zeros(3))
        counts["beside"] += 1
        if a.decided:
            assert int(f[q]) == a.found and np.array_equal(u[q].view(np.uint64), a.u_opt.view(np.uint64)), (sc.tag, "mixed", q)
            counts["mixed"] += 1


def new_counts():
    return dict(check=0, validate=0, window=0, memory=0, mixed=0, beside=0, body=0, widest=0, cells=0.0)


def report(what, counts):
    print("\n%s: poses per path: check %d, validate %d, window %d, memory %d, beside the window (decided) %d, body layer %d; "
          "widest box on the window path %d columns, r_out / res %.1f"
          % (what, counts["check"], counts["validate"], counts["window"], counts["memory"], counts["mixed"], counts["body"],
             counts["widest"], counts["cells"]))


# ---- the plain footprint -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,res", es.CASES)
def test_plain_footprint(family, res):
    devs, counts = Devices(), new_counts()
    for sc in es.families(family, res):
        # (the launch that mixes the paths: every scene of one cell, and of the hollow blocks the free ones)
        plain_paths(devs.of(sc.w), sc, counts, mixed=len(sc.x0) > 1 or not sc.hit[0])
    assert counts["check"] > 0 and counts["memory"] > 0 and (counts["window"] > 0) == (res != es.RES_NO_WINDOW)
    # the robots at twice the limits move 6.75 cells: three in four of them are decided where they arrive, and compared
    assert counts["beside"] > 0 and counts["mixed"] >= 0.75 * counts["beside"], (counts["mixed"], counts["beside"])
    report("%s at %g m" % (family, res), counts)


@pytest.mark.parametrize("res", es.FAN_RES)
@pytest.mark.parametrize("name", es.FAN_NAMES)
def test_fan(name, res):
    """P = N robots with the same x0 and vb; robot r's vref is sample r, so u_opt == sample r exactly when lane r is free"""
    n_free = 0
    for N in es.FAN_N:
        f = es.fan(name, res, N)
        assert es.fits(name, res, W=1, nsamp=N) and pr.limits_reach(f.dwa, res) == 1.0 and f.ambiguous()          # the window path
        sd = Scene(f.w)
        x0, vb = np.tile(f.x0, (N, 1)), np.zeros((N, 3))
        u, found = sd.dwa_both(f.dwa, f.verts, x0, vb, vref=f.robot.u)
        for r in range(N):
            a = pr.dwa_control(f.w, f.verts, f.dwa, f.robot, vref=f.robot.u[r])
            assert a.decided and int(found[r]) == a.found == 1, (f.tag, r)
            assert np.array_equal(u[r].view(np.uint64), a.u_opt.view(np.uint64)), (f.tag, r, u[r], a.u_opt)
            assert np.array_equal(u[r], f.robot.u[r]) == bool(f.free[r]), (f.tag, r)
        # ... and lane by lane through validate_control: sample r as robot r's twist
        v = sd.validate_both(f.verts, x0, f.robot.u, es.DT, es.DT)
        assert np.array_equal(v, f.free.astype(np.int32)), (f.tag, np.nonzero(v != f.free)[0][:8])
        n_free += int(f.free.sum())
    print("\nfan %s at %g m: %d lanes, %d of them free" % (name, res, sum(es.FAN_N), n_free))


# ---- the body layer's instances ----------------------------------------------------------------------------------------------------

def body_paths(bd, ref, x0, want, tag, counts, Ws):
    """the poses as robot 0's through the layer's check entry, validate_control and the dynamic window on both paths, each the
    four ways of Bodies; the restatement gives the verdicts the scene recorded"""
    P = len(x0)
    me = i32(np.zeros(P))
    poses = es.judged(x0)
    r_hit, r_margin = br.check(ref, poses, me)
    assert np.array_equal(r_hit, want) and (r_margin >= es.MARGIN).all(), tag
    want = want.astype(np.int32)
    hit = bd.check(poses, me)
    assert np.array_equal(hit, want), (tag, "check", np.nonzero(hit != want)[0][:8])
    v = bd.validate(x0, np.zeros((P, 3)), es.DT, es.DT, me)
    assert np.array_equal(v, 1 - want), (tag, "validate", np.nonzero(v != 1 - want)[0][:8])
    for W in tuple(Ws) + (es.W_MEMORY,):
        u, f = bd.dwa(es.dwa_cfg(bd.w.res, W), x0, np.zeros((P, 3)), me, vref=np.zeros((P, 3)))
        assert np.array_equal(f, 1 - want), (tag, "dwa", W, np.nonzero(f != 1 - want)[0][:8])
        assert (u.view(np.uint64) == ZERO_BITS).all()
    counts["body"] += P


@pytest.mark.parametrize("res", es.BODY_RES)
def test_body_layer_single_cell(res):
    """family A twice: the one cell a cell of the grid while another stamped robot stands far away (no window holds a body
    bit: the field's verdict on a free pose stands); and the grid empty, the only occupied cells the stamp of a second robot
    (the window's body flag is what sends a pose the field calls free to the exact test)"""
    counts = new_counts()
    names = es.BODY_NAMES
    w0, cell = es.single_cell_world(res, es.names_at(res))
    for name in names:
        sc = es.family_a(res, name, w0, cell)
        w, layer_poses, mask = es.with_far_robot(sc)
        ref = br.Layer(w, sc.verts, layer_poses, mask)
        assert ref.flags.tolist() == [False, True] and ref.decided()[1]
        bd = Bodies(w, sc.verts, 2)
        bd.update(layer_poses, mask)
        body_paths(bd, ref, sc.x0, sc.hit, sc.tag + "-far", counts, window_reaches(res))
        bd.close()
        w, layer_poses, mask, x0, hit, _ = es.stamp_probes(res, name)
        assert not w.data.any() and hit.any() and not hit.all() and len(hit) >= 48 * len(sc.verts)
        ref = br.Layer(w, sc.verts, layer_poses, mask)
        assert ref.flags.tolist() == [False, True] and ref.decided()[1]
        bd = Bodies(w, sc.verts, 2)
        bd.update(layer_poses, mask)
        body_paths(bd, ref, x0, hit, "stamp-%s-%g" % (name, res), counts, window_reaches(res))
        bd.close()
    report("body layer, one cell / a stamp, at %g m" % res, counts)


@pytest.mark.parametrize("res", es.BODY_RES)
def test_body_layer_hollow_block(res):
    """family C with the probing robot itself stamped where it stands: its own body has to come out of the window's bits"""
    counts = new_counts()
    for name in es.BODY_NAMES:
        for sc in es.family_c(res, name):
            ref = br.Layer(sc.w, sc.verts, sc.poses)
            assert ref.flags.all() and ref.decided().all() and ref.cover.sum() > 0
            bd = Bodies(sc.w, sc.verts, 1)
            bd.update(sc.poses)
            body_paths(bd, ref, sc.x0, sc.hit, sc.tag, counts, (es.W_DEFAULT,))
            bd.close()
    report("body layer, hollow block, at %g m" % res, counts)

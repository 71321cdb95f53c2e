"""The frontier auction on the device (include/ergodic_amd.h: eea_frontier_auction; csrc/auction_kernel.hip).

Checker: tests/auction_restatement.py (held to a second, independent statement and to the invariants of any answer by
tests/test_auction.py).  The five outputs and d_state[0, 2, 3] are compared BITWISE as whole buffers, doubles by their bits.
Every output sits between guard elements and holds a sentinel before the call; every input and the workspace sit between
guards and come back unchanged.  The rank plane, the records and the state a call reads come from a real eea_frontier_regions
call on the same device grid.  Scenes: tests/auction_scenes.py; the guarded buffers are tests/test_gpu_geodesic.py's."""
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ergodic_exploration_amd import capi
from tests import auction_restatement as ar
from tests import auction_scenes as scn
from tests import frontier_restatement as fr
from tests import sense_restatement as sr
from tests import test_gpu_frontier as tf
from tests import test_gpu_geodesic as tg

pytestmark = pytest.mark.gpu

ROOT = tg.ROOT
G_IN, G_OUT, S_GEO, S_STATE, S_PATH = tg.G_IN, tg.G_OUT, tg.S_GEO, tg.S_STATE, tg.S_PATH
S_REGION, S_COST = tf.S_REGION, 0x6B0B0B0B
WS_GUARD = 64
_guarded, _bits = tg._guarded, tg._bits

Got = __import__("collections").namedtuple("Got", "goal_region goal_cell goal_cost path length state")


class _Device(tf._Device):
    """tests/test_gpu_frontier.py's device grid; the frontier of the grid by one eea_frontier_regions call, whose records and
    state stay on the device; a guarded workspace for the auction"""

    def __init__(self, sc, P=None):
        super().__init__(sc.g, sc.grid)
        if sc.sq is not None:
            self.use_sq(sc.sq)
        self.sc, self.P = sc, len(sc.poses) if P is None else P
        _, region, self.rec, self.fstate = self.regions(capi.FRONTIER_OF_GRID, max_regions=sc.max_regions)
        self.region = region
        self.d_region = self.upload(region, np.int32)                       # (an input from here on: it must come back unchanged)
        self.records_before = None if self.d_rec is None else self.d_rec.cpu().numpy().copy()
        self.fstate_before = self.d_state.cpu().numpy().copy()
        self.d_fstate = self.d_state
        self.d_pose = self.upload(sc.poses[:self.P], np.float64).view(-1, 3) if self.P else None
        self.n_aws = capi.frontier_auction_ws_bytes(self.cfg, self.P, sc.max_regions)
        self._aws = torch.full((self.n_aws + 2 * WS_GUARD,), G_IN, dtype=torch.uint8, device="cuda")
        self.d_aws = self._aws[WS_GUARD:WS_GUARD + self.n_aws]
        assert self.d_aws.data_ptr() % 8 == 0
        self.outs = None

    def fresh_outputs(self, n_steps, P=None):
        P = self.P if P is None else P
        self.outs = dict(region=_guarded(np.full(P, S_REGION, np.int32), G_OUT, np.int32), cell=_guarded(np.full(P, S_GEO, np.int32), G_OUT, np.int32),
                         cost=_guarded(np.full(P, S_COST, np.int32), G_OUT, np.int32), length=_guarded(np.full(P, S_GEO, np.int32), G_OUT, np.int32),
                         path=_guarded(np.full(P * n_steps * 3, S_PATH), 2.5, np.float64),
                         state=_guarded(np.full(4, S_STATE, np.uint32).view(np.int32), G_OUT, np.int32))

    def auction(self, max_rounds=0, stream=None, keep_outputs=False, n_steps=None, **over):
        """one call; the six buffers after every guard was looked at"""
        sc, P = self.sc, self.P
        n_steps = sc.n_steps if n_steps is None else n_steps
        if not keep_outputs or self.outs is None:
            self.fresh_outputs(n_steps)
        o = self.outs
        args = dict(scn.call_args(sc), max_rounds=max_rounds, stream=stream)
        args.update(over)
        torch.cuda.synchronize()
        capi.frontier_auction(self.cfg, self.d_grid, self.d_region, self.d_rec, self.d_fstate, sc.max_regions, self.d_pose, o["region"][2],
                              o["cell"][2], o["cost"][2], self.d_aws, o["state"][2], path=o["path"][2].view(P, n_steps, 3) if n_steps else None,
                              length=o["length"][2], sq=self.d_sq, **args)
        torch.cuda.synchronize()
        w = self._aws.cpu().numpy()
        assert (w[:WS_GUARD] == G_IN).all() and (w[-WS_GUARD:] == G_IN).all(), "a guard byte of the auction's workspace was written"
        if self.records_before is not None:
            assert np.array_equal(self.d_rec.cpu().numpy(), self.records_before), "a record was written"
        assert np.array_equal(self.d_fstate.cpu().numpy(), self.fstate_before), "the frontier's state was written"
        return Got(self.check(o["region"][1]).copy(), self.check(o["cell"][1]).copy(), self.check(o["cost"][1]).copy(),
                   self.check(o["path"][1], 2.5).reshape(P, n_steps, 3).copy(), self.check(o["length"][1]).copy(),
                   self.check(o["state"][1]).view(np.uint32).copy())


def _same(got, want):
    """whole buffers, bit for bit; of the state the words the definition fixes"""
    for name in ("goal_region", "goal_cell", "goal_cost", "length"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype == np.int32 and a.tobytes() == b.tobytes(), (name, a.tolist(), b.tolist())
    assert got.path.shape == want.path.shape and np.array_equal(_bits(got.path), _bits(want.path)), np.argwhere(_bits(got.path) != _bits(want.path))[:5]
    assert [int(got.state[k]) for k in (0, 2, 3)] == [int(want.state[k]) for k in (0, 2, 3)], (got.state, want.state)


@pytest.mark.parametrize("name", scn.NAMES)
def test_scenes_in_the_waiting_form_are_the_restatement(name):
    """every scene with every field built to the end: robots off the grid, on a wall, on an unknown cell that blocks (placed
    through the waiver), sealed in, on a member; ties of cost settled by the index and of region by the rank; a capacity above
    one; regions below min_size and past max_regions; a winner of the second round; robots left over; a walk longer than
    n_steps; a grid without a region; a seed that cannot be entered; and in `crowd` 300 robots bidding for one region with
    room for 7 -- two workgroups of the rank launch, each counting against two LDS tiles of bids: exactly the 7 smallest
    (cost, robot) win"""
    sc = scn.scene(name)
    dev = _Device(sc)
    kept = int(dev.fstate[1])
    assert np.array_equal(dev.region, scn.regions(name)[1]) and dev.rec[:kept].tobytes() == scn.regions(name)[2].tobytes()
    got = dev.auction()
    want = scn.answer(name)
    _same(got, want)
    assert got.state[1] > 0 or name == "no_region"
    if name == "crowd":
        assert dev.P == 300 > 256 and got.state.tolist()[2:] == [7, 1]
        ranked = sorted((d, q) for q, (d, r) in want.bids[0].items())
        assert sorted(np.flatnonzero(got.goal_region == 0).tolist()) == sorted(q for _, q in ranked[:7])
        assert ranked[6][0] == ranked[7][0]


@pytest.mark.parametrize("name", ["hall", "maze"])
def test_a_generous_budget_on_another_stream_gives_the_same_bits(name):
    """max_rounds > 0: everything is enqueued on a stream of the caller's, nothing is read on the host; with more tile rounds
    than any field of the scene needs d_state[0] is 1 and the bits are the waiting form's"""
    sc = scn.scene(name)
    dev = _Device(sc)
    st = torch.cuda.Stream()
    got = dev.auction(max_rounds=4 * 3 * scn.T, stream=st.cuda_stream)
    assert got.state[0] == 1
    _same(got, scn.answer(name))


def test_a_budget_of_one_tile_round_says_so_and_stays_in_range():
    """the 3 x 3-tile maze with one tile round per field: d_state[0] is 0, every output element is -1, the pose, or in range,
    and no guard is touched"""
    sc = scn.scene("maze")
    dev = _Device(sc)
    got = dev.auction(max_rounds=1)
    g, P = sc.g, dev.P
    n = int(dev.fstate[1])
    assert got.state[0] == 0 and got.state[2] <= P and got.state[3] <= sc.n_auction
    assert ((got.goal_region >= -1) & (got.goal_region < n)).all() and ((got.goal_cell >= -1) & (got.goal_cell < g.xsize * g.ysize)).all()
    assert (got.goal_cost >= -1).all() and ((got.length >= -1) & (got.length <= sc.n_steps)).all()
    assert got.state[2] == (got.goal_region >= 0).sum()
    for q in range(P):
        if got.goal_region[q] < 0:
            assert got.goal_cell[q] == got.goal_cost[q] == got.length[q] == -1
            assert np.array_equal(_bits(got.path[q]), _bits(np.repeat(sc.poses[q][None], sc.n_steps, axis=0)))
            continue
        assert got.goal_cell[q] >= 0 and got.length[q] >= 0
        for x, y, th in got.path[q]:
            i, j = sr.world2grid(g, x, y)
            assert i < g.ysize and j < g.xsize and (x, y) == ar.geo.cell_centre(g, i, j) and -3.2 < th < 3.2


def test_a_second_call_into_the_same_buffers_gives_the_same_answer():
    """the caller hands the buffers of the first call back -- d_goal_region and d_goal_cell hold its answers, the workspace
    its planes --: the second call's results are identical, and so are those of a third with another n_steps in between"""
    sc = scn.scene("hall")
    dev = _Device(sc)
    first = dev.auction()
    _same(first, scn.answer("hall"))
    again = dev.auction(keep_outputs=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:5], again[:5])) and again.state[[0, 2, 3]].tolist() == first.state[[0, 2, 3]].tolist()
    # one round only, into the same workspace: the nearest-frontier rule, nothing left of the rounds before
    _, region, rec, fstate = scn.regions("hall")
    want = ar.auction(sc.g, sc.grid, region, rec, fstate, sc.max_regions, sc.poses, n_steps=3, sq=sc.sq, **dict(scn.call_args(sc), n_auction=1))
    _same(dev.auction(n_steps=3, n_auction=1), want)
    _same(dev.auction(), scn.answer("hall"))


def test_no_steps_no_lengths_and_no_robots():
    """n_steps == 0 with d_path NULL and d_len NULL; P == 0 writes d_state and nothing else"""
    sc = scn.scene("hall")
    dev = _Device(sc)
    o_want = scn.answer("hall")
    dev.fresh_outputs(0)
    o = dev.outs
    torch.cuda.synchronize()
    capi.frontier_auction(dev.cfg, dev.d_grid, dev.d_region, dev.d_rec, dev.d_fstate, sc.max_regions, dev.d_pose, o["region"][2], o["cell"][2],
                          o["cost"][2], dev.d_aws, o["state"][2], path=None, length=None, sq=dev.d_sq, **scn.call_args(sc))
    torch.cuda.synchronize()
    assert np.array_equal(dev.check(o["region"][1]), o_want.goal_region) and np.array_equal(dev.check(o["cell"][1]), o_want.goal_cell)
    assert np.array_equal(dev.check(o["cost"][1]), o_want.goal_cost) and (dev.check(o["length"][1]) == S_GEO).all()
    empty = _Device(sc, P=0)
    empty.fresh_outputs(2, P=1)                                             # (room for one robot: the sentinels stay)
    o = empty.outs
    empty_pose = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    capi.frontier_auction(empty.cfg, empty.d_grid, empty.d_region, empty.d_rec, empty.d_fstate, sc.max_regions, empty_pose, o["region"][2],
                          o["cell"][2], o["cost"][2], empty.d_aws, o["state"][2], path=o["path"][2].view(1, 2, 3), length=o["length"][2],
                          **scn.call_args(sc))
    torch.cuda.synchronize()
    assert empty.check(o["state"][1]).view(np.uint32).tolist() == [1, 0, 0, 0]
    assert empty.check(o["region"][1])[0] == S_REGION and empty.check(o["cell"][1])[0] == S_GEO and empty.check(o["cost"][1])[0] == S_COST
    assert empty.check(o["length"][1])[0] == S_GEO and (empty.check(o["path"][1], 2.5) == S_PATH).all()
    assert (empty._aws.cpu().numpy() == G_IN).all(), "the workspace was written for an empty fleet"


def test_host_mirror_frontier_auction():
    """host/build/frontier_auction_tests (FrontierRegions::auction in frontier_regions.hpp) runs, and its printed answers are
    the restatement's"""
    exe = os.path.join(ROOT, "ergodic_exploration_amd", "host", "build", "frontier_auction_tests")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    m = {}
    for line in out.stdout.splitlines():
        w = line.split()
        m.setdefault(w[0], []).append(w[1:])
    W, H, res, ox, oy = m["map"][0][:5]
    W, H = int(W), int(H)
    flags, max_regions, n_auction, min_size, cells_per_robot, n_steps = (int(v) for v in m["map"][0][5:])
    g = sr.Geometry(float(ox), float(oy), float(res), W, H, 0.8)
    grid = tf._host_map(W, H)
    poses = np.array([[float(v) for v in p[1:4]] for p in m["robot"]])
    _, region, rec, fstate = fr.regions(fr.OF_GRID, grid, 0.8, max_regions=max_regions)
    want = ar.auction(g, grid, region, rec, fstate, max_regions, poses, n_auction=n_auction, min_size=min_size,
                      cells_per_robot=cells_per_robot, n_steps=n_steps, flags=flags)
    assert [int(v) for v in m["state"][0]] == [int(want.state[k]) for k in (0, 2, 3)]
    goal = np.array([[int(v) for v in r] for r in m["goal"]])
    assert np.array_equal(goal[:, 0], np.arange(len(poses)))
    for k, a in enumerate((want.goal_region, want.goal_cell, want.goal_cost, want.length)):
        assert np.array_equal(goal[:, k + 1], a), (k, goal[:, k + 1], a)
    path = np.array([[float(v) for v in r[2:]] for r in m["path"]]).reshape(len(poses), n_steps, 3)
    assert np.array_equal(_bits(path), _bits(want.path))
    # the fixed robots are worth printing: some go, some in a later round, some cannot
    assert (want.goal_region >= 0).sum() >= 3 and (want.goal_region < 0).sum() >= 3 and want.state[3] >= 2 and (want.goal_cost == 0).any()

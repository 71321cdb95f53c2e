"""Goal paths on the device (include/ergodic_amd.h: eea_geodesic_goto_batch; csrc/goto_kernel.hip).

Checker: tests/goto_restatement.py (held to a second, independent statement and to the invariants of any answer by
tests/test_goto.py).  d_cost, d_status, d_path, d_len and d_state are compared BITWISE as whole buffers, doubles by their bits.
Every output sits between guard elements and holds a sentinel before the call -- which a masked-out robot's elements must still
hold after it --; every input sits between guards and comes back unchanged.  Scenes: tests/goto_scenes.py; the guarded
buffers are tests/test_gpu_geodesic.py's."""
import collections
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ergodic_exploration_amd import capi
from tests import geodesic_restatement as geo
from tests import goto_restatement as gr
from tests import goto_scenes as scn
from tests import sense_restatement as sr
from tests import test_gpu_geodesic as tg

pytestmark = pytest.mark.gpu

ROOT = tg.ROOT
G_OUT, S_STATE = tg.G_OUT, tg.S_STATE
S_COST, S_STATUS, S_PATH, S_LEN = scn.UNTOUCHED
_guarded, _bits = tg._guarded, lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)

Got = collections.namedtuple("Got", "cost status path length state")


class _Device(tg._Device):
    """tests/test_gpu_geodesic.py's device grid with the scene's robots, goals and mask as guarded inputs"""

    def __init__(self, sc, P=None):
        super().__init__(sc.g, sc.grid)
        self.ws_used = False
        if sc.sq is not None:
            self.use_sq(sc.sq)
        self.sc, self.P = sc, len(sc.poses) if P is None else P
        self.d_pose = self.upload(sc.poses[:self.P], np.float64).view(-1, 3) if self.P else None
        self.d_goal = self.upload(sc.goals[:self.P], np.int32) if self.P else None
        self.d_mask = None if sc.mask is None or not self.P else self.upload(sc.mask[:self.P], np.int32)
        self.outs = None

    def check(self, buf, guard=G_OUT):
        """tests/test_gpu_geodesic.py's check with the inputs compared by their bytes: a scene's poses hold NaNs"""
        got = buf.cpu().numpy()
        assert (got[:tg.GUARD] == guard).all() and (got[-tg.GUARD:] == guard).all(), "a guard element was written"
        for img, ibuf, _ in self.inputs:
            assert ibuf.cpu().numpy().tobytes() == img.tobytes(), "an input was written"
        w = self._ws.cpu().numpy()
        assert (w == tg.G_IN).all() or self.ws_used, "the geodesic workspace was written by a call that takes none"
        assert (w[:tg.WS_GUARD] == tg.G_IN).all() and (w[-tg.WS_GUARD:] == tg.G_IN).all(), "a guard byte of the workspace was written"
        return got[tg.GUARD:-tg.GUARD]

    def field(self, *args, **kw):
        self.ws_used = True
        return super().field(*args, **kw)

    def fresh_outputs(self, n_steps, P=None):
        P = self.P if P is None else P
        self.outs = dict(cost=_guarded(np.full(P, S_COST, np.int32), G_OUT, np.int32), status=_guarded(np.full(P, S_STATUS, np.int32), G_OUT, np.int32),
                         length=_guarded(np.full(P, S_LEN, np.int32), G_OUT, np.int32), path=_guarded(np.full(P * n_steps * 3, S_PATH), 2.5, np.float64),
                         state=_guarded(np.full(4, S_STATE, np.uint32).view(np.int32), G_OUT, np.int32))

    def read(self, n_steps, P=None):
        P = self.P if P is None else P
        o = self.outs
        return Got(self.check(o["cost"][1]).copy(), self.check(o["status"][1]).copy(), self.check(o["path"][1], 2.5).reshape(P, n_steps, 3).copy(),
                   self.check(o["length"][1]).copy(), self.check(o["state"][1]).view(np.uint32).copy())

    def goto(self, stream=None, keep_outputs=False, n_steps=None, with_path=True, with_len=True, **over):
        """one call; the five buffers after every guard was looked at"""
        sc, P = self.sc, self.P
        n_steps = sc.n_steps if n_steps is None else n_steps
        if not keep_outputs or self.outs is None:
            self.fresh_outputs(n_steps)
        o = self.outs
        args = dict(scn.call_args(sc), stream=stream)
        args.update(over)
        torch.cuda.synchronize()
        capi.geodesic_goto_batch(self.cfg, self.d_grid, self.d_pose, self.d_goal, o["cost"][2], o["status"][2], o["state"][2],
                                 path=o["path"][2].view(P, n_steps, 3) if with_path else None, length=o["length"][2] if with_len else None,
                                 mask=self.d_mask, sq=self.d_sq, **args)
        torch.cuda.synchronize()
        return self.read(n_steps)


def _same(got, want):
    """whole buffers, bit for bit"""
    for name in ("cost", "status", "length"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype == np.int32 and a.tobytes() == b.tobytes(), (name, np.flatnonzero(a != b)[:8], a[a != b][:8], b[a != b][:8])
    assert got.path.shape == want.path.shape and np.array_equal(_bits(got.path), _bits(want.path)), np.argwhere(_bits(got.path) != _bits(want.path))[:5]
    assert got.state.tolist() == want.state.tolist(), (got.state, want.state)


@pytest.mark.parametrize("name", scn.NAMES)
def test_scenes_are_the_restatement(name):
    """every scene: windows clipped on each side, 1 x N and N x 1, a robot on its goal, the move order on ties, a wall whose gap
    a margin reaches or not, no corner cutting, a path many times the window's side, the waivers and every status, a masked-out
    robot, a window of exactly the cap and one past it, a margin of 2^32 - 1, and more robots than the launch has workgroups"""
    _same(_Device(scn.scene(name)).goto(), scn.answer(name))


@pytest.mark.parametrize("name", ["wall_m12", "waivers_block"])
def test_another_stream_gives_the_same_bits(name):
    st = torch.cuda.Stream()
    _same(_Device(scn.scene(name)).goto(stream=st.cuda_stream), scn.answer(name))


def test_a_second_call_into_the_same_buffers_gives_the_same_answer():
    """the caller hands the buffers of the first call back: the second call's results are identical; and a call with another
    margin in between leaves nothing behind"""
    dev = _Device(scn.scene("wall_m12"))
    first = dev.goto()
    _same(first, scn.answer("wall_m12"))
    again = dev.goto(keep_outputs=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    _same(dev.goto(keep_outputs=True, margin=0), scn.answer("wall_m0"))
    _same(dev.goto(keep_outputs=True), scn.answer("wall_m12"))


@pytest.mark.parametrize("name, n_steps", [("serpentine_m0", 7), ("open_m5", 1), ("waivers_block", 2)])
def test_fewer_steps_than_the_path_keep_the_whole_cost(name, n_steps):
    want = scn.answer(name, n_steps)
    full = scn.answer(name)
    assert np.array_equal(want.cost, full.cost) and (want.length == n_steps).any() and (full.length > n_steps).any()
    _same(_Device(scn.scene(name)).goto(n_steps=n_steps), want)


def test_no_steps_no_lengths_and_no_robots():
    """n_steps == 0 with d_path NULL and d_len NULL; P == 0 writes d_state and nothing else"""
    sc = scn.scene("waivers_block")
    want = scn.answer("waivers_block", 0)
    dev = _Device(sc)
    got = dev.goto(n_steps=0, with_path=False, with_len=False)
    assert got.cost.tobytes() == want.cost.tobytes() and got.status.tobytes() == want.status.tobytes()
    assert got.state.tolist() == want.state.tolist() and (got.length == S_LEN).all() and got.path.size == 0
    empty = _Device(sc, P=0)
    empty.fresh_outputs(2, P=1)                                             # (room for one robot: the sentinels stay)
    o = empty.outs
    no_pose, no_goal = torch.zeros((0, 3), dtype=torch.float64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")
    for pose, goal in ((no_pose, no_goal), (None, None)):
        o["state"][2].fill_(S_STATE)
        capi.geodesic_goto_batch(empty.cfg, empty.d_grid, pose, goal, o["cost"][2], o["status"][2], o["state"][2],
                                 path=o["path"][2].view(1, 2, 3), length=o["length"][2], **scn.call_args(sc))
        torch.cuda.synchronize()
        got = empty.read(2, P=1)
        assert got.state.tolist() == [0, 0, 0, 0]
        assert got.cost[0] == S_COST and got.status[0] == S_STATUS and got.length[0] == S_LEN and (got.path == S_PATH).all()


def _many_on_traversable_cells():
    """32 robots of `many` that stand on traversable cells, with their goals, at a margin that makes the window the grid"""
    sc = scn.scene("many")
    trav = geo.traversable(sc.g, sc.grid, None, 0, sc.flags)
    cells = [sr.world2grid(sc.g, p[0], p[1]) for p in sc.poses[:400]]
    pick = np.array([q for q, (i, j) in enumerate(cells) if trav[i, j] and 0 <= sc.goals[q]][:32])
    return scn.Scene(sc.g, sc.grid, sc.poses[pick], sc.goals[pick], 96, 40, None, 0, sc.flags, None)


@pytest.mark.parametrize("which", ["many", "wall"])
def test_a_window_that_is_the_grid_is_the_field_and_its_path_from_the_same_library(which):
    """library against library on a grid of at most EEA_GOTO_MAX_CELLS cells with margin >= its side -- the 96 x 96 grid of
    `many`, and the wall scene with its robots that no margin helps --: for robots on traversable cells the answers are bitwise
    eea_geodesic_field(d_cells = [g_q]) + eea_geodesic_path_batch(pose q)"""
    sub = _many_on_traversable_cells() if which == "many" else scn.scene("wall_m0")._replace(margin=30)
    g, n_steps = sub.g, sub.n_steps
    assert g.xsize * g.ysize <= capi.GOTO_MAX_CELLS and sub.margin >= max(g.xsize, g.ysize) and sub.mask is None and sub.sq is None
    trav = geo.traversable(g, sub.grid, None, 0, sub.flags)
    cells = [sr.world2grid(g, p[0], p[1]) for p in sub.poses]
    assert all(trav[i, j] for i, j in cells)
    dev = _Device(sub)
    got = dev.goto()
    assert (got.status == gr.OK).sum() >= 6 and (got.status != gr.WINDOW).all()
    assert (got.status == (gr.NO_GOAL if which == "many" else gr.CUT_OFF)).sum() >= 3
    assert (got.length == n_steps).any() == (which == "many") and ((got.length >= 0) & (got.length < n_steps)).any()
    for k in range(len(cells)):
        field, state = dev.field(cells=np.array([sub.goals[k]], dtype=np.int32), flags=sub.flags)
        path, length = dev.path(field, sub.poses[k:k + 1], n_steps)
        i, j = cells[k]
        assert got.cost[k] == field[i, j] and got.length[k] == length[0], (k, got.cost[k], field[i, j], got.length[k], length)
        assert np.array_equal(_bits(got.path[k]), _bits(path[0])), k
        assert (got.status[k] == gr.OK) == (field[i, j] >= 0) and (got.status[k] == gr.NO_GOAL) == (state[2] == 0)


def test_host_mirror_goal_paths():
    """host/build/goal_paths_tests (GoalPaths::go in goal_paths.hpp) runs, and its printed answers are the restatement's"""
    exe = os.path.join(ROOT, "ergodic_exploration_amd", "host", "build", "goal_paths_tests")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    m = {}
    for line in out.stdout.splitlines():
        w = line.split()
        m.setdefault(w[0], []).append(w[1:])
    W, H = int(m["map"][0][0]), int(m["map"][0][1])
    res, ox, oy = (float(v) for v in m["map"][0][2:5])
    flags, margin, n_steps = (int(v) for v in m["map"][0][5:8])
    g = sr.Geometry(ox, oy, res, W, H, 0.8)
    grid = np.array([int(v) for row in m["row"] for v in row], dtype=np.int8).reshape(H, W)
    poses = np.array([[float(v) for v in p[1:4]] for p in m["robot"]])
    goals = np.array([int(p[4]) for p in m["robot"]], dtype=np.int32)
    want = gr.goto(g, grid, poses, goals, margin, n_steps, flags=flags)
    assert [int(v) for v in m["state"][0]] == want.state.tolist()
    ans = np.array([[int(v) for v in r] for r in m["answer"]])
    assert np.array_equal(ans[:, 0], np.arange(len(poses)))
    for k, a in enumerate((want.cost, want.status, want.length)):
        assert np.array_equal(ans[:, k + 1], a), (k, ans[:, k + 1], a)
    path = np.array([[float(v) for v in r[2:]] for r in m["path"]]).reshape(len(poses), n_steps, 3)
    assert np.array_equal(_bits(path), _bits(want.path))
    # the fixed robots are worth printing: every status among them
    assert sorted(set(want.status.tolist())) == [gr.OK, gr.NO_ROBOT, gr.NO_GOAL, gr.WINDOW, gr.CUT_OFF] and (want.cost == 0).any()

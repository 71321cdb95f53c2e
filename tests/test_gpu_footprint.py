"""Footprint collision on the device (eea_footprint_check_batch / eea_footprint_traj_first: csrc/footprint_kernel.hip) against the
numpy restatement of tests/footprint_restatement.py (checked against itself in tests/test_footprint.py).  The verdict is pinned
wherever no occupied centre lies within 1e-9 m of the footprint's boundary (the device's sine and cosine are within a few ulp
of numpy's): such poses are "decided", and at most 0.5 % of a case may be undecided.  With and without the distance field the
device runs the same arithmetic: those two are compared bit for bit over all poses.  Every output buffer is longer than the
call needs and pre-filled with a value no answer has."""
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ergodic_exploration_amd import capi
from tests import clearance_restatement as cr
from tests import footprint_restatement as fr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -77
PAD = 70
NAMES = list(fr.FOOTPRINTS)
COMBOS = [(n, name) for n in range(len(cr.SETS)) for name in NAMES]
RADII = (0.3, 1.2, 0.1)          # what eea_distance_field checks of a configuration; the footprint calls read none of them


class Scene:
    """a grid on the device with its distance field, and the calls on it"""

    def __init__(self, data, xmin, ymin, res, threshold=0.8):
        self.data, self.xmin, self.ymin, self.res, self.threshold = data, xmin, ymin, res, threshold
        ys, xs = data.shape
        self.cfg = capi.make_collision_cfg(xmin, ymin, res, xs, ys, *RADII, threshold)
        self.d_grid = torch.as_tensor(np.ascontiguousarray(data)).cuda()
        self.d_sq = torch.full((ys, xs), FILL, dtype=torch.int32, device="cuda")
        capi.distance_field(self.cfg, self.d_grid, self.d_sq)

    def check(self, verts, poses, with_sq):
        P = len(poses)
        d_pose = torch.as_tensor(np.ascontiguousarray(poses, dtype=np.float64)).cuda().reshape(P, 3)
        hit = torch.full((P + PAD,), FILL, dtype=torch.int32, device="cuda")
        capi.footprint_check_batch(self.cfg, capi.Footprint.of(verts), self.d_grid, d_pose, hit, self.d_sq if with_sq else None)
        torch.cuda.synchronize()
        got = hit.cpu().numpy()
        assert (got[P:] == FILL).all()                     # nothing past P
        assert np.isin(got[:P], (0, 1)).all(), np.unique(got[:P])
        return got[:P].astype(bool)

    def first(self, verts, traj, with_sq):
        B = len(traj)
        d_traj = torch.as_tensor(np.ascontiguousarray(traj, dtype=np.float64)).cuda()
        step = torch.full((B + PAD,), FILL, dtype=torch.int32, device="cuda")
        capi.footprint_traj_first(self.cfg, capi.Footprint.of(verts), self.d_grid, d_traj, step, self.d_sq if with_sq else None)
        torch.cuda.synchronize()
        got = step.cpu().numpy()
        assert (got[B:] == FILL).all()
        return got[:B]

    def brute(self, verts, poses):
        return fr.brute(self.res, self.xmin, self.ymin, self.data, self.threshold, verts, poses)

    def classes(self, verts, poses):
        return fr.filtered(self.res, self.xmin, self.ymin, self.data, self.threshold, verts, poses)[1]

    def both(self, verts, poses, what=""):
        """the device's verdicts, the same with and without the field over ALL poses and the restatement's on the decided ones"""
        plain, through = self.check(verts, poses, False), self.check(verts, poses, True)
        bad = np.nonzero(plain != through)[0]
        assert len(bad) == 0, (what, "with and without d_sq differ", bad[:10], np.asarray(poses)[bad[:10]])
        ref, margin = self.brute(verts, poses)
        decided = margin >= fr.DECIDED
        print(what, "poses:", len(poses), "hits:", int(ref.sum()), "undecided:", int((~decided).sum()),
              "smallest margin: %.3g m" % (margin.min() if len(margin) else np.inf))
        assert (~decided).sum() <= 0.005 * len(poses), (what, int((~decided).sum()))
        bad = np.nonzero((plain != ref) & decided)[0]
        assert len(bad) == 0, (what, bad[:10], np.asarray(poses)[bad[:10]], margin[bad[:10]], ref[bad[:10]])
        return plain


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for n, (res, coll, _) in enumerate(cr.SETS):
        data, poses, xmin, ymin = fr.scene(res, coll)
        out[n] = (Scene(data, xmin, ymin, res, coll[3]), poses)
    return out


@pytest.mark.parametrize("n,name", COMBOS)
def test_verdicts_of_the_24_combinations(scenes, n, name):
    """3000 poses up to 30 cells outside the 90 x 70 map (corners, the column fx == xsize and the row fy == ysize, 1e9, NaN among
    them), headings in (-pi, pi); behind them six poses 2^32 cells away that world2Grid's wrap folds on to an occupied cell"""
    scene, poses = scenes[n]
    wrapped = fr.wrap_poses(scene.res, scene.xmin, scene.ymin)
    got = scene.both(fr.FOOTPRINTS[name], np.concatenate([poses, wrapped]), (n, name))
    assert got.sum() > 100 and not got[:len(poses)][~np.isfinite(poses).all(1)].any()
    assert not got[len(poses):].any()


@pytest.mark.parametrize("P", [1, 63, 64, 65, 4097])
def test_batch_sizes(scenes, P):
    """one pose, one lane short of a wavefront, one wavefront, one more, and many workgroups with a ragged end"""
    scene, poses = scenes[2]
    rng = np.random.default_rng(P)
    pick = poses[rng.integers(8, len(poses), P)]
    got = scene.both(fr.FOOTPRINTS["tri"], pick, P)
    assert P < 63 or (got.any() and not got.all())


def test_wavefronts_by_their_ambiguous_lanes(scenes):
    """four groups of 64 poses (a wavefront's lanes): only lane 0 ambiguous, only lane 63, none, all 64 -- the others surely free
    or sure hits by the field; the ambiguous poses are hits and misses alike"""
    scene, poses = scenes[2]
    verts = fr.FOOTPRINTS["oct"]
    cls = scene.classes(verts, poses)
    ref, margin = scene.brute(verts, poses)
    assert (margin >= fr.DECIDED).all()
    sure = np.nonzero(np.isin(cls, (fr.FREE, fr.HIT)))[0]
    amb_hit, amb_free = np.nonzero((cls == fr.AMBIGUOUS) & ref)[0], np.nonzero((cls == fr.AMBIGUOUS) & ~ref)[0]
    assert len(sure) >= 64 and len(amb_hit) >= 33 and len(amb_free) >= 33 and (cls[sure] == fr.HIT).any() and (cls[sure] == fr.FREE).any()
    mixed = np.stack([amb_hit[:32], amb_free[:32]], 1).reshape(-1)
    idx = np.concatenate([[amb_hit[32]], sure[:63], sure[1:64], [amb_free[32]], sure[:64], mixed])
    batch = poses[idx]
    c = scene.classes(verts, batch).reshape(4, 64) == fr.AMBIGUOUS
    assert c[0].tolist() == [True] + [False] * 63 and c[1].tolist() == [False] * 63 + [True] and not c[2].any() and c[3].all()
    got = scene.both(verts, batch)
    assert np.array_equal(got, ref[idx]) and got[0] and not got[127] and got[192:].sum() == 32


def _around(scene, rng, P, reach):
    """P poses within `reach` metres of the grid, any heading"""
    ys, xs = scene.data.shape
    x = rng.uniform(scene.xmin - reach, scene.xmin + xs * scene.res + reach, P)
    y = rng.uniform(scene.ymin - reach, scene.ymin + ys * scene.res + reach, P)
    return np.stack([x, y, rng.uniform(-np.pi, np.pi, P)], 1)


@pytest.mark.parametrize("name", NAMES)
def test_small_empty_and_full_grids(name):
    """a 1 x 1 grid, occupied and not; a 7 x 5 grid that lies wholly inside the box of every pose near it; an empty grid (the
    field is -1 everywhere: everything is free) and a full one"""
    verts = fr.FOOTPRINTS[name]
    rng = np.random.default_rng(len(name))
    one = Scene(np.array([[100]], dtype=np.int8), 0.3, -0.2, 0.1)
    got = one.both(verts, _around(one, rng, 300, 1.2), "1 x 1")
    assert got.any() and not got.all()
    none = Scene(np.array([[79]], dtype=np.int8), 0.3, -0.2, 0.1)
    assert not none.both(verts, _around(none, rng, 300, 1.2), "1 x 1 free").any()
    data = np.zeros((5, 7), dtype=np.int8)
    data[0, 0] = data[4, 6] = data[2, 3] = 100
    small = Scene(data, -0.35, -0.25, 0.1)
    box = fr.thresholds(*fr.planes(verts)[3:], 0.1)[2]
    near = _around(small, rng, 400, 1.0)
    near[:100, :2] = rng.uniform(-0.1, 0.1, (100, 2))     # these within a cell of the grid's centre: the box covers all 7 x 5 cells
    assert box >= 4
    got = small.both(verts, near, "7 x 5")
    assert got.any() and not got.all()
    empty = Scene(np.zeros((33, 70), dtype=np.int8), -2.0, -1.0, 0.1)
    assert (empty.d_sq.cpu().numpy() == -1).all()
    assert not empty.both(verts, _around(empty, rng, 500, 1.5), "empty").any()
    full = Scene(np.full((33, 70), 100, dtype=np.int8), -2.0, -1.0, 0.1)
    poses = _around(full, rng, 500, 1.5)
    got = full.both(verts, poses, "full")
    inside = fr.cells(0.1, -2.0, -1.0, 70, 33, poses)[0]
    assert got[inside].all() and not got.all()


@pytest.mark.parametrize("n", range(len(cr.SETS)))
def test_poses_out_of_every_range(scenes, n):
    """NaN and +-inf in each component, 1e9 and -1e300 in each coordinate, and the six poses 2^32 cells away that world2Grid's x86
    wrap folds on to an occupied cell of the grid (a sure hit, were the cell taken from that lookup): all free, with and without
    the field (their boxes are clamped as doubles before anything is converted); with and without the field agree on the whole
    batch, headings of 1e9 and -1e300 included; finite neighbours in the same wavefronts keep their answers"""
    scene, poses = scenes[n]
    nan, inf = float("nan"), float("inf")
    x, y = 0.5, 0.5
    odd = np.array([[nan, y, 0], [x, nan, 0], [x, y, nan], [inf, y, 0], [-inf, y, 0], [x, inf, 0], [x, -inf, 0], [x, y, inf], [x, y, -inf],
                    [1e9, y, 0], [-1e9, y, 1], [x, 1e9, 2], [x, -1e9, 3], [-1e300, y, 0], [1e300, y, 0], [x, -1e300, 0], [x, 1e300, 0],
                    [1e300, 1e300, 1e300], [nan, nan, nan], [inf, -inf, nan]])
    wrapped = fr.wrap_poses(scene.res, scene.xmin, scene.ymin)
    turned = np.array([[x, y, 1e9], [x, y, -1e300]])         # finite: the verdict is the geometry's, whatever it is
    never = len(odd) + len(wrapped)
    batch = np.concatenate([odd, wrapped, turned, poses[8:50]])
    assert scene.data[0, 5] == 100                          # where the wrap would put the six
    for name in NAMES:
        ref, margin = scene.brute(fr.FOOTPRINTS[name], batch)
        assert not ref[:never].any()
        plain, through = scene.check(fr.FOOTPRINTS[name], batch, False), scene.check(fr.FOOTPRINTS[name], batch, True)
        assert np.array_equal(plain, through), (name, np.nonzero(plain != through)[0])
        assert not plain[:never].any(), (name, plain[:never])
        assert np.array_equal(plain[never + len(turned):], ref[never + len(turned):]), name


def test_fact_scenes():
    """`rect` (0.9 m x 0.5 m) in a corridor of 0.7 m is free along it and hits across it -- no disc says both; `offc` with a
    wall 0.7 m ahead hits facing it and is free facing away.  Every wall centre is 0.05 m or more from the boundary"""
    for walls, pose_xy, name, expect in ((fr.CORRIDOR, fr.CORRIDOR_POSE, "rect", {0.0: False, np.pi / 2: True, np.pi: False, -np.pi / 2: True}),
                                         (fr.WALL_AHEAD, fr.WALL_POSE, "offc", {0.0: True, np.pi: False, np.pi / 2: False})):
        scene = Scene(fr.fact_scene(walls), cr.XMIN41, cr.YMIN41, cr.RES41)
        poses = np.array([[pose_xy[0], pose_xy[1], th] for th in expect])
        for with_sq in (False, True):
            assert scene.check(fr.FOOTPRINTS[name], poses, with_sq).tolist() == list(expect.values()), (name, with_sq)
    # the discs of the issue on the corridor, by the reference-exact ring search: 0.51 m cannot enter, 0.25 m fits at any heading
    scene = Scene(fr.fact_scene(fr.CORRIDOR), cr.XMIN41, cr.YMIN41, cr.RES41)
    pose = torch.as_tensor(np.array([[fr.CORRIDOR_POSE[0], fr.CORRIDOR_POSE[1], np.pi / 2]])).cuda()
    for radius, expect in ((0.51, 1), (0.25, 0)):
        hit = torch.full((1,), FILL, dtype=torch.int32, device="cuda")
        capi.collision_check_batch(capi.make_collision_cfg(cr.XMIN41, cr.YMIN41, cr.RES41, cr.N41, cr.N41, radius, 1.0, 0.0, 0.8),
                                   scene.d_grid, pose, hit)
        torch.cuda.synchronize()
        assert int(hit[0]) == expect, radius


@pytest.mark.parametrize("n,name", [(0, "oct"), (1, "offc"), (2, "rect"), (5, "tri")])
def test_relation_to_the_distance_query(scenes, n, name):
    """on the poses with a cell: a hit => the field's sq at the pose <= sq_free; 0 <= sq <= sq_hit => a hit"""
    scene, poses = scenes[n]
    verts = fr.FOOTPRINTS[name]
    has = fr.cells(scene.res, scene.xmin, scene.ymin, 90, 70, poses)[0]
    pick = poses[has]
    near = torch.full((70, 90), FILL, dtype=torch.int32, device="cuda")
    capi.distance_field(scene.cfg, scene.d_grid, scene.d_sq, near)
    out = torch.full((len(pick), 4), FILL, dtype=torch.int32, device="cuda")
    capi.distance_query_batch(scene.cfg, scene.d_sq, near, torch.as_tensor(pick).cuda(), out)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[:, 0] != capi.COLLISION_OFF_GRID).all() and (out[:, 1] >= 0).all()
    sq = out[:, 1]
    pl = fr.planes(verts)
    sq_hit, sq_free, _ = fr.thresholds(pl[3], pl[4], scene.res)
    for with_sq in (False, True):
        got = scene.check(verts, pick, with_sq)
        assert (sq[got] <= sq_free).all() and got[sq <= sq_hit].all()
    assert got.any() and (sq > sq_free).any() == (not (name == "offc" and n == 0)) and ((sq <= sq_hit).any() == (sq_hit >= 0))


@pytest.mark.parametrize("B", [1, 130])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 200])
def test_first_colliding_step(scenes, T, B):
    """trajectories drawn from the scene's poses: free throughout (-1), a hit only in the first chunk of 64 steps, a hit only
    in the last chunk, hits anywhere; each result is first_step of the per-pose verdicts of eea_footprint_check_batch on the
    same steps, and the restatement's"""
    scene, poses = scenes[2]
    verts = fr.FOOTPRINTS["rect"]
    ref, margin = scene.brute(verts, poses)
    assert (margin >= fr.DECIDED).all()
    fin = np.isfinite(poses).all(1)
    free, hits = np.nonzero(~ref & fin)[0], np.nonzero(ref)[0]
    rng = np.random.default_rng(1000 * T + B)
    idx = rng.choice(free, (B, T))
    last0 = 64 * ((T - 1) // 64)                            # the first step of the last chunk
    for b in range(B):
        kind = (b + (T % 4)) % 4 if B > 1 else 2
        if kind == 1:                                       # only in the first chunk
            idx[b, rng.integers(0, min(T, 64))] = rng.choice(hits)
        elif kind == 2:                                     # only in the last chunk (with two hits there when it has room)
            t = rng.integers(last0, T)
            idx[b, t] = rng.choice(hits)
            idx[b, rng.integers(t, T)] = rng.choice(hits)
        elif kind == 3:                                     # anywhere, many
            where = rng.random(T) < 0.1
            idx[b, where] = rng.choice(hits, int(where.sum()))
    traj = poses[idx]
    want = fr.first_step(ref[idx])
    assert B == 1 or ((want == -1).any() and (want >= last0).any() and ((want >= 0) & (want < 64)).any())
    per_pose = scene.check(verts, traj.reshape(B * T, 3), True).reshape(B, T)
    for with_sq in (False, True):
        got = scene.first(verts, traj, with_sq)
        assert got.dtype == np.int32 and np.array_equal(got, fr.first_step(per_pose)), (with_sq, got, fr.first_step(per_pose))
        assert np.array_equal(got, want), (with_sq, np.nonzero(got != want)[0][:10])
    if B == 1:                                              # and the free trajectory
        assert scene.first(verts, poses[rng.choice(free, (1, T))], True).tolist() == [-1]
        assert scene.first(verts, poses[rng.choice(free, (1, T))], False).tolist() == [-1]


def test_host_mirror_prints_the_restatements_answers():
    """host/build/footprint_tests (Footprint in footprint.hpp: check with and without a DistanceField, firstStep, the malformed
    footprints) runs once; what it prints against the restatement on the same grid"""
    exe = os.path.join(ROOT, "ergodic_exploration_amd", "host", "build", "footprint_tests")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.splitlines()]
    assert lines[0][0] == "grid" and (int(lines[0][1]), int(lines[0][2])) == (50, 40)
    res, ox, oy = (float(v) for v in lines[0][3:6])
    assert (res, ox, oy) == (0.1, -1.0, -2.0)
    data = np.zeros((40, 50), dtype=np.int8)
    data[10:14, 20:26] = 100
    data[30, 5], data[31, 7], data[25, 40], data[3, 44], data[38, 30] = 80, 79, 100, 100, 100
    data[5:8, 2] = -1
    assert [l for l in lines if l[0] == "refused"] == [["refused", "5"]]
    for f, name in enumerate(("rect", "offc")):
        verts = fr.FOOTPRINTS[name]
        radii = [l for l in lines if l[0] == "radii" and int(l[1]) == f][0]
        assert (float(radii[2]), float(radii[3])) == tuple(float(v) for v in fr.planes(verts)[3:])      # (17 significant digits)
        rows = [l for l in lines if l[0] == "check" and int(l[1]) == f]
        assert len(rows) == 154
        poses = np.array([[float(v) for v in l[3:6]] for l in rows])
        plain, through = np.array([int(l[6]) for l in rows], dtype=bool), np.array([int(l[7]) for l in rows], dtype=bool)
        ref, margin = fr.brute(res, ox, oy, data, 0.8, verts, poses)
        decided = margin >= fr.DECIDED
        assert (~decided).sum() <= 0.005 * len(poses)          # (of 154: none)
        assert np.array_equal(plain, through) and np.array_equal(plain, ref)
        assert ref.any() and not ref.all()
        firsts = [l for l in lines if l[0] == "first" and int(l[1]) == f]
        assert len(firsts) == 7
        for l in firsts:
            b, T = int(l[2]), int(l[3])
            want = int(fr.first_step(ref[None, b:b + T])[0])
            assert int(l[4]) == want and int(l[5]) == want, l
        assert len({int(l[4]) for l in firsts}) > 2

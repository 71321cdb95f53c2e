"""The distance field on the device (eea_distance_field / eea_distance_query_batch / eea_distance_traj_min:
csrc/distance_kernel.hip) bit for bit against the numpy restatements of tests/distance_restatement.py (checked against each
other and related to the oracle's ring search in tests/test_distance_field.py).  Every output buffer is pre-filled with a
value no answer has."""
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pyoracle as po
from ergodic_exploration_amd import capi
from tests import clearance_restatement as cr
from tests import distance_restatement as dr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -77
COLL = (0.7, 1.0, 0.2)          # boundary, search, obstacle threshold of the build-only tests (the build reads the fourth only)


def _cfg(ys, xs, threshold):
    return capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, *COLL, threshold)


def _build(cfg, data, with_nearest=True, sq=None, near=None):
    """(sq, nearest) int32 [ysize][xsize] of eea_distance_field for the int8 array data; sq / near: device buffers to build into"""
    ys, xs = data.shape
    d_grid = torch.as_tensor(np.ascontiguousarray(data)).cuda()
    if sq is None:
        sq = torch.empty(ys * xs, dtype=torch.int32, device="cuda")
        near = torch.empty(ys * xs, dtype=torch.int32, device="cuda")
    sq.fill_(FILL)
    near.fill_(FILL)
    capi.distance_field(cfg, d_grid, sq, near if with_nearest else None)
    torch.cuda.synchronize()
    got_sq, got_near = sq.cpu().numpy(), near.cpu().numpy()
    assert (got_sq[ys * xs:] == FILL).all() and (got_near[ys * xs:] == FILL).all()       # nothing past the grid
    if not with_nearest:
        assert (got_near == FILL).all()
    return got_sq[:ys * xs].reshape(ys, xs), got_near[:ys * xs].reshape(ys, xs)


def _check(got, ref, what=""):
    for name, a, b in (("sq", got[0], ref[0]), ("nearest", got[1], ref[1])):
        bad = np.argwhere(a != b)
        assert len(bad) == 0, (what, name, len(bad), bad[:8].tolist(), a[tuple(bad[:8].T)].tolist(), b[tuple(bad[:8].T)].tolist())


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ---- the build ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("threshold", [0.8, 0.5])
@pytest.mark.parametrize("ys,xs", dr.SHAPES)
def test_field_is_the_brute_force_minimum(ys, xs, threshold):
    """one row, one column, fewer rows than strips, rows and columns that are no multiple of a wavefront, several workgroups
    of the column pass and several strides of the row pass; about 2 % of the cells take 100 / 80 / 79 / 50 / 49 / -1 / -128 /
    127; d_sq and d_nearest exactly, and d_sq the same without d_nearest"""
    data = dr.random_grid(ys, xs, seed=ys * 1000 + xs)
    ref = dr.brute_force(data, threshold)
    cfg = _cfg(ys, xs, threshold)
    _check(_build(cfg, data), ref)
    alone, _ = _build(cfg, data, with_nearest=False)
    assert np.array_equal(alone, ref[0])


def test_single_cell_grids():
    for value, threshold, expect in ((100, 0.8, (0, 0)), (80, 0.8, (0, 0)), (79, 0.8, (-1, -1)), (0, 0.8, (-1, -1)), (-1, 0.5, (-1, -1)),
                                     (50, 0.5, (0, 0))):
        sq, near = _build(_cfg(1, 1, threshold), np.array([[value]], dtype=np.int8))
        assert (int(sq[0, 0]), int(near[0, 0])) == expect, (value, threshold)


def test_worst_cases_have_their_closed_forms():
    """129 x 257: one occupied cell in each corner in turn (every lane of the row pass walks to it), no occupied cell, every
    cell occupied"""
    ys, xs = 129, 257
    cfg = _cfg(ys, xs, 0.8)
    ii, jj = np.mgrid[0:ys, 0:xs]
    for ci, cj in ((0, 0), (0, xs - 1), (ys - 1, 0), (ys - 1, xs - 1)):
        data = np.zeros((ys, xs), dtype=np.int8)
        data[ci, cj] = 100
        sq, near = _build(cfg, data)
        assert np.array_equal(sq, (ii - ci) ** 2 + (jj - cj) ** 2) and (near == ci * xs + cj).all(), (ci, cj)
    sq, near = _build(cfg, np.zeros((ys, xs), dtype=np.int8))
    assert (sq == -1).all() and (near == -1).all()
    sq, _ = _build(cfg, np.zeros((ys, xs), dtype=np.int8), with_nearest=False)
    assert (sq == -1).all()
    sq, near = _build(cfg, np.full((ys, xs), 100, dtype=np.int8))
    assert (sq == 0).all() and np.array_equal(near.reshape(-1), np.arange(ys * xs))


TIES = [[(-6, 0), (6, 0)], [(0, -6), (0, 6)], [(-4, -4), (4, 4)], [(4, -4), (-4, 4)], [(-7, 0), (7, 0), (0, -7), (0, 7)],
        [(5, 0), (-5, 0), (0, 5), (0, -5), (3, 4), (4, 3)], [(5, 0), (-5, 0), (0, 5), (3, 4), (4, 3), (-3, -4), (-4, -3)]]


@pytest.mark.parametrize("cells", TIES)
def test_ties_go_to_the_smallest_index(cells):
    """41 x 41, occupied cells as offsets (dx, dy) from the centre (20, 20): pairs equidistant left / right, up / down and on
    the two diagonals, the four axis cells at distance 5 with (3, 4) and (4, 3): the smallest row-major index wins at the
    centre and along the bisectors"""
    n = cr.N41
    data = np.zeros((n, n), dtype=np.int8)
    for dx, dy in cells:
        data[20 + dy, 20 + dx] = 100
    ref = dr.brute_force(data, 0.8)
    got = _build(_cfg(n, n, 0.8), data)
    _check(got, ref, cells)
    idx = sorted((20 + dy) * n + 20 + dx for dx, dy in cells)
    dist = {(i // n - 20) ** 2 + (i % n - 20) ** 2 for i in idx}
    if len(dist) == 1:                                           # all cells tie at the centre
        assert got[1][20, 20] == idx[0] and got[0][20, 20] == dist.pop()
    a, b = idx[0], idx[1]                                        # along the bisector of the two smallest: never the larger one
    ii, jj = np.mgrid[0:n, 0:n]
    tie = (ii - a // n) ** 2 + (jj - a % n) ** 2 == (ii - b // n) ** 2 + (jj - b % n) ** 2
    assert tie.sum() >= 20 and not (got[1][tie] == b).any()


def test_a_larger_grid_against_the_separable_form():
    ys, xs = 300, 700
    data = dr.random_grid(ys, xs, seed=300700, fraction=0.002)
    data[40:44, 100:230] = 90                                    # a wall, and a wide empty region to its right
    data[:, 400:] = 0
    data[299, 699] = 80
    _check(_build(_cfg(ys, xs, 0.8), data), dr.separable(data, 0.8))


def test_no_stale_state_between_builds():
    """A (63 x 65), then B (129 x 257, other content) into the same buffers, then A again: both A builds are the restatement's,
    bit for bit; the same after eea_release_collision_caches (the calls keep nothing between them)"""
    a = dr.random_grid(63, 65, seed=1)
    b = dr.random_grid(129, 257, seed=2, fraction=0.2)
    ref_a, ref_b = dr.brute_force(a, 0.8), dr.brute_force(b, 0.5)
    sq = torch.empty(129 * 257 + 64, dtype=torch.int32, device="cuda")
    near = torch.empty(129 * 257 + 64, dtype=torch.int32, device="cuda")
    first = _build(_cfg(63, 65, 0.8), a, sq=sq, near=near)
    _check(first, ref_a, "A")
    _check(_build(_cfg(129, 257, 0.5), b, sq=sq, near=near), ref_b, "B")
    again = _build(_cfg(63, 65, 0.8), a, sq=sq, near=near)
    _check(again, ref_a, "A again")
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    _check(_build(_cfg(63, 65, 0.8), np.zeros_like(a), sq=sq, near=near), (np.full(a.shape, -1), np.full(a.shape, -1)), "empty")
    capi.release_collision_caches()
    _check(_build(_cfg(63, 65, 0.8), a, sq=sq, near=near), ref_a, "A after the release")


# ---- the queries -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scenes():
    """per parameter set: the 90 x 70 scene, its field by the separable restatement and the restated answers of the 3000 poses,
    computed once"""
    out = {}
    for res, coll, _ in cr.SETS:
        g, data, poses, xmin, ymin = cr.scene(res, coll)
        sq, near = dr.separable(data, coll[3])
        out[(res, coll)] = (g, data, poses, xmin, ymin, sq, near, dr.query(res, coll, g, sq, near, poses))
    return out


def _device_field(cfg, data):
    ys, xs = data.shape
    sq = torch.full((ys, xs), FILL, dtype=torch.int32, device="cuda")
    near = torch.full((ys, xs), FILL, dtype=torch.int32, device="cuda")
    capi.distance_field(cfg, torch.as_tensor(data).cuda(), sq, near)
    return sq, near


def _query(cfg, sq, near, poses):
    P = len(poses)
    d_pose = torch.as_tensor(np.ascontiguousarray(poses)).cuda()
    out = torch.full((P, 4), FILL, dtype=torch.int32, device="cuda")
    dmin = torch.full((P,), float(FILL), dtype=torch.float64, device="cuda")
    disp = torch.full((P, 2), float(FILL), dtype=torch.float64, device="cuda")
    capi.distance_query_batch(cfg, sq, near, d_pose, out, dmin, disp)
    torch.cuda.synchronize()
    return out.cpu().numpy(), dmin.cpu().numpy(), disp.cpu().numpy()


@pytest.mark.parametrize("res,coll,n_off", cr.SETS)
def test_query_is_the_restatement(scenes, res, coll, n_off):
    """msg, sqrd_obs, dx, dy of 3000 poses up to 30 cells outside the 90 x 70 map (first the corners, just outside the lower
    edge, 1e9, NaN) exactly; dmin and disp bitwise numpy's sqrt(sq) * res - boundary_radius and res * (dx, dy); every class
    occurs (none: on an empty field); each output alone"""
    g, data, poses, xmin, ymin, ref_sq, ref_near, (ref, ref_dmin, ref_disp) = scenes[(res, coll)]
    cfg = capi.make_collision_cfg(xmin, ymin, res, 90, 70, *coll)
    sq, near = _device_field(cfg, data)
    out, dmin, disp = _query(cfg, sq, near, poses)
    _check((sq.cpu().numpy(), near.cpu().numpy()), (ref_sq, ref_near))
    bad = np.nonzero((out != ref).any(1))[0]
    assert len(bad) == 0, (bad[:10], out[bad[:10]], ref[bad[:10]], poses[bad[:10]])
    assert _same_bits(dmin, ref_dmin), np.nonzero(dmin != ref_dmin)[0][:10]
    assert _same_bits(disp, ref_disp), np.nonzero(disp != ref_disp)[0][:10]
    counts = [int((ref[:, 0] == m).sum()) for m in (dr.CRASH, dr.OBSTACLE, dr.NONE, dr.OFF_GRID)]
    print("crash / obstacle / none / off grid:", counts)
    assert counts[0] > 0 and counts[1] > 0 and counts[2] == 0 and counts[3] > 0      # (a field with a cell never says none)
    assert (ref_dmin[ref[:, 0] == dr.CRASH] < 0).any() or coll[0] == 0.0             # negative inside the bounding radius
    # each output alone; dmin alone needs no d_nearest
    P = len(poses)
    d_pose = torch.as_tensor(poses).cuda()
    o1 = torch.full((P, 4), FILL, dtype=torch.int32, device="cuda")
    o2 = torch.full((P,), float(FILL), dtype=torch.float64, device="cuda")
    o3 = torch.full((P, 2), float(FILL), dtype=torch.float64, device="cuda")
    capi.distance_query_batch(cfg, sq, near, d_pose, o1)
    capi.distance_query_batch(cfg, sq, None, d_pose, None, o2)
    capi.distance_query_batch(cfg, sq, near, d_pose, None, None, o3)
    torch.cuda.synchronize()
    assert np.array_equal(o1.cpu().numpy(), ref) and _same_bits(o2.cpu().numpy(), ref_dmin) and _same_bits(o3.cpu().numpy(), ref_disp)
    # an empty field: none on the grid, off the grid as before
    empty = np.zeros_like(data)
    esq, enear = _device_field(cfg, empty)
    out, dmin, disp = _query(cfg, esq, enear, poses)
    minus = np.full(data.shape, -1, dtype=np.int32)
    eref, eref_dmin, eref_disp = dr.query(res, coll, g, minus, minus, poses)
    assert np.array_equal(out, eref) and _same_bits(dmin, eref_dmin) and _same_bits(disp, eref_disp)
    assert (eref[:, 0] == dr.NONE).sum() == counts[0] + counts[1] and (eref_dmin[eref[:, 0] == dr.NONE] == dr.DBL_MAX).all()


@pytest.mark.parametrize("res,coll,n_off", cr.SETS)
def test_a_crash_of_the_ring_search_is_a_crash_of_the_field(scenes, res, coll, n_off):
    """eea_clearance_batch (the device's reference-exact call) says crash on an on-grid pose => the query says crash"""
    g, data, poses, xmin, ymin, _, _, (ref, _, _) = scenes[(res, coll)]
    cfg = capi.make_collision_cfg(xmin, ymin, res, 90, 70, *coll)
    d_grid = torch.as_tensor(data).cuda()
    ring = torch.full((len(poses), 4), FILL, dtype=torch.int32, device="cuda")
    capi.clearance_batch(cfg, d_grid, torch.as_tensor(poses).cuda(), ring)
    sq, near = _device_field(cfg, data)
    out, _, _ = _query(cfg, sq, near, poses)
    ring = ring.cpu().numpy()
    on = out[:, 0] != dr.OFF_GRID
    crash = on & (ring[:, 0] == cr.CRASH)
    assert crash.sum() > 0 and (out[crash, 0] == dr.CRASH).all()
    assert ((out[:, 0] == dr.CRASH) & ~crash).sum() > 0          # and the field sees crashes the rings miss


@pytest.mark.parametrize("T", [1, 63, 64, 65, 200])
def test_worst_step_is_the_restatement(scenes, T):
    """37 random walks that start on the 90 x 70 map and partly leave it; trajectory 0 is off the grid at step 0, trajectory 1
    has two equal minima (the earlier step wins); then the same through an empty field"""
    res, coll, _ = cr.SETS[2]
    g, data, _, xmin, ymin, ref_sq, ref_near, _ = scenes[(res, coll)]
    cfg = capi.make_collision_cfg(xmin, ymin, res, 90, 70, *coll)
    B = 37
    rng = np.random.default_rng(T)
    traj = np.zeros((B, T, 3))
    start = np.stack([rng.uniform(xmin + res, xmin + 89 * res, B), rng.uniform(ymin + res, ymin + 69 * res, B)], 1)
    traj[:, :, :2] = start[:, None, :] + np.cumsum(rng.normal(0.0, 2.5 * res, (B, T, 2)), axis=1) - rng.normal(0.0, 2.5 * res, (B, 1, 2))
    traj[:, 0, :2] = start
    traj[0, 0, :2] = (xmin - 3 * res, ymin + 5 * res)
    far = np.unravel_index(np.argmax(ref_sq), ref_sq.shape)                    # the cell furthest from every occupied cell
    near_cell = np.argwhere(ref_sq == 1)[0]
    traj[1, :, :2] = (xmin + (far[1] + 0.5) * res, ymin + (far[0] + 0.5) * res)
    if T > 9:
        traj[1, 5, :2] = traj[1, 9, :2] = (xmin + (near_cell[1] + 0.5) * res, ymin + (near_cell[0] + 0.5) * res)
    ref, ref_step, ref_dmin = dr.worst_step(res, coll, g, ref_sq, ref_near, traj)
    assert ref_step[0] == 0 and ref[0, 0] == dr.OFF_GRID and ref_step[1] == (5 if T > 9 else 0)
    assert T < 64 or ((ref[:, 0] == dr.OFF_GRID).sum() > 1 and (ref[:, 0] != dr.OFF_GRID).sum() > 1)

    sq, near = _device_field(cfg, data)
    d_traj = torch.as_tensor(traj).cuda()

    def run(sq, near, with_out=True, with_step=True, with_dmin=True):
        out = torch.full((B, 4), FILL, dtype=torch.int32, device="cuda")
        step = torch.full((B,), FILL, dtype=torch.int32, device="cuda")
        dmin = torch.full((B,), float(FILL), dtype=torch.float64, device="cuda")
        capi.distance_traj_min(cfg, sq, near, d_traj, out if with_out else None, step if with_step else None, dmin if with_dmin else None)
        torch.cuda.synchronize()
        return out.cpu().numpy(), step.cpu().numpy(), dmin.cpu().numpy()

    out, step, dmin = run(sq, near)
    assert np.array_equal(step, ref_step), (np.nonzero(step != ref_step)[0], step, ref_step)
    assert np.array_equal(out, ref) and _same_bits(dmin, ref_dmin)
    # each output alone (the step and dmin need no d_nearest)
    o, s, d = run(sq, near, with_step=False, with_dmin=False)
    assert np.array_equal(o, ref) and (s == FILL).all() and (d == FILL).all()
    o, s, d = run(sq, None, with_out=False, with_dmin=False)
    assert np.array_equal(s, ref_step) and (o == FILL).all()
    o, s, d = run(sq, None, with_out=False, with_step=False)
    assert _same_bits(d, ref_dmin)
    # an empty field: none at step 0 unless a step is off the grid
    minus = np.full(data.shape, -1, dtype=np.int32)
    eref, eref_step, eref_dmin = dr.worst_step(res, coll, g, minus, minus, traj)
    esq, enear = _device_field(cfg, np.zeros_like(data))
    out, step, dmin = run(esq, enear)
    assert np.array_equal(step, eref_step) and np.array_equal(out, eref) and _same_bits(dmin, eref_dmin)
    assert tuple(eref[1]) == (dr.NONE, -1, 0, 0) and eref_step[1] == 0 and eref_dmin[1] == dr.DBL_MAX


# ---- the host mirror --------------------------------------------------------------------------------------------------------

def test_host_mirror_prints_the_restatements_answers():
    """host/build/distance_field_tests (DistanceField in distance_field.hpp: update on three maps in turn, query, worstStep) runs
    once; the planes, the answers of the poses and the worst steps it prints against the restatement on the same grid"""
    exe = os.path.join(ROOT, "ergodic_exploration_amd", "host", "build", "distance_field_tests")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    W, H = int(lines[0].split()[1]), int(lines[0].split()[2])
    res, ox, oy = (float(v) for v in lines[0].split()[3:6])
    assert (W, H, res, ox, oy) == (50, 40, 0.1, -1.0, -2.0)
    data = np.zeros((H, W), dtype=np.int8)
    data[10:14, 20:26] = 100
    data[30, 5], data[31, 7], data[25, 40], data[3, 44], data[38, 30] = 80, 79, 100, 100, 100
    data[5:8, 2] = -1
    coll = (0.3, 1.2, 0.1, 0.8)
    g = po.GridMap(ox, ox + W * res, oy, oy + H * res, res, data.reshape(-1))
    sq, near = dr.brute_force(data, coll[3])
    got_sq = np.array([[int(v) for v in l.split()[2:]] for l in lines if l.startswith("field ")], dtype=np.int32)
    got_near = np.array([[int(v) for v in l.split()[2:]] for l in lines if l.startswith("near ")], dtype=np.int32)
    assert got_sq.shape == (H, W) and got_near.shape == (H, W)
    _check((got_sq, got_near), (sq, near))
    batch = [l.split() for l in lines if l.startswith("batch ")]
    worst = [l.split() for l in lines if l.startswith("worst ")]
    assert len(batch) == 154 and len(worst) == 6
    poses = np.array([[float(b[2]), float(b[3]), 0.0] for b in batch])
    ref, ref_dmin, ref_disp = dr.query(res, coll, g, sq, near, poses)
    got = np.array([[int(v) for v in b[4:8]] for b in batch], dtype=np.int32)
    assert np.array_equal(got, ref), np.nonzero((got != ref).any(1))[0][:10]
    assert _same_bits(np.array([float(b[8]) for b in batch]), ref_dmin)          # (printed with 17 significant digits)
    assert _same_bits(np.array([[float(b[9]), float(b[10])] for b in batch]), ref_disp)
    assert all((ref[:, 0] == m).any() for m in (dr.CRASH, dr.OBSTACLE, dr.OFF_GRID))
    for w in worst:
        b, T = int(w[1]), int(w[2])
        wref, wstep, wdmin = dr.worst_step(res, coll, g, sq, near, poses[None, b:b + T])
        assert [int(v) for v in w[3:7]] == wref[0].tolist() and int(w[7]) == wstep[0], w
        assert _same_bits(np.array([float(w[8])]), wdmin), w
    assert len({int(w[3]) for w in worst}) > 1

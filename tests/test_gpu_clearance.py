"""Clearance queries on the device (eea_clearance_batch / eea_clearance_field = Collision::minDistance / minDirection,
reference collision.cpp:65-124) bit for bit against the oracle's search: the state it leaves behind (hit, sqrd_obs, dx, dy)
determines both reference functions.  Both forms of the lookup -- one wavefront per pose, and the key map -- run every case;
the numpy restatement of tests/clearance_restatement.py (checked against the oracle in tests/test_clearance.py) is the second
opinion."""
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pyoracle as po
from ergodic_exploration_amd import capi
from tests import clearance_restatement as cr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING, MAP = 1, 2


class forced:
    """EEA_OPT_COLLISION_IMPL pinned to one form for the block, then back to what it was"""

    def __init__(self, impl):
        self.impl = impl

    def __enter__(self):
        self.before = capi.get_option(capi.OPT_COLLISION_IMPL)
        capi.set_option(capi.OPT_COLLISION_IMPL, self.impl)

    def __exit__(self, *exc):
        capi.set_option(capi.OPT_COLLISION_IMPL, self.before)


def _batch(cfg, d_grid, poses, impl=None):
    """(out [P][4] int32, dmin [P], disp [P][2]) of eea_clearance_batch, the buffers pre-filled with a value no answer has"""
    P = len(poses)
    d_pose = torch.as_tensor(np.ascontiguousarray(poses)).cuda()
    out = torch.full((P, 4), -77, dtype=torch.int32, device="cuda")
    dmin = torch.full((P,), -77.0, dtype=torch.float64, device="cuda")
    disp = torch.full((P, 2), -77.0, dtype=torch.float64, device="cuda")
    if impl is None:
        capi.clearance_batch(cfg, d_grid, d_pose, out, dmin, disp)
    else:
        with forced(impl):
            capi.clearance_batch(cfg, d_grid, d_pose, out, dmin, disp)
    torch.cuda.synchronize()
    return out.cpu().numpy(), dmin.cpu().numpy(), disp.cpu().numpy()


def _field(cfg, d_grid, xs, ys, impl=None):
    field = torch.full((ys, xs, 4), -77, dtype=torch.int32, device="cuda")
    dmin = torch.full((ys, xs), -77.0, dtype=torch.float64, device="cuda")
    if impl is None:
        capi.clearance_field(cfg, d_grid, field, dmin)
    else:
        with forced(impl):
            capi.clearance_field(cfg, d_grid, field, dmin)
    torch.cuda.synchronize()
    return field.cpu().numpy().reshape(-1, 4), dmin.cpu().numpy().reshape(-1)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.fixture(scope="module")
def references():
    """per parameter set: the scene and the oracle's answers, computed once"""
    refs = {}
    for res, coll, _ in cr.SETS:
        g, data, poses, xmin, ymin = cr.scene(res, coll)
        refs[(res, coll)] = (g, data, poses, xmin, ymin, cr.oracle(coll, g, poses))
    return refs


@pytest.mark.parametrize("impl", [RING, MAP])
@pytest.mark.parametrize("res,coll,n_off", cr.SETS)
def test_batch_is_the_oracles_search(references, res, coll, n_off, impl):
    """msg (crash iff the oracle's hit, none iff sqrd_obs == -1), sqrd_obs, dx, dy of 3000 poses up to 30 cells outside the
    90 x 70 map (the corners, just outside the lower edge, 1e9, NaN among them) bit for bit; dmin and disp bitwise the numpy
    expressions sqrt((double)sqrd_obs) * resolution - boundary_radius and resolution * (dx, dy)"""
    g, data, poses, xmin, ymin, ref = references[(res, coll)]
    cfg = capi.make_collision_cfg(xmin, ymin, res, 90, 70, *coll)
    out, dmin, disp = _batch(cfg, torch.as_tensor(data).cuda(), poses, impl)
    bad = np.nonzero((out != ref).any(1))[0]
    assert len(bad) == 0, (bad[:10], out[bad[:10]], ref[bad[:10]], poses[bad[:10]])
    assert np.array_equal(cr.restate(res, coll, g, data, poses), ref)
    ref_dmin, ref_disp = cr.doubles(res, coll, ref)
    assert _same_bits(dmin, ref_dmin), np.nonzero(dmin != ref_dmin)[0][:10]
    assert _same_bits(disp, ref_disp), np.nonzero(disp != ref_disp)[0][:10]
    counts = [int((ref[:, 0] == m).sum()) for m in (cr.CRASH, cr.OBSTACLE, cr.NONE)]
    if coll == (0.4, 0.4, 0.5, 0.8):      # r_col beyond r_max: the obstacle class is empty by construction
        assert counts[0] > 0 and counts[1] == 0 and counts[2] > 0
    else:
        assert min(counts) > 0, counts


def test_outputs_are_optional_one_by_one_and_the_cost_model_answers_the_same(references):
    """each of the three outputs alone, with the dispatch left to the cost model, at a small and at a large P"""
    res, coll, _ = cr.SETS[5]
    g, data, poses, xmin, ymin, ref = references[(res, coll)]
    cfg = capi.make_collision_cfg(xmin, ymin, res, 90, 70, *coll)
    d_grid = torch.as_tensor(data).cuda()
    ref_dmin, ref_disp = cr.doubles(res, coll, ref)
    for P in (37, 3000):
        d_pose = torch.as_tensor(poses[:P]).cuda()
        out = torch.full((P, 4), -77, dtype=torch.int32, device="cuda")
        dmin = torch.full((P,), -77.0, dtype=torch.float64, device="cuda")
        disp = torch.full((P, 2), -77.0, dtype=torch.float64, device="cuda")
        capi.clearance_batch(cfg, d_grid, d_pose, out)
        capi.clearance_batch(cfg, d_grid, d_pose, None, dmin)
        capi.clearance_batch(cfg, d_grid, d_pose, None, None, disp)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), ref[:P])
        assert _same_bits(dmin.cpu().numpy(), ref_dmin[:P]) and _same_bits(disp.cpu().numpy(), ref_disp[:P])
    assert capi.get_option(capi.OPT_COLLISION_IMPL) == 0


@pytest.mark.parametrize("impl", [RING, MAP])
@pytest.mark.parametrize("coll", cr.FACT_COLLS)
def test_hand_made_scenes(coll, impl):
    """ties (Q1 of a ring's first step wins; the axis cells of ring 5 come before its (3, 4)), the gap cell (6, 6), a cell
    inside r_bnd, a crash: exactly the expected values, in both forms"""
    cfg = capi.make_collision_cfg(cr.XMIN41, cr.YMIN41, cr.RES41, cr.N41, cr.N41, *coll)
    for cells, expect in cr.FACTS:
        g, data, pose = cr.fact_scene(cells)
        out, dmin, disp = _batch(cfg, torch.as_tensor(data).cuda(), pose, impl)
        assert tuple(out[0]) == expect, (cells, expect, out[0])
        ref_dmin, ref_disp = cr.doubles(cr.RES41, coll, np.array([expect], dtype=np.int32))
        assert _same_bits(dmin, ref_dmin) and _same_bits(disp, ref_disp), (cells, dmin, disp)


def _scene41(seed):
    rng = np.random.default_rng(seed)
    data = np.zeros((cr.N41, cr.N41), dtype=np.int8)
    data[rng.integers(0, cr.N41, 14), rng.integers(0, cr.N41, 14)] = 100
    data[30:33, 5:9] = 90
    g = po.GridMap(cr.XMIN41, cr.XMIN41 + cr.N41 * cr.RES41, cr.YMIN41, cr.YMIN41 + cr.N41 * cr.RES41, cr.RES41, data.reshape(-1))
    return g, data


@pytest.mark.parametrize("impl", [RING, MAP])
def test_field_is_the_batch_at_the_cell_centres_and_the_oracle(references, impl):
    """eea_clearance_field on a 41 x 41 and on the 90 x 70 scene = eea_clearance_batch at the world centres of all cells, and
    = the oracle on every cell of the 41 x 41 one"""
    coll = cr.FACT_COLLS[0]
    g, data = _scene41(41)
    cfg = capi.make_collision_cfg(cr.XMIN41, cr.YMIN41, cr.RES41, cr.N41, cr.N41, *coll)
    d_grid = torch.as_tensor(data).cuda()
    poses = cr.cell_centres(g, cr.N41, cr.N41)
    field, fmin = _field(cfg, d_grid, cr.N41, cr.N41, impl)
    out, dmin, _ = _batch(cfg, d_grid, poses, impl)
    ref = cr.oracle(coll, g, poses)
    assert np.array_equal(field, ref), np.nonzero((field != ref).any(1))[0][:10]
    assert np.array_equal(out, ref) and _same_bits(fmin, dmin) and _same_bits(fmin, cr.doubles(cr.RES41, coll, ref)[0])
    assert all((ref[:, 0] == m).any() for m in (cr.CRASH, cr.OBSTACLE, cr.NONE))
    # each output alone
    only = torch.full((cr.N41, cr.N41), -77.0, dtype=torch.float64, device="cuda")
    with forced(impl):
        capi.clearance_field(cfg, d_grid, None, only)
    torch.cuda.synchronize()
    assert _same_bits(only.cpu().numpy().reshape(-1), fmin)

    res, coll, _ = cr.SETS[2]
    g, data, _, xmin, ymin, _ = references[(res, coll)]
    cfg = capi.make_collision_cfg(xmin, ymin, res, 90, 70, *coll)
    d_grid = torch.as_tensor(data).cuda()
    poses = cr.cell_centres(g, 90, 70)
    field, fmin = _field(cfg, d_grid, 90, 70, impl)
    out, dmin, _ = _batch(cfg, d_grid, poses, impl)
    assert np.array_equal(field, out) and _same_bits(fmin, dmin)
    assert np.array_equal(field, cr.restate(res, coll, g, data, poses))
    assert all((field[:, 0] == m).any() for m in (cr.CRASH, cr.OBSTACLE, cr.NONE))


def test_field_cache_holds_no_stale_keys():
    """a second field call on another grid content on the same stream is right -- the first scene's keys are gone --, and so is
    one after eea_release_collision_caches; a smaller and a larger map in between reuse / regrow the buffer"""
    coll = cr.FACT_COLLS[0]
    cfg = capi.make_collision_cfg(cr.XMIN41, cr.YMIN41, cr.RES41, cr.N41, cr.N41, *coll)
    d_buf = torch.zeros((cr.N41, cr.N41), dtype=torch.int8, device="cuda")      # one device grid whose content changes
    answers = {}
    for seed in (1, 2):
        g, data = _scene41(seed)
        answers[seed] = cr.oracle(coll, g, cr.cell_centres(g, cr.N41, cr.N41))
        d_buf.copy_(torch.as_tensor(data))
        field, _ = _field(cfg, d_buf, cr.N41, cr.N41, MAP)
        assert np.array_equal(field, answers[seed]), seed
    assert not np.array_equal(answers[1], answers[2])
    # an empty grid after a full one: nothing may be left
    d_buf.zero_()
    field, fmin = _field(cfg, d_buf, cr.N41, cr.N41, MAP)
    assert (field == np.array([cr.NONE, -1, 0, 0])).all() and (fmin == cr.DBL_MAX).all()
    # a smaller map (another row pitch in the same buffer), then the first again
    small = capi.make_collision_cfg(cr.XMIN41, cr.YMIN41, cr.RES41, 17, 13, *coll)
    sdata = np.zeros((13, 17), dtype=np.int8)
    sdata[6, 8] = 100
    sg = po.GridMap(cr.XMIN41, cr.XMIN41 + 17 * cr.RES41, cr.YMIN41, cr.YMIN41 + 13 * cr.RES41, cr.RES41, sdata.reshape(-1))
    field, _ = _field(small, torch.as_tensor(sdata).cuda(), 17, 13, MAP)
    assert np.array_equal(field, cr.oracle(coll, sg, cr.cell_centres(sg, 17, 13)))
    g, data = _scene41(1)
    d_buf.copy_(torch.as_tensor(data))
    for impl in (MAP, None):
        field, _ = _field(cfg, d_buf, cr.N41, cr.N41, impl)
        assert np.array_equal(field, answers[1])
    capi.release_collision_caches()
    for impl in (MAP, None, RING):
        field, _ = _field(cfg, d_buf, cr.N41, cr.N41, impl)
        assert np.array_equal(field, answers[1])
    out, _, _ = _batch(cfg, d_buf, cr.cell_centres(g, cr.N41, cr.N41), MAP)
    assert np.array_equal(out, answers[1])


def test_host_mirror_prints_the_oracles_answers():
    """host/build/clearance_tests (Collision::minDistance / minDirection and their batched form in collision.hpp) runs once; its
    printed answers against the oracle on the same grid and the poses it prints"""
    exe = os.path.join(ROOT, "ergodic_exploration_amd", "host", "build", "clearance_tests")
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
    batch = [l.split() for l in lines if l.startswith("batch ")]
    single = [l.split() for l in lines if l.startswith("single ")]
    assert len(batch) == 154 and len(single) == 18
    poses = np.array([[float(b[2]), float(b[3]), 0.0] for b in batch])
    ref = cr.oracle(coll, g, poses)
    ref_dmin, ref_disp = cr.doubles(res, coll, ref)
    got = np.array([[int(v) for v in b[4:8]] for b in batch], dtype=np.int32)
    assert np.array_equal(got, ref), np.nonzero((got != ref).any(1))[0][:10]
    assert _same_bits(np.array([float(b[8]) for b in batch]), ref_dmin)          # (printed with 17 significant digits)
    assert _same_bits(np.array([[float(b[9]), float(b[10])] for b in batch]), ref_disp)
    assert all((ref[:, 0] == m).any() for m in (cr.CRASH, cr.OBSTACLE, cr.NONE))
    for s in single:
        q = int(s[1])
        assert int(s[2]) == ref[q, 0] == int(s[4]), s
        assert _same_bits(np.array([float(s[3])]), ref_dmin[q:q + 1]) and _same_bits(np.array([float(s[5]), float(s[6])]), ref_disp[q]), s

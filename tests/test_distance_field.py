"""The distance field (eea_distance_field / eea_distance_query_batch / eea_distance_traj_min: csrc/distance_kernel.hip) without a
GPU: the entry points, the argument errors that come before the device is selected, the two numpy restatements of
tests/distance_restatement.py against each other, and the relation of the exact field to the reference's ring search
(pyoracle.collision_check) -- the ring search never sees what the field misses, and misses part of what the field sees."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ergodic_exploration_amd import capi

from tests import clearance_restatement as cr
from tests import distance_restatement as dr

ENTRIES = {"eea_distance_field": 6, "eea_distance_query_batch": 10, "eea_distance_traj_min": 11}


def test_entries_are_declared_exported_and_bound():
    raw = C.CDLL(capi.LIB_PATH)
    L = capi.lib()
    for name, n_args in ENTRIES.items():
        assert name in capi.declared_symbols() and hasattr(raw, name), name
        assert len(getattr(L, name).argtypes) == n_args, name
    for name in ("distance_field", "distance_query_batch", "distance_traj_min"):
        assert callable(getattr(capi, name)), name
    assert capi.COLLISION_OFF_GRID == 3 and capi.DISTANCE_MAX_SIDE == 8192
    assert L.eea_abi_version() == 6


def test_header_states_the_limit_and_the_enumerator(tmp_path):
    src = tmp_path / "limit.c"
    src.write_text('#include <stdio.h>\n#include "ergodic_amd.h"\nint main(void) {\n'
                   'printf("%d %d\\n", EEA_DISTANCE_MAX_SIDE, EEA_COLLISION_OFF_GRID);\nreturn 0; }\n')
    exe = tmp_path / "limit"
    subprocess.run(["gcc", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert got == [str(capi.DISTANCE_MAX_SIDE), str(capi.COLLISION_OFF_GRID)]
    side = capi.DISTANCE_MAX_SIDE          # the limit keeps squared distances and cell indices inside int
    assert 2 * (side - 1) ** 2 < 2 ** 31 and side * side < 2 ** 31


def test_argument_errors_come_before_the_device():
    """null cfg / grid / field / poses, no output, outputs that need d_nearest without it, the configuration errors, an empty
    grid, T == 0 and a grid above the limit are answered without a device (the buffers are host arrays nothing may touch);
    P == 0 and B == 0 are EEA_OK"""
    L = capi.lib()
    xs, ys = 80, 60
    good = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 0.8)
    grid = np.zeros(xs * ys, dtype=np.int8)
    sq, near = np.full((ys, xs), 7, dtype=np.int32), np.full((ys, xs), 7, dtype=np.int32)
    pose, traj = np.zeros((4, 3)), np.zeros((4, 5, 3))
    out, dmin, disp, step = np.full((4, 4), 7, dtype=np.int32), np.full(4, 7.0), np.full((4, 2), 7.0), np.full(4, 7, dtype=np.int32)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def build(cfg, g=grid, s=sq, n=near):
        return L.eea_distance_field(0, None if cfg is None else C.byref(cfg), p(g), p(s), p(n), None)

    def query(cfg, s=sq, n=near, ps=pose, P=4, o=out, dm=dmin, ds=disp):
        return L.eea_distance_query_batch(0, None if cfg is None else C.byref(cfg), p(s), p(n), p(ps), P, p(o), p(dm), p(ds), None)

    def worst(cfg, s=sq, n=near, tr=traj, B=4, T=5, o=out, st=step, dm=dmin):
        return L.eea_distance_traj_min(0, None if cfg is None else C.byref(cfg), p(s), p(n), p(tr), B, T, p(o), p(st), p(dm), None)

    INV, UNS = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED
    assert build(None) == INV and query(None) == INV and worst(None) == INV
    assert build(good, g=None) == INV and build(good, s=None) == INV
    assert query(good, s=None) == INV and query(good, ps=None) == INV
    assert worst(good, s=None) == INV and worst(good, tr=None) == INV
    assert query(good, o=None, dm=None, ds=None) == INV and b"output" in L.eea_last_error()
    assert worst(good, o=None, st=None, dm=None) == INV and b"output" in L.eea_last_error()
    assert query(good, n=None) == INV and query(good, n=None, o=None) == INV and b"d_nearest" in L.eea_last_error()
    assert worst(good, n=None) == INV and b"d_nearest" in L.eea_last_error()
    assert worst(good, T=0) == INV
    swapped = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 1.0, 0.7, 0.2, 0.8)
    assert build(swapped) == INV and query(swapped) == INV and worst(swapped) == INV and b"Search radius" in L.eea_last_error()
    for bad in (capi.make_collision_cfg(-2.0, -1.0, 0.1, 0, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, 0, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.0, xs, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, -0.1, xs, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 100.5)):
        assert build(bad) == INV and query(bad) == INV and worst(bad) == INV
    for big in (capi.make_collision_cfg(-2.0, -1.0, 0.1, 1 << 20, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, capi.DISTANCE_MAX_SIDE + 1, 0.7, 1.0, 0.2, 0.8)):
        assert build(big) == UNS and query(big) == UNS and worst(big) == UNS and b"EEA_DISTANCE_MAX_SIDE" in L.eea_last_error()
    # accepted without a device: nothing to do
    assert query(good, P=0) == capi.OK and worst(good, B=0) == capi.OK
    assert query(good, n=None, o=None, ds=None, P=0) == capi.OK and worst(good, n=None, o=None, B=0) == capi.OK
    widest = capi.make_collision_cfg(-2.0, -1.0, 0.1, capi.DISTANCE_MAX_SIDE, capi.DISTANCE_MAX_SIDE, 0.7, 1.0, 0.2, 0.8)
    assert query(widest, P=0) == capi.OK
    assert (sq == 7).all() and (near == 7).all() and (out == 7).all() and (dmin == 7.0).all() and (disp == 7.0).all() and (step == 7).all()


@pytest.mark.parametrize("threshold", [0.8, 0.5])
@pytest.mark.parametrize("ys,xs", [(1, 1)] + dr.SHAPES)
def test_brute_force_is_the_separable_form(ys, xs, threshold):
    data = dr.random_grid(ys, xs, seed=ys * 1000 + xs)
    occ = dr.occupied(data, threshold)
    assert xs * ys == 1 or (occ.any() and not occ.all())
    sq, near = dr.brute_force(data, threshold)
    sq2, near2 = dr.separable(data, threshold)
    assert np.array_equal(sq, sq2) and np.array_equal(near, near2)
    assert (sq[occ] == 0).all() and (near.reshape(-1)[occ.reshape(-1)] == np.nonzero(occ.reshape(-1))[0]).all()
    # the occupancy test: 80 is occupied at 0.8 and 79 is not; 50 / 49 at 0.5; -1 and -128 never, 127 always
    assert np.array_equal(dr.occupied(dr.VALUES, threshold),
                          np.array([True, True, threshold == 0.5, threshold == 0.5, False, False, False, True]))


def test_restatements_on_empty_full_and_tied_grids():
    for form in (dr.brute_force, dr.separable):
        sq, near = form(np.zeros((5, 7), dtype=np.int8), 0.8)
        assert (sq == -1).all() and (near == -1).all()
        sq, near = form(np.full((5, 7), 100, dtype=np.int8), 0.8)
        assert (sq == 0).all() and np.array_equal(near.reshape(-1), np.arange(35))
        # the four axis cells at distance 5 with (3, 4) and (4, 3) around (20, 20): the smallest index is the cell above
        data = np.zeros((41, 41), dtype=np.int8)
        for dx, dy in [(5, 0), (-5, 0), (0, 5), (0, -5), (3, 4), (4, 3)]:
            data[20 + dy, 20 + dx] = 100
        sq, near = form(data, 0.8)
        assert sq[20, 20] == 25 and near[20, 20] == 15 * 41 + 20


# the relation of the exact field to the ring search on the 90 x 70 scene, per parameter set of cr.SETS: poses whose cell is on
# the grid; of those the oracle's crashes; those with an occupied cell within r_col by the field; the latter without the
# former ("field only"); oracle obstacles further away than the true nearest cell
TABLE = [(1017, 934, 1013, 79, 70), (1029, 249, 283, 34, 5), (995, 335, 376, 41, 18), (1052, 138, 163, 25, 34),
         (964, 268, 783, 515, 0), (997, 203, 237, 34, 83)]


@pytest.mark.parametrize("n", range(len(cr.SETS)))
def test_ring_search_never_sees_what_the_field_misses(n):
    res, coll, _ = cr.SETS[n]
    g, data, poses, _, _ = cr.scene(res, coll)
    ref = cr.oracle(coll, g, poses)
    sq, near = dr.separable(data, coll[3])
    out, _, _ = dr.query(res, coll, g, sq, near, poses)
    on = out[:, 0] != dr.OFF_GRID
    r_col = cr.radii(res, coll)[1]
    within = on & (out[:, 1] >= 0) & (out[:, 1] <= r_col * r_col)
    assert np.array_equal(within, out[:, 0] == dr.CRASH)
    crash = on & (ref[:, 0] == cr.CRASH)
    obst = on & (ref[:, 0] == cr.OBSTACLE)
    assert not (crash & ~within).any()                            # oracle crash => field sq <= r_col^2
    assert (out[obst, 1] >= 0).all() and (out[obst, 1] <= ref[obst, 1]).all()      # oracle obstacle => field sq <= the oracle's
    row = (int(on.sum()), int(crash.sum()), int(within.sum()), int((within & ~crash).sum()), int((out[obst, 1] < ref[obst, 1]).sum()))
    print("on grid / oracle crash / field within r_col / field only / oracle further than the nearest:", row)
    assert row[3] > 0                                             # the scene exercises the gaps at all
    assert row == TABLE[n]


def test_fact_scenes_the_ring_search_misses():
    """the lone cell at (6, 6) -- a gap of the rings -- and the cell at (1, 0) inside r_bnd: the oracle says none, the field
    obstacle at sq 72 and crash at sq 1"""
    for coll in cr.FACT_COLLS:
        for cells, msg, s, dx, dy in (([(6, 6)], dr.OBSTACLE, 72, 6, 6), ([(1, 0)], dr.CRASH, 1, 1, 0)):
            g, data, pose = cr.fact_scene(cells)
            assert tuple(cr.oracle(coll, g, pose)[0]) == (cr.NONE, -1, 0, 0)
            for form in (dr.brute_force, dr.separable):
                sq, near = form(data, coll[3])
                out, dmin, disp = dr.query(cr.RES41, coll, g, sq, near, pose)
                assert tuple(out[0]) == (msg, s, dx, dy), (cells, out[0])
                assert dmin[0] == np.sqrt(np.float64(s)) * cr.RES41 - coll[0] and tuple(disp[0]) == (cr.RES41 * dx, cr.RES41 * dy)


def test_worst_step_rules():
    g, data, pose = cr.fact_scene([(6, 6)])
    coll = cr.FACT_COLLS[0]
    sq, near = dr.brute_force(data, coll[3])
    c = lambda j, i: [cr.XMIN41 + (j + 0.5) * cr.RES41, cr.YMIN41 + (i + 0.5) * cr.RES41, 0.0]
    traj = np.array([[c(20, 20), c(24, 26), c(28, 26), c(3, 3)],          # two equal minima (sq 4): the earlier step
                     [c(20, 20), c(26, 26), c(-3, 5), c(50, 5)],          # off the grid beats the occupied cell itself
                     [c(-1, 0), c(26, 26), c(26, 26), c(26, 26)]])        # off the grid at step 0
    out, step, dmin = dr.worst_step(cr.RES41, coll, g, sq, near, traj)
    assert step.tolist() == [1, 2, 0]
    assert tuple(out[0]) == (dr.CRASH, 4, 2, 0) and out[1, 0] == out[2, 0] == dr.OFF_GRID and dmin[1] == 0.0
    empty = np.full_like(sq, -1)
    out, step, dmin = dr.worst_step(cr.RES41, coll, g, empty, empty, traj)
    assert step.tolist() == [0, 2, 0] and tuple(out[0]) == (dr.NONE, -1, 0, 0) and dmin[0] == dr.DBL_MAX

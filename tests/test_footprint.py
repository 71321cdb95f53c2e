"""Footprint collision (eea_footprint_radii / eea_footprint_check_batch / eea_footprint_traj_first: csrc/footprint_planes.hpp,
csrc/footprint_kernel.hip) without a GPU: the entry points and the struct, the host-only radii bit for bit, the argument errors
that come before the device is selected, the two numpy restatements of tests/footprint_restatement.py against each other on
the 24 combinations of six scenes and four footprints, and the sanitized check program of the host-only header."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from ergodic_exploration_amd import capi

from tests import clearance_restatement as cr
from tests import distance_restatement as dr
from tests import footprint_restatement as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"eea_footprint_radii": 3, "eea_footprint_check_batch": 9, "eea_footprint_traj_first": 10}
NAMES = list(fr.FOOTPRINTS)
COMBOS = [(n, name) for n in range(len(cr.SETS)) for name in NAMES]


def test_entries_are_declared_exported_and_bound():
    raw = C.CDLL(capi.LIB_PATH)
    L = capi.lib()
    for name, n_args in ENTRIES.items():
        assert name in capi.declared_symbols() and hasattr(raw, name), name
        assert len(getattr(L, name).argtypes) == n_args, name
    for name in ("Footprint", "footprint_radii", "footprint_check_batch", "footprint_traj_first"):
        assert callable(getattr(capi, name)), name
    assert capi.FOOTPRINT_MAX_VERTICES == fr.MAX_VERTICES == 16
    assert L.eea_abi_version() == 6


def test_struct_layout_matches_the_compiler(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ergodic_amd.h"\nint main(void) {\n'
                   'printf("%d %zu %zu %zu %zu\\n", EEA_FOOTPRINT_MAX_VERTICES, sizeof(eea_footprint), offsetof(eea_footprint, n),\n'
                   '       offsetof(eea_footprint, x), offsetof(eea_footprint, y));\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    F = capi.Footprint
    assert got == [capi.FOOTPRINT_MAX_VERTICES, C.sizeof(F), F.n.offset, F.x.offset, F.y.offset]


@pytest.mark.parametrize("name", NAMES)
def test_radii_are_the_restatements_bits(name):
    verts = fr.FOOTPRINTS[name]
    assert fr.valid(verts)
    r_in, r_out = capi.footprint_radii(capi.Footprint.of(verts))
    _, _, h, ref_in, ref_out = fr.planes(verts)
    assert np.float64(r_in).view(np.uint64) == np.float64(ref_in).view(np.uint64)
    assert np.float64(r_out).view(np.uint64) == np.float64(ref_out).view(np.uint64)
    assert 0.0 < r_in <= r_out and (h > 0).all()
    # either output alone
    L = capi.lib()
    one = C.c_double(7.0)
    assert L.eea_footprint_radii(C.byref(capi.Footprint.of(verts)), None, C.byref(one)) == capi.OK and one.value == r_out
    assert L.eea_footprint_radii(C.byref(capi.Footprint.of(verts)), C.byref(one), None) == capi.OK and one.value == r_in


BAD_FOOTPRINTS = {
    "clockwise": fr.FOOTPRINTS["rect"][::-1],
    "collinear vertex": [(0.45, -0.25), (0.45, 0.0), (0.45, 0.25), (-0.45, 0.25), (-0.45, -0.25)],
    "repeated vertex": [(0.45, -0.25), (0.45, 0.25), (0.45, 0.25), (-0.45, 0.25), (-0.45, -0.25)],
    "reflex vertex": [(0.45, -0.25), (0.1, 0.0), (0.45, 0.25), (-0.45, 0.25), (-0.45, -0.25)],
    "origin on an edge": [(0.9, -0.2), (0.9, 0.2), (0.0, 0.2), (0.0, -0.2)],
    "origin outside": [(0.9, -0.2), (0.9, 0.2), (0.1, 0.2), (0.1, -0.2)],
    "n = 2": [(0.5, 0.0), (-0.5, 0.0)],
    "n = 0": [],
    "n = 17": [(0.5 * np.cos(k * 2 * np.pi / 17), 0.5 * np.sin(k * 2 * np.pi / 17)) for k in range(17)],
    "NaN vertex": [(0.6, 0.0), (float("nan"), 0.35), (-0.3, -0.35)],
    "infinite vertex": [(0.6, 0.0), (-0.3, float("inf")), (-0.3, -0.35)],
}


def test_argument_errors_come_before_the_device():
    """every refusal of the header is answered without a device: the buffers are host arrays nothing may touch; P == 0 and
    B == 0 are EEA_OK"""
    L = capi.lib()
    xs, ys = 80, 60
    good = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 0.8)
    rect = capi.Footprint.of(fr.FOOTPRINTS["rect"])
    grid = np.zeros(xs * ys, dtype=np.int8)
    sq = np.full((ys, xs), 7, dtype=np.int32)
    pose, traj = np.zeros((4, 3)), np.zeros((4, 5, 3))
    hit, step = np.full(4, 7, dtype=np.int32), np.full(4, 7, dtype=np.int32)
    radii = [C.c_double(7.0), C.c_double(7.0)]
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    ref = lambda s: None if s is None else C.byref(s)

    def check(cfg=good, fp=rect, g=grid, s=sq, ps=pose, P=4, o=hit):
        return L.eea_footprint_check_batch(0, ref(cfg), ref(fp), p(g), p(s), p(ps), P, p(o), None)

    def first(cfg=good, fp=rect, g=grid, s=sq, tr=traj, B=4, T=5, o=step):
        return L.eea_footprint_traj_first(0, ref(cfg), ref(fp), p(g), p(s), p(tr), B, T, p(o), None)

    def radii_of(fp):
        return L.eea_footprint_radii(ref(fp), C.byref(radii[0]), C.byref(radii[1]))

    INV, UNS = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED
    # required pointers (d_sq is not one)
    assert radii_of(None) == INV
    assert check(cfg=None) == INV and check(fp=None) == INV and check(g=None) == INV and check(ps=None) == INV and check(o=None) == INV
    assert first(cfg=None) == INV and first(fp=None) == INV and first(g=None) == INV and first(tr=None) == INV and first(o=None) == INV
    # the footprint's own refusals, with the reason
    for what, verts in BAD_FOOTPRINTS.items():
        assert not fr.valid(verts), what
        fp = capi.Footprint.of(verts)
        assert radii_of(fp) == INV and check(fp=fp) == INV and first(fp=fp) == INV, what
        assert b"footprint" in L.eea_last_error(), what
    huge = capi.Footprint.of(fr.FOOTPRINTS["tri"])
    huge.n = 0xffffffff
    assert radii_of(huge) == INV and check(fp=huge) == INV
    # the grid's refusals; the radii and the threshold are neither read nor checked
    for bad in (capi.make_collision_cfg(-2.0, -1.0, 0.1, 0, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, 0, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.0, xs, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, -0.1, xs, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, float("nan"), xs, ys, 0.7, 1.0, 0.2, 0.8)):
        assert check(cfg=bad) == INV and first(cfg=bad) == INV
    assert first(T=0) == INV and first(T=1 << 31) == INV and first(T=0, B=0) == INV
    for big in (capi.make_collision_cfg(-2.0, -1.0, 0.1, 1 << 16, (1 << 15) + 1, 0.7, 1.0, 0.2, 0.8),):
        assert check(cfg=big) == UNS and first(cfg=big) == UNS and b"2^31" in L.eea_last_error()
    r_out = capi.footprint_radii(rect)[1]
    fine = capi.make_collision_cfg(-2.0, -1.0, r_out / 1024.5, xs, ys, 0.7, 1.0, 0.2, 0.8)
    assert check(cfg=fine) == UNS and first(cfg=fine) == UNS and b"1024" in L.eea_last_error()
    # accepted without a device: nothing to do
    swapped = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 1.0, 0.7, 0.2, 100.5)
    assert check(P=0) == capi.OK and first(B=0) == capi.OK and check(s=None, P=0) == capi.OK and first(s=None, B=0) == capi.OK
    assert check(cfg=swapped, P=0) == capi.OK and first(cfg=swapped, B=0, T=(1 << 31) - 1) == capi.OK
    limit = capi.make_collision_cfg(-2.0, -1.0, r_out / 1024.0, 1 << 16, 1 << 15, 0.7, 1.0, 0.2, 0.8)
    assert check(cfg=limit, P=0) == capi.OK
    assert (hit == 7).all() and (step == 7).all() and (sq == 7).all() and [r.value for r in radii] == [7.0, 7.0]


# per combination (parameter set of cr.SETS x footprint, in COMBOS' order) the restatement's exact class counts: hits; hits of
# poses without a cell; ambiguous poses with a cell; poses without a cell that take the exact test; sure hits; surely free
TABLE = [(947, 261, 565, 683, 344, 82), (833, 236, 685, 749, 256, 50), (1118, 316, 173, 631, 700, 118), (944, 279, 902, 1226, 89, 0),
         (153, 34, 229, 222, 42, 734), (133, 28, 328, 222, 42, 635), (189, 44, 167, 163, 104, 734), (145, 31, 477, 264, 0, 528),
         (424, 98, 486, 365, 92, 388), (361, 83, 569, 365, 92, 305), (550, 124, 317, 316, 261, 388), (413, 96, 822, 582, 42, 102),
         (390, 92, 441, 349, 84, 494), (311, 76, 545, 349, 84, 390), (500, 107, 292, 302, 233, 494), (391, 99, 806, 589, 42, 171),
         (426, 93, 486, 371, 80, 374), (362, 82, 560, 371, 80, 300), (531, 116, 315, 322, 251, 374), (402, 97, 779, 636, 29, 132),
         (405, 110, 456, 388, 69, 445), (349, 98, 528, 388, 69, 373), (523, 132, 299, 329, 226, 445), (390, 110, 745, 631, 25, 200)]


@pytest.fixture(scope="module")
def scenes():
    return {n: fr.scene(res, coll) for n, (res, coll, _) in enumerate(cr.SETS)}


@pytest.mark.parametrize("n,name", COMBOS)
def test_filter_never_contradicts_the_definition(scenes, n, name):
    """filtered == brute over all 3000 poses (no exclusion: both use numpy's sin / cos); the class counts are the table's; at
    most 0.5 % of the poses are undecided (margin below 1e-9 m) -- here none is, the smallest margin is 3.8e-6 m"""
    res, coll, _ = cr.SETS[n]
    data, poses, xmin, ymin = scenes[n]
    verts = fr.FOOTPRINTS[name]
    hit, margin = fr.brute(res, xmin, ymin, data, coll[3], verts, poses)
    fhit, cls = fr.filtered(res, xmin, ymin, data, coll[3], verts, poses)
    bad = np.nonzero(hit != fhit)[0]
    assert len(bad) == 0, (bad[:10], cls[bad[:10]], poses[bad[:10]])
    has = fr.cells(res, xmin, ymin, 90, 70, poses)[0]
    row = (int(hit.sum()), int((hit & ~has).sum()), int((cls == fr.AMBIGUOUS).sum()), int((cls == fr.NO_CELL).sum()),
           int((cls == fr.HIT).sum()), int((cls == fr.FREE).sum()))
    undecided = int((margin < fr.DECIDED).sum())
    print("hits / of poses without a cell / ambiguous / without a cell, tested / sure hits / surely free:", row,
          "undecided:", undecided, "smallest margin: %.3g m" % margin.min())
    assert undecided <= 0.005 * len(poses)
    assert margin.min() >= 3.7e-6
    pl = fr.planes(verts)
    sq_hit = fr.thresholds(pl[3], pl[4], res)[0]
    assert (row[4] > 0) == (sq_hit >= 0) and (row[5] > 0) == (not (name == "offc" and res == 0.05))
    assert 125 <= row[0] <= 1118 and 28 <= row[1] <= 316 and 167 <= row[2] <= 902
    assert row == TABLE[COMBOS.index((n, name))]
    assert (has == np.isin(cls, (fr.FREE, fr.HIT, fr.AMBIGUOUS))).all()


@pytest.mark.parametrize("n", range(len(cr.SETS)))
def test_poses_the_grid_lookup_would_misplace_have_no_cell(scenes, n):
    """world2Grid (grid.cpp:143-159) is not where a pose's cell comes from.  Its == size step takes the column fx == xsize into
    the last column and the row fy == ysize into the last row: every scene holds finite poses of both kinds, and they are ALL
    the scene's poses that the lookup places on the grid without a cell (23 - 32 per scene; none of the scene's own poses is
    folded by the x86 wrap -- its 1e9 m poses wrap to cells far off the grid).  Poses the wrap does fold are added here
    (footprint_restatement.wrap_poses: 2^32 cells away, folded on to an occupied cell of the wall in row 0).  Both kinds are
    without a cell, and none of them is decided by the field"""
    res, coll, _ = cr.SETS[n]
    data, poses, xmin, ymin = scenes[n]
    g = cr.scene(res, coll)[0]
    wrapped = fr.wrap_poses(res, xmin, ymin)
    poses = np.concatenate([poses, wrapped])
    W = np.arange(len(poses)) >= len(poses) - len(wrapped)
    has, fx, fy = fr.cells(res, xmin, ymin, 90, 70, poses)
    cx, cy = cr.centres(g, poses)
    on_by_lookup = (cx >= 0) & (cx < 90) & (cy >= 0) & (cy < 70)
    finite = np.isfinite(poses).all(1)
    column = finite & ~W & (fx == 90) & (fy >= 0) & (fy <= 70)            # (fy == 70 with it: the corner)
    row = finite & ~W & (fy == 70) & (fx >= 0) & (fx <= 90)
    assert column.sum() > 0 and on_by_lookup[column].all() and (cx[column] == 89).all()
    assert row.sum() > 0 and on_by_lookup[row].all() and (cy[row] == 69).all()
    misplaced = finite & on_by_lookup & ~has
    print("poses the lookup places on the grid without a cell:", int(misplaced.sum()), "in the column fx == xsize:", int(column.sum()),
          "in the row fy == ysize:", int(row.sum()), "folded by the wrap (added):", int(W.sum()))
    assert np.array_equal(misplaced & ~W, column | row)  # the scene itself: the == size steps of both axes and nothing else
    assert 23 <= (misplaced & ~W).sum() <= 33
    # the wrap: on the grid for the lookup, in the occupied cell (row 0, column 5); 2^32 cells away here
    assert on_by_lookup[W].all() and (cx[W] == 5).all() and (cy[W] == 0).all() and data[0, 5] == 100 and not has[W].any()
    assert (np.maximum(np.abs(fx[W]), np.abs(fy[W])) >= 2.0 ** 32 - 6).all()
    assert (has <= on_by_lookup).all()                    # a pose with a cell is on the grid for the lookup too, in that cell
    assert (cx[has] == fx[has]).all() and (cy[has] == fy[has]).all()
    far = finite & (np.abs(poses[:, 0]) == 1e9)           # the scene's own far pose: off the grid for the lookup as well
    assert far.sum() == 1 and not on_by_lookup[far].any() and not has[far].any()
    for name in NAMES:
        hit, margin = fr.brute(res, xmin, ymin, data, coll[3], fr.FOOTPRINTS[name], poses)
        fhit, cls = fr.filtered(res, xmin, ymin, data, coll[3], fr.FOOTPRINTS[name], poses)
        assert np.isin(cls[misplaced], (fr.NO_CELL, fr.NO_CELL_REJECTED)).all()
        assert (cls[W] == fr.NO_CELL_REJECTED).all() and not hit[W].any() and not fhit[W].any() and np.isinf(margin[W]).sum() == 0
        assert np.array_equal(hit, fhit)
        # what taking the cell from the lookup would do to the wrapped poses: the field is 0 there, a sure hit wherever one exists
        assert dr.brute_force(data, coll[3])[0][0, 5] == 0


def test_fact_scenes():
    """41 x 41 at 0.1 m.  `rect` (0.9 m x 0.5 m) in a corridor of 0.7 m: free along it, a hit across it.  `offc` with a wall
    0.7 m ahead: a hit facing it, free facing away.  Every wall centre is 0.05 m or more from the footprint's boundary"""
    threshold = 0.8
    for walls, pose_xy, name, expect in ((fr.CORRIDOR, fr.CORRIDOR_POSE, "rect", {0.0: False, np.pi / 2: True, np.pi: False, -np.pi / 2: True}),
                                         (fr.WALL_AHEAD, fr.WALL_POSE, "offc", {0.0: True, np.pi: False, np.pi / 2: False})):
        data = fr.fact_scene(walls)
        poses = np.array([[pose_xy[0], pose_xy[1], th] for th in expect])
        hit, margin = fr.brute(cr.RES41, cr.XMIN41, cr.YMIN41, data, threshold, fr.FOOTPRINTS[name], poses)
        assert hit.tolist() == list(expect.values()), (name, hit)
        assert (margin >= 0.05 - 1e-12).all(), margin
        fhit, cls = fr.filtered(cr.RES41, cr.XMIN41, cr.YMIN41, data, threshold, fr.FOOTPRINTS[name], poses)
        assert np.array_equal(fhit, hit)
    # the disc cannot say either: one radius for both headings
    data = fr.fact_scene(fr.CORRIDOR)
    assert data[16].all() and data[24].all() and not data[17:24].any()


def test_edge_poses():
    """not finite in any component: free; far away: free; over the map's edge: the in-grid cells under the base count"""
    data = np.zeros((cr.N41, cr.N41), dtype=np.int8)
    data[20, 0] = 100                                     # a cell in the first column
    x0, y0 = fr.centre41(0, 20)
    nan, inf = float("nan"), float("inf")
    poses = np.array([[nan, y0, 0], [x0, nan, 0], [x0, y0, nan], [inf, y0, 0], [x0, -inf, 0], [x0, y0, inf], [1e9, y0, 0], [x0, -1e300, 0],
                      [x0 - 0.3, y0, 0.0], [x0 - 0.3, y0, np.pi / 2], [x0 - 0.5, y0, 0.0]])
    verts = fr.FOOTPRINTS["rect"]
    hit, _ = fr.brute(cr.RES41, cr.XMIN41, cr.YMIN41, data, 0.8, verts, poses)
    assert hit.tolist() == [False] * 8 + [True, False, False]
    fhit, cls = fr.filtered(cr.RES41, cr.XMIN41, cr.YMIN41, data, 0.8, verts, poses)
    assert np.array_equal(fhit, hit) and (cls[:8] == fr.NO_CELL_REJECTED).all() and (cls[8:] == fr.NO_CELL).all()


def test_first_step_rules():
    hits = np.array([[0, 0, 1, 0, 1], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0], [0, 0, 0, 0, 1]], dtype=bool)
    assert fr.first_step(hits).tolist() == [2, 0, -1, 4] and fr.first_step(hits).dtype == np.int32
    assert fr.first_step(np.zeros((0, 3), dtype=bool)).tolist() == []
    assert fr.first_step(np.array([[True]])).tolist() == [0] and fr.first_step(np.array([[False]])).tolist() == [-1]


def test_planes_header_under_the_sanitizers(tmp_path):
    """tests/footprint_planes_check.cpp (csrc/footprint_planes.hpp alone: validation, half-planes, radii, thresholds) built with
    the address and undefined-behaviour sanitizers and run as a process of its own"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/footprint_planes_check.cpp")
    exe = str(tmp_path / "footprint_planes_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "footprint_planes_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "footprint planes: ok", (out.returncode, out.stdout, out.stderr)

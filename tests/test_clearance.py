"""Clearance queries (eea_clearance_batch / eea_clearance_field: Collision::minDistance / minDirection, reference
collision.cpp:65-124) without a GPU: the entry points and their struct, the argument errors that come before the device is
selected, the visit-ordered walk of csrc/hit_map_table.hpp (tests/clearance_walk_check.cpp under the address and undefined-
behaviour sanitizers, a process of its own), and the order-free restatement of tests/clearance_restatement.py against the
oracle's search -- the second opinion of tests/test_gpu_clearance.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from ergodic_exploration_amd import capi

from tests import clearance_restatement as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_and_exported():
    L = C.CDLL(capi.LIB_PATH)
    for name in ("eea_clearance_batch", "eea_clearance_field"):
        assert name in capi.declared_symbols() and hasattr(L, name), name
    assert (capi.COLLISION_CRASH, capi.COLLISION_OBSTACLE, capi.COLLISION_NONE) == (0, 1, 2)
    assert capi.lib().eea_abi_version() == 6


def test_struct_layout_against_the_c_compiler(tmp_path):
    assert C.sizeof(capi.Clearance) == 16
    lines = ['printf("size %zu\\n", sizeof(eea_clearance));']
    for fname, _ in capi.Clearance._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(eea_clearance, %s));' % (fname, fname))
    lines.append('printf("msgs %d %d %d\\n", EEA_COLLISION_CRASH, EEA_COLLISION_OBSTACLE, EEA_COLLISION_NONE);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ergodic_amd.h"\nint main(void) {\n%s\nreturn 0; }\n'
                   % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)], check=True)
    got = dict(line.split(None, 1) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == 16 and got["msgs"].split() == ["0", "1", "2"]
    for fname, _ in capi.Clearance._fields_:
        assert int(got[fname]) == getattr(capi.Clearance, fname).offset, fname
    assert [getattr(capi.Clearance, f).offset for f, _ in capi.Clearance._fields_] == [0, 4, 8, 12]


def test_argument_errors_come_before_the_device():
    """null cfg / grid / pose, no output, search_radius < boundary_radius, an empty grid and the key bound are answered without
    a device (the buffers are host arrays nothing may touch); P == 0 is EEA_OK"""
    L = capi.lib()
    xs, ys = 80, 60
    good = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 0.7, 1.0, 0.2, 0.8)
    grid, pose = np.zeros(xs * ys, dtype=np.int8), np.zeros((4, 3))
    out, dmin, disp = np.full((4, 4), 7, dtype=np.int32), np.full(4, 7.0), np.full((4, 2), 7.0)
    field, fmin = np.full((ys, xs, 4), 7, dtype=np.int32), np.full((ys, xs), 7.0)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def batch(cfg, g=grid, ps=pose, P=4, o=out, dm=dmin, ds=disp):
        return L.eea_clearance_batch(0, None if cfg is None else C.byref(cfg), p(g), p(ps), P, p(o), p(dm), p(ds), None)

    def fld(cfg, g=grid, f=field, dm=fmin):
        return L.eea_clearance_field(0, None if cfg is None else C.byref(cfg), p(g), p(f), p(dm), None)

    INV, UNS = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED
    assert batch(None) == INV and fld(None) == INV
    assert batch(good, g=None) == INV and batch(good, ps=None) == INV and fld(good, g=None) == INV
    assert batch(good, o=None, dm=None, ds=None) == INV and b"output" in L.eea_last_error()
    assert fld(good, f=None, dm=None) == INV and b"output" in L.eea_last_error()
    swapped = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 1.0, 0.7, 0.2, 0.8)
    assert batch(swapped) == INV and fld(swapped) == INV and b"Search radius" in L.eea_last_error()
    for bad in (capi.make_collision_cfg(-2.0, -1.0, 0.1, 0, ys, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, 0, 0.7, 1.0, 0.2, 0.8),
                capi.make_collision_cfg(-2.0, -1.0, 0.0, xs, ys, 0.7, 1.0, 0.2, 0.8)):
        assert batch(bad) == INV and fld(bad) == INV
    # the key bound: r_bnd = 0 with r_max = 196 cells is the last that fits (tests/clearance_walk_check.cpp); 197 and a
    # radius the walk is never enumerated for are refused
    for search, res in ((19.75, 0.1), (1.0, 0.001), (1.0e6, 0.1)):
        far = capi.make_collision_cfg(-2.0, -1.0, res, xs, ys, 0.0, search, 0.2, 0.8)
        assert batch(far) == UNS and fld(far) == UNS and b"32 bits" in L.eea_last_error(), (search, res)
    assert batch(good, P=0) == capi.OK
    fits = capi.make_collision_cfg(-2.0, -1.0, 0.1, xs, ys, 0.0, 19.65, 0.2, 0.8)      # 196 cells: accepted (P == 0: no device)
    assert batch(fits, P=0) == capi.OK
    assert (out == 7).all() and (dmin == 7.0).all() and (disp == 7.0).all() and (field == 7).all() and (fmin == 7.0).all()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/clearance_walk_check.cpp")
    exe = str(tmp_path_factory.mktemp("clearance_walk") / "clearance_walk_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "clearance_walk_check.cpp"),
                    "-o", exe], check=True)
    return exe


def test_walk_program(program):
    """the offsets within r_col are ring_offsets(); every ring starts at (r, 0); reach and the largest squared distance; the key
    bound accepts the six parameter sets and r_bnd = r_max = 0 and refuses from r_max = 197 (r_bnd = 0) on"""
    out = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "clearance walk: ok", (out.returncode, out.stdout, out.stderr)


@pytest.mark.parametrize("res,coll,n_off", cr.SETS)
def test_walk_is_the_restatements(program, res, coll, n_off):
    r_bnd, _, r_max = cr.radii(res, coll)
    out = subprocess.run([program, str(r_bnd), str(r_max)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.stdout, out.stderr)
    offsets = np.array([[int(v) for v in line.split()] for line in out.stdout.splitlines()], dtype=np.int64).reshape(-1, 2)
    assert len(offsets) == n_off
    assert np.array_equal(offsets, cr.walk(r_bnd, r_max))


@pytest.mark.parametrize("res,coll,n_off", cr.SETS)
def test_canonical_form_is_the_oracles_search(res, coll, n_off):
    """the smallest (|d|^2, visit index) key over the occupied cells a centre reaches is what the ordered search with its early
    stop leaves behind: class, sqrd_obs, dx and dy of 3000 poses up to 30 cells outside the 90 x 70 map"""
    g, data, poses, _, _ = cr.scene(res, coll)
    ref = cr.oracle(coll, g, poses)
    got = cr.restate(res, coll, g, data, poses)
    bad = np.nonzero((got != ref).any(1))[0]
    assert len(bad) == 0, (bad[:10], got[bad[:10]], ref[bad[:10]])
    counts = [int((ref[:, 0] == m).sum()) for m in (cr.CRASH, cr.OBSTACLE, cr.NONE)]
    print("crash / obstacle / none:", counts)
    r_bnd, r_col, r_max = cr.radii(res, coll)
    assert len(cr.walk(r_bnd, r_max)) == n_off
    if coll == (0.4, 0.4, 0.5, 0.8):      # r_col beyond r_max: whatever the search sees is a crash
        assert r_col > r_max and counts[0] > 0 and counts[1] == 0 and counts[2] > 0
    else:
        assert min(counts) > 0


@pytest.mark.parametrize("coll", cr.FACT_COLLS)
def test_hand_made_scenes(coll):
    """ties, the gap cell, inside r_bnd, crash: the oracle's answer at the centre cell is the expected one, and the restatement's"""
    assert cr.radii(cr.RES41, coll) == ((3, 4, 12) if coll == cr.FACT_COLLS[0] else (2, 4, 11))
    for cells, expect in cr.FACTS:
        g, data, pose = cr.fact_scene(cells)
        assert tuple(cr.oracle(coll, g, pose)[0]) == expect, (cells, expect)
        assert tuple(cr.restate(cr.RES41, coll, g, data, pose)[0]) == expect, (cells, expect)


def test_restated_field_is_the_oracles_on_every_cell():
    """the key map read at every cell of a 41 x 41 scene = the oracle at that cell's world centre"""
    coll = cr.FACT_COLLS[0]
    rng = np.random.default_rng(41)
    data = np.zeros((cr.N41, cr.N41), dtype=np.int8)
    data[rng.integers(0, cr.N41, 14), rng.integers(0, cr.N41, 14)] = 100
    data[30:33, 5:9] = 90
    g = po.GridMap(cr.XMIN41, cr.XMIN41 + cr.N41 * cr.RES41, cr.YMIN41, cr.YMIN41 + cr.N41 * cr.RES41, cr.RES41, data.reshape(-1))
    poses = cr.cell_centres(g, cr.N41, cr.N41)
    ref = cr.oracle(coll, g, poses)
    assert np.array_equal(cr.restate(cr.RES41, coll, g, data, poses), ref)
    assert all((ref[:, 0] == m).any() for m in (cr.CRASH, cr.OBSTACLE, cr.NONE))

"""CPU checks of the fleet layer (include/ergodic_amd.h: eea_fleet_layer_*, eea_tick_batch_fleet; csrc/fleet_spans.hpp,
csrc/fleet_layer_kernel.hip): the row spans of the offset set F against a brute-force F (tests/fleet_spans_check.cpp, built
with the address and undefined-behaviour sanitizers and run as a process of its own) and against the oracle's collisionCheck
around one robot's body; the argument checks of the C ABI that need no device; and the scenario of the GPU tick test on the
oracle alone -- the layer has to change verdicts there, or the GPU test would pass on a fleet that never meets."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from ergodic_exploration_amd import capi
from tests import fleet_layer_restatement as fr
from tests.test_host_mirror import DWA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 41


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/fleet_spans_check.cpp")
    exe = str(tmp_path_factory.mktemp("fleet_spans") / "fleet_spans_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(ROOT, "tests", "fleet_spans_check.cpp"),
                    "-o", exe], check=True)
    return exe


def test_spans_are_the_brute_force_offset_set(program):
    """several (r_bnd, r_col, r_max, body), body = 0 and r_bnd = 0 among them: membership == brute force on a window wider
    than the reach, spans sorted and maximal, F = -F, the reach is R'; the program stops at the first wrong answer"""
    out = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "fleet spans: ok", (out.returncode, out.stdout, out.stderr)


@pytest.mark.parametrize("body", [4, 0, 2])
def test_offset_set_is_the_oracles_view_of_a_body(program, body):
    """One robot's body -- the disc d.d <= body^2 -- in the middle of a 41 x 41 grid: the oracle's collisionCheck at the
    centre of every cell is "(body's cell - this cell) in F", for the spans of the library and the restatement of the tests"""
    r_bnd, r_col, r_max = fr.radii(fr.COLL_S, fr.RES)
    assert (r_bnd, r_col, r_max) == (4, 6, 8)
    out = subprocess.run([program, str(r_bnd), str(r_col), str(r_max), str(body)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.stdout, out.stderr)
    spans = [tuple(int(v) for v in line.split()) for line in out.stdout.splitlines()]
    assert len(set(spans)) == len(spans) > 0
    F = fr.offset_set(r_bnd, r_col, r_max, body)
    assert set(spans) == F and all((-x, -y) in F for (x, y) in F)
    assert max(x for x, _ in F) == r_col + body == max(y for _, y in F)
    mid = N // 2
    data = fr.robot_grid(np.zeros((N, N), dtype=np.int8), [(mid, mid), (0, 0)], 1, body)
    assert data.sum() == 100 * len(fr.disc(body))
    xmin, ymin = -2.0, -1.0
    g = po.GridMap(xmin, xmin + N * fr.RES, ymin, ymin + N * fr.RES, fr.RES, data.reshape(-1))
    assert (g.xsize, g.ysize) == (N, N)
    hits = set()
    for i in range(N):
        for j in range(N):
            x, y = xmin + (j + 0.5) * fr.RES, ymin + (i + 0.5) * fr.RES
            assert g.world2grid(x, y) == (i, j)
            if po.collision_check(fr.COLL_S, g, np.array([x, y, 0.0]))[0]:
                hits.add((j - mid, i - mid))      # centre - body's cell
    assert hits == F
    # what the header says of the ring search: a body smaller than the hollow is not seen from its own cell
    assert ((0, 0) in F) == (body >= r_bnd)


def test_fleet_symbols_and_argument_errors_do_not_need_a_device():
    """every argument error of create / tick is raised before any HIP call"""
    L = capi.lib()
    names = ("eea_fleet_layer_create", "eea_fleet_layer_destroy", "eea_fleet_layer_update", "eea_fleet_layer_reach",
             "eea_fleet_layer_read", "eea_fleet_collision_check_batch", "eea_tick_batch_fleet")
    for name in names:
        assert name in capi.declared_symbols() and hasattr(L, name), name
    assert L.eea_abi_version() == 6
    good = lambda **kw: capi.make_collision_cfg(*[kw.get(k, v) for k, v in (
        ("xmin", -1.0), ("ymin", -1.0), ("resolution", fr.RES), ("xsize", 240), ("ysize", 120), ("boundary_radius", fr.COLL_S[0]),
        ("search_radius", fr.COLL_S[1]), ("obstacle_threshold", fr.COLL_S[2]), ("occupied_threshold", fr.COLL_S[3]))])

    def create(cfg, body, B, out=True):
        h = C.c_void_p(77)
        st = L.eea_fleet_layer_create(0, C.byref(cfg) if cfg is not None else None, body, B, C.byref(h) if out else None)
        assert not out or h.value is None          # no layer comes back with an error
        return st, L.eea_last_error().decode()

    assert create(None, 4, 8)[0] == capi.ERR_INVALID_ARGUMENT
    assert create(good(), 4, 8, out=False)[0] == capi.ERR_INVALID_ARGUMENT
    assert create(good(), 4, 0)[0] == capi.ERR_INVALID_ARGUMENT
    assert create(good(), -1, 8)[0] == capi.ERR_INVALID_ARGUMENT
    assert create(good(search_radius=0.1), 4, 8)[0] == capi.ERR_INVALID_ARGUMENT        # below the boundary radius
    assert create(good(occupied_threshold=101.0), 4, 8)[0] == capi.ERR_INVALID_ARGUMENT
    assert create(good(xsize=0), 4, 8)[0] == capi.ERR_INVALID_ARGUMENT
    assert create(good(resolution=0.0), 4, 8)[0] == capi.ERR_INVALID_ARGUMENT
    # the reach r_col + body: 6 + 121 = 127 is the last one taken (not tried here: it would allocate), 128 is refused
    st, msg = create(good(), 122, 8)
    assert st == capi.ERR_UNSUPPORTED and "127" in msg
    st, _ = create(good(boundary_radius=6.4, search_radius=7.0), 0, 8)                  # r_col = 130 alone
    assert st == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.EngineError) as ei:
        capi.FleetLayer(good(), 4, 0)
    assert ei.value.status == capi.ERR_INVALID_ARGUMENT
    # null handles
    one = C.c_void_p(8)
    assert L.eea_fleet_layer_reach(None) == -1
    assert L.eea_fleet_layer_update(None, one, None, None) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_fleet_layer_read(None, one, one) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_fleet_collision_check_batch(None, None, one, None, 3, one, None) == capi.ERR_INVALID_ARGUMENT
    L.eea_fleet_layer_destroy(None)
    io, t = capi.BatchIO(), capi.TickIO()
    dcfg = capi.DwaCfg(*DWA["omni"])
    assert L.eea_tick_batch_fleet(None, 4, C.byref(io), C.byref(t), C.byref(good()), C.byref(dcfg), one, None) == capi.ERR_INVALID_ARGUMENT


def run_scenario_on_the_oracle(model):
    """The tick scenario of tests/test_gpu_fleet_layer.py: 12 small robots, 8 ticks, every robot an independent oracle loop on
    a grid of its own that is rebuilt every tick from the other robots' cells; the fleet moves by the oracles' twists.
    Returns (the (tick, robot) pairs whose validate_control verdict differs between the plain and the robot's own grid, the
    sources seen)."""
    _, data = fr.plain_grid(po)
    plain = fr.grid_map(po, data)
    g = fr.sr.Geometry(fr.BOUNDS[0], fr.BOUNDS[2], fr.RES, data.shape[1], data.shape[0], fr.COLL_S[3])
    body = fr.radii(fr.COLL_S, fr.RES)[0]
    poses = fr.start_poses(model)
    B = len(poses)
    ors = [fr.FleetOracle(po, model, DWA[model]) for _ in range(B)]
    vb = np.zeros((B, 3))
    bites, seen = [], set()
    for t in range(fr.TICKS):
        cells = fr.cells_of(g, poses)
        assert (cells != fr.NOT_STAMPED).all()
        grids = [fr.grid_map(po, fr.robot_grid(data, cells, b, body)) for b in range(B)]
        if t == 0:      # no robot starts in collision, with the other robots or the block
            for b in range(B):
                assert po.validate_control(fr.COLL_S, grids[b], poses[b], np.zeros(3), fr.VAL_DT, fr.VAL_HORIZON), b
        out = []
        for b, o in enumerate(ors):
            o.grid = grids[b]
            out.append(o.tick(poses[b], vb[b]))
            own = po.validate_control(fr.COLL_S, grids[b], poses[b], o.u_checked, fr.VAL_DT, fr.VAL_HORIZON)
            if own != po.validate_control(fr.COLL_S, plain, poses[b], o.u_checked, fr.VAL_DT, fr.VAL_HORIZON):
                bites.append((t, b))
            seen.add(out[-1][1])
        u = np.array([o[0] for o in out])
        for b in range(B):
            poses[b] = po.integrate_twist(poses[b], u[b], fr.DT)
        vb = u.copy()
    return bites, seen


@pytest.mark.parametrize("model", ["omni", "simple_cart"])
def test_the_layer_bites_in_the_tick_scenario(model):
    bites, seen = run_scenario_on_the_oracle(model)
    assert len(bites) >= 3, bites
    assert seen >= {"ergodic", "dwa-reference"}, seen

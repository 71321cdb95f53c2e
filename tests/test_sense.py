"""CPU checks of the fleet's range sensor (include/ergodic_amd.h: eea_sense_reveal_batch, eea_grid_census;
csrc/sense_kernel.hip): the numpy restatement tests/sense_restatement.py against an independent statement in exact
fractions, the facts the header states about the ray set, the behaviour at walls, thresholds and unknown cells, the argument
checks of the C ABI that need no device, and the kernels' presence in the gfx950 build."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from ergodic_exploration_amd import capi
from tests import sense_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _geom(xsize, ysize, res=0.1, xmin=0.0, ymin=0.0, thr=0.8):
    return sr.Geometry(xmin, ymin, res, xsize, ysize, thr)


def _centre(g, i, j):
    """a pose in the middle of cell (i, j)"""
    return [g.xmin + (j + 0.5) * g.resolution, g.ymin + (i + 0.5) * g.resolution, 0.0]


def _round_half_away(fr):
    """a non-negative Fraction to the nearest integer, halves up"""
    return math.floor(fr + Fraction(1, 2))


def _brute_reveal(g, R, truth, known, poses):
    """the contract of ergodic_amd.h once more, on its own: targets by walking the square's perimeter, steps by rounding
    s |m| / R in exact fractions, the robot's cell by a plain floor (the poses used here need no wrap)"""
    perimeter = ([(R, -R + k) for k in range(2 * R)] + [(R - k, R) for k in range(2 * R)] +
                 [(-R, R - k) for k in range(2 * R)] + [(-R + k, -R) for k in range(2 * R)])
    ranges = np.full((len(poses), 8 * R), -1, dtype=np.int32)
    for b, (x, y, _) in enumerate(poses):
        j0 = int(np.floor((x - g.xmin) / g.resolution))
        i0 = int(np.floor((y - g.ymin) / g.resolution))
        j0 -= 1 if j0 == g.xsize else 0
        i0 -= 1 if i0 == g.ysize else 0
        if not (0 <= i0 < g.ysize and 0 <= j0 < g.xsize):
            continue
        known[i0, j0] = truth[i0, j0]
        for q, (tx, ty) in enumerate(perimeter):
            for s in range(1, R + 1):
                dx = int(np.sign(tx)) * _round_half_away(Fraction(s * abs(tx), R))
                dy = int(np.sign(ty)) * _round_half_away(Fraction(s * abs(ty), R))
                if dx * dx + dy * dy > R * R or not (0 <= i0 + dy < g.ysize and 0 <= j0 + dx < g.xsize):
                    break
                cell = truth[i0 + dy, j0 + dx]
                known[i0 + dy, j0 + dx] = cell
                if not (np.float64(cell) / np.float64(100.0) < np.float64(g.occupied_threshold)):
                    ranges[b, q] = s
                    break
    return ranges


@pytest.mark.parametrize("R", range(1, 13))
def test_restatement_is_the_statement_in_exact_fractions(R):
    """every R <= 12: the integer closed form of a step against s |m| / R rounded half away from zero in Fractions, and a
    whole reveal (cluttered grid, robots in the open, at the rim and off the grid) against the brute-force statement"""
    for m in range(-R, R + 1):
        for s in range(1, R + 1):
            want = (1 if m > 0 else -1 if m < 0 else 0) * _round_half_away(Fraction(s * abs(m), R))
            assert sr.step_offset(m, s, R) == want, (m, s)
    targets = [sr.ray_target(q, R) for q in range(8 * R)]
    assert len(set(targets)) == 8 * R and all(max(abs(tx), abs(ty)) == R for tx, ty in targets)
    assert capi.sense_ray_count(R) == 8 * R == len(targets)
    rng = np.random.default_rng(R)
    g = _geom(31, 27)
    truth = rng.choice(np.array([0, 0, 0, 0, 0, 0, 100, -1, 79, 80], dtype=np.int8), size=(27, 31))
    poses = [_centre(g, 13, 15), _centre(g, 0, 0), _centre(g, 26, 30), _centre(g, 5, 29), [3.1, 2.7, 1.0], [-0.5, 1.0, 0.0],
             [1.0, 2.75, 0.0]]
    k1, k2 = np.full_like(truth, -1), np.full_like(truth, -1)
    r1 = sr.reveal(g, R, truth, k1, poses)
    r2 = _brute_reveal(g, R, truth, k2, poses)
    assert np.array_equal(k1, k2) and np.array_equal(r1, r2)
    assert (k1 != -1).any() and (r1 >= 1).any()


@pytest.mark.parametrize("R", [1, 2, 3, 5, 9, 20, 50])
def test_rays_cover_the_disc_and_nothing_else(R):
    """in an obstacle-free grid the rays reach every cell of dx^2 + dy^2 <= R^2 and none outside; the set of offsets is
    closed under x <-> -x, y <-> -y and x <-> y"""
    seen = set()
    for ray in sr.ray_offsets(R):
        for dx, dy in ray:
            if dx * dx + dy * dy > R * R:
                break
            seen.add((int(dx), int(dy)))
    disc = {(dx, dy) for dx in range(-R, R + 1) for dy in range(-R, R + 1) if dx * dx + dy * dy <= R * R} - {(0, 0)}
    assert seen == disc
    every = {tuple(int(v) for v in o) for o in sr.ray_offsets(R).reshape(-1, 2)}   # the uncut steps as well
    for f in (lambda x, y: (-x, y), lambda x, y: (x, -y), lambda x, y: (y, x)):
        assert {f(*o) for o in every} == every
    if R <= 9:   # ... and through reveal(): the robot's own cell and the disc, nothing else
        n = 2 * R + 5
        g = _geom(n, n)
        truth, known = np.zeros((n, n), dtype=np.int8), np.full((n, n), -1, dtype=np.int8)
        ranges = sr.reveal(g, R, truth, known, [_centre(g, R + 2, R + 2)])
        ii, jj = np.nonzero(known == 0)
        assert {(int(j) - R - 2, int(i) - R - 2) for i, j in zip(ii, jj)} == disc | {(0, 0)}
        assert (ranges == -1).all()


def _room():
    """a closed room of 100-walls in a 30 x 24 grid: interior rows 5 .. 17, columns 4 .. 21; clutter outside"""
    truth = np.zeros((24, 30), dtype=np.int8)
    truth[:4], truth[19:], truth[:, :3], truth[:, 23:] = 55, 55, -1, 100   # what must stay hidden
    truth[4:19, 3:23] = 100
    truth[5:18, 4:22] = 0
    return _geom(30, 24), truth


def test_closed_room_hides_what_is_outside():
    g, truth = _room()
    known = np.full_like(truth, -1)
    poses = [_centre(g, 6, 5), _centre(g, 16, 20), _centre(g, 11, 12)]
    ranges = sr.reveal(g, 30, truth, known, poses)
    inside = np.zeros_like(truth, dtype=bool)
    inside[4:19, 3:23] = True
    assert (known[~inside] == -1).all()
    assert np.array_equal(known[5:18, 4:22], truth[5:18, 4:22])      # the whole interior (convex: every cell is seen)
    assert (ranges >= 1).all()                                       # R = 30 spans the room: every ray ends on a wall
    seen_wall = known[inside] == 100
    assert seen_wall.any()


def test_threshold_pair_79_80():
    """occupied_threshold = 0.8: a cell of 80 blocks (!(0.8 < 0.8)), a cell of 79 does not; both become known"""
    g = _geom(21, 5)
    truth = np.zeros((5, 21), dtype=np.int8)
    truth[2, 13], truth[2, 7] = 80, 79
    known = np.full_like(truth, -1)
    R = 8
    ranges = sr.reveal(g, R, truth, known, [_centre(g, 2, 10)])
    east, west = 0 * 2 * R + R, 2 * 2 * R + R                  # side 0, k = R: (R, 0); side 2, k = R: (-R, 0)
    assert sr.ray_target(east, R) == (R, 0) and sr.ray_target(west, R) == (-R, 0)
    assert ranges[0, east] == 3 and known[2, 13] == 80 and known[2, 14] == -1
    assert ranges[0, west] == -1 and known[2, 7] == 79 and known[2, 6] == 0 and known[2, 2] == 0
    assert sr.blocks(80, 0.8) and not sr.blocks(79, 0.8) and not sr.blocks(-1, 0.8) and not sr.blocks(-1, 0.0)


def test_unknown_truth_cells_let_rays_through():
    g = _geom(21, 5)
    truth = np.zeros((5, 21), dtype=np.int8)
    truth[:, 12:15] = -1
    truth[:, 17] = 100
    known = np.full_like(truth, 7)      # a sentinel that is neither: a -1 in truth is written as -1
    R = 9
    ranges = sr.reveal(g, R, truth, known, [_centre(g, 2, 10)])
    assert ranges[0, R] == 7 and (known[2, 12:15] == -1).all() and known[2, 15] == 0 and known[2, 17] == 100
    assert known[2, 18] == 7


def test_a_second_call_changes_nothing():
    g, truth = _room()
    truth[9:12, 10] = 100
    known = np.full_like(truth, -1)
    poses = [_centre(g, 6, 5), _centre(g, 11, 14), [-3.0, 1.0, 0.0]]
    mask = np.array([1, 1, 1], dtype=np.int32)
    r1 = sr.reveal(g, 7, truth, known, poses, mask)
    once = known.copy()
    r2 = sr.reveal(g, 7, truth, known, poses, mask)
    assert np.array_equal(known, once) and np.array_equal(r1, r2) and (r1[2] == -1).all()
    # a masked robot is left out, its row of ranges included
    fresh, rows = np.full_like(truth, -1), np.full((3, 56), -77, dtype=np.int32)
    sr.reveal(g, 7, truth, fresh, poses, np.array([0, 1, 1], dtype=np.int32), rows)
    assert (rows[0] == -77).all() and np.array_equal(rows[1:], r1[1:]) and fresh[6, 5] == -1
    assert sr.census(g, once) == (int((once < 0).sum()), int(((once >= 0) & (once < 80)).sum()), int((once >= 80).sum()))


def test_world2grid_restated_with_the_x86_wrap():
    g = _geom(23, 19, res=0.1, xmin=-1.0, ymin=-2.0)
    assert sr.world2grid(g, -1.0, -2.0) == (0, 0)
    g2 = _geom(8, 4, res=0.25)
    assert sr.world2grid(g2, 2.0, 1.0) == (3, 7)                      # exactly xmax / ymax: the decrement rule
    assert sr.world2grid(g2, -0.05, 0.1) == (0, 4294967295)           # negative: wraps, fails gridBounds
    assert sr.world2grid(g2, 1e9, 0.0)[1] == (4000000000 & 0xFFFFFFFF)
    assert sr.world2grid(g2, float("nan"), 0.0) == (0, 0)


def test_sense_symbols_and_argument_errors_do_not_need_a_device():
    """every argument error is raised before any HIP call (as test_field_argument_errors_do_not_need_a_device)"""
    L = capi.lib()
    for name in ("eea_sense_ray_count", "eea_sense_reveal_batch", "eea_grid_census"):
        assert name in capi.declared_symbols() and hasattr(L, name), name
    assert L.eea_abi_version() == 6
    assert L.eea_sense_ray_count(50) == 400 and capi.sense_ray_count(1) == 8
    one, two = C.c_void_p(8), C.c_void_p(16)   # never dereferenced: the argument checks come first
    # (radii that Collision::Collision would refuse: the sensor does not read them)
    good = capi.make_collision_cfg(0.0, 0.0, 0.1, 23, 19, 0.7, 0.1, 0.2, 0.8)
    ok = dict(cfg=C.byref(good), R=5, truth=one, known=two, pose=one, mask=None, P=3, ranges=None)

    def reveal(**kw):
        a = dict(ok, **kw)
        return L.eea_sense_reveal_batch(0, a["cfg"], a["R"], a["truth"], a["known"], a["pose"], a["mask"], a["P"], a["ranges"], None)

    for name in ("cfg", "truth", "known", "pose"):
        assert reveal(**{name: None}) == capi.ERR_INVALID_ARGUMENT, name
        assert b"null" in L.eea_last_error()
    assert reveal(known=one) == capi.ERR_INVALID_ARGUMENT and b"different" in L.eea_last_error()
    assert reveal(R=0) == capi.ERR_INVALID_ARGUMENT and b"range_cells" in L.eea_last_error()
    assert reveal(R=1025) == capi.ERR_UNSUPPORTED and b"1024" in L.eea_last_error()
    assert reveal(R=1024, P=0) == capi.OK          # nothing to do: nothing launched, no device needed
    for field, bad, word in (("xsize", 0, b"xsize"), ("ysize", 0, b"xsize"), ("resolution", 0.0, b"resolution"),
                             ("resolution", -0.1, b"resolution"), ("resolution", float("nan"), b"resolution")):
        cfg = capi.make_collision_cfg(0.0, 0.0, 0.1, 23, 19, 0.7, 1.0, 0.2, 0.8)
        setattr(cfg, field, bad)
        assert reveal(cfg=C.byref(cfg)) == capi.ERR_INVALID_ARGUMENT, (field, bad)
        assert word in L.eea_last_error()
        assert L.eea_grid_census(0, C.byref(cfg), one, two, None) == capi.ERR_INVALID_ARGUMENT, (field, bad)
    for args in ((None, one, two), (C.byref(good), None, two), (C.byref(good), one, None)):
        assert L.eea_grid_census(0, args[0], args[1], args[2], None) == capi.ERR_INVALID_ARGUMENT
        assert b"null" in L.eea_last_error()


def test_sense_kernels_are_in_the_library():
    """the kernels of csrc/sense_kernel.hip are gfx950 code in the build and use no scratch; the reveal kernels' LDS is sized
    per launch ((2R + 1)^2 bytes), none of it static"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    obj = os.path.join(os.path.dirname(capi.LIB_PATH), "..", "csrc", "build", "sense_kernel.o")
    names = {}
    for k in kr.kernels(obj):
        if "vgpr_count" in k:
            names[subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.strip()] = k
    want = ("sense_reveal_lds_kernel", "sense_reveal_global_kernel", "grid_census_kernel")
    for w in want:
        found = [k for n, k in names.items() if w + "(" in n]
        assert len(found) == 1, (w, sorted(names))
        assert int(found[0]["private_segment_fixed_size"]) == 0, found[0]
        if w != "grid_census_kernel":
            assert int(found[0]["group_segment_fixed_size"]) == 0, found[0]


def test_host_wrapper_has_the_sense_calls(tmp_path):
    """host/include/ergodic_exploration/sensing.hpp: senseReveal and gridCensus compile against the C header"""
    src = tmp_path / "use.cpp"
    src.write_text("#include <ergodic_exploration/sensing.hpp>\n"
                   "void use(const eea_collision_cfg& cfg, const int8_t* truth, int8_t* known, const double* pose, int* ranges,\n"
                   "         const int* mask, unsigned long long* counts)\n"
                   "{ ergodic_exploration::senseReveal(cfg, 50u, truth, known, pose, 4096u);\n"
                   "  ergodic_exploration::senseReveal(cfg, 50u, truth, known, pose, 4096u, ranges, mask, nullptr);\n"
                   "  ergodic_exploration::gridCensus(cfg, known, counts);\n"
                   "  ergodic_exploration::gridCensus(cfg, known, counts, nullptr);\n"
                   "  static_assert(sizeof(ergodic_exploration::senseRayCount(50u)) == sizeof(unsigned), \"\"); }\n"
                   "int main() { return 0; }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROOT, "ergodic_exploration_amd", "host", "include"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(os.environ.get("ROCM", "/opt/rocm"), "include"), str(src)], check=True)

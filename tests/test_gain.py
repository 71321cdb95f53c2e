"""CPU checks of the information-gain field (include/ergodic_amd.h: eea_sense_gain_field, eea_set_target_gain;
csrc/gain_kernel.hip): the numpy restatement tests/gain_restatement.py against an independent statement in exact fractions,
the closed-form value in an empty unknown world, the zero of a fully known one, the relation to what a reveal would change,
the stride lattice, the 79 / 80 threshold pair, the argument checks of the C ABI that need no device, and the kernels' presence
in the gfx950 build."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from ergodic_exploration_amd import capi
from tests import gain_restatement as gr
from tests import gain_scenes as gs
from tests import sense_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _brute_gain(g, R, stride, known):
    """the contract of ergodic_amd.h once more, on its own: targets by walking the square's perimeter, steps by rounding
    s |m| / R half away from zero in exact fractions, the blocking rule by the literal division"""
    perimeter = ([(R, -R + k) for k in range(2 * R)] + [(R - k, R) for k in range(2 * R)] +
                 [(-R, R - k) for k in range(2 * R)] + [(-R + k, -R) for k in range(2 * R)])
    stops = lambda cell: not (np.float64(cell) / np.float64(100.0) < np.float64(g.occupied_threshold))
    gain = np.zeros((g.ysize, g.xsize), dtype=np.uint32)
    for i0 in range(g.ysize):
        for j0 in range(g.xsize):
            if i0 % stride or j0 % stride or stops(known[i0, j0]):
                continue
            n = int(known[i0, j0] < 0)
            for tx, ty in perimeter:
                for s in range(1, R + 1):
                    dx = int(np.sign(tx)) * math.floor(Fraction(s * abs(tx), R) + Fraction(1, 2))
                    dy = int(np.sign(ty)) * math.floor(Fraction(s * abs(ty), R) + Fraction(1, 2))
                    if dx * dx + dy * dy > R * R or not (0 <= i0 + dy < g.ysize and 0 <= j0 + dx < g.xsize):
                        break
                    n += int(known[i0 + dy, j0 + dx] < 0)
                    if stops(known[i0 + dy, j0 + dx]):
                        break
            gain[i0, j0] = n
    return gain


@pytest.mark.parametrize("R", range(1, 9))
def test_restatement_is_the_statement_in_exact_fractions(R):
    """every R <= 8, stride 1 and 3, on a cluttered 17 x 13 grid with unknown, free, 79, 80 and 100 cells"""
    rng = np.random.default_rng(40 + R)
    g = sr.Geometry(0.0, 0.0, 0.1, 17, 13, 0.8)
    known = rng.choice(np.array([-1, -1, -1, 0, 0, 0, 0, 100, 79, 80], dtype=np.int8), size=(13, 17))
    for stride in (1, 3):
        got = gr.gain_field(g, R, stride, known)
        assert got.dtype == np.uint32 and np.array_equal(got, _brute_gain(g, R, stride, known)), stride
        assert got.max() > 0 and got.max() <= 8 * R * R + 1


@pytest.mark.parametrize("R", [1, 2, 5, 8])
def test_empty_unknown_world_has_the_closed_form(R):
    """all unknown, no obstacle: every candidate at least R from the edges sees 1 + #{(q, s) inside the disc}; 161 at R = 5"""
    steps = sum(1 for ray in sr.ray_offsets(R) for k, (dx, dy) in enumerate(ray)
                if all(x * x + y * y <= R * R for x, y in ray[:k + 1]))
    if R == 5:
        assert 1 + steps == 161
    n = 2 * R + 4
    g = sr.Geometry(0.0, 0.0, 0.1, n + 1, n, 0.8)
    gain = gr.gain_field(g, R, 1, np.full((n, n + 1), -1, dtype=np.int8))
    assert (gain[R:n - R, R:n + 1 - R] == 1 + steps).all()
    assert gain[0, 0] < 1 + steps and gain[0, 0] > 0          # a corner sees less: its rays leave the grid
    assert gain.max() == 1 + steps <= 8 * R * R + 1


def test_fully_known_grid_is_zero():
    g, known = gs.partly_revealed(23, 19)
    full = np.where(known < 0, 0, known).astype(np.int8)
    assert (full == 100).any() and (gr.gain_field(g, 4, 1, full) == 0).all()


@pytest.mark.parametrize("xs,ys,R,stride", [(23, 19, 3, 1), (23, 19, 9, 1), (64, 41, 17, 3), (40, 30, 5, 2)])
def test_gain_bounds_what_a_reveal_would_change(xs, ys, R, stride):
    """T = `known` with its unknown cells free: the cells a reveal of T from a non-blocking candidate changes number at most
    the candidate's gain (the gain counts per beam) and are none exactly where the gain is 0"""
    g, known = gs.partly_revealed(xs, ys)
    gain = gr.gain_field(g, R, stride, known)
    T = np.where(known < 0, 0, known).astype(np.int8)
    seen = 0
    for i0 in range(0, ys, stride):
        for j0 in range(0, xs, stride):
            if sr.blocks(known[i0, j0], g.occupied_threshold):
                assert gain[i0, j0] == 0
                continue
            after = known.copy()
            sr.reveal(g, R, T, after, [gs.centre(g, i0, j0)])
            changed = int((after != known).sum())
            assert changed <= gain[i0, j0] and (changed > 0) == (gain[i0, j0] > 0), (i0, j0, changed, gain[i0, j0])
            seen += 1
    assert seen > 20 and (gain > 0).any()
    assert R > 5 or (gain[::stride, ::stride] == 0).any()     # (from R = 9 on every candidate of these grids sees a frontier)


@pytest.mark.parametrize("stride", [2, 3, 5, 64])
def test_stride_keeps_the_lattice_values(stride):
    g, known = gs.partly_revealed(40, 30)
    one, lat = gr.gain_field(g, 5, 1, known), gr.gain_field(g, 5, stride, known)
    on = np.zeros_like(one, dtype=bool)
    on[::stride, ::stride] = True
    assert (lat[~on] == 0).all() and np.array_equal(lat[on], one[on]) and lat[0, 0] == one[0, 0]


def test_threshold_pair_79_80():
    """occupied_threshold = 0.8: the unknown cells behind a cell of 80 are not seen, those behind a cell of 79 are; a candidate
    ON a cell of 80 gets 0, one on a cell of 79 counts"""
    g = sr.Geometry(0.0, 0.0, 0.1, 21, 5, 0.8)
    R = 8
    east = np.zeros((5, 21), dtype=np.int8)
    east[2, 13], east[2, 14:] = 80, -1
    assert gr.gain_field(g, R, 1, east)[2, 10] == 0
    east[2, 13] = 79
    assert gr.gain_field(g, R, 1, east)[2, 10] > 0
    west = np.zeros((5, 21), dtype=np.int8)
    west[2, 7], west[2, :7] = 79, -1
    assert gr.gain_field(g, R, 1, west)[2, 10] == 5          # the ray due west: columns 6 .. 2, the rest is out of range
    on = np.full((5, 21), -1, dtype=np.int8)
    on[2, 10] = 80
    assert gr.gain_field(g, R, 1, on)[2, 10] == 0
    on[2, 10] = 79
    assert gr.gain_field(g, R, 1, on)[2, 10] > 0
    # a blocking cell that is itself negative cannot exist at this threshold; at a negative one (where every cell that lets a
    # ray through is negative) the contract counts it, then ends the ray: the wall costs the cells behind it, not itself
    neg = sr.Geometry(0.0, 0.0, 0.1, 21, 5, -0.5)
    assert sr.blocks(-1, -0.5) and not sr.blocks(-100, -0.5)
    open_, wall = np.full((5, 21), -100, dtype=np.int8), np.full((5, 21), -100, dtype=np.int8)
    wall[:, 11] = -1
    a, b = gr.gain_field(neg, 2, 1, open_), gr.gain_field(neg, 2, 1, wall)
    assert np.array_equal(b, _brute_gain(neg, 2, 1, wall)) and (b[:, 11] == 0).all()
    # R = 2: step 1 of all 16 rays is in the disc, step 2 of the 4 axis rays only; the wall takes (2, 12) from the ray due east
    assert a[2, 10] == 1 + 16 + 4 and b[2, 10] == a[2, 10] - 1


def test_value_grid():
    g, known = gs.partly_revealed(23, 19)
    gain = gr.gain_field(g, 3, 2, known)
    v = gr.value_grid(g, 2, known, gain, 0.5)
    on = np.zeros_like(known, dtype=bool)
    on[::2, ::2] = True
    free = on & (known < 80)
    assert (v[~free] == 0).all() and np.array_equal(v[free], gain[free] + 0.5) and (known[on] >= 80).any()
    assert gr.value_grid(g, 2, known, gain, 0.5, np.float32).dtype == np.float32


def test_gain_symbols_and_argument_errors_do_not_need_a_device():
    """every argument error is raised before any HIP call (as test_sense_symbols_and_argument_errors_do_not_need_a_device):
    the pointers are never dereferenced, the engine neither"""
    L = capi.lib()
    for name in ("eea_sense_gain_field", "eea_set_target_gain"):
        assert name in capi.declared_symbols() and hasattr(L, name), name
    assert L.eea_abi_version() == 6
    one, two, eng = C.c_void_p(8), C.c_void_p(16), C.c_void_p(64)
    good = capi.make_collision_cfg(0.0, 0.0, 0.1, 23, 19, 0.7, 0.1, 0.2, 0.8)
    ok = dict(e=eng, cfg=C.byref(good), R=5, stride=2, known=one, gain=two, floor=0.5, lx=2.2, ly=1.8)

    def field(**kw):
        a = dict(ok, **kw)
        return L.eea_sense_gain_field(0, a["cfg"], a["R"], a["stride"], a["known"], a["gain"], None)

    def target(**kw):
        a = dict(ok, **kw)
        return L.eea_set_target_gain(a["e"], a["cfg"], a["R"], a["stride"], a["known"], a["floor"], a["lx"], a["ly"], a["gain"], None)

    for name in ("cfg", "known", "gain"):
        assert field(**{name: None}) == capi.ERR_INVALID_ARGUMENT and b"null" in L.eea_last_error(), name
    for name in ("e", "cfg", "known"):
        assert target(**{name: None}) == capi.ERR_INVALID_ARGUMENT and b"null" in L.eea_last_error(), name
    for call in (field, target):
        assert call(R=0) == capi.ERR_INVALID_ARGUMENT and b"range_cells" in L.eea_last_error()
        assert call(stride=0) == capi.ERR_INVALID_ARGUMENT and b"stride" in L.eea_last_error()
        assert call(R=1025) == capi.ERR_UNSUPPORTED and b"1024" in L.eea_last_error()
        for fld, bad, word in (("xsize", 0, b"xsize"), ("ysize", 0, b"xsize"), ("resolution", 0.0, b"resolution"),
                               ("resolution", -0.1, b"resolution"), ("resolution", float("nan"), b"resolution")):
            cfg = capi.make_collision_cfg(0.0, 0.0, 0.1, 23, 19, 0.7, 1.0, 0.2, 0.8)
            setattr(cfg, fld, bad)
            assert call(cfg=C.byref(cfg)) == capi.ERR_INVALID_ARGUMENT, (fld, bad)
            assert word in L.eea_last_error()
    for bad in (-0.5, float("nan"), float("inf")):
        assert target(floor=bad) == capi.ERR_INVALID_ARGUMENT and b"floor" in L.eea_last_error(), bad
    for kw in (dict(lx=0.0), dict(ly=-1.0), dict(lx=float("nan"))):
        assert target(**kw) == capi.ERR_INVALID_ARGUMENT, kw
    big = capi.make_collision_cfg(0.0, 0.0, 0.1, 1 << 16, (1 << 15) + 1, 0.7, 0.1, 0.2, 0.8)
    assert target(cfg=C.byref(big)) == capi.ERR_UNSUPPORTED and b"2^31" in L.eea_last_error()


def test_gain_kernels_are_in_the_library():
    """the kernels of csrc/gain_kernel.hip are gfx950 code in the build and use no scratch; the LDS window is sized per launch,
    none of it static"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    obj = os.path.join(os.path.dirname(capi.LIB_PATH), "..", "csrc", "build", "gain_kernel.o")
    names = {}
    for k in kr.kernels(obj):
        if "vgpr_count" in k:
            names[subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.strip()] = k
    for w in ("gain_field_lds_kernel(", "gain_field_global_kernel(", "gain_values_kernel<double>(", "gain_values_kernel<float>("):
        found = [k for n, k in names.items() if w in n]
        assert len(found) == 1, (w, sorted(names))
        assert int(found[0]["private_segment_fixed_size"]) == 0, found[0]
        assert int(found[0]["group_segment_fixed_size"]) == 0, found[0]


def test_host_wrapper_has_the_gain_calls(tmp_path):
    """host/include/ergodic_exploration/sensing.hpp: senseGainField and setTargetGain compile against the C header"""
    src = tmp_path / "use.cpp"
    src.write_text("#include <ergodic_exploration/sensing.hpp>\n"
                   "void use(eea_engine* e, const eea_collision_cfg& cfg, const int8_t* known, unsigned int* gain)\n"
                   "{ ergodic_exploration::senseGainField(cfg, 50u, 4u, known, gain);\n"
                   "  ergodic_exploration::senseGainField(cfg, 50u, 4u, known, gain, nullptr);\n"
                   "  ergodic_exploration::setTargetGain(e, cfg, 50u, 4u, known, 0.5, 10.0, 5.0);\n"
                   "  ergodic_exploration::setTargetGain(e, cfg, 50u, 4u, known, 0.5, 10.0, 5.0, gain, nullptr); }\n"
                   "int main() { return 0; }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROOT, "ergodic_exploration_amd", "host", "include"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(os.environ.get("ROCM", "/opt/rocm"), "include"), str(src)], check=True)

"""CPU checks of the mutual-information field (include/ergodic_amd.h: eea_sense_mi_table, eea_sense_mi_field, eea_set_target_mi;
csrc/mi_kernel.hip): the library's table against the formula in multi-precision, the argument checks of the C ABI that need no
device, the restatement tests/mi_restatement.py against the entropy of the beam's measurement over every map in exact
fractions, the closed form of an unknown world, the zero set and the bound it shares with the gain count, the discounting the
count lacks, the stride lattice, and the kernels' presence in the gfx950 build.

Multi-precision: mpmath where it is installed; otherwise the logs are summed as series in exact fractions (_ln below), which
is independent of math.log as well."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from ergodic_exploration_amd import capi
from tests import gain_restatement as gr
from tests import mi_restatement as mr
from tests import mi_scenes as ms
from tests import sense_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2 = math.log(2.0)
EPS = 2.0 ** -53

try:
    import mpmath
    mpmath.mp.prec = 200
except ImportError:                                        # pragma: no cover
    mpmath = None


def _atanh_series(z, terms=60):
    z2, acc, power = z * z, Fraction(0), z
    for n in range(terms):
        acc += power / (2 * n + 1)
        power = (power * z2).limit_denominator(10 ** 60)
    return 2 * acc


def _ln(x):
    """ln of a positive Fraction to ~1e-50: x = m 2^e with m in [3/4, 3/2), ln m = 2 atanh((m - 1) / (m + 1)), |z| <= 1/5"""
    if mpmath is not None:
        return mpmath.log(mpmath.mpf(x.numerator) / mpmath.mpf(x.denominator))
    e, m = 0, Fraction(x)
    while m >= Fraction(3, 2):
        m, e = m / 2, e + 1
    while m < Fraction(3, 4):
        m, e = m * 2, e - 1
    return e * _atanh_series(Fraction(1, 3)) + _atanh_series((m - 1) / (m + 1))


def _num(x):
    """a Fraction as a number _ln's results combine with"""
    return mpmath.mpf(x.numerator) / mpmath.mpf(x.denominator) if mpmath is not None else x


def _entropy(o):
    """-o ln o - (1 - o) ln(1 - o) of an exact Fraction 0 < o < 1, in multi-precision"""
    return -_num(o) * _ln(o) - _num(1 - o) * _ln(1 - o)


def _cfg(thr):
    return capi.make_collision_cfg(0.0, 0.0, 0.1, 23, 19, 0.7, 0.1, 0.2, thr)


@pytest.mark.parametrize("p_unknown", [0.5, 0.2])
@pytest.mark.parametrize("thr", [0.8, 0.5])
def test_table_h_entries(thr, p_unknown):
    """every h entry within 4 ulp of the formula at the same double o, evaluated in multi-precision: both terms are
    non-negative, so the relative errors do not amplify: each log <= 1 ulp, two products of half an ulp each, one sum; the
    entries of v = 0 and v >= 100 are exactly 0.0 and every negative v shares the p_unknown entry"""
    h, _ = capi.sense_mi_table(_cfg(thr), p_unknown)
    worst = 0.0
    for v in range(-128, 128):
        o = p_unknown if v < 0 else min(v, 100) / 100.0
        got = float(h[v + 128])
        if v == 0 or v >= 100:
            assert got == 0.0 and not np.signbit(h[v + 128]), v
            continue
        want = _entropy(Fraction(o))
        err = abs(_num(Fraction(got)) - want) / math.ulp(float(want))
        worst = max(worst, float(err))
        assert err <= 4, (v, got, float(want), float(err))
    print("threshold %.1f, p_unknown %.1f: worst h entry %.2f ulp" % (thr, p_unknown, worst))
    assert (h[:128] == h[127]).all() and h[127] > 0.0


@pytest.mark.parametrize("p_unknown", [0.5, 0.2])
@pytest.mark.parametrize("thr", [0.8, 0.5])
def test_table_pass_entries(thr, p_unknown):
    """pass is BITWISE 1.0 - o, or 0.0 where the value blocks; at 0.8 the pair 79 / 80 sits on either side"""
    _, p = capi.sense_mi_table(_cfg(thr), p_unknown)
    for v in range(-128, 128):
        o = p_unknown if v < 0 else min(v, 100) / 100.0
        want = 0.0 if sr.blocks(v, thr) else 1.0 - o
        assert p[v + 128].tobytes() == np.float64(want).tobytes(), (v, p[v + 128], want)
    if thr == 0.8:
        assert p[128 + 79] == 1.0 - 0.79 and p[128 + 79] > 0.0 and p[128 + 80].tobytes() == np.float64(0.0).tobytes()
    assert p[127] == 1.0 - p_unknown and p[0] == p[127]      # an unknown cell never blocks at these thresholds


def test_mi_symbols_and_argument_errors_do_not_need_a_device():
    """every argument error is raised before any HIP call: the pointers are never dereferenced, the engine neither"""
    L = capi.lib()
    for name in ("eea_sense_mi_table", "eea_sense_mi_field", "eea_set_target_mi"):
        assert name in capi.declared_symbols() and hasattr(L, name), name
    assert L.eea_abi_version() == 6
    one, two, eng = C.c_void_p(8), C.c_void_p(16), C.c_void_p(64)
    good = _cfg(0.8)
    ok = dict(e=eng, cfg=C.byref(good), R=5, stride=2, p=0.5, known=one, mi=two, floor=0.5, lx=2.2, ly=1.8)
    h, ps = np.zeros(256), np.zeros(256)

    def tab(**kw):
        a = dict(dict(cfg=C.byref(good), p=0.5, h=h.ctypes.data_as(C.c_void_p), ps=ps.ctypes.data_as(C.c_void_p)), **kw)
        return L.eea_sense_mi_table(a["cfg"], a["p"], a["h"], a["ps"])

    def field(**kw):
        a = dict(ok, **kw)
        return L.eea_sense_mi_field(0, a["cfg"], a["R"], a["stride"], a["p"], a["known"], a["mi"], None)

    def target(**kw):
        a = dict(ok, **kw)
        return L.eea_set_target_mi(a["e"], a["cfg"], a["R"], a["stride"], a["p"], a["known"], a["floor"], a["lx"], a["ly"], a["mi"],
                                   None)

    assert tab() == capi.OK and h[127] == LN2
    for name in ("cfg", "h", "ps"):
        assert tab(**{name: None}) == capi.ERR_INVALID_ARGUMENT and b"null" in L.eea_last_error(), name
    for name in ("cfg", "known", "mi"):
        assert field(**{name: None}) == capi.ERR_INVALID_ARGUMENT and b"null" in L.eea_last_error(), name
    for name in ("e", "cfg", "known"):
        assert target(**{name: None}) == capi.ERR_INVALID_ARGUMENT and b"null" in L.eea_last_error(), name
    for call in (tab, field, target):
        for bad in (0.0, 1.0, -0.1, float("nan"), float("inf")):
            assert call(p=bad) == capi.ERR_INVALID_ARGUMENT and b"p_unknown" in L.eea_last_error(), (call.__name__, bad)
    for call in (field, target):
        assert call(R=0) == capi.ERR_INVALID_ARGUMENT and b"range_cells" in L.eea_last_error()
        assert call(stride=0) == capi.ERR_INVALID_ARGUMENT and b"stride" in L.eea_last_error()
        assert call(R=1025) == capi.ERR_UNSUPPORTED and b"1024" in L.eea_last_error()
        for fld, bad, word in (("xsize", 0, b"xsize"), ("ysize", 0, b"xsize"), ("resolution", 0.0, b"resolution"),
                               ("resolution", float("nan"), b"resolution")):
            cfg = _cfg(0.8)
            setattr(cfg, fld, bad)
            assert call(cfg=C.byref(cfg)) == capi.ERR_INVALID_ARGUMENT, (fld, bad)
            assert word in L.eea_last_error()
    for bad in (-0.5, float("nan"), float("inf")):
        assert target(floor=bad) == capi.ERR_INVALID_ARGUMENT and b"floor" in L.eea_last_error(), bad
    for kw in (dict(lx=0.0), dict(ly=-1.0), dict(lx=float("nan"))):
        assert target(**kw) == capi.ERR_INVALID_ARGUMENT, kw
    big = capi.make_collision_cfg(0.0, 0.0, 0.1, 1 << 16, (1 << 15) + 1, 0.7, 0.1, 0.2, 0.8)
    assert target(cfg=C.byref(big)) == capi.ERR_UNSUPPORTED and b"2^31" in L.eea_last_error()
    assert target(mi=None, e=None) == capi.ERR_INVALID_ARGUMENT     # (d_mi is optional: the engine is what is missing)


def _measurement_entropy(cells, thr, p_unknown):
    """H(Z) of an ideal beam through `cells` (the values it crosses, in order), over ALL maps of those cells in exact
    probabilities: every cell is occupied independently with probability o(v); the beam ends on the first occupied cell, and
    on a blocking cell whatever its state (the hard stop), so Z is the index of the first occupied cell up to and including
    the first blocking one, or "none"."""
    n = len(cells)
    occ = [Fraction(p_unknown) if v < 0 else Fraction(min(v, 100), 100) for v in cells]
    stop = next((s for s, v in enumerate(cells) if sr.blocks(v, thr)), n - 1)
    dist = {}
    for m in range(1 << n):
        prob, z = Fraction(1), None
        for s in range(n):
            full = (m >> s) & 1
            prob *= occ[s] if full else 1 - occ[s]
            if z is None and full and s <= stop:
                z = s
        dist[z] = dist.get(z, Fraction(0)) + prob
    assert sum(dist.values()) == 1
    return sum(-_num(pz) * _ln(pz) for pz in dist.values() if pz > 0)


@pytest.mark.parametrize("p_unknown", [0.5, 0.2])
@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_restatement_is_the_mutual_information(R, p_unknown):
    """a cluttered 17 x 13 grid of unknown, free, 12, 30, 50, 79, 80 and 100 cells: every beam of a few candidates equals H(Z)
    of its cells within (n + 4) 2^-53 relative, n the beam's steps: n sums and n products in sequence, and the table"""
    rng = np.random.default_rng(60 + R)
    g = sr.Geometry(0.0, 0.0, 0.1, 17, 13, 0.8)
    known = rng.choice(np.array([-1, -1, 0, 0, 12, 30, 50, 79, 80, 100], dtype=np.int8), size=(13, 17))
    h, pass_ = mr.table(g, p_unknown)
    cells = known.tolist()
    rays = [[(int(dx), int(dy)) for dx, dy in ray] for ray in sr.ray_offsets(R)]
    beams, worst = 0, -math.inf
    for i0, j0 in ((0, 0), (6, 8), (12, 16), (5, 3), (9, 11)):
        for ray in rays:
            value, crossed = mr.beam(g, R, cells, h, pass_, i0, j0, ray)
            if not crossed:
                assert value == 0.0
                continue
            want = _measurement_entropy(crossed, g.occupied_threshold, p_unknown)
            n = len(crossed)
            if want == 0:
                assert value == 0.0, (i0, j0, crossed)
                continue
            rel = float(abs(_num(Fraction(value)) - want) / want)
            worst = max(worst, rel / EPS - n)
            assert rel <= (n + 4) * EPS, (i0, j0, crossed, value, float(want), rel / EPS)
            beams += 1
    print("R = %d, p_unknown %.1f: %d beams, worst relative error n + %.2f units of 2^-53" % (R, p_unknown, beams, worst))
    assert beams > 8 * R
    # the field the other tests use is these beams, candidate by candidate: the same bits
    for stride in (1, 3):
        a, b = mr.mi_field(g, R, stride, known, h, pass_), mr.mi_field_loops(g, R, stride, known, h, pass_)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and (a > 0).any()


@pytest.mark.parametrize("R", [1, 2, 5, 8])
def test_unknown_world_has_the_closed_form(R):
    """all unknown at p_unknown = 0.5: every cell is a fair coin, a beam of n steps is worth ln 2 (2 - 2^(1 - n)), so a
    candidate at least R from the edges gets ln 2 (1 + sum_q (2 - 2^(1 - n_q))), n_q the steps of ray q inside the disc; within
    (N + 4) 2^-53 relative, N the number of summed terms"""
    n_q = [sum(1 for k in range(len(ray)) if all(x * x + y * y <= R * R for x, y in ray[:k + 1])) for ray in sr.ray_offsets(R)]
    want = _ln(Fraction(2)) * _num(1 + sum(2 - Fraction(2) ** (1 - n) for n in n_q))
    N = 1 + sum(n_q)
    n = 2 * R + 4
    g = sr.Geometry(0.0, 0.0, 0.1, n + 1, n, 0.8)
    h, pass_ = mr.table(g, 0.5)
    mi = mr.mi_field(g, R, 1, np.full((n, n + 1), -1, dtype=np.int8), h, pass_)
    inner = mi[R:n - R, R:n + 1 - R]
    assert inner.size >= 4 and (inner == inner[0, 0]).all()
    rel = float(abs(_num(Fraction(float(inner[0, 0]))) - want) / want)
    print("R = %d: %d terms, relative error %.2f units of 2^-53" % (R, N, rel / EPS))
    assert rel <= (N + 4) * EPS
    assert 0.0 < mi[0, 0] < inner[0, 0] and mi.max() == inner[0, 0] <= LN2 * (8 * R * R + 1)


def _three_valued(xs, ys, seed):
    rng = np.random.default_rng(seed)
    blocks = rng.choice(np.array([-1, 0, 100], dtype=np.int8), size=(ys // 2 + 1, xs // 3 + 1), p=[0.35, 0.5, 0.15])
    return np.ascontiguousarray(np.kron(blocks, np.ones((2, 3), dtype=np.int8))[:ys, :xs])


def test_known_grid_is_plus_zero():
    """a grid of only 0 and 100 holds nothing to learn: +0.0 everywhere, the bit pattern included"""
    g = sr.Geometry(0.0, 0.0, 0.1, 23, 19, 0.8)
    known = np.where(_three_valued(23, 19, 3) < 0, 0, _three_valued(23, 19, 3)).astype(np.int8)
    assert (known == 100).any() and (known == 0).any()
    h, pass_ = mr.table(g, 0.5)
    for stride in (1, 2):
        assert (mr.mi_field(g, 4, stride, known, h, pass_).view(np.uint64) == 0).all()


@pytest.mark.parametrize("p_unknown", [0.5, 0.2])
@pytest.mark.parametrize("xs,ys,R,stride", [(23, 19, 3, 1), (31, 17, 6, 2)])
def test_zero_set_and_bound_of_the_gain_count(xs, ys, R, stride, p_unknown):
    """values -1, 0 and 100 only: a term is positive exactly where the count counts a cell, so mi > 0 exactly where the gain is,
    and every counted cell is worth at most ln 2: mi <= ln 2 gain (1 + 2^-50)"""
    g = sr.Geometry(0.0, 0.0, 0.1, xs, ys, 0.8)
    known = _three_valued(xs, ys, xs)
    h, pass_ = mr.table(g, p_unknown)
    mi, gain = mr.mi_field(g, R, stride, known, h, pass_), gr.gain_field(g, R, stride, known)
    assert (gain > 0).any() and (gain[::stride, ::stride] == 0).any()
    assert np.array_equal(mi > 0, gain > 0)
    assert (mi <= LN2 * gain * (1 + 2.0 ** -50)).all()


def test_unknown_cells_behind_unknown_cells_are_discounted():
    """what the count lacks.  One row, R = 2: only the rays due east and due west stay on the grid, two steps each.  A robot
    between two unknown cells and a robot facing two unknown cells in a row have the same gain count, 2; the first expects
    2 ln 2, the second ln 2 (1 + 1/2): the far cell is seen only if the near one is free"""
    g = sr.Geometry(0.0, 0.0, 0.1, 5, 1, 0.8)
    beside = np.array([[0, -1, 0, -1, 0]], dtype=np.int8)
    in_a_row = np.array([[0, 0, 0, -1, -1]], dtype=np.int8)
    h, pass_ = mr.table(g, 0.5)
    assert gr.gain_field(g, 2, 1, beside)[0, 2] == gr.gain_field(g, 2, 1, in_a_row)[0, 2] == 2
    a, b = mr.mi_field(g, 2, 1, beside, h, pass_)[0, 2], mr.mi_field(g, 2, 1, in_a_row, h, pass_)[0, 2]
    assert a > b > 0.0
    assert a == 2 * LN2 and b == 1.5 * LN2
    # ... and behind a cell that is probably occupied there is little left: 0.79 in front of the unknown cell
    graded = np.array([[0, 0, 0, 79, -1]], dtype=np.int8)
    c = mr.mi_field(g, 2, 1, graded, h, pass_)[0, 2]
    assert c == h[128 + 79] + (1.0 - 0.79) * LN2


@pytest.mark.parametrize("stride", [2, 3, 5, 64])
def test_stride_keeps_the_lattice_values(stride):
    g, known = ms.graded(40, 30)
    h, pass_ = mr.table(g, 0.2)
    one, lat = mr.mi_field(g, 5, 1, known, h, pass_), mr.mi_field(g, 5, stride, known, h, pass_)
    on = np.zeros_like(one, dtype=bool)
    on[::stride, ::stride] = True
    assert (lat[~on].view(np.uint64) == 0).all() and np.array_equal(lat[on].view(np.uint64), one[on].view(np.uint64))
    assert lat[0, 0] == one[0, 0] and (one > 0).any()


def test_graded_scene_has_what_it_promises():
    for xs, ys in ((23, 19), (64, 41)):
        g, known = ms.graded(xs, ys)
        flat = known.reshape(-1)
        assert (flat == 127).sum() == 1 and (flat == -128).sum() == 1
        assert ((known[:, :-1] == 79) & (known[:, 1:] == 80)).any()
        assert len(set(flat.tolist()) & set(range(1, 100))) >= 40 and (flat == -1).any() and (flat == 100).any()


def test_value_grid():
    g, known = ms.graded(23, 19)
    h, pass_ = mr.table(g, 0.5)
    mi = mr.mi_field(g, 3, 2, known, h, pass_)
    v = mr.value_grid(g, 2, known, mi, 0.25)
    on = np.zeros_like(known, dtype=bool)
    on[::2, ::2] = True
    free = on & (known < 80)
    assert (v[~free] == 0).all() and np.array_equal(v[free], mi[free] + 0.25) and (known[on] >= 80).any()
    assert mr.value_grid(g, 2, known, mi, 0.25, np.float32).dtype == np.float32


def test_mi_kernels_are_in_the_library():
    """the kernels of csrc/mi_kernel.hip are gfx950 code in the build and use no scratch; the table and the window are LDS
    sized per launch, none of it static (the table sits at the 16-byte aligned base)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    obj = os.path.join(os.path.dirname(capi.LIB_PATH), "..", "csrc", "build", "mi_kernel.o")
    names = {}
    for k in kr.kernels(obj):
        if "vgpr_count" in k:
            names[subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.strip()] = k
    for w in ("mi_field_lds_kernel(", "mi_field_global_kernel(", "mi_values_kernel<double>(", "mi_values_kernel<float>("):
        found = [k for n, k in names.items() if w in n]
        assert len(found) == 1, (w, sorted(names))
        assert int(found[0]["private_segment_fixed_size"]) == 0, found[0]
        assert int(found[0]["group_segment_fixed_size"]) == 0, found[0]


def test_host_wrapper_has_the_mi_calls(tmp_path):
    """host/include/ergodic_exploration/sensing.hpp: senseMiTable, senseMiField and setTargetMi compile against the C header"""
    src = tmp_path / "use.cpp"
    src.write_text("#include <ergodic_exploration/sensing.hpp>\n"
                   "void use(eea_engine* e, const eea_collision_cfg& cfg, const int8_t* known, double* mi, double* h, double* p)\n"
                   "{ ergodic_exploration::senseMiTable(cfg, 0.5, h, p);\n"
                   "  ergodic_exploration::senseMiField(cfg, 50u, 4u, 0.5, known, mi);\n"
                   "  ergodic_exploration::senseMiField(cfg, 50u, 4u, 0.5, known, mi, nullptr);\n"
                   "  ergodic_exploration::setTargetMi(e, cfg, 50u, 4u, 0.5, known, 0.25, 10.0, 5.0);\n"
                   "  ergodic_exploration::setTargetMi(e, cfg, 50u, 4u, 0.5, known, 0.25, 10.0, 5.0, mi, nullptr); }\n"
                   "int main() { return 0; }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROOT, "ergodic_exploration_amd", "host", "include"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(os.environ.get("ROCM", "/opt/rocm"), "include"), str(src)], check=True)

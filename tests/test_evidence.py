"""CPU checks of the evidence grid (include/ergodic_amd.h: eea_evidence_table, eea_sense_observe_batch, eea_evidence_publish;
csrc/evidence_kernel.hip): the numpy restatement tests/evidence_restatement.py against an independent statement written from
the contract's closed forms, its independence of the robots' order, the library's table against 50-digit decimals, the noise
stream, the argument checks of the C ABI that need no device, the probabilities the published grid holds, the host mirror's
sensor model, and the kernels' presence in the gfx950 build."""
import ctypes as C
import decimal
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from ergodic_exploration_amd import capi
from tests import evidence_restatement as er
from tests import sense_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISY = er.Evidence(25, 7, 1024, er.QUANTUM, 1 << 30, (1 << 32) // 20, 0xDEADBEEF, 0x0BADF00D)


def _centre(g, i, j):
    return [g.xmin + (j + 0.5) * g.resolution, g.ymin + (i + 0.5) * g.resolution, 0.0]


def _philox_ints(c, k):
    """Philox4x32-10 once more, in Python integers (Salmon et al., SC'11: two 32 x 32 -> 64 bit products per round)"""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def _brute_observe(g, ev, R, scan, robot0, truth, evid, poses):
    """the contract of ergodic_amd.h once more, on its own: targets by walking the square's perimeter, steps by rounding
    s |m| / R in exact fractions, the robot's cell by a plain floor, the noise word of a cell from the scalar Philox above,
    the evidence kept in Python integers"""
    half_up = lambda fr: math.floor(fr + Fraction(1, 2))
    perimeter = ([(R, -R + k) for k in range(2 * R)] + [(R - k, R) for k in range(2 * R)] +
                 [(-R, R - k) for k in range(2 * R)] + [(-R + k, -R) for k in range(2 * R)])
    ranges = np.full((len(poses), 8 * R), -1, dtype=np.int32)
    total = [[int(v) for v in row] for row in evid]
    for b, (x, y, _) in enumerate(poses):
        j0 = int(np.floor((x - g.xmin) / g.resolution))
        i0 = int(np.floor((y - g.ymin) / g.resolution))
        j0 -= 1 if j0 == g.xsize else 0
        i0 -= 1 if i0 == g.ysize else 0
        if not (0 <= i0 < g.ysize and 0 <= j0 < g.xsize):
            continue

        def appears(i, j):
            r = _philox_ints((j >> 2, i, robot0 + b, scan), (ev.seed_lo, ev.seed_hi))[j & 3]
            if not (np.float64(truth[i, j]) / np.float64(100.0) < np.float64(g.occupied_threshold)):
                return not (r < ev.thr_miss)
            return r < ev.thr_false

        hit_cells, touched = set(), {(i0, j0)}
        for q, (tx, ty) in enumerate(perimeter):
            for s in range(1, R + 1):
                dx = int(np.sign(tx)) * half_up(Fraction(s * abs(tx), R))
                dy = int(np.sign(ty)) * half_up(Fraction(s * abs(ty), R))
                if dx * dx + dy * dy > R * R or not (0 <= i0 + dy < g.ysize and 0 <= j0 + dx < g.xsize):
                    break
                touched.add((i0 + dy, j0 + dx))
                if appears(i0 + dy, j0 + dx):
                    hit_cells.add((i0 + dy, j0 + dx))
                    ranges[b, q] = s
                    break
        for (i, j) in touched:
            total[i][j] += ev.w_occ if (i, j) in hit_cells else -ev.w_free
    return np.array(total, dtype=np.int64), ranges


def _scene_13x9():
    g = sr.Geometry(0.0, 0.0, 0.1, 13, 9, 0.8)
    rng = np.random.default_rng(139)
    truth = rng.choice(np.array([0, 0, 0, 0, 0, 100, 100, -1, 79, 80], dtype=np.int8), size=(9, 13))
    poses = [_centre(g, 4, 6), _centre(g, 0, 0), _centre(g, 8, 12), _centre(g, 3, 11), [0.31, 0.27, 1.0], [-0.5, 0.4, 0.0],
             [1.3, 0.55, 0.0], [0.65, 0.9, 0.0], _centre(g, 4, 6)]
    return g, truth, poses


@pytest.mark.parametrize("R", [1, 2, 5])
def test_restatement_is_the_independent_statement(R):
    """a 13 x 9 grid with clutter, robots in the open, in the corners, on xmax / ymax, off the grid and two in one cell, a
    noisy sensor, two scans on top of one another from robot0 = 3: evidence and ranges are equal"""
    g, truth, poses = _scene_13x9()
    evid = np.zeros((9, 13), dtype=np.int32)
    brute = evid.astype(np.int64)
    flipped = False
    for scan in (0, 7):
        r1 = er.observe(g, NOISY, R, scan, 3, truth, evid, poses)
        brute, r2 = _brute_observe(g, NOISY, R, scan, 3, truth, brute, poses)
        assert np.array_equal(evid.astype(np.int64), brute) and np.array_equal(r1, r2)
        ideal = sr.reveal(g, R, truth, np.zeros_like(truth), poses)
        flipped = flipped or not np.array_equal(ideal, r1)
    assert (evid > 0).any() and (evid < 0).any()
    assert R == 1 or flipped                       # the noise did change what the rays met


def test_restatement_does_not_depend_on_the_order_of_the_robots():
    g, truth, poses = _scene_13x9()
    rng = np.random.default_rng(5)
    want = np.zeros((9, 13), dtype=np.int32)
    want_ranges = er.observe(g, NOISY, 5, 2, 0, truth, want, poses)
    for _ in range(3):
        order = rng.permutation(len(poses)).tolist()
        evid = np.zeros((9, 13), dtype=np.int32)
        ranges = er.observe(g, NOISY, 5, 2, 0, truth, evid, poses, order=order)
        assert np.array_equal(evid, want) and np.array_equal(ranges, want_ranges), order
    # ... and an int32 that wraps does so as two's complement, in either order
    hi = np.full((9, 13), 2 ** 31 - 3, dtype=np.int32)
    er.observe(g, er.Evidence(25, 7, 1024, er.QUANTUM, 0, 0, 0, 0), 2, 0, 0, np.full((9, 13), 100, np.int8), hi, poses[:1])
    assert int(hi.min()) == -2 ** 31 + 25 - 3 and int(hi[4, 6]) == 2 ** 31 - 3 - 7


def test_table_against_fifty_digits():
    """all 2049 entries of eea_evidence_table at quantum = 0.0884341726294605, e_clip = 1024 against 100 sigma(e quantum)
    in 50-digit decimals.  First: no exact value lies within 1e-3 of a rounding tie (measured: the nearest is 3.9e-3 away), so
    the comparison depends on nobody's libm -- an exp that is off by many ulps moves 100 sigma by 1e-13"""
    ctx = decimal.Context(prec=50)
    q = decimal.Decimal(er.QUANTUM)               # the double, exactly
    ecfg = capi.EvidenceCfg(25, 7, 1024, er.QUANTUM, 0, 0, 0, 0)
    got = capi.evidence_table(ecfg)
    assert got.dtype == np.int8 and got.shape == (2049,)
    want, nearest = [], None
    for e in range(-1024, 1025):
        ex = ctx.exp(ctx.multiply(decimal.Decimal(e), q))
        v = ctx.multiply(decimal.Decimal(100), ctx.divide(ex, ctx.add(decimal.Decimal(1), ex)))
        frac = v - v.to_integral_value(rounding=decimal.ROUND_FLOOR)
        gap = abs(frac - decimal.Decimal("0.5"))
        nearest = gap if nearest is None else min(nearest, gap)
        want.append(min(max(int((v + decimal.Decimal("0.5")).to_integral_value(rounding=decimal.ROUND_FLOOR)), 1), 99))
    print("nearest rounding tie: %.3e" % float(nearest))
    assert nearest > decimal.Decimal("1e-3")
    assert got.tolist() == want
    assert np.array_equal(er.table(er.Evidence(25, 7, 1024, er.QUANTUM, 0, 0, 0, 0)), got)
    assert (np.diff(got.astype(np.int64)) >= 0).all() and got[0] == 1 and got[-1] == 99
    assert got[1024 - 7] == 35 and got[1024 + 25] == 90
    # a small table, and a quantum so large that exp overflows: 1 | 50 | 99
    small = capi.evidence_table(capi.EvidenceCfg(1, 1, 1, 1.0e6, 0, 0, 0, 0))
    assert small.tolist() == [1, 50, 99] == er.table(er.Evidence(1, 1, 1, 1.0e6, 0, 0, 0, 0)).tolist()


def test_noise_stream():
    """4096 draws at thr = 2^31: five standard deviations of a fair coin over 4096 draws are 0.039, so the share below the
    threshold lies in 0.5 +- 0.04 -- per robot, per scan, and per word of the four a call yields; at thr = 0 nothing flips"""
    g = sr.Geometry(0.0, 0.0, 0.1, 64, 64, 0.8)
    ev = er.Evidence(25, 7, 1024, er.QUANTUM, 1 << 31, 1 << 31, 0xDEADBEEF, 0x0BADF00D)
    words = er.noise_words(g, ev, [0, 1, 70000], 3)
    assert words.shape == (3, 64, 64) and int(words.max()) < 2 ** 32
    for b in range(3):
        share = float((words[b] < np.uint64(1 << 31)).mean())
        assert abs(share - 0.5) < 0.04, (b, share)
    assert not np.array_equal(words[0], words[1]) and not np.array_equal(words[0], er.noise_words(g, ev, [0], 4)[0])
    # the word of cell (i, j) is word j & 3 at the counter (j >> 2, i, robot, scan): spot checks against the scalar Philox
    for b, robot in enumerate((0, 1, 70000)):
        for i, j in ((0, 0), (5, 3), (5, 4), (63, 62), (17, 41)):
            assert int(words[b, i, j]) == _philox_ints((j >> 2, i, robot, 3), (ev.seed_lo, ev.seed_hi))[j & 3]
    truth = np.random.default_rng(1).choice(np.array([0, 100, -1, 79, 80], dtype=np.int8), size=(64, 64))
    half = er.appears_blocking(g, ev, truth, [9], 0)[0]
    blocking = ~(truth.astype(np.float64) / 100.0 < 0.8)
    for cells in (blocking, ~blocking):            # (five standard deviations of a fair coin over the cells of each kind)
        assert abs(float(half[cells].mean()) - 0.5) < 2.5 / math.sqrt(int(cells.sum()))
    quiet = er.appears_blocking(g, ev._replace(thr_miss=0, thr_false=0), truth, [9], 0)[0]
    assert np.array_equal(quiet, blocking)


def test_evidence_symbols_and_argument_errors_do_not_need_a_device():
    """every refusal of the three entries is raised before any HIP call"""
    L = capi.lib()
    for name in ("eea_evidence_table", "eea_sense_observe_batch", "eea_evidence_publish"):
        assert name in capi.declared_symbols() and hasattr(L, name), name
    assert L.eea_abi_version() == 6
    one, two = C.c_void_p(8), C.c_void_p(16)   # never dereferenced: the argument checks come first
    good = capi.make_collision_cfg(0.0, 0.0, 0.1, 23, 19, 0.7, 0.1, 0.2, 0.8)   # (radii Collision::Collision would refuse)
    egood = capi.EvidenceCfg(25, 7, 1024, er.QUANTUM, 1, 2, 3, 4)
    ok = dict(cfg=C.byref(good), ecfg=C.byref(egood), R=5, truth=one, evid=two, pose=one, known=one, P=3)

    def observe(**kw):
        a = dict(ok, **kw)
        return L.eea_sense_observe_batch(0, a["cfg"], a["ecfg"], a["R"], 0, 0, a["truth"], a["evid"], a["pose"], None, a["P"], None,
                                         None)

    def publish(**kw):
        a = dict(ok, **kw)
        return L.eea_evidence_publish(0, a["cfg"], a["ecfg"], a["evid"], a["known"], None, None)

    for name in ("cfg", "ecfg", "truth", "evid", "pose"):
        assert observe(**{name: None}) == capi.ERR_INVALID_ARGUMENT, name
        assert b"null" in L.eea_last_error()
    for name in ("cfg", "ecfg", "evid", "known"):
        assert publish(**{name: None}) == capi.ERR_INVALID_ARGUMENT, name
        assert b"null" in L.eea_last_error()
    table = np.zeros(2049, dtype=np.int8)
    assert L.eea_evidence_table(None, table.ctypes.data_as(C.c_void_p)) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_evidence_table(C.byref(egood), None) == capi.ERR_INVALID_ARGUMENT and b"null" in L.eea_last_error()
    assert observe(R=0) == capi.ERR_INVALID_ARGUMENT and b"range_cells" in L.eea_last_error()
    assert observe(R=128) == capi.ERR_UNSUPPORTED and b"127" in L.eea_last_error()
    assert observe(R=128, P=0) == capi.ERR_UNSUPPORTED
    assert observe(R=127, P=0) == capi.OK          # nothing to do: nothing launched, no device needed
    for field, bad, word in (("xsize", 0, b"xsize"), ("ysize", 0, b"xsize"), ("resolution", 0.0, b"resolution"),
                             ("resolution", -0.1, b"resolution"), ("resolution", float("nan"), b"resolution")):
        cfg = capi.make_collision_cfg(0.0, 0.0, 0.1, 23, 19, 0.7, 1.0, 0.2, 0.8)
        setattr(cfg, field, bad)
        assert observe(cfg=C.byref(cfg)) == capi.ERR_INVALID_ARGUMENT, (field, bad)
        assert word in L.eea_last_error()
        assert publish(cfg=C.byref(cfg)) == capi.ERR_INVALID_ARGUMENT, (field, bad)
        assert word in L.eea_last_error()
    for field, bad, word in (("w_occ", 0, b"w_occ"), ("w_occ", 32768, b"w_occ"), ("w_occ", -1, b"w_occ"), ("w_free", 0, b"w_free"),
                             ("w_free", 32768, b"w_free"), ("e_clip", 0, b"e_clip"), ("e_clip", 1025, b"e_clip"),
                             ("e_clip", -5, b"e_clip"), ("quantum", 0.0, b"quantum"), ("quantum", -1.0, b"quantum"),
                             ("quantum", float("inf"), b"quantum"), ("quantum", float("nan"), b"quantum")):
        ecfg = capi.EvidenceCfg(25, 7, 1024, er.QUANTUM, 1, 2, 3, 4)
        setattr(ecfg, field, bad)
        for call in (lambda: observe(ecfg=C.byref(ecfg)), lambda: publish(ecfg=C.byref(ecfg)),
                     lambda: L.eea_evidence_table(C.byref(ecfg), table.ctypes.data_as(C.c_void_p))):
            assert call() == capi.ERR_INVALID_ARGUMENT, (field, bad)
            assert word in L.eea_last_error()
    assert (table == 0).all()                       # no refused call wrote the table
    for w in (1, 32767):
        edge = capi.EvidenceCfg(w, w, 1, 1e-300, 0, 0xFFFFFFFF, 0, 0)
        assert observe(ecfg=C.byref(edge), P=0) == capi.OK
    with pytest.raises(capi.EngineError) as ei:
        capi.evidence_table(capi.EvidenceCfg(25, 7, 2000000000, er.QUANTUM, 0, 0, 0, 0))
    assert ei.value.status == capi.ERR_INVALID_ARGUMENT


def test_published_join_scene_holds_probabilities():
    """the scene of the GPU join test, by the restatement alone: the published grid holds values strictly between 1 and 99
    other than one miss (35) and one hit (90) -- the probability path of eea_sense_mi_field is fed -- and unknown cells"""
    g, ev, R, truth, poses, evid = er.join_scene()
    known = er.publish(ev, evid)
    assert known.shape == (40, 48) and known.dtype == np.int8
    inner = known[(known > 1) & (known < 99)]
    others = sorted(set(int(v) for v in inner) - {35, 90})
    print("published values strictly inside (1, 99) other than 35 and 90:", others)
    assert len(others) >= 3
    assert (known == -1).any() and (known >= 80).any() and ((known >= 1) & (known < 80)).any()
    assert np.array_equal(known == -1, evid == 0)
    # hand-made evidence: the clamp is applied at publication only
    e = np.array([[-2 ** 31, -1025, -1024, -7, -1, 0, 1, 25, 1024, 1025, 2 ** 31 - 1]], dtype=np.int32)
    tab = er.table(ev)
    assert er.publish(ev, e).tolist() == [[1, 1, 1, 35, int(tab[1023]), -1, int(tab[1025]), 90, 99, 99, 99]]


def test_host_mirror_evidence_model(tmp_path):
    """host/include/ergodic_exploration/sensing.hpp: EvidenceModel::fromProbabilities(0.90, 0.35, 7, 1024) is (25, 7) units of
    quantum 0.0884341726294605 (a log, a quotient and a division in doubles: a few ulps at the most between libms), and the
    wrappers compile against the C header"""
    include = ["-I", os.path.join(ROOT, "ergodic_exploration_amd", "host", "include"), "-I", os.path.join(ROOT, "include"),
               "-I", os.path.join(os.environ.get("ROCM", "/opt/rocm"), "include")]
    use = tmp_path / "use.cpp"
    use.write_text("#include <ergodic_exploration/sensing.hpp>\n"
                   "void use(const eea_collision_cfg& cfg, const ergodic_exploration::EvidenceModel& m, const int8_t* truth,\n"
                   "         int32_t* evid, int8_t* known, const double* pose, int* ranges, const int* mask,\n"
                   "         unsigned long long* counts, int8_t* table)\n"
                   "{ ergodic_exploration::senseObserve(cfg, m, 50u, 3u, truth, evid, pose, 4096u);\n"
                   "  ergodic_exploration::senseObserve(cfg, m, 50u, 3u, truth, evid, pose, 4096u, 8192u, ranges, mask, nullptr);\n"
                   "  ergodic_exploration::evidencePublish(cfg, m, evid, known);\n"
                   "  ergodic_exploration::evidencePublish(cfg, m, evid, known, counts, nullptr);\n"
                   "  ergodic_exploration::evidenceTable(m, table); }\n"
                   "int main() { return 0; }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__"] + include + [str(use)],
                   check=True)
    # the model itself is host arithmetic: a program that calls nothing of the library, so it links against nothing
    src = tmp_path / "model.cpp"
    src.write_text("#include <cstdio>\n#include <ergodic_exploration/sensing.hpp>\n"
                   "int main() {\n"
                   "  const ergodic_exploration::EvidenceModel m = ergodic_exploration::EvidenceModel::fromProbabilities(0.90, 0.35, 7, 1024);\n"
                   "  std::printf(\"%d %d %d %.17g %u %u\\n\", m.cfg.w_occ, m.cfg.w_free, m.cfg.e_clip, m.cfg.quantum, m.cfg.thr_miss,\n"
                   "              m.cfg.thr_false);\n  return 0; }\n")
    exe = tmp_path / "model"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__"] + include + [str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out[:3]] == [25, 7, 1024] and [int(v) for v in out[4:]] == [0, 0]
    assert abs(float(out[3]) - er.QUANTUM) <= 4 * math.ulp(er.QUANTUM), out[3]


def test_evidence_kernels_are_in_the_library():
    """the kernels of csrc/evidence_kernel.hip are gfx950 code in the build and use no scratch (the publish launch's table is
    read from the kernel arguments, not copied to private memory); the observe kernel's LDS is sized per launch"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    obj = os.path.join(os.path.dirname(capi.LIB_PATH), "..", "csrc", "build", "evidence_kernel.o")
    names = {}
    for k in kr.kernels(obj):
        if "vgpr_count" in k:
            names[subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.strip()] = k
    for w in ("evidence_observe_kernel", "evidence_publish_kernel"):
        found = [k for n, k in names.items() if w + "(" in n]
        assert len(found) == 1, (w, sorted(names))
        assert int(found[0]["private_segment_fixed_size"]) == 0, found[0]
        if w == "evidence_observe_kernel":
            assert int(found[0]["group_segment_fixed_size"]) == 0, found[0]

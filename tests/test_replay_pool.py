"""CPU checks of the pooled replay memory (include/ergodic_amd.h, eea_replay_pool_sample): the entry is declared, exported and
bound; the numpy restatement tests/pool_restatement.py -- what tests/test_gpu_replay_pool.py holds the kernels to, bitwise --
against a brute-force pool (the stores concatenated, the robot's own segment deleted), its uniformity, the separation of its
random stream from the own-memory draws, and the argument checks of the C ABI that need no device."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

from ergodic_exploration_amd import capi
from tests import pool_restatement as pr
from tests import replay_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "eea_replay_pool_sample"


def test_entry_is_declared_exported_and_bound():
    assert ENTRY in capi.declared_symbols()
    with open(os.path.join(ROOT, "ergodic_exploration_amd", "csrc", "exports.map")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    exported = re.search(r"global:(.*?)local:", text, flags=re.S).group(1)
    patterns = [p.strip() for p in exported.split(";") if p.strip()]
    assert any(fnmatch.fnmatchcase(ENTRY, p) for p in patterns), patterns
    fn = getattr(capi.lib(), ENTRY)                       # in the built library ...
    assert fn.argtypes is not None and len(fn.argtypes) == 9   # ... and bound with its nine arguments
    assert callable(getattr(capi.ReplayMemory, "sample_pool"))
    assert capi.lib().eea_abi_version() == 6              # additive: the version stays


def _filled(counts, capacity, seed=1, robot0=0, dtype=np.float64):
    """a restated memory whose pose in (robot q, slot i) is (q, i, 0.25): a column names where it came from"""
    m = rr.ReplayMemory(len(counts), capacity, 1, seed=seed, robot0=robot0, dtype=dtype)
    for q, n in enumerate(counts):
        m.store[q, :n, 0], m.store[q, :n, 1], m.store[q, :n, 2] = q, np.arange(n), 0.25
    m.count[:] = counts
    return m


def _brute_force(m, b, draw, n_cols, exclude_self):
    """the columns of robot b from the pool as an ARRAY: the stores concatenated, the robot's own segment deleted, the draw
    in Python integers"""
    parts = [m.store[q, :m.count[q]] for q in range(m.B) if not (exclude_self and q == b)]
    pool = np.concatenate(parts) if parts else np.zeros((0, 3))
    n_pool = len(pool)
    if n_pool <= n_cols:
        return pool
    r64 = pr.pool_r64(m.seed, draw, [m.robot0 + b], n_cols)[0]
    return pool[[(int(r) * n_pool) >> 64 for r in r64]]


RAGGED = [0, 0, 5, 1, 0, 0, 0, 7, 2, 0, 9, 0, 0]   # empty robots in front, in runs in the middle, at the end: N = 24


@pytest.mark.parametrize("exclude_self", [False, True])
def test_restatement_equals_the_brute_force_pool(exclude_self):
    """ragged counts; n_cols runs through every regime for every robot: N_b < n_cols, N_b == n_cols, N_b == n_cols + 1 (N_b is
    24 without exclusion, 24 - n_b in {24, 19, 23, 17, 22, 15} with it) and far fewer columns than poses"""
    m = _filled(RAGGED, capacity=9, seed=0xabcdef0123456789, robot0=3)
    n_b = {24 - (c if exclude_self else 0) for c in RAGGED}
    tried = set()
    for n_cols in (1, 4, 14, 15, 16, 17, 18, 19, 21, 22, 23, 24, 25, 40):
        for draw in (0, 7 + 2**33):
            cols, n_mem = np.full((m.B, n_cols + 2, 3), -7.0), np.full(m.B, -1)
            pr.sample_pool(m, draw, n_cols, cols, n_mem, exclude_self=exclude_self)
            for b in range(m.B):
                want = _brute_force(m, b, draw, n_cols, exclude_self)
                assert n_mem[b] == len(want) == min(24 - (RAGGED[b] if exclude_self else 0), n_cols)
                assert np.array_equal(cols[b, :len(want)], want), (n_cols, draw, b)
                assert (cols[b, len(want):] == -7.0).all()
                assert not exclude_self or not (want[:, 0] == b).any()         # never one of its own poses
                assert (np.asarray(RAGGED)[want[:, 0].astype(int)] > want[:, 1]).all()   # a stored slot of a non-empty robot
        tried |= {n - n_cols for n in n_b}
    assert {0, 1} <= tried                               # N_b == n_cols and N_b == n_cols + 1 were met


def test_restatement_at_an_empty_pool():
    """N_b == 0: nobody has a pose; and the fleet whose only non-empty robot is the one that leaves itself out"""
    for counts, exclude_self, want in (([0, 0, 0], False, [0, 0, 0]), ([0, 0, 0], True, [0, 0, 0]),
                                       ([0, 6, 0], True, [4, 0, 4]), ([0, 6, 0], False, [4, 4, 4]), ([6], True, [0])):
        m = _filled(counts, capacity=8)
        cols, n_mem = np.full((m.B, 4, 3), -7.0), np.full(m.B, -1)
        pr.sample_pool(m, 3, 4, cols, n_mem, exclude_self=exclude_self)
        assert n_mem.tolist() == want, (counts, exclude_self)
        for b in range(m.B):
            assert (cols[b, n_mem[b]:] == -7.0).all() and (cols[b, :n_mem[b], 0] == 1).all()


def test_restatement_accumulates_behind_what_the_row_holds():
    m = _filled(RAGGED, capacity=9, seed=5)
    plain, n_plain = np.full((m.B, 6, 3), -7.0), np.zeros(m.B, dtype=np.int64)
    pr.sample_pool(m, 2, 6, plain, n_plain)
    assert n_plain.tolist() == [6] * m.B
    cols, n_mem = np.full((m.B, 8, 3), -7.0), np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, -3, 2, 2])
    pr.sample_pool(m, 2, 6, cols, n_mem, accumulate=True)
    base = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0, 2, 2]
    assert n_mem.tolist() == [x + max(0, min(6, 8 - x)) for x in base]   # (a row that already holds 9 of 8 stays at 9)
    for b, x in enumerate(base):
        k = max(0, min(6, 8 - x))
        assert np.array_equal(cols[b, x:x + k], plain[b, :k]) and (cols[b, :min(x, 8)] == -7.0).all()


def test_mulhi_wide_is_exact():
    rng = np.random.default_rng(1)
    r = rng.integers(0, 2**64, 500, dtype=np.uint64)
    r[:4] = [0, 1, 2**64 - 1, 2**63]
    for n in (1, 2**32 - 1, 2**32, 2**32 + 1, 3 * 2**40 + 17, 2**63, 2**64 - 1):
        assert [int(x) for x in pr.mulhi64_wide(r, np.uint64(n))] == [(int(x) * n) >> 64 for x in r], n


def test_pooled_draws_are_uniform_over_the_pool():
    """B = 16 robots with counts uniform in [0, 128] (seed fixed: deterministic), 500 columns x 400 ticks = 2 x 10^5 draws per
    robot and regime: every pose of the robot's pool is hit draws / N_b times within 6 sigma (sigma^2 = draws p (1 - p),
    p = 1 / N_b: a binomial count), nothing outside the pool is ever hit"""
    rng = np.random.default_rng(2024)
    counts = rng.integers(0, 129, 16)
    counts[5] = 0
    B, cap, n_cols, ticks, off = 16, 128, 500, 400, pr.offsets(counts)
    draws = n_cols * ticks
    assert off[B] - counts.max() > n_cols                  # every robot draws, in both regimes
    stored = np.arange(cap)[None, :] < counts[:, None]
    for exclude_self in (False, True):
        hits = np.zeros((B, B, cap), dtype=np.int64)        # [viewing robot][owner][slot]
        for t in range(ticks):
            owner, slot, w = pr.pool_indices(counts, seed=77, robot0=40, draw=t * 2**20 + 3, n_cols=n_cols, exclude_self=exclude_self)
            assert (w == n_cols).all()
            np.add.at(hits, (np.arange(B)[:, None], owner, slot), 1)
        for b in range(B):
            in_pool = stored.copy()
            if exclude_self:
                in_pool[b] = False
            n_pool = int(in_pool.sum())
            assert n_pool == off[B] - (counts[b] if exclude_self else 0)
            assert hits[b][~in_pool].sum() == 0 and hits[b].sum() == draws
            p = 1.0 / n_pool
            worst = np.abs(hits[b][in_pool] - draws * p).max() / np.sqrt(draws * p * (1.0 - p))
            assert worst < 6.0, (exclude_self, b, worst)


def test_pooled_draws_are_not_the_own_memory_draws():
    """what the key xor buys: at equal (seed, draw, robot, column) the r64 of a pooled draw is not the r64 of the robot's own
    draw (rr.draw_indices: index = mulhi64(r64, n)) -- with one key both would sit at the same relative position of their pools"""
    for seed, draw in ((0, 0), (2020, 11), (0x9E3779B900000000, 3), (2**64 - 1, 2**40 + 5)):
        for robot in (0, 9, 4095):
            j = np.arange(100, dtype=np.uint64)
            o = rr.philox4x32_10((j, robot, draw & rr.MASK32, draw >> 32), (seed & rr.MASK32, seed >> 32))
            own = o[0] | (o[1] << np.uint64(32))
            assert np.array_equal(rr.mulhi64(own, 5000).astype(np.int64), rr.draw_indices(5000, 100, seed, draw, robot))
            pooled = pr.pool_r64(seed, draw, [robot], 100)[0]
            assert (pooled != own).all()
            assert not np.array_equal(rr.mulhi64(pooled, 5000), rr.mulhi64(own, 5000))


def test_pool_argument_errors_do_not_need_a_device():
    """every error is found before the handle is used: a live handle needs a device, so the handle here is only non-null"""
    L = capi.lib()
    fake, cols, n = C.create_string_buffer(256), np.full((2, 4, 3), -7.0), np.full(2, -1, dtype=np.int32)
    h, pc, pn = C.cast(fake, C.c_void_p), capi._ptr(cols), capi._ptr(n)
    for args, word in (((None, 0, 4, 0, 0, pc, pn, 4, None), b"null"), ((h, 0, 4, 0, 0, None, pn, 4, None), b"null"),
                       ((h, 0, 4, 0, 0, pc, None, 4, None), b"null"), ((h, 0, 0, 0, 0, pc, pn, 4, None), b"n_cols"),
                       ((h, 0, 0, 0, 1, pc, pn, 4, None), b"n_cols"), ((h, 0, 4, 0, 0, pc, pn, 3, None), b"mem_stride"),
                       ((h, 0, 4, 1, 0, pc, pn, 0, None), b"mem_stride"), ((h, 0, 4, 0, 1, pc, pn, 0, None), b"mem_stride")):
        assert L.eea_replay_pool_sample(*args) == capi.ERR_INVALID_ARGUMENT, args
        assert word in L.eea_last_error(), (args, L.eea_last_error())
    assert (cols == -7.0).all() and (n == -1).all() and fake.raw == bytes(256)


def test_pool_kernels_are_in_the_library():
    """the kernels behind the entry are gfx950 code in the build: the sampler with its 8 KB coarse table in LDS, no scratch
    and <= 64 registers (eight wavefronts per SIMD: a gather hides its latency with resident wavefronts), the one-workgroup
    scan with the 16 wavefront totals in LDS and no scratch"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    obj = os.path.join(os.path.dirname(capi.LIB_PATH), "..", "csrc", "build", "replay_kernel.o")
    names = {}
    for k in kr.kernels(obj):
        if "vgpr_count" in k:
            names[subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.strip()] = k
    sample = [k for n, k in names.items() if "pool_sample_kernel<" in n]
    scan = [k for n, k in names.items() if "pool_offsets_kernel(" in n]
    assert len(sample) == 2 and len(scan) == 1, sorted(names)   # fp64 / fp32
    for k in sample:
        assert int(k["vgpr_count"]) <= 64 and int(k["private_segment_fixed_size"]) == 0 and int(k["group_segment_fixed_size"]) == 8192, k
    assert int(scan[0]["vgpr_count"]) <= 64 and int(scan[0]["private_segment_fixed_size"]) == 0 and int(scan[0]["group_segment_fixed_size"]) == 128


def test_host_wrapper_has_sample_pool(tmp_path):
    """FleetReplayMemory::samplePool (host/include/ergodic_exploration/replay_memory.hpp) against the C header"""
    src = tmp_path / "use.cpp"
    src.write_text("#include <ergodic_exploration/replay_memory.hpp>\n"
                   "void f(ergodic_exploration::FleetReplayMemory& m, void* c, int* n) { m.samplePool(3, 16, c, n, 116, true, true, nullptr); }\n"
                   "int main() { return 0; }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROOT, "ergodic_exploration_amd", "host", "include"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(os.environ.get("ROCM", "/opt/rocm"), "include"), str(src)], check=True)

"""CPU checks of the fleet replay memory (include/ergodic_amd.h, eea_replay_*): the random stream of the numpy restatement
(tests/replay_restatement.py -- what tests/test_gpu_replay_memory.py holds the kernels to, bitwise) against the published
known answers of Philox4x32-10, the index map, and the argument checks of the C ABI that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np

from ergodic_exploration_amd import capi
from tests import replay_restatement as rr


def _words(text):
    return [int(w, 16) for w in text.split()]


def test_philox_known_answers():
    """the three known answers of Random123's kat_vectors for philox4x32, 10 rounds"""
    kats = [("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
            ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
            ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, out in kats:
        got = [int(x) for x in rr.philox4x32_10(_words(ctr), _words(key))]
        assert got == _words(out), (ctr, key, ["%08x" % g for g in got])
    # vectorised over the first counter word = the scalar calls
    many = rr.philox4x32_10((np.arange(5), 7, 9, 11), (13, 17))
    for j in range(5):
        assert [int(w[j]) for w in many] == [int(x) for x in rr.philox4x32_10((j, 7, 9, 11), (13, 17))]


def test_mulhi_is_exact():
    rng = np.random.default_rng(0)
    r = rng.integers(0, 2**64, 2000, dtype=np.uint64)
    r[:4] = [0, 1, 2**64 - 1, 2**63]
    for n in (1, 2, 3, 101, 4097, 2**32 - 1):
        want = [(int(x) * n) >> 64 for x in r]
        assert [int(x) for x in rr.mulhi64(r, n)] == want


def test_indices_are_in_range_and_depend_on_every_input():
    for n in (1, 2, 9, 101, 5000, 2**32 - 1):
        idx = rr.draw_indices(n, 100, seed=0x123456789abcdef, draw=3, robot=17)
        assert idx.shape == (100,) and (idx >= 0).all() and (idx < n).all()
    assert (rr.draw_indices(1, 100, 5, 5, 5) == 0).all()
    base = rr.draw_indices(5000, 100, seed=1, draw=2, robot=3)
    assert np.array_equal(base, rr.draw_indices(5000, 100, seed=1, draw=2, robot=3))
    for other in (dict(seed=2, draw=2, robot=3), dict(seed=1 + 2**32, draw=2, robot=3), dict(seed=1, draw=3, robot=3),
                  dict(seed=1, draw=2 + 2**32, robot=3), dict(seed=1, draw=2, robot=4)):
        assert not np.array_equal(base, rr.draw_indices(5000, 100, **other)), other
    assert len(set(base.tolist())) > 90   # columns differ from one another


def test_index_map_is_uniform():
    """Pearson's chi-squared of the index map at n = 101 (the first memory size that is sampled at the shipped batch size of
    100) over 40 robots x 50 ticks x 100 columns = 200 000 draws, seed fixed (deterministic: not flaky).  Bound: the 99.9 %
    quantile of chi-squared with n - 1 = 100 degrees of freedom, 149.449 (tables; scipy.stats.chi2.ppf(0.999, 100))."""
    n, batch = 101, 100
    hist = np.zeros(n, dtype=np.int64)
    for robot in range(40):
        for draw in range(50):
            hist += np.bincount(rr.draw_indices(n, batch, seed=2020, draw=draw, robot=robot), minlength=n)
    total = hist.sum()
    assert total == 40 * 50 * batch
    expected = total / n
    chi2 = float(((hist - expected) ** 2 / expected).sum())
    print("chi-squared(100) = %.2f" % chi2)
    assert chi2 < 149.449


def test_restated_memory_follows_the_reference_branches():
    """buffer.cpp: nothing stored -> no columns; <= batch size -> the stored poses in order; a full store drops"""
    m = rr.ReplayMemory(2, capacity=6, batch_size=4, seed=1)
    cols, n_mem = np.full((2, 4, 3), -1.0), np.full(2, -1)
    m.sample(0, cols, n_mem)
    assert n_mem.tolist() == [0, 0] and (cols == -1.0).all()
    for t in range(8):
        m.append(np.array([[t, 0.5, 0.0], [t, 1.5, 0.0]]), mask=[1, t % 2])
    assert m.count.tolist() == [6, 4] and m.dropped == 2
    m.sample(5, cols, n_mem)
    assert n_mem.tolist() == [4, 4]
    assert cols[1, :, 0].tolist() == [1.0, 3.0, 5.0, 7.0]                  # all of robot 1's four poses, in order
    slots, ncols = m.indices(5)
    assert ncols.tolist() == [4, 4] and slots[1].tolist() == [0, 1, 2, 3]
    assert slots[0].tolist() == rr.draw_indices(6, 4, seed=1, draw=5, robot=0).tolist()   # robot 0 (6 > 4) draws
    assert cols[0, :, 0].tolist() == slots[0].tolist() and (slots[0] <= 5).all()           # (its pose x is the slot number)
    # a robot's draws are those of its GLOBAL id, whatever shard holds it
    shard = rr.ReplayMemory(1, capacity=6, batch_size=4, seed=1, robot0=7)
    whole = rr.ReplayMemory(8, capacity=6, batch_size=4, seed=1)
    for t in range(6):
        shard.append(np.zeros((1, 3)))
        whole.append(np.zeros((8, 3)))
    assert shard.indices(3)[0][0].tolist() == whole.indices(3)[0][7].tolist()


def test_replay_argument_errors_do_not_need_a_device():
    L = capi.lib()
    h = C.c_void_p()
    for args in ((0, 10, 4, 8), (3, 0, 4, 8), (3, 10, 0, 8), (3, 10, 4, 2), (3, 10, 4, 16)):
        B, cap, batch, rs = args
        assert L.eea_replay_create(0, B, cap, batch, 1, 0, rs, C.byref(h)) == capi.ERR_INVALID_ARGUMENT, args
        assert not h.value
    assert L.eea_replay_create(0, 3, 10, 4, 1, 0, 8, None) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_replay_create(0, 3, 10, 4, 1, 0, 5, C.byref(h)) == capi.ERR_INVALID_ARGUMENT and b"real_size" in L.eea_last_error()
    # a store whose byte count overflows is an error with a message, never a crash
    assert L.eea_replay_create(0, 2**32 - 1, 2**32 - 1, 4, 1, 0, 8, C.byref(h)) == capi.ERR_HIP
    assert b"overflow" in L.eea_last_error() and not h.value
    # every other entry refuses a null handle
    assert L.eea_replay_append(None, None, None, None) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_replay_sample(None, 0, None, None, 4, None) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_replay_append_sample(None, None, None, 0, None, None, 4, None) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_replay_counts(None, None, None) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_replay_read(None, 0, 0, 0, None) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_replay_reset(None, None) == capi.ERR_INVALID_ARGUMENT
    L.eea_replay_destroy(None)


def test_replay_kernels_are_in_the_library():
    """the kernels of csrc/replay_kernel.hip are gfx950 code in the build: no scratch, no LDS, and <= 64 registers -- the
    most a wavefront may hold with all eight wavefront slots of a SIMD in use (512 / 8): a gather hides its latency with
    resident wavefronts"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as kr
    obj = os.path.join(os.path.dirname(capi.LIB_PATH), "..", "csrc", "build", "replay_kernel.o")
    names = {}
    for k in kr.kernels(obj):
        if "vgpr_count" in k:
            names[subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.strip()] = k
    sample = [k for n, k in names.items() if "replay_sample_kernel<" in n]
    append = [k for n, k in names.items() if "replay_append_kernel<" in n]
    assert len(sample) == 4 and len(append) == 2, sorted(names)   # fp64 / fp32 x with / without the fused append
    for k in sample + append:
        assert int(k["vgpr_count"]) <= 64 and int(k["private_segment_fixed_size"]) == 0 and int(k["group_segment_fixed_size"]) == 0, k


def test_host_wrapper_compiles(tmp_path):
    """host/include/ergodic_exploration/replay_memory.hpp (the RAII wrapper beside agent_batch.hpp) against the C header"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "use.cpp"
    src.write_text("#include <ergodic_exploration/replay_memory.hpp>\n"
                   "int main() { return sizeof(ergodic_exploration::FleetReplayMemory) > 0 ? 0 : 1; }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(root, "ergodic_exploration_amd", "host", "include"), "-I", os.path.join(root, "include"),
                    "-I", os.path.join(os.environ.get("ROCM", "/opt/rocm"), "include"), str(src)], check=True)   # (ROCM: as host/Makefile)

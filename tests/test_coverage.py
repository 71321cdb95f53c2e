"""CPU checks of the coverage entry points (include/ergodic_amd.h: eea_replay_history_records, eea_records_metric;
csrc/coverage_kernel.hip): the numpy restatement tests/coverage_restatement.py against the oracle's trajCoeff, the argument
checks of the C ABI that need no device, and the kernels' presence in the gfx950 build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from ergodic_exploration_amd import capi
from tests import coverage_restatement as cr

BOUNDS = (-1.5, 10.5, 0.75, 6.75)   # map_pos = (-1.5, 0.75) != 0, lx = 12, ly = 6


@pytest.mark.parametrize("K", [5, 10])
@pytest.mark.parametrize("n", [1, 7, 300])
def test_restated_record_is_the_oracles_traj_coeff(K, n):
    """rec[:K^2] / n against Basis::trajCoeff of the shifted poses (<= 1e-13), the count and the padding; the poses overhang
    the domain on every side (nothing is clipped)"""
    lx, ly, pos = BOUNDS[1] - BOUNDS[0], BOUNDS[3] - BOUNDS[2], (BOUNDS[0], BOUNDS[2])
    rng = np.random.default_rng(100 * K + n)
    poses = np.stack([rng.uniform(BOUNDS[0] - 2.0, BOUNDS[1] + 2.0, n), rng.uniform(BOUNDS[2] - 2.0, BOUNDS[3] + 2.0, n),
                      rng.uniform(-np.pi, np.pi, n)], 1)
    rec = cr.history_record(poses, K, lx, ly, pos)
    assert rec.shape == (cr.record_len(K),) and cr.record_len(K) % 2 == 0 and cr.record_len(K) >= K * K + 1
    assert rec[K * K] == n and (rec[K * K + 1:] == 0.0).all()
    shifted = (poses[:, :2] - np.asarray(pos)).T.copy()
    want = po.traj_coeff(lx, ly, K, shifted)
    assert np.abs(rec[:K * K] / n - want).max() <= 1e-13


def test_restated_metric_and_the_zero_count_rule():
    K = 5
    rng = np.random.default_rng(2)
    phik, lam = rng.uniform(-1, 1, K * K), rng.uniform(0.01, 1, K * K)
    empty = cr.history_record(np.zeros((0, 3)), K, 12.0, 6.0, (0.0, 0.0))
    assert (empty == 0.0).all()
    some = cr.history_record(rng.uniform(0, 6, (9, 3)), K, 12.0, 6.0, (0.5, 0.25))
    eps, ck = cr.records_metric(np.stack([empty, some]), K, phik, lam)
    assert (ck[0] == 0.0).all() and eps[0] == pytest.approx(float((lam * phik ** 2).sum()), rel=1e-15)
    assert np.array_equal(ck[1], some[:K * K] / 9.0)
    assert eps[1] == pytest.approx(float((lam * (some[:K * K] / 9.0 - phik) ** 2).sum()), rel=1e-15)
    # sum records are closed under addition: two halves of a history add up to the whole
    poses = rng.uniform(-1, 7, (40, 3))
    a, b = (cr.history_record(p, K, 12.0, 6.0, (0.5, 0.25)) for p in (poses[:15], poses[15:]))
    whole = cr.history_record(poses, K, 12.0, 6.0, (0.5, 0.25))
    assert np.abs(a + b - whole).max() <= 1e-12 and (a + b)[K * K] == 40


def test_coverage_argument_errors_do_not_need_a_device():
    """null arguments are refused before any HIP call (as test_replay_argument_errors_do_not_need_a_device)"""
    L = capi.lib()
    one = C.c_void_p(8)   # never dereferenced: a null among the others is found first
    assert L.eea_replay_history_records(None, None, None, None) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_replay_history_records(None, one, one, None) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_replay_history_records(one, None, one, None) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_replay_history_records(one, one, None, None) == capi.ERR_INVALID_ARGUMENT
    assert b"null" in L.eea_last_error()
    assert L.eea_records_metric(None, 1, None, None, None, None) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_records_metric(None, 1, one, one, None, None) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_records_metric(one, 1, None, one, None, None) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_records_metric(one, 1, one, None, None, None) == capi.ERR_INVALID_ARGUMENT
    assert L.eea_abi_version() == 6
    assert {"eea_replay_history_records", "eea_records_metric"} <= set(capi.declared_symbols())


def test_coverage_kernels_are_in_the_library():
    """the kernels of csrc/coverage_kernel.hip are gfx950 code in the build: no scratch; the history kernel's [pose][mode]
    tiles are its only LDS (2 axes x 64 poses x (16 tiles + 2) reals), the metric kernel uses none"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as kr
    obj = os.path.join(os.path.dirname(capi.LIB_PATH), "..", "csrc", "build", "coverage_kernel.o")
    names = {}
    for k in kr.kernels(obj):
        if "vgpr_count" in k:
            names[subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.strip()] = k
    history = {n: k for n, k in names.items() if "history_records_kernel<" in n}
    metric = [k for n, k in names.items() if "records_metric_kernel<" in n]
    assert len(history) == 4 and len(metric) == 2, sorted(names)   # fp64 / fp32 x one / 2 x 2 tiles; fp64 / fp32
    for n, k in history.items():
        size, tiles = (8 if "<double" in n else 4), (2 if ", 2>" in n else 1)
        assert int(k["private_segment_fixed_size"]) == 0, k
        assert int(k["group_segment_fixed_size"]) == 2 * 64 * (16 * tiles + 2) * size, k
    for k in metric:
        assert int(k["private_segment_fixed_size"]) == 0 and int(k["group_segment_fixed_size"]) == 0, k


def test_host_wrapper_has_the_coverage_calls(tmp_path):
    """host/include/ergodic_exploration/replay_memory.hpp: FleetReplayMemory::historyRecords and recordsMetric compile
    against the C header"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "use.cpp"
    src.write_text("#include <ergodic_exploration/replay_memory.hpp>\n"
                   "void use(ergodic_exploration::FleetReplayMemory& m, eea_engine* e, void* d)\n"
                   "{ m.historyRecords(e, d, nullptr); ergodic_exploration::recordsMetric(e, 1u, d, d, nullptr, nullptr); }\n"
                   "int main() { return 0; }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(root, "ergodic_exploration_amd", "host", "include"), "-I", os.path.join(root, "include"),
                    "-I", os.path.join(os.environ.get("ROCM", "/opt/rocm"), "include"), str(src)], check=True)

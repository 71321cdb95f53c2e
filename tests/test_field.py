"""CPU checks of the coverage fields (include/ergodic_amd.h: eea_records_field; csrc/field_kernel.hip): the numpy restatement
tests/field_restatement.py against the oracle's fourierBasis on the oracle's grid, a sanity case of the density, the argument
checks of the C ABI that need no device, and the kernels' presence in the gfx950 build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from ergodic_exploration_amd import capi
from tests import coverage_restatement as cr
from tests import field_restatement as fr

KINDS = (fr.DENSITY, fr.DEFICIT, fr.POTENTIAL)


def test_constants_are_the_headers():
    assert (capi.FIELD_DENSITY, capi.FIELD_DEFICIT, capi.FIELD_POTENTIAL) == KINDS == (0, 1, 2)
    with open(capi.HEADER_PATH) as f:
        assert "EEA_FIELD_DENSITY = 0, EEA_FIELD_DEFICIT = 1, EEA_FIELD_POTENTIAL = 2" in f.read()


@pytest.mark.parametrize("K", [5, 10])
def test_restated_field_is_the_oracles_basis_sum(K):
    """sum_m a_m fourierBasis(p)[m] over the points of phi_grid, all three kinds, records with counts 0, 1, 37 and -1:
    within 1e-13 sum |a_m| (the bound of test_restated_record_is_the_oracles_traj_coeff)"""
    nx, ny, res = 13, 7, 0.5
    lx, ly = 6.0, 3.0
    rng = np.random.default_rng(K)
    phik, lam = rng.uniform(-1, 1, K * K), po.basis_init(K)[1]
    rec = np.zeros((4, cr.record_len(K)))
    for j, n in enumerate((0, 1, 37, -1)):
        rec[j, :K * K] = rng.uniform(-1, 1, K * K) * abs(n)
        rec[j, K * K] = n
    grid = po.phi_grid(nx, ny, res)
    basis = np.stack([po.fourier_basis(lx, ly, K, grid[:, p].copy()) for p in range(nx * ny)])     # [point][m]
    for kind in KINDS:
        field, S = fr.records_field(kind, rec, K, lx, ly, res, phik, lam, nx, ny)
        a = fr.coefficients(kind, rec, K, lx, ly, phik, lam)
        assert field.shape == (4, ny, nx) and np.array_equal(S, np.abs(a).sum(axis=1))
        want = (a @ basis.T).reshape(4, ny, nx)
        for j in range(4):
            err = np.abs(field[j] - want[j]).max()
            print("K = %d kind %d record %d: max |restated - oracle| = %.3e, S = %.3e" % (K, kind, j, err, S[j]))
            assert err <= 1e-13 * S[j]
        # counts 0 and -1: c = 0 -- no visits, the whole target as deficit, -lamda phi as potential
        for j in (0, 3):
            assert np.array_equal(a[j], fr.coefficients(kind, np.zeros_like(rec[0]), K, lx, ly, phik, lam)[0])
    assert (fr.records_field(fr.DENSITY, rec[0], K, lx, ly, res, phik, lam, nx, ny)[0] == 0.0).all()
    # a row tile is the slice of the whole grid
    whole = fr.records_field(fr.POTENTIAL, rec, K, lx, ly, res, phik, lam, nx, ny)[0]
    tile = fr.records_field(fr.POTENTIAL, rec, K, lx, ly, res, phik, lam, nx, ny, 2, 3)[0]
    assert np.array_equal(tile, whole[:, 2:5])


def test_density_of_one_pose_peaks_at_the_nearest_grid_point():
    """the exact record of ONE pose (rec[m] = f_m(p), count 1), K = 10 on the shipped 121 x 61 grid: the band-limited
    density has its maximum at the grid point nearest p, and its mean over the domain is 1 / (lx ly) (trapezoid rule:
    exact for cosines below the grid's Nyquist mode)"""
    K, nx, ny, res, lx, ly = 10, 121, 61, 0.1, 12.0, 6.0
    p = np.array([4.23, 2.71])
    rec = np.zeros(cr.record_len(K))
    rec[:K * K] = po.fourier_basis(lx, ly, K, p)
    rec[K * K] = 1.0
    field = fr.records_field(fr.DENSITY, rec, K, lx, ly, res, np.zeros(K * K), np.ones(K * K), nx, ny)[0][0]
    r, i = np.unravel_index(np.argmax(field), field.shape)
    assert (i, r) == (42, 27), (i, r)
    wx, wy = np.ones(nx), np.ones(ny)
    wx[[0, -1]] = wy[[0, -1]] = 0.5
    mean = float(wy @ field @ wx) / ((nx - 1) * (ny - 1))
    assert mean == pytest.approx(1.0 / (lx * ly), rel=1e-12)


def test_field_argument_errors_do_not_need_a_device():
    """every argument error is raised before the engine is read and before any HIP call (as
    test_coverage_argument_errors_do_not_need_a_device)"""
    L = capi.lib()
    one = C.c_void_p(8)   # never dereferenced: the argument checks come first
    call = L.eea_records_field
    ok = dict(e=one, kind=capi.FIELD_DENSITY, n_rec=1, rec=one, nx=7, ny=5, row0=0, nrows=5, out=one)

    def status(**kw):
        a = dict(ok, **kw)
        return call(a["e"], a["kind"], a["n_rec"], a["rec"], a["nx"], a["ny"], a["row0"], a["nrows"], a["out"], None)

    for name in ("e", "rec", "out"):
        assert status(**{name: None}) == capi.ERR_INVALID_ARGUMENT, name
        assert b"null" in L.eea_last_error()
    for name in ("n_rec", "nx", "ny", "nrows"):
        assert status(**{name: 0}) == capi.ERR_INVALID_ARGUMENT, name
        assert b"positive" in L.eea_last_error()
    for row0, nrows in ((0, 6), (5, 1), (3, 3), (2 ** 32 - 1, 2)):
        assert status(row0=row0, nrows=nrows) == capi.ERR_INVALID_ARGUMENT, (row0, nrows)
        assert b"row0 + nrows" in L.eea_last_error()
    for kind in (-1, 3, 99):
        assert status(kind=kind) == capi.ERR_INVALID_ARGUMENT, kind
        assert b"kind" in L.eea_last_error()
    assert status(nx=2 ** 16, ny=2 ** 15 + 1, nrows=1) == capi.ERR_UNSUPPORTED
    assert b"2^31" in L.eea_last_error()
    assert L.eea_abi_version() == 6
    assert "eea_records_field" in capi.declared_symbols() and hasattr(L, "eea_records_field")


def test_field_kernels_are_in_the_library():
    """the kernels of csrc/field_kernel.hip are gfx950 code in the build, fp64 and fp32: no scratch; their LDS is sized
    per launch (K columns x 128 + K x rows + K^2 reals), none of it static"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_resources as kr
    obj = os.path.join(os.path.dirname(capi.LIB_PATH), "..", "csrc", "build", "field_kernel.o")
    names = {}
    for k in kr.kernels(obj):
        if "vgpr_count" in k:
            names[subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.strip()] = k
    field = {n: k for n, k in names.items() if "records_field_kernel<" in n}
    assert len(field) == 2 and any("<double>" in n for n in field) and any("<float>" in n for n in field), sorted(names)
    for n, k in field.items():
        assert int(k["private_segment_fixed_size"]) == 0, k
        assert int(k["group_segment_fixed_size"]) == 0, k


def test_host_wrapper_has_the_field_call(tmp_path):
    """host/include/ergodic_exploration/replay_memory.hpp: recordsField compiles against the C header"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "use.cpp"
    src.write_text("#include <ergodic_exploration/replay_memory.hpp>\n"
                   "void use(eea_engine* e, const void* rec, void* out)\n"
                   "{ ergodic_exploration::recordsField(e, EEA_FIELD_DEFICIT, 1u, rec, 121u, 61u, 0u, 61u, out);\n"
                   "  ergodic_exploration::recordsField(e, EEA_FIELD_POTENTIAL, 1u, rec, 121u, 61u, 3u, 7u, out, nullptr); }\n"
                   "int main() { return 0; }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(root, "ergodic_exploration_amd", "host", "include"), "-I", os.path.join(root, "include"),
                    "-I", os.path.join(os.environ.get("ROCM", "/opt/rocm"), "include"), str(src)], check=True)

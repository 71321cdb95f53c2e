"""numpy restatement of eea_records_field (include/ergodic_amd.h): what the call is defined to compute, in a few lines.
tests/test_field.py holds it to the oracle's fourierBasis on the oracle's grid."""
import numpy as np

DENSITY, DEFICIT, POTENTIAL = 0, 1, 2


def axis(n, resolution):
    """coordinates by repeated += resolution from 0 (ergodic_control.hpp:387-408; pyoracle.phi_grid)"""
    out, v = np.empty(n), 0.0
    for i in range(n):
        out[i] = v
        v += resolution
    return out


def coefficients(kind, rec, K, lx, ly, phik, lamdak):
    """a_m [n][K^2], m = k2 K + k1, of sum records [n][>= K^2 + 1]: c = rec / count, 0 where the count is <= 0"""
    rec = np.atleast_2d(np.asarray(rec, dtype=np.float64))
    n = rec[:, K * K]
    ck = np.where(n[:, None] > 0, rec[:, :K * K] / np.where(n > 0, n, 1.0)[:, None], 0.0)
    if kind == POTENTIAL:
        return lamdak[None, :] * (ck - phik[None, :])
    w = np.where(np.arange(K) > 0, 2.0, 1.0)
    wgt = np.outer(w, w).reshape(-1)       # w_k2 w_k1 at k2 K + k1
    if kind == DENSITY:
        return wgt[None, :] * ck / (lx * ly)
    if kind == DEFICIT:
        return wgt[None, :] * (phik[None, :] - ck) / (lx * ly)
    raise ValueError("unknown field kind %r" % (kind,))


def records_field(kind, rec, K, lx, ly, resolution, phik, lamdak, nx, ny, row0=0, nrows=None):
    """(field [n][nrows][nx], S [n] = sum_m |a_m| per record): field[j][r][i] = sum_m a_m cos((k1 pi / lx) x_i)
    cos((k2 pi / ly) y_{row0 + r})"""
    nrows = ny - row0 if nrows is None else nrows
    a = coefficients(kind, rec, K, lx, ly, phik, lamdak)
    k = np.arange(K, dtype=np.float64)
    cx = np.cos(np.outer(k * (np.pi / lx), axis(nx, resolution)))                          # [k1][i]
    cy = np.cos(np.outer(k * (np.pi / ly), axis(ny, resolution)[row0:row0 + nrows]))       # [k2][r]
    A = a.reshape(-1, K, K)                                                                # [j][k2][k1]
    return np.einsum("jba,br,ai->jri", A, cy, cx), np.abs(a).sum(axis=1)

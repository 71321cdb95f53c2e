"""numpy restatement of the coverage entry points (include/ergodic_amd.h: eea_replay_history_records, eea_records_metric):
what the two calls are defined to compute, in a few lines.  tests/test_coverage.py holds it to the oracle's trajCoeff."""
import numpy as np


def record_len(K):
    """eea_ck_record_len: K^2 + 1 rounded up to an even number"""
    return (K * K + 2) // 2 * 2


def history_record(poses, K, lx, ly, map_pos):
    """the sum record of the stored poses [n][>= 2] (map frame): Basis::trajCoeff (basis.cpp:109-120) without the 1/N,
    col = k2 * K + k1; element K^2 = n; padding 0.  No poses: all zeros."""
    poses, k = np.asarray(poses, dtype=np.float64).reshape(-1, 3), np.arange(K)
    cx = np.cos(np.outer(k, (np.pi / lx) * (poses[:, 0] - map_pos[0])))     # [k1][i]
    cy = np.cos(np.outer(k, (np.pi / ly) * (poses[:, 1] - map_pos[1])))     # [k2][i]
    rec = np.zeros(record_len(K))
    rec[:K * K] = (cy @ cx.T).reshape(-1)
    rec[K * K] = len(poses)
    return rec


def records_metric(rec, K, phik, lamdak):
    """(eps [n], c_k [n][K^2]) of sum records [n][record_len]: c = rec / count, 0 where the count is <= 0"""
    rec = np.atleast_2d(np.asarray(rec, dtype=np.float64))
    n = rec[:, K * K]
    ck = np.where(n[:, None] > 0, rec[:, :K * K] / np.where(n > 0, n, 1.0)[:, None], 0.0)
    return (lamdak[None, :] * (ck - phik[None, :]) ** 2).sum(axis=1), ck

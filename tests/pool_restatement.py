"""numpy restatement of the POOLED replay memory (include/ergodic_amd.h, eea_replay_pool_sample): the checker of
tests/test_replay_pool.py (CPU) and tests/test_gpu_replay_pool.py, on top of the stores of tests/replay_restatement.py.

The pool: every stored pose of every robot in robot-major order, off[q] = sum_{p<q} n_p, N = off[B].  Robot b draws from
N_b = N (or N - n_b without its own poses): all N_b poses in order while N_b <= n_cols (buffer.cpp:75-89), otherwise n_cols
draws g = (r64 * N_b) >> 64 with Philox4x32-10, counter (j, robot0 + b, draw_lo, draw_hi), key (seed_lo, seed_hi ^ 0x9E3779B9).
Without its own poses g >= off[b] stands for g + n_b; the owner of g is the last q with off[q] <= g, the slot g - off[q]."""
import numpy as np

from tests.replay_restatement import MASK32, mulhi64, philox4x32_10

KEY_XOR = 0x9E3779B9   # keeps the pooled draws apart from the own-memory draws at the same (seed, draw, robot, column)


def pool_r64(seed, draw, robot, n_cols):
    """r64 [len(robot)][n_cols] of the pooled draws of the robots with the GLOBAL ids `robot` in tick `draw`"""
    j = np.arange(n_cols, dtype=np.uint64)[None, :]
    rob = (np.asarray(robot, dtype=np.int64) & MASK32).astype(np.uint64).reshape(-1, 1)
    o = philox4x32_10((j, rob, draw & MASK32, (draw >> 32) & MASK32), (seed & MASK32, ((seed >> 32) & MASK32) ^ KEY_XOR))
    return o[0] | (o[1] << np.uint64(32))


def mulhi64_wide(r64, n):
    """(r64 * n) >> 64 for uint64 arrays with n up to 2^64 - 1: mulhi64 of the low word of n plus the high word's product"""
    r64, n = np.broadcast_arrays(np.asarray(r64, dtype=np.uint64), np.asarray(n, dtype=np.uint64))
    if not (n >> np.uint64(32)).any():
        return mulhi64(r64, n)
    n_lo, n_hi = n & np.uint64(MASK32), n >> np.uint64(32)
    r_lo, r_hi = r64 & np.uint64(MASK32), r64 >> np.uint64(32)
    # r64 * n = r64 * n_lo + (r64 * n_hi) << 32;  r64 * n_lo = top * 2^64 + mid * 2^32 + (low 32 bits)
    top = mulhi64(r64, n_lo)                                                            # bits 64 .. of r64 * n_lo
    mid = (r_hi * n_lo + ((r_lo * n_lo) >> np.uint64(32))) & np.uint64(MASK32)       # bits 32 .. 63 of r64 * n_lo
    a = r_lo * n_hi + mid                                                               # < 2^64: (2^32 - 1)^2 + 2^32 - 1
    return top + r_hi * n_hi + (a >> np.uint64(32))                                   # the true quotient is < 2^64


def offsets(count):
    """off [B + 1]: the exclusive prefix sum of the counts"""
    off = np.zeros(len(count) + 1, dtype=np.int64)
    np.cumsum(np.asarray(count, dtype=np.int64), out=off[1:])
    return off


def owner_slot(off, g):
    """(owner, slot) of the pool indices g (each < off[-1]): the LAST q with off[q] <= g -- robots without poses have equal
    consecutive offsets and are never it -- and g - off[q]"""
    g = np.asarray(g, dtype=np.int64)
    q = np.searchsorted(off, g, side="right") - 1
    return q, g - off[q]


def pool_indices(count, seed, robot0, draw, n_cols, exclude_self):
    """(owner [B][n_cols], slot [B][n_cols], w [B]): the store position behind column j of robot b; entries at j >= w[b] mean
    nothing"""
    count = np.asarray(count, dtype=np.int64)
    B, off = len(count), offsets(count)
    own = count if exclude_self else np.zeros(B, dtype=np.int64)
    n_pool = off[B] - own
    w = np.minimum(n_pool, n_cols)
    drawn = mulhi64_wide(pool_r64(seed, draw, robot0 + np.arange(B), n_cols), n_pool.astype(np.uint64)[:, None]).astype(np.int64)
    g = np.where((n_pool <= n_cols)[:, None], np.arange(n_cols, dtype=np.int64)[None, :], drawn)
    g = np.where(g >= off[:B, None], g + own[:, None], g)            # the robot's own segment is skipped
    if off[B] == 0:
        return np.zeros_like(g), np.zeros_like(g), w
    valid = np.arange(n_cols)[None, :] < w[:, None]
    owner, slot = owner_slot(off, np.where(valid, g, 0))
    return owner, slot, w


def sample_pool(mem, draw, n_cols, mem_cols, n_mem, exclude_self=False, accumulate=False):
    """eea_replay_pool_sample on a tests.replay_restatement.ReplayMemory: writes the columns into mem_cols [B][stride][3]
    (other columns untouched) and n_mem [B]"""
    stride = mem_cols.shape[1]
    owner, slot, w = pool_indices(mem.count, mem.seed, mem.robot0, draw, n_cols, exclude_self)
    base = np.maximum(np.asarray(n_mem, dtype=np.int64), 0) if accumulate else np.zeros(mem.B, dtype=np.int64)
    w = np.minimum(w, np.maximum(stride - base, 0))                  # a clipped robot keeps the first columns of its sequence
    for b in range(mem.B):
        k = int(w[b])
        if k:
            mem_cols[b, base[b]:base[b] + k] = mem.store[owner[b, :k], slot[b, :k]]
    n_mem[:] = base + w

"""numpy restatement of the fleet replay memory (include/ergodic_amd.h, eea_replay_*): the checker of
tests/test_replay_memory.py (CPU) and tests/test_gpu_replay_memory.py.

ReplayBuffer::append / sampleMemory (reference buffer.cpp:54-62, 64-111) per robot, with the documented random stream in place
of Armadillo's global one: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
with counter (j, robot0 + b, draw_lo, draw_hi) and key (seed_lo, seed_hi); r64 = out[0] | out[1] << 32;
index = (r64 * n) >> 64."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two; returns the four output words as uint64 arrays < 2^32"""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK32) for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]          # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK32),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK32)]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c


def mulhi64(r64, n):
    """(r64 * n) >> 64 for uint64 arrays r64 and n < 2^32, in 32-bit limbs (exact)"""
    r64 = np.asarray(r64, dtype=np.uint64)
    n = np.asarray(n, dtype=np.uint64)
    lo, hi = r64 & np.uint64(MASK32), r64 >> np.uint64(32)
    # r64 * n = hi * n * 2^32 + lo * n, both products < 2^64
    return (hi * n + ((lo * n) >> np.uint64(32))) >> np.uint64(32)


def draw_indices(n, batch_size, seed, draw, robot):
    """the batch_size indices robot `robot` (global id) draws from a memory of n poses in tick `draw`"""
    j = np.arange(batch_size, dtype=np.uint64)
    o = philox4x32_10((j, robot & MASK32, draw & MASK32, (draw >> 32) & MASK32), (seed & MASK32, (seed >> 32) & MASK32))
    return mulhi64(o[0] | (o[1] << np.uint64(32)), n).astype(np.int64)


class ReplayMemory:
    """B host-side stores with the semantics of the device replay memory (vectorised over the robots)"""

    def __init__(self, B, capacity, batch_size, seed=0, robot0=0, dtype=np.float64):
        self.B, self.capacity, self.batch_size, self.seed, self.robot0 = B, capacity, batch_size, seed, robot0
        self.store = np.zeros((B, capacity, 3), dtype=dtype)
        self.count = np.zeros(B, dtype=np.int64)
        self.dropped = 0

    def append(self, pose, mask=None):
        """ReplayBuffer::append per robot with a non-zero mask entry (None: all)"""
        pose = np.asarray(pose, dtype=self.store.dtype)
        asked = np.ones(self.B, dtype=bool) if mask is None else np.asarray(mask) != 0
        room = self.count < self.capacity
        rows = np.nonzero(asked & room)[0]
        self.store[rows, self.count[rows]] = pose[rows]
        self.count[rows] += 1
        self.dropped += int((asked & ~room).sum())          # "WARNING: Buffer is full" (buffer.cpp:61)

    def indices(self, draw):
        """(slots [B][batch_size], columns per robot [B]): the store slot behind column j of robot b in tick `draw`; entries
        at j >= columns[b] mean nothing"""
        j = np.arange(self.batch_size, dtype=np.uint64)[None, :]
        robot = ((self.robot0 + np.arange(self.B)) & MASK32).astype(np.uint64)[:, None]
        o = philox4x32_10((j, robot, draw & MASK32, (draw >> 32) & MASK32), (self.seed & MASK32, (self.seed >> 32) & MASK32))
        drawn = mulhi64(o[0] | (o[1] << np.uint64(32)), self.count.astype(np.uint64)[:, None]).astype(np.int64)
        everything = (self.count <= self.batch_size)[:, None]          # buffer.cpp:75-89: the stored poses in order
        slots = np.where(everything, np.broadcast_to(j.astype(np.int64), drawn.shape), drawn)
        return slots, np.minimum(self.count, self.batch_size)

    def sample(self, draw, mem_cols, n_mem):
        """writes the columns into mem_cols [B][stride][3] (columns past n_mem untouched) and n_mem [B]"""
        slots, cols = self.indices(draw)
        valid = np.arange(self.batch_size)[None, :] < cols[:, None]
        picked = self.store[np.arange(self.B)[:, None], np.where(valid, slots, 0)]
        head = mem_cols[:, :self.batch_size]
        head[valid] = picked[valid]
        n_mem[:] = cols

    def append_sample(self, pose, draw, mem_cols, n_mem, mask=None):
        self.append(pose, mask)
        self.sample(draw, mem_cols, n_mem)

"""numpy restatement of the evidence grid (include/ergodic_amd.h: eea_evidence_table, eea_sense_observe_batch,
eea_evidence_publish): what the calls are defined to compute, written for clarity.  The sensor -- world2grid, blocks, the ray
set and its step offsets -- is tests/sense_restatement.py, the noise stream is philox4x32_10 of tests/replay_restatement.py,
both imported unchanged.  Integers throughout; the only floating-point steps are the sensor's own two and the table's exp."""
import collections
import math

import numpy as np

from tests import sense_restatement as sr
from tests.replay_restatement import philox4x32_10

# eea_evidence_cfg
Evidence = collections.namedtuple("Evidence", "w_occ w_free e_clip quantum thr_miss thr_false seed_lo seed_hi")

QUANTUM = 0.0884341726294605     # -logit(0.35) / 7: the reference's (0.90, 0.35) sensor model is (25, 7) units of it


def table(ev):
    """int8 [2 e_clip + 1]: entry e + e_clip = clamp(floor(100 sigma(e quantum) + 0.5), 1, 99), sigma(l) = 1 - 1 / (1 + exp(l))"""
    out = np.empty(2 * ev.e_clip + 1, dtype=np.int8)
    for e in range(-ev.e_clip, ev.e_clip + 1):
        l = float(e) * ev.quantum
        ex = math.exp(l) if l < 709.0 else math.inf          # (math.exp raises where C's exp returns +inf)
        sigma = 1.0 - 1.0 / (1.0 + ex)
        out[e + ev.e_clip] = min(max(int(math.floor(100.0 * sigma + 0.5)), 1), 99)
    return out


def noise_words(g, ev, robots, scan):
    """uint64 [len(robots)][ysize][xsize]: the word r of every cell for the global robot ids `robots` in scan `scan` -- word
    j & 3 of Philox at the counter (j >> 2, i, robot, scan) under the key (seed_lo, seed_hi)"""
    robots = np.asarray(robots, dtype=np.uint64).reshape(-1, 1, 1)
    i = np.arange(g.ysize, dtype=np.uint64).reshape(1, -1, 1)
    j = np.arange(g.xsize, dtype=np.uint64).reshape(1, 1, -1)
    words = philox4x32_10((j >> np.uint64(2), i, robots, int(scan) & 0xFFFFFFFF), (ev.seed_lo, ev.seed_hi))
    lane = np.broadcast_to(j & np.uint64(3), words[0].shape)
    return np.choose(lane.astype(np.int64), words)


def appears_blocking(g, ev, truth, robots, scan):
    """bool [len(robots)][ysize][xsize]: blocks(truth) ? !(r < thr_miss) : (r < thr_false) (the robot's own cell is dealt with
    by observe)"""
    truth = np.asarray(truth, dtype=np.int8).reshape(g.ysize, g.xsize)
    blocking = ~(truth.astype(np.float64) / 100.0 < g.occupied_threshold)
    r = noise_words(g, ev, robots, scan)
    return np.where(blocking[None], ~(r < np.uint64(ev.thr_miss)), r < np.uint64(ev.thr_false))


def _add_i32(a, d):
    """a + d as a two's-complement int32 add"""
    return (int(a) + int(d) + 2 ** 31) % 2 ** 32 - 2 ** 31


def observe(g, ev, R, scan, robot0, truth, evid, poses, mask=None, ranges=None, order=None):
    """one scan of every robot, added into evid (int32 [ysize][xsize]) in place; returns ranges int32 [P][8R] (`ranges` itself
    when given: the rows of robots the mask leaves out are not written).  order (optional): the sequence the robots are applied
    in -- the result must not depend on it"""
    P = len(poses)
    if ranges is None:
        ranges = np.full((P, 8 * R), -1, dtype=np.int32)
    off = sr.ray_offsets(R).tolist()
    chunk = max(1, (1 << 22) // (g.xsize * g.ysize))
    seen_of = {}                                               # chunk start -> appears_blocking of the chunk's robots
    for b in (range(P) if order is None else order):
        if mask is not None and mask[b] == 0:
            continue
        ranges[b, :] = -1
        i0, j0 = sr.world2grid(g, poses[b][0], poses[b][1])
        if not (i0 <= g.ysize - 1 and j0 <= g.xsize - 1):      # gridBounds: the robot touches nothing and hits nothing
            continue
        c0 = (b // chunk) * chunk
        if c0 not in seen_of:
            seen_of.clear()
            ids = [(robot0 + k) & 0xFFFFFFFF for k in range(c0, min(c0 + chunk, P))]
            seen_of[c0] = appears_blocking(g, ev, truth, ids, scan)
        seen = seen_of[c0][b - c0]
        touched = {(i0, j0): False}                            # the robot's own cell: touched, never appears blocking
        for q in range(8 * R):
            for s in range(1, R + 1):
                dx, dy = off[q][s - 1]
                if dx * dx + dy * dy > R * R:
                    break
                i, j = i0 + dy, j0 + dx
                if not (0 <= i < g.ysize and 0 <= j < g.xsize):
                    break
                hit = bool(seen[i, j])
                touched[(i, j)] = hit
                if hit:
                    ranges[b, q] = s
                    break
        for (i, j), hit in touched.items():                    # once per cell, however many rays crossed it
            evid[i, j] = _add_i32(evid[i, j], ev.w_occ if hit else -ev.w_free)
    return ranges


def publish(ev, evid, tab=None):
    """int8 grid: -1 where evid is 0, else table[clamp(e, -e_clip, e_clip) + e_clip]"""
    tab = table(ev) if tab is None else np.asarray(tab, dtype=np.int8)
    e = np.asarray(evid, dtype=np.int64)
    return np.where(e == 0, np.int8(-1), tab[np.clip(e, -ev.e_clip, ev.e_clip) + ev.e_clip]).astype(np.int8)


def join_scene():
    """the scene of the join test: a 48 x 40 grid with walls, 6 robots, 8 noisy scans at R = 6; returns (g, ev, R, truth,
    poses, evid after the scans).  Computed once: callers must not change what it returns"""
    if not _JOIN:
        g = sr.Geometry(-1.0, -2.0, 0.25, 48, 40, 0.8)
        ev = Evidence(25, 7, 1024, QUANTUM, 1 << 30, (1 << 32) // 20, 0x1234ABCD, 0x00C0FFEE)
        truth = np.zeros((40, 48), dtype=np.int8)
        truth[0], truth[-1], truth[:, 0], truth[:, -1] = 100, 100, 100, 100
        truth[:26, 18] = 100
        truth[14:, 33] = 100
        truth[30, 5:14] = 100
        centre = lambda i, j: [g.xmin + (j + 0.5) * g.resolution, g.ymin + (i + 0.5) * g.resolution, 0.0]
        poses = [centre(5, 5), centre(20, 14), centre(28, 22), centre(10, 26), centre(33, 40), centre(6, 42)]
        evid = np.zeros((40, 48), dtype=np.int32)
        for scan in range(8):
            observe(g, ev, 6, scan, 0, truth, evid, poses)
        evid.setflags(write=False)
        _JOIN.append((g, ev, 6, truth, poses, evid))
    return _JOIN[0]


_JOIN = []

"""The evidence grid on the device (include/ergodic_amd.h: eea_sense_observe_batch, eea_evidence_publish;
csrc/evidence_kernel.hip): the fleet's noisy scans are fused into integer evidence and published as occupancy probabilities.

Checker: the numpy restatement tests/evidence_restatement.py (held to an independent statement by tests/test_evidence.py).
Everything is integers: evidence, ranges and the published grid are compared BITWISE, as whole buffers -- each sits between
guard elements and starts 37 elements into its allocation, so no buffer is aligned to more than its element."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ergodic_exploration_amd import capi
from tests import evidence_restatement as er
from tests import mi_restatement as mr
from tests import sense_restatement as sr
from tests import test_gpu_sense as tgs

pytestmark = pytest.mark.gpu

GUARD = tgs.GUARD
G_EVID, G_RANGES, G_KNOWN = 0x5A5A5A5A, -123456789, 0x3C
S_RANGES = -77                   # what `ranges` holds before a call: not a range
IDEAL = er.Evidence(25, 7, 1024, er.QUANTUM, 0, 0, 0xDEADBEEF, 0x0BADF00D)
NOISY = IDEAL._replace(thr_miss=1 << 30, thr_false=(1 << 32) // 20)


def _ecfg(ev):
    return capi.EvidenceCfg(*ev)


def _same(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s differs at buffer offsets %s (payload starts at %d): got %s want %s" % (
        what, bad[:8], GUARD, got[bad[:8]], want[bad[:8]])


class _Device:
    """truth and evidence of one grid on the device, and the host image the restatement is replayed on"""

    def __init__(self, g, truth, ev):
        self.g, self.cfg, self.ev, self.ecfg = g, tgs._cfg(g), ev, _ecfg(ev)
        self.truth = np.ascontiguousarray(truth, dtype=np.int8)
        _, self._tbuf, self.d_truth = tgs._guarded(self.truth, 0x11, np.int8)
        self.evid = np.zeros(self.truth.shape, dtype=np.int32)
        _, self._ebuf, self.d_evid = tgs._guarded(self.evid, G_EVID, np.int32)

    def observe(self, R, scan, poses, mask=None, want_ranges=True, robot0=0, stream=None, replay=True):
        """one call on the device and (replay) in the restatement; returns (ranges image of the device, expected image)"""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        P = poses.shape[0]
        d_pose = torch.as_tensor(poses).cuda()
        d_mask = None if mask is None else torch.as_tensor(np.asarray(mask, dtype=np.int32)).cuda()
        rows = np.full((P, 8 * R), S_RANGES, dtype=np.int32)
        want_img, rbuf, d_ranges = tgs._guarded(rows, G_RANGES, np.int32)
        torch.cuda.synchronize()     # (the uploads above ran on torch's stream)
        capi.sense_observe_batch(self.cfg, self.ecfg, R, scan, self.d_truth, self.d_evid, d_pose, d_ranges if want_ranges else None,
                                 d_mask, robot0=robot0, stream=stream)
        torch.cuda.synchronize()
        if not replay:
            return rbuf.cpu().numpy(), None
        er.observe(self.g, self.ev, R, scan, robot0, self.truth, self.evid, poses, mask, rows)
        if not want_ranges:
            rows[:] = S_RANGES
        want_img[GUARD:GUARD + rows.size] = rows.reshape(-1)
        return rbuf.cpu().numpy(), want_img

    def image(self):
        return self._ebuf.cpu().numpy()

    def check_evid(self):
        guard = np.full(GUARD, G_EVID, np.int32)
        _same(self.image(), np.concatenate([guard, self.evid.reshape(-1), guard]), "evid")
        assert np.array_equal(self._tbuf.cpu().numpy()[GUARD:GUARD + self.truth.size], self.truth.reshape(-1))   # read only


@pytest.mark.parametrize("R", [1, 3, 6])
def test_ideal_sensor_is_the_reveal(R):
    """thr_miss = thr_false = 0 on the scene of test_gpu_sense.py, grid 37 x 29: the ranges are the reveal's bit for bit, the
    cells with evidence are exactly the cells the reveal wrote, and the evidence is the restatement's"""
    g, truth, poses = tgs._scene(37, 29)
    dev = _Device(g, truth, IDEAL)
    got, want = dev.observe(R, 0, poses)
    _same(got, want, "ranges")
    dev.check_evid()
    rev = tgs._Device(g, truth)
    rev_got, rev_want = rev.reveal(R, poses)
    _same(rev_got, rev_want, "the reveal's ranges")
    assert np.array_equal(got, rev_got)
    rev.check_known()
    written = rev._kbuf.cpu().numpy()[GUARD:-GUARD].reshape(29, 37) != tgs.S_KNOWN
    assert np.array_equal(dev.image()[GUARD:-GUARD].reshape(29, 37) != 0, written) and written.any() and not written.all()
    # an ideal sensor raises no false alarm: a cell that does not block holds a whole number of misses
    e = dev.evid
    blocking = ~(truth.astype(np.float64) / 100.0 < g.occupied_threshold)
    assert (e[~blocking] <= 0).all() and (e[~blocking] % 7 == 0).all() and (e[blocking] > 0).any()


@functools.lru_cache(maxsize=None)
def _noisy_scene():
    """the 37 x 29 scene at R = 6 with the noisy sensor: the restatement's evidence and ranges after each of three scans, and
    the proof that scans 0 and 1 differ in a range"""
    g, truth, poses = tgs._scene(37, 29)
    evid, after = np.zeros((29, 37), dtype=np.int32), []
    for scan in range(3):
        ranges = er.observe(g, NOISY, 6, scan, 0, truth, evid, poses)
        after.append((evid.copy(), ranges))
    assert not np.array_equal(after[0][1], after[1][1])
    return g, truth, poses, after


def test_noisy_scans_accumulate():
    """thr_miss = 2^30, thr_false = 2^32 / 20: scans 0, 1, 2 into one grid, evidence and ranges equal to the restatement after
    each; scans 0 and 1 differ in at least one range"""
    g, truth, poses, after = _noisy_scene()
    dev = _Device(g, truth, NOISY)
    rows = []
    for scan in range(3):
        got, want = dev.observe(6, scan, poses)
        _same(got, want, "ranges of scan %d" % scan)
        dev.check_evid()
        assert np.array_equal(dev.evid, after[scan][0])
        assert np.array_equal(got[GUARD:-GUARD].reshape(len(poses), 48), after[scan][1])
        rows.append(got)
    assert not np.array_equal(rows[0], rows[1])
    assert (dev.evid > 25).any() and (dev.evid < -7).any()


def test_contention_in_one_cell():
    """64 robots in one cell with the ideal sensor: 64 workgroups add to the same cells -- 64 x the single robot's grid"""
    g, truth, poses = tgs._scene(37, 29)
    one = _Device(g, truth, IDEAL)
    _same(*one.observe(6, 0, [poses[1]]), "ranges")
    one.check_evid()
    many = _Device(g, truth, IDEAL)
    got, want = many.observe(6, 0, [poses[1]] * 64, replay=False)
    many.evid = 64 * one.evid
    many.check_evid()
    assert (one.evid != 0).sum() > 50
    rows = got[GUARD:-GUARD].reshape(64, 48)
    assert (rows == rows[0]).all() and (rows[0] > 0).any()


@pytest.mark.parametrize("xs,ys", [(5, 4), (300, 3)])
def test_clipped_windows_at_the_lds_limit(xs, ys):
    """R = 127 (the largest window: 255 x 255 bytes of LDS) on grids far smaller than it, one with rows longer than a
    wavefront's stride: robots in the corners, in the middle, on the xmax / ymax decrement rule, off the grid on every side,
    and masked out; noisy sensor, two scans"""
    g = tgs._geom(xs, ys)
    rng = np.random.default_rng(xs)
    truth = rng.choice(np.array([0] * 12 + [100, -1, 79, 80], dtype=np.int8), size=(ys, xs))
    xmax, ymax = tgs.XMIN + xs * tgs.RES, tgs.YMIN + ys * tgs.RES
    poses = [tgs._centre(g, 0, 0), tgs._centre(g, 0, xs - 1), tgs._centre(g, ys - 1, 0), tgs._centre(g, ys - 1, xs - 1),
             tgs._centre(g, ys // 2, xs // 2), tgs._centre(g, 1, xs // 3),
             [xmax, ymax, 0.0], [xmax, tgs.YMIN + 1.1 * tgs.RES, 0.0], [tgs.XMIN + 2.5 * tgs.RES, ymax, 0.0],
             [tgs.XMIN - 0.3, 0.0, 0.0], [xmax + 0.3, 0.0, 0.0], [0.0, tgs.YMIN - 5.0, 0.0], [0.0, ymax + tgs.RES, 0.0],
             tgs._centre(g, 1, 1), tgs._centre(g, ys - 1, xs // 2)]
    mask = np.ones(len(poses), dtype=np.int32)
    mask[-2:] = 0
    dev = _Device(g, truth, NOISY)
    for scan in (0, 1):
        got, want = dev.observe(127, scan, poses, mask=mask)
        _same(got, want, "ranges")
        dev.check_evid()
    rows = got[GUARD:-GUARD].reshape(len(poses), 8 * 127)
    assert (rows[9:13] == -1).all() and (rows[-2:] == S_RANGES).all() and (rows[:9] > 0).any()
    assert (dev.evid > 0).any() and (dev.evid < 0).any()


def test_masked_off_grid_and_corner_robot_in_one_call():
    """the robot of a workgroup's turn is the reveal's (csrc/sense_rays.hpp: robot_cell), here in a scan: 23 x 19, R = 3, three
    robots in one call -- masked out (its row of ranges is not written, no evidence), off the grid (a row of -1, no evidence), in
    a corner (the clipped scan) -- ranges and evidence equal to the restatement bit for bit, noisy sensor"""
    g = tgs._geom(23, 19)
    truth = np.random.default_rng(23).choice(np.array([0] * 6 + [100, -1], dtype=np.int8), size=(19, 23))
    truth[16, 0] = truth[17, 2] = truth[18, 2] = 100      # a wall around the corner robot
    poses =[tgs._centre(g, 9, 11), [tgs.XMIN - 0.3, 0.0, 0.0], tgs._centre(g, 18, 0)]
    dev = _Device(g, truth, NOISY)
    got, want = dev.observe(3, 0, poses, mask=[0, 1, 1])
    _same(got, want, "ranges")
    dev.check_evid()
    rows = got[GUARD:-GUARD].reshape(3, 24)
    assert (rows[0] == S_RANGES).all() and (rows[1] == -1).all() and (rows[2] != S_RANGES).all() and (rows[2] > 0).any()
    only_corner = np.zeros((19, 23), dtype=np.int32)
    er.observe(g, NOISY, 3, 0, 2, truth, only_corner, [poses[2]])
    assert np.array_equal(dev.evid, only_corner) and (only_corner != 0).sum() >= 9 and (only_corner > 0).any()


@functools.lru_cache(maxsize=None)
def _strided_fleet():
    """65536 + 3 robots on an 8 x 8 grid (a few off it), noisy sensor at R = 1: the restatement's evidence and ranges"""
    P = 65536 + 3
    rng = np.random.default_rng(65539)
    g = tgs._geom(8, 8)
    truth = rng.choice(np.array([0, 0, 0, 100], dtype=np.int8), size=(8, 8))
    poses = np.stack([rng.uniform(tgs.XMIN - 0.1, tgs.XMIN + 8 * tgs.RES + 0.1, P),
                      rng.uniform(tgs.YMIN - 0.1, tgs.YMIN + 8 * tgs.RES + 0.1, P), np.zeros(P)], 1)
    evid = np.zeros((8, 8), dtype=np.int32)
    ranges = er.observe(g, NOISY, 1, 5, 0, truth, evid, poses)
    return g, truth, poses, evid, ranges


def test_workgroups_stride_over_the_robots():
    """more robots than workgroups in a launch (65536): the last three are served by workgroups on their second turn, with
    their own noise"""
    g, truth, poses, evid, ranges = _strided_fleet()
    dev = _Device(g, truth, NOISY)
    got, _ = dev.observe(1, 5, poses, replay=False)
    dev.evid = evid.copy()
    dev.check_evid()
    guard = np.full(GUARD, G_RANGES, np.int32)
    _same(got, np.concatenate([guard, ranges.reshape(-1), guard]), "ranges")
    assert (ranges[-3:] != ranges[:3]).any()


def test_sharding_by_robot0():
    """one call over P robots equals two calls over the halves with robot0 = 0 and robot0 = P / 2, bitwise (and a call that
    starts the whole fleet at robot0 = P / 2 does not)"""
    g, truth, poses = tgs._fleet(300)
    whole = _Device(g, truth, NOISY)
    got, want = whole.observe(9, 4, poses)
    _same(got, want, "ranges")
    whole.check_evid()
    halves = _Device(g, truth, NOISY)
    lo, _ = halves.observe(9, 4, poses[:150], robot0=0, replay=False)
    hi, _ = halves.observe(9, 4, poses[150:], robot0=150, replay=False)
    assert np.array_equal(halves.image(), whole.image())
    assert np.array_equal(np.concatenate([lo[GUARD:-GUARD], hi[GUARD:-GUARD]]), got[GUARD:-GUARD])
    other = _Device(g, truth, NOISY)
    other.observe(9, 4, poses, robot0=150, replay=False)
    assert not np.array_equal(other.image(), whole.image())


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_publish_is_the_table_lookup(shift):
    """a 70 x 3 grid of hand-made evidence with the int32 extremes and both sides of the clamp; the evidence starts 37 .. 40
    elements into its allocation (the kernel loads 16 bytes at a time from the first 16-byte boundary on: every head length),
    `known` 37 .. 40 bytes into its own.  known = the table lookup; d_counts = eea_grid_census of the published grid and is
    overwritten, not added to; with d_counts null nothing else changes"""
    g = tgs._geom(70, 3)
    ev = IDEAL
    rng = np.random.default_rng(shift)
    evid = rng.integers(-1100, 1101, size=(3, 70)).astype(np.int32)
    special = [-2 ** 31, -1025, -1024, -1, 0, 1, 1024, 1025, 2 ** 31 - 1, -7, 25, 0, 0]
    evid.reshape(-1)[rng.permutation(210)[:len(special)]] = special
    evid[0, 0], evid[2, 69] = -2 ** 31, 2 ** 31 - 1
    ebuf = torch.as_tensor(np.concatenate([np.full(GUARD + shift, G_EVID, np.int32), evid.reshape(-1),
                                           np.full(GUARD, G_EVID, np.int32)])).cuda()
    d_evid = ebuf[GUARD + shift:GUARD + shift + 210]
    table = capi.evidence_table(_ecfg(ev))
    want = er.publish(ev, evid, table)
    assert np.array_equal(want, er.publish(ev, evid)) and {-1, 1, 99, 35, 90} <= set(want.reshape(-1).tolist())
    images = []
    for with_counts in (True, False):
        kbuf = torch.full((2 * GUARD + shift + 210,), G_KNOWN, dtype=torch.int8, device="cuda")
        d_known = kbuf[GUARD + shift:GUARD + shift + 210]
        counts = torch.full((5,), 123456789, dtype=torch.int64, device="cuda")
        census = torch.zeros(3, dtype=torch.int64, device="cuda")
        for _ in range(2):
            capi.evidence_publish(tgs._cfg(g), _ecfg(ev), d_evid, d_known, counts[1:4] if with_counts else None)
        capi.grid_census(tgs._cfg(g), d_known, census)
        torch.cuda.synchronize()
        got = kbuf.cpu().numpy()
        _same(got, np.concatenate([np.full(GUARD + shift, G_KNOWN, np.int8), want.reshape(-1), np.full(GUARD, G_KNOWN, np.int8)]),
              "known")
        c = counts.cpu().numpy()
        assert c[0] == c[4] == 123456789
        if with_counts:
            assert tuple(int(v) for v in c[1:4]) == tuple(int(v) for v in census.cpu().numpy()) == sr.census(g, want)
            assert int(c[1:4].sum()) == 210 and (c[1:4] > 0).all()
        else:
            assert (c[1:4] == 123456789).all()
        images.append(got)
    assert np.array_equal(images[0], images[1])
    assert np.array_equal(ebuf.cpu().numpy()[GUARD + shift:GUARD + shift + 210], evid.reshape(-1))   # read only


@pytest.mark.parametrize("shift", [0, 3])
def test_publish_past_both_launch_caps(shift):
    """2048 x 1025 cells: 524 800 loads of four cells.  A counting launch is capped at 256 workgroups (its threads take nine
    steps of the body loop), one without counts at 2048 (the first threads take a second step); every smaller grid in this file
    gives each thread at most one load.  known = the table lookup, whole and between guard bytes; d_counts = eea_grid_census of
    the published grid, between guard words"""
    xs, ys = 2048, 1025
    n = xs * ys
    assert n // 4 - 1 > 2048 * 256
    g, ev = tgs._geom(xs, ys), IDEAL
    rng = np.random.default_rng(100 + shift)
    evid = rng.integers(-1100, 1101, size=(ys, xs)).astype(np.int32)
    evid[rng.random((ys, xs)) < 0.2] = 0
    evid[0, :8], evid[-1, -8:] = -2 ** 31, 2 ** 31 - 1
    ebuf = torch.as_tensor(np.concatenate([np.full(GUARD + shift, G_EVID, np.int32), evid.reshape(-1),
                                           np.full(GUARD, G_EVID, np.int32)])).cuda()
    d_evid = ebuf[GUARD + shift:GUARD + shift + n]
    want = er.publish(ev, evid, capi.evidence_table(_ecfg(ev)))
    image = np.concatenate([np.full(GUARD + shift, G_KNOWN, np.int8), want.reshape(-1), np.full(GUARD, G_KNOWN, np.int8)])
    for with_counts in (True, False):
        kbuf = torch.full((2 * GUARD + shift + n,), G_KNOWN, dtype=torch.int8, device="cuda")
        d_known = kbuf[GUARD + shift:GUARD + shift + n]
        counts = torch.full((5,), 123456789, dtype=torch.int64, device="cuda")
        census = torch.zeros(3, dtype=torch.int64, device="cuda")
        capi.evidence_publish(tgs._cfg(g), _ecfg(ev), d_evid, d_known, counts[1:4] if with_counts else None)
        capi.grid_census(tgs._cfg(g), d_known, census)
        torch.cuda.synchronize()
        _same(kbuf.cpu().numpy(), image, "known")
        c = counts.cpu().numpy()
        assert c[0] == c[4] == 123456789
        assert tuple(int(v) for v in census.cpu().numpy()) == sr.census(g, want)
        if with_counts:
            assert tuple(int(v) for v in c[1:4]) == sr.census(g, want) and (c[1:4] > 100000).all()
        else:
            assert (c[1:4] == 123456789).all()
    assert np.array_equal(ebuf.cpu().numpy()[GUARD + shift:GUARD + shift + n], evid.reshape(-1))   # read only


def test_join_feeds_the_mutual_information():
    """a 48 x 40 grid with walls, 6 robots, 8 noisy scans, then the publication: evidence and published grid equal the
    restatement, and eea_sense_mi_field on the published grid (R = 6, stride 1) equals tests/mi_restatement.py bit for bit"""
    g, ev, R, truth, poses, evid = er.join_scene()
    dev = _Device(g, truth, ev)
    for scan in range(8):
        dev.observe(R, scan, poses, want_ranges=False, replay=False)
    dev.evid = evid.copy()
    dev.check_evid()
    _, kbuf, d_known = tgs._guarded(np.full((40, 48), 55, np.int8), G_KNOWN, np.int8)
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    d_mi = torch.full((40, 48), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    capi.evidence_publish(dev.cfg, dev.ecfg, dev.d_evid, d_known, counts)
    capi.sense_mi_field(dev.cfg, R, 1, d_known, d_mi, p_unknown=0.5)
    torch.cuda.synchronize()
    known = er.publish(ev, evid)
    _same(kbuf.cpu().numpy(), np.concatenate([np.full(GUARD, G_KNOWN, np.int8), known.reshape(-1), np.full(GUARD, G_KNOWN, np.int8)]),
          "known")
    assert tuple(int(v) for v in counts.cpu().numpy()) == sr.census(g, known)
    h, pass_ = capi.sense_mi_table(dev.cfg, 0.5)
    want = mr.mi_field(g, R, 1, known, h, pass_)
    got = d_mi.cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert (got > 0).any()


def test_a_second_stream_and_the_same_bits_twice():
    """observe, observe, publish on a non-default stream, twice on fresh evidence: identical bits, equal to the restatement"""
    g, truth, poses, after = _noisy_scene()
    stream = torch.cuda.Stream()
    images = []
    for _ in range(2):
        dev = _Device(g, truth, NOISY)
        kbuf = torch.full((2 * GUARD + 29 * 37,), G_KNOWN, dtype=torch.int8, device="cuda")
        counts = torch.zeros(3, dtype=torch.int64, device="cuda")
        d_pose = torch.as_tensor(np.asarray(poses, dtype=np.float64)).cuda()
        d_ranges = torch.full((2, len(poses), 48), S_RANGES, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for scan in range(2):
            capi.sense_observe_batch(dev.cfg, dev.ecfg, 6, scan, dev.d_truth, dev.d_evid, d_pose, d_ranges[scan],
                                     stream=stream.cuda_stream)
        capi.evidence_publish(dev.cfg, dev.ecfg, dev.d_evid, kbuf[GUARD:-GUARD], counts, stream=stream.cuda_stream)
        # P == 0: EEA_OK, nothing launched
        capi.check(capi.lib().eea_sense_observe_batch(0, dev.cfg, dev.ecfg, 6, 9, 0, dev.d_truth.data_ptr(), dev.d_evid.data_ptr(),
                                                      d_pose.data_ptr(), None, 0, None, stream.cuda_stream))
        stream.synchronize()
        dev.evid = after[1][0].copy()
        dev.check_evid()
        assert np.array_equal(d_ranges.cpu().numpy(), np.stack([after[0][1], after[1][1]]))
        images.append((dev.image(), kbuf.cpu().numpy(), counts.cpu().numpy(), d_ranges.cpu().numpy()))
    for a, b in zip(*images):
        assert np.array_equal(a, b)
    known = er.publish(NOISY, after[1][0])
    assert np.array_equal(images[0][1][GUARD:-GUARD].reshape(29, 37), known)
    assert tuple(int(v) for v in images[0][2]) == sr.census(g, known)

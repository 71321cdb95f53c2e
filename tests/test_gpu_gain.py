"""The information-gain field and target on the device (include/ergodic_amd.h: eea_sense_gain_field, eea_set_target_gain;
csrc/gain_kernel.hip): what a scan from each cell of the known grid would reveal, and phi_k from it without a host wait.

Checker: the numpy restatement tests/gain_restatement.py (held to an independent statement in exact fractions by
tests/test_gain.py).  The field is integers and is compared BITWISE, as a whole buffer: d_gain sits between guard elements and
holds a sentinel before the call (every element must be overwritten), `known` sits between guard bytes 37 bytes into its
allocation and must come back unchanged.  phi_k is compared bitwise with the two existing entries it is defined by."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import pyoracle as po
from ergodic_exploration_amd import capi
from tests import gain_restatement as gr
from tests import gain_scenes as gs
from tests import sense_restatement as sr

pytestmark = pytest.mark.gpu

GUARD = 37                        # elements in front of and behind every checked buffer
G_KNOWN, G_GAIN = 0x3C, 0x5A5A5A5A
S_GAIN = 0x7BCDEF01               # what d_gain holds before a call: above 8 R^2 + 1 for every R


def _cfg(g):
    # (radii Collision::Collision would refuse: the field must not look at them)
    return capi.make_collision_cfg(g.xmin, g.ymin, g.resolution, g.xsize, g.ysize, 0.7, 0.1, 0.2, g.occupied_threshold)


def _guarded(values, guard_value, dtype):
    flat = np.asarray(values, dtype=dtype).reshape(-1)
    img = np.concatenate([np.full(GUARD, guard_value, dtype), flat, np.full(GUARD, guard_value, dtype)])
    buf = torch.as_tensor(img).cuda()
    return img, buf, buf[GUARD:GUARD + flat.size]


class _Device:
    """`known` of one grid on the device between guard bytes, and a guarded, sentinel-filled d_gain per call"""

    def __init__(self, g, known):
        self.g, self.cfg, self.known = g, _cfg(g), np.ascontiguousarray(known, dtype=np.int8)
        self._kimg, self._kbuf, self.d_known = _guarded(self.known, G_KNOWN, np.int8)

    def gain_buffer(self):
        return _guarded(np.full(self.known.size, S_GAIN, np.int32), G_GAIN, np.int32)

    def field(self, R, stride, stream=None):
        """one call; returns the field as uint32 [ysize][xsize] after checking the guards and that `known` is unchanged"""
        img, buf, d_gain = self.gain_buffer()
        torch.cuda.synchronize()      # (the uploads above ran on torch's stream)
        capi.sense_gain_field(self.cfg, R, stride, self.d_known, d_gain, stream=stream)
        torch.cuda.synchronize()
        return self.checked(buf)

    def checked(self, buf):
        got = buf.cpu().numpy()
        assert (got[:GUARD] == G_GAIN).all() and (got[-GUARD:] == G_GAIN).all(), "a guard element of d_gain was written"
        assert np.array_equal(self._kbuf.cpu().numpy(), self._kimg), "known was written"
        return got[GUARD:-GUARD].view(np.uint32).reshape(self.known.shape)


def _same(got, want):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "gain differs at %s: got %s want %s" % (bad[:6].tolist(), [int(got[tuple(b)]) for b in bad[:6]],
                                                                   [int(want[tuple(b)]) for b in bad[:6]])


@functools.lru_cache(maxsize=None)
def _restated(xs, ys, R, stride):
    g, known = gs.partly_revealed(xs, ys)
    want = gr.gain_field(g, R, stride, known)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("xs,ys", [(23, 19), (64, 41)])
@pytest.mark.parametrize("stride", [1, 2, 3, 5])
@pytest.mark.parametrize("R", [1, 2, 3, 9, 17])
def test_field_is_the_restatement(R, stride, xs, ys):
    """the partly revealed scenes of tests/gain_scenes.py: frontiers in the open and behind walls, blocking candidates, the
    79 / 80 pair, candidates whose rays leave the grid on every side; (64, 41) is two tiles wide at stride 1 (ragged), and more
    than one tile high from stride 1 to 5 down to a single ragged tile"""
    g, known = gs.partly_revealed(xs, ys)
    got = _Device(g, known).field(R, stride)
    _same(got, _restated(xs, ys, R, stride))
    assert (got > 0).any() and got.max() <= 8 * R * R + 1


@functools.lru_cache(maxsize=None)
def _clutter(xs, ys, seed=7):
    """a random grid in blocks of 3 x 5 cells: 45 % unknown, 45 % free, walls, and the 79 / 80 pair sprinkled in"""
    rng = np.random.default_rng(seed + xs)
    blocks = rng.choice(np.array([-1, 0, 100], dtype=np.int8), size=(ys // 3 + 1, xs // 5 + 1), p=[0.45, 0.45, 0.1])
    known = np.ascontiguousarray(np.kron(blocks, np.ones((3, 5), dtype=np.int8))[:ys, :xs])
    known[rng.integers(0, ys, 12), rng.integers(0, xs, 12)] = 79
    known[rng.integers(0, ys, 12), rng.integers(0, xs, 12)] = 80
    known.setflags(write=False)
    return sr.Geometry(gs.XMIN, gs.YMIN, gs.RES, xs, ys, gs.THR), known


@pytest.mark.parametrize("stride", [1, 3])
def test_more_than_one_tile_in_both_directions(stride):
    """150 x 70 at R = 3: a tile is 32 x 8 candidates, so 5 x 9 tiles at stride 1 and 2 x 3 at stride 3, the last tile ragged in
    both directions, 150 and 70 multiples of neither 32, 8 nor 3"""
    g, known = _clutter(150, 70)
    _same(_Device(g, known).field(3, stride), gr.gain_field(g, 3, stride, known))


@pytest.mark.parametrize("xs,ys,stride", [(1, 1, 1), (1, 1, 4), (65, 1, 1), (1, 65, 1), (65, 1, 2), (3, 5, 7), (33, 9, 32)])
@pytest.mark.parametrize("cell", [-1, 0])
def test_degenerate_grids(xs, ys, stride, cell):
    """one cell, one row and one column of 65 (the 33rd lane group / the 9th candidate row start a tile), a grid smaller than
    the stride (one candidate, (0, 0)) and a stride of a whole tile row; all unknown and all free"""
    g = sr.Geometry(gs.XMIN, gs.YMIN, gs.RES, xs, ys, gs.THR)
    known = np.full((ys, xs), cell, dtype=np.int8)
    known[ys // 2, xs // 2] = -1 if cell == 0 else 100
    for R in (1, 4):
        _same(_Device(g, known).field(R, stride), gr.gain_field(g, R, stride, known))


@pytest.mark.parametrize("R,stride,lds", [(3, 16, True), (3, 17, False), (118, 1, True), (119, 1, False), (60, 8, True),
                                          (61, 8, False), (256, 64, False)])
def test_each_side_of_every_switch(R, stride, lds):
    """the march runs in an LDS window of (31 stride + 1 + 2R) x (7 stride + 1 + 2R) bytes when that fits 64 KB and in global
    memory otherwise: the last (R, stride) on the LDS side and the first on the global side along stride (R = 3), along R
    (stride 1) and at stride 8, and an R far on the global side.  Small grids: the restatement's cost is candidates x rays x steps;
    here the rays mostly end at the grid's edge."""
    W, H = 31 * stride + 1 + 2 * R, 7 * stride + 1 + 2 * R
    assert (W * H <= 65536) == lds
    xs, ys = (150, 70) if R == 3 else (41, 9) if R < 256 else (70, 3)
    g, known = _clutter(xs, ys)
    _same(_Device(g, known).field(R, stride), gr.gain_field(g, R, stride, known))


def test_more_tiles_than_workgroups():
    """a launch has at most 65 536 workgroups, which stride over the tiles: one row of 65 539 tiles and 5 cells (the third
    switch of the kernel).  The restatement would take minutes on 2 097 253 candidates, so it is held on three windows -- the
    first tiles, the tiles around number 65 536, the last ones: with R = 1 a candidate more than a cell inside a window sees
    the window only -- and the whole row against the contract written out for one row at R = 1: of the 8 rays only (1, 0) and
    (-1, 0) stay on the row, one step each, so gain[j] = [k[j] < 0] + [k[j - 1] < 0] + [k[j + 1] < 0] unless k[j] blocks."""
    xs = 32 * 65539 + 5
    rng = np.random.default_rng(5)
    known = rng.choice(np.array([-1, -1, 0, 0, 0, 100, 79, 80], dtype=np.int8), size=(1, xs))
    g = sr.Geometry(gs.XMIN, gs.YMIN, gs.RES, xs, 1, gs.THR)
    got = _Device(g, known).field(1, 1)
    unknown = np.concatenate([[0], (known[0] < 0).astype(np.uint32), [0]])
    want = np.where(known[0] >= 80, 0, unknown[1:-1] + unknown[:-2] + unknown[2:]).astype(np.uint32)
    _same(got, want[None, :])
    for a, b in ((0, 200), (32 * 65536 - 100, 32 * 65536 + 100), (xs - 200, xs)):
        w = sr.Geometry(gs.XMIN, gs.YMIN, gs.RES, b - a, 1, gs.THR)
        part = gr.gain_field(w, 1, 1, known[:, a:b])
        lo, hi = (0 if a == 0 else 1), (b - a if b == xs else b - a - 1)
        _same(got[:, a + lo:a + hi], part[:, lo:hi])


def test_calls_in_a_row_and_on_a_second_stream():
    """two calls in a row on one stream and a call on a second stream: the same bits (a pure function of its arguments)"""
    g, known = gs.partly_revealed(64, 41)
    dev = _Device(g, known)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    first = dev.field(9, 2, stream=s1.cuda_stream)
    _same(first, _restated(64, 41, 9, 2))
    _same(dev.field(9, 2, stream=s1.cuda_stream), first)
    _same(dev.field(9, 2, stream=s2.cuda_stream), first)
    # back to back into two buffers without a synchronisation in between
    (_, b1, g1), (_, b2, g2) = dev.gain_buffer(), dev.gain_buffer()
    torch.cuda.synchronize()
    capi.sense_gain_field(dev.cfg, 9, 2, dev.d_known, g1, stream=s1.cuda_stream)
    capi.sense_gain_field(dev.cfg, 9, 2, dev.d_known, g2, stream=s1.cuda_stream)
    torch.cuda.synchronize()
    _same(dev.checked(b1), first)
    _same(dev.checked(b2), first)


def _engine(K, res, precision=capi.PREC_F64):
    lim = np.array([1.0, 1.0, 2.0])
    return capi.Engine(capi.make_config(capi.MODEL_OMNI, 0.1, 2.0, res, 1.0, K, np.diag([1.0, 1.0, 2.0]), -lim, lim,
                                        precision=precision))


@pytest.mark.parametrize("precision", [pytest.param(capi.PREC_F64, id="fp64"), pytest.param(capi.PREC_F32, id="fp32")])
@pytest.mark.parametrize("floor", [0.5, 0.0])
def test_set_target_gain(precision, floor):
    """phi_k of eea_set_target_gain is BITWISE that of eea_spatial_coeff_rows (whole grid) + eea_set_phik_from_sums fed the
    host-built value grid; in fp64 it is within 1e-11 (the bound tests/test_gpu_phik_parity.py holds the normalised occupancy
    target to) of the oracle's spatialCoeff on v / sum(v); the optional d_gain is the field call's; a second call on a second
    stream gives the same bits"""
    xs, ys, R, stride, K = 64, 41, 9, 2, 10
    g, known = gs.partly_revealed(xs, ys)
    npt, tt = (np.float32, torch.float32) if precision == capi.PREC_F32 else (np.float64, torch.float64)
    lx, ly = (xs - 1) * g.resolution, (ys - 1) * g.resolution
    gain = _restated(xs, ys, R, stride)
    v = gr.value_grid(g, stride, known, gain, floor, npt)
    assert v.sum() > 0 and (v[::stride, ::stride] == 0).any()      # (blocking candidates: no floor there)
    dev = _Device(g, known)
    eng = _engine(K, g.resolution, precision)
    _, buf, d_gain = dev.gain_buffer()
    torch.cuda.synchronize()
    eng.set_target_gain(dev.cfg, R, stride, dev.d_known, lx, ly, floor=floor, gain=d_gain)
    torch.cuda.synchronize()
    _same(dev.checked(buf), gain)
    got = eng.phik()
    d_v = torch.as_tensor(v).cuda()
    sums = torch.empty(K * K, dtype=tt, device="cuda")
    eng.spatial_coeff_rows(xs, ys, 0, ys, d_v, lx, ly, sums)
    eng.set_phik_from_sums(sums, lx, ly)
    torch.cuda.synchronize()
    want = eng.phik()
    assert np.isfinite(want).all() and np.array_equal(got, want), np.abs(got - want).max()
    if precision == capi.PREC_F64:
        ref = po.spatial_coeff(lx, ly, K, (v / v.sum()).reshape(-1), po.phi_grid(xs, ys, g.resolution))
        err = np.abs(got - ref).max()
        print("max |phi_k - oracle| = %.3e" % err)
        assert err < 1e-11
    st = torch.cuda.Stream()
    eng.set_target_gain(dev.cfg, R, stride, dev.d_known, lx, ly, floor=floor, stream=st.cuda_stream)   # (no d_gain: the engine's)
    torch.cuda.synchronize()
    assert np.array_equal(eng.phik(), want)
    dev.checked(buf)
    eng.close()


def _entropy_target(occ):
    lut = np.array([po.lib().eo_entropy(float(np.int8(np.uint8(b))) / 100.0) for b in range(256)])
    ent = lut[occ.reshape(-1).view(np.uint8)]
    return ent / ent.sum()


def test_closed_loop_with_the_gain_target():
    """the geometry of test_gpu_sense.py::test_closed_loop_reveals_the_map (6 robots, 25 ticks, 120 x 60 cells) with the
    re-target replaced by eea_set_target_gain (R 15, stride 2, floor 0.5): per tick reveal -> census -> gain target -> tick on
    the known grid -> motion, nothing between them but enqueues.  The final known grid is the restatement replayed over the
    recorded poses, the unknown count never rises, and the last phi_k is the oracle's for the restated gain of the final grid
    (1e-11).  The unknown count per tick is printed beside the entropy-target loop's; which explores faster is not asserted
    (nobody has measured it)."""
    B, ticks, R, K, res, dt, stride, floor = 6, 25, 15, 10, 0.1, 0.1, 2, 0.5
    xs, ys = 120, 60
    g = sr.Geometry(0.0, 0.0, res, xs, ys, gs.THR)
    truth = np.zeros((ys, xs), dtype=np.int8)
    truth[0], truth[-1], truth[:, 0], truth[:, -1] = 100, 100, 100, 100
    truth[:38, 45:47] = 100
    truth[25:, 80:82] = 100
    truth[28:32, 20:30] = 100
    ccfg = capi.make_collision_cfg(0.0, 0.0, res, xs, ys, 0.2, 0.4, 0.05, gs.THR)
    dcfg = capi.DwaCfg(0.1, 1.0, 0.2, 2.5, 2.5, 1.0, 1.0, -1.0, 1.0, -1.0, 2.0, -2.0, 3, 8, 5)
    lx, ly = (xs - 1) * res, (ys - 1) * res
    poses0 = np.array([[1.5, 1.5, 0.0], [3.0, 4.5, 1.0], [6.2, 1.2, 2.0], [6.5, 4.8, -1.0], [10.0, 3.0, 3.0], [9.2, 1.0, 0.5]])
    zeros = lambda *s, dtype=torch.float64: torch.zeros(s, dtype=dtype, device="cuda")
    d_truth = torch.as_tensor(truth).cuda()

    def loop(retarget):
        eng = _engine(K, res)
        T = eng.T
        d_pose = torch.as_tensor(poses0).cuda()
        d_known = torch.full((ys, xs), -1, dtype=torch.int8, device="cuda")
        d_counts = zeros(3, dtype=torch.int64)
        d_ut, d_traj = zeros(B, T, 3), zeros(B, T, 3)
        d_follow, d_count, d_valid, d_skip = (zeros(B, dtype=torch.int32) for _ in range(4))
        d_u, d_vb = zeros(B, 3), zeros(B, 3)
        recorded, unknown = [], []
        for _ in range(ticks):
            torch.cuda.synchronize()
            recorded.append(d_pose.cpu().numpy().copy())
            capi.sense_reveal_batch(ccfg, R, d_truth, d_known, d_pose)
            capi.grid_census(ccfg, d_known, d_counts)
            retarget(eng, d_known)
            eng.tick_batch(B, d_pose, d_ut, d_follow, d_count, d_u, d_vb, d_known, d_traj, d_valid, d_skip, ccfg, dcfg, 0.1, 0.5,
                           grid_epoch=0)
            capi.integrate_twist_batch(d_pose, d_u, dt, normalize_heading=True)
            d_vb.copy_(d_u)
            torch.cuda.synchronize()
            c = d_counts.cpu().numpy()
            assert int(c.sum()) == xs * ys
            unknown.append(int(c[0]))
        phik = eng.phik()
        eng.close()
        return recorded, unknown, d_known.cpu().numpy(), phik

    recorded, unknown, got, phik = loop(lambda eng, d_known: eng.set_target_gain(ccfg, R, stride, d_known, lx, ly, floor=floor))
    _, unknown_entropy, _, _ = loop(lambda eng, d_known: eng.set_target_occupancy(xs, ys, d_known, lx, ly))
    print("unknown cells per tick, gain target:   ", unknown)
    print("unknown cells per tick, entropy target:", unknown_entropy)
    known = np.full((ys, xs), -1, dtype=np.int8)
    for p in recorded:
        sr.reveal(g, R, truth, known, p)
    assert np.array_equal(got, known)
    assert unknown[-1] == int((known < 0).sum())
    assert all(b <= a for a, b in zip(unknown, unknown[1:]))
    assert np.isfinite(recorded[-1]).all() and np.abs(recorded[-1] - recorded[0]).max() > 0.0
    v = gr.value_grid(g, stride, known, gr.gain_field(g, R, stride, known), floor)
    ref = po.spatial_coeff(lx, ly, K, (v / v.sum()).reshape(-1), po.phi_grid(xs, ys, res))
    err = np.abs(phik - ref).max()
    print("max |phi_k - oracle| after the last re-target: %.3e" % err)
    assert err < 1e-11


def test_gain_argument_errors_write_nothing():
    g, known = gs.partly_revealed(23, 19)
    dev = _Device(g, known)
    _, buf, d_gain = dev.gain_buffer()
    eng = _engine(5, g.resolution)
    before = eng.phik()
    lx, ly = 22 * g.resolution, 18 * g.resolution
    for kw, status in ((dict(R=0), capi.ERR_INVALID_ARGUMENT), (dict(stride=0), capi.ERR_INVALID_ARGUMENT),
                       (dict(R=1025), capi.ERR_UNSUPPORTED), (dict(known=None), capi.ERR_INVALID_ARGUMENT)):
        a = dict(dict(R=5, stride=2, known=dev.d_known), **kw)
        with pytest.raises(capi.EngineError) as ei:
            capi.sense_gain_field(dev.cfg, a["R"], a["stride"], a["known"], d_gain)
        assert ei.value.status == status, kw
        with pytest.raises(capi.EngineError) as ei:
            eng.set_target_gain(dev.cfg, a["R"], a["stride"], a["known"], lx, ly, floor=0.5, gain=d_gain)
        assert ei.value.status == status, kw
    for kw in (dict(floor=-1.0), dict(floor=float("nan")), dict(lx=0.0)):
        a = dict(dict(floor=0.5, lx=lx), **kw)
        with pytest.raises(capi.EngineError) as ei:
            eng.set_target_gain(dev.cfg, 5, 2, dev.d_known, a["lx"], ly, floor=a["floor"], gain=d_gain)
        assert ei.value.status == capi.ERR_INVALID_ARGUMENT, kw
    with pytest.raises(capi.EngineError) as ei:
        capi.sense_gain_field(dev.cfg, 5, 2, dev.d_known, None)
    assert ei.value.status == capi.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert (dev.checked(buf) == S_GAIN).all() and np.array_equal(eng.phik(), before)   # no refused call wrote anything
    eng.close()

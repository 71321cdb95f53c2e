"""The mutual-information field and target on the device (include/ergodic_amd.h: eea_sense_mi_field, eea_set_target_mi;
csrc/mi_kernel.hip): the information a scan from each cell of the known grid is expected to yield, and phi_k from it without a
host wait.

Checker: the restatement tests/mi_restatement.py (held to the entropy of the beam's measurement over every map by
tests/test_mi.py), fed THE LIBRARY'S OWN TABLE (eea_sense_mi_table): the field is fp64 in a fixed order and is compared BITWISE,
as a whole buffer, whatever libm evaluated the logs.  d_mi sits between guard elements and holds a NaN sentinel before the call
(every element must be overwritten), `known` sits between guard bytes 37 bytes into its allocation and must come back unchanged.
phi_k is compared bitwise with the two existing entries it is defined by."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ergodic_exploration_amd import capi
from tests import gain_scenes as gs
from tests import mi_restatement as mr
from tests import mi_scenes as ms
from tests import sense_restatement as sr

pytestmark = pytest.mark.gpu

GUARD = 37                                         # elements in front of and behind every checked buffer
G_KNOWN, G_MI = 0x3C, 0x40934A0000000000           # (the guard of d_mi: the double 1234.5)
S_MI = 0x7FF8DEADBEEF0001                          # what d_mi holds before a call: a NaN no sum produces


def _cfg(g):
    # (radii Collision::Collision would refuse: the field must not look at them)
    return capi.make_collision_cfg(g.xmin, g.ymin, g.resolution, g.xsize, g.ysize, 0.7, 0.1, 0.2, g.occupied_threshold)


def _guarded(values, guard_value, dtype):
    flat = np.asarray(values, dtype=dtype).reshape(-1)
    img = np.concatenate([np.full(GUARD, guard_value, dtype), flat, np.full(GUARD, guard_value, dtype)])
    buf = torch.as_tensor(img).cuda()
    return img, buf, buf[GUARD:GUARD + flat.size]


class _Device:
    """`known` of one grid on the device between guard bytes, and a guarded, sentinel-filled d_mi (as int64 bits) per call"""

    def __init__(self, g, known):
        self.g, self.cfg, self.known = g, _cfg(g), np.ascontiguousarray(known, dtype=np.int8)
        self._kimg, self._kbuf, self.d_known = _guarded(self.known, G_KNOWN, np.int8)

    def mi_buffer(self):
        return _guarded(np.full(self.known.size, S_MI, np.int64), G_MI, np.int64)

    def field(self, R, stride, p_unknown, stream=None):
        """one call; returns the field's bits as uint64 [ysize][xsize] after checking the guards and that `known` is unchanged"""
        _, buf, d_mi = self.mi_buffer()
        torch.cuda.synchronize()      # (the uploads above ran on torch's stream)
        capi.sense_mi_field(self.cfg, R, stride, self.d_known, d_mi, p_unknown=p_unknown, stream=stream)
        torch.cuda.synchronize()
        return self.checked(buf)

    def checked(self, buf):
        got = buf.cpu().numpy()
        assert (got[:GUARD] == G_MI).all() and (got[-GUARD:] == G_MI).all(), "a guard element of d_mi was written"
        assert np.array_equal(self._kbuf.cpu().numpy(), self._kimg), "known was written"
        return got[GUARD:-GUARD].view(np.uint64).reshape(self.known.shape)

    def restated(self, R, stride, p_unknown):
        h, pass_ = capi.sense_mi_table(self.cfg, p_unknown)
        return mr.mi_field(self.g, R, stride, self.known, h, pass_)


def _same(got_bits, want):
    want_bits = np.ascontiguousarray(want, dtype=np.float64).view(np.uint64)
    bad = np.argwhere(got_bits != want_bits)
    assert bad.size == 0, "mi differs at %s: got %s want %s" % (
        bad[:6].tolist(), [float(got_bits[tuple(b)].view(np.float64)) for b in bad[:6]], [float(want[tuple(b)]) for b in bad[:6]])


@functools.lru_cache(maxsize=None)
def _restated(xs, ys, R, stride, p_unknown):
    g, known = ms.graded(xs, ys)
    want = _Device.restated(_HostOnly(g, known), R, stride, p_unknown)
    want.setflags(write=False)
    return want


class _HostOnly:
    """what _Device.restated reads, without a device buffer"""

    def __init__(self, g, known):
        self.g, self.cfg, self.known = g, _cfg(g), known


@pytest.mark.parametrize("xs,ys", [(23, 19), (64, 41)])
@pytest.mark.parametrize("p_unknown", [0.5, 0.2])
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("R", [1, 3, 9, 17])
def test_field_is_the_restatement(R, stride, p_unknown, xs, ys):
    """the graded scenes of tests/mi_scenes.py: frontiers in the open and behind walls, a ramp of the values 1 .. 99, the
    79 / 80 pair, 127 and -128, blocking candidates, candidates whose rays leave the grid on every side; (64, 41) is two ragged
    tiles wide at stride 1"""
    g, known = ms.graded(xs, ys)
    got = _Device(g, known).field(R, stride, p_unknown)
    want = _restated(xs, ys, R, stride, p_unknown)
    _same(got, want)
    assert (want > 0).any() and want.max() <= np.log(2.0) * (8 * R * R + 1)


@functools.lru_cache(maxsize=None)
def _clutter(xs, ys, thr=gs.THR, values=None, seed=11):
    """a random grid in blocks of 3 x 5 cells of unknown, free and wall, with graded cells sprinkled over a third of it"""
    rng = np.random.default_rng(seed + xs)
    blocks = rng.choice(np.array([-1, 0, 100], dtype=np.int8), size=(ys // 3 + 1, xs // 5 + 1), p=[0.4, 0.5, 0.1])
    known = np.ascontiguousarray(np.kron(blocks, np.ones((3, 5), dtype=np.int8))[:ys, :xs])
    n = xs * ys // 3
    pool = np.arange(1, 100) if values is None else np.array(values)
    known[rng.integers(0, ys, n), rng.integers(0, xs, n)] = rng.choice(pool, n).astype(np.int8)
    known.setflags(write=False)
    return sr.Geometry(gs.XMIN, gs.YMIN, gs.RES, xs, ys, thr), known


@pytest.mark.parametrize("stride", [1, 3])
def test_more_than_one_tile_in_both_directions(stride):
    """150 x 70 at R = 3: a tile is 32 x 8 candidates, so 5 x 9 tiles at stride 1 and 2 x 3 at stride 3, the last tile ragged in
    both directions"""
    g, known = _clutter(150, 70)
    dev = _Device(g, known)
    _same(dev.field(3, stride, 0.5), dev.restated(3, stride, 0.5))


@pytest.mark.parametrize("xs,ys,stride", [(1, 1, 1), (65, 1, 1), (1, 65, 1), (3, 5, 7), (33, 9, 32)])
@pytest.mark.parametrize("cell", [-1, 0])
def test_degenerate_grids(xs, ys, stride, cell):
    """one cell, one row and one column of 65 (the 33rd lane group / the 9th candidate row start a tile), a grid smaller than
    the stride (one candidate, (0, 0)) and a stride of a whole tile row; all unknown and all free"""
    g = sr.Geometry(gs.XMIN, gs.YMIN, gs.RES, xs, ys, gs.THR)
    known = np.full((ys, xs), cell, dtype=np.int8)
    dev = _Device(g, known)
    for R in (1, 4):
        got = dev.field(R, stride, 0.5)
        _same(got, dev.restated(R, stride, 0.5))
        assert (got != 0).any() == (cell < 0)


def _window_fits(R, stride):
    return (31 * stride + 1 + 2 * R) * (7 * stride + 1 + 2 * R) + 1648 <= 65536


@pytest.mark.parametrize("R,stride,lds", [(119, 1, False), (116, 1, True), (117, 1, False), (58, 8, True), (59, 8, False)])
def test_each_side_of_the_lds_limit(R, stride, lds):
    """the march runs in LDS when the window of (31 stride + 1 + 2R) x (7 stride + 1 + 2R) class bytes and the 1648-byte table
    fit 64 KB, and in global memory otherwise: R = 119 at stride 1 (a window past 64 KB by itself), and the last (R, stride) on
    the LDS side with the first on the global side at strides 1 and 8.  40 x 30 cells: the restatement is cheap because the
    rays leave the grid early, and both forms of a pair see the same grid"""
    assert _window_fits(R, stride) == lds
    g, known = _clutter(40, 30)
    dev = _Device(g, known)
    _same(dev.field(R, stride, 0.2), dev.restated(R, stride, 0.2))


@pytest.mark.parametrize("thr", [-0.5, 1.1, -2.0])
def test_thresholds_outside_zero_to_one(thr):
    """blocks() looks at the cell VALUE.  At -0.5 the cells -50 .. -1 block and -128 .. -51 do not, although they share
    p_unknown: the compact classes of the LDS form cannot tell them apart and the call marches in global memory.  At 1.1 a
    cell of 105 does not block and one of 115 does, both with h = 0 and pass = 0: only the candidate's own cell tells them
    apart.  At -2 every cell blocks: +0.0 everywhere"""
    g, known = _clutter(41, 23, thr, (-100, -60, -51, -50, -1, 0, 50, 100, 105, 109, 110, 115, 127))
    dev = _Device(g, known)
    for R, stride in ((3, 1), (5, 2)):
        got, want = dev.field(R, stride, 0.5), dev.restated(R, stride, 0.5)
        _same(got, want)
        assert (want > 0).any() == (thr > -2.0)


@pytest.mark.parametrize("R", [1, 2])
def test_device_uses_the_table(R):
    """one row holding every int8 value once: at R = 1 only the rays due east and west stay on the grid, one step each, so
    mi[j] = h(v[j]) + h(v[j + 1]) + h(v[j - 1]) in that order for a cell that does not block -- every h the kernel used; at
    R = 2 the second step brings pass(v[j +- 1]) h(v[j +- 2]): every pass.  The values are shuffled so that neighbours vary"""
    values = np.random.default_rng(3).permutation(np.arange(-128, 128)).astype(np.int8)[None, :]
    g = sr.Geometry(gs.XMIN, gs.YMIN, gs.RES, 256, 1, gs.THR)
    dev = _Device(g, values)
    for p_unknown in (0.5, 0.2):
        got, want = dev.field(R, 1, p_unknown), dev.restated(R, 1, p_unknown)
        _same(got, want)
        if R == 1:
            h, _ = capi.sense_mi_table(dev.cfg, p_unknown)
            v = values[0].astype(int) + 128
            j = np.arange(1, 255)
            direct = np.where(values[0, j] >= 80, 0.0, (h[v[j]] + h[v[j + 1]]) + h[v[j - 1]])
            _same(got[:, 1:255], direct[None, :])


def test_calls_in_a_row_and_on_a_second_stream():
    """two calls in a row on one stream and a call on a second stream: the same bits (a pure function of its arguments)"""
    g, known = ms.graded(64, 41)
    dev = _Device(g, known)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    first = dev.field(9, 3, 0.2, stream=s1.cuda_stream)
    _same(first, _restated(64, 41, 9, 3, 0.2))
    assert np.array_equal(dev.field(9, 3, 0.2, stream=s1.cuda_stream), first)
    assert np.array_equal(dev.field(9, 3, 0.2, stream=s2.cuda_stream), first)
    # into two buffers from two streams without a synchronisation in between
    (_, b1, m1), (_, b2, m2) = dev.mi_buffer(), dev.mi_buffer()
    torch.cuda.synchronize()
    capi.sense_mi_field(dev.cfg, 9, 3, dev.d_known, m1, p_unknown=0.2, stream=s1.cuda_stream)
    capi.sense_mi_field(dev.cfg, 9, 3, dev.d_known, m2, p_unknown=0.2, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(dev.checked(b1), first) and np.array_equal(dev.checked(b2), first)


def _engine(K, res, precision=capi.PREC_F64):
    lim = np.array([1.0, 1.0, 2.0])
    return capi.Engine(capi.make_config(capi.MODEL_OMNI, 0.1, 2.0, res, 1.0, K, np.diag([1.0, 1.0, 2.0]), -lim, lim,
                                        precision=precision))


def _control(eng, npt, tt):
    """the buffers of one control_batch of 4 seeded poses on a fresh zero ut"""
    B = 4
    rng = np.random.default_rng(21)
    poses = np.stack([rng.uniform(1.0, 12.0, B), rng.uniform(1.0, 8.0, B), rng.uniform(-3.0, 3.0, B)], 1).astype(npt)
    d_pose = torch.as_tensor(poses).cuda()
    d_ut = torch.zeros((B, eng.T, 3), dtype=tt, device="cuda")
    d_u0 = torch.empty((B, 3), dtype=tt, device="cuda")
    torch.cuda.synchronize()
    return d_pose, d_ut, d_u0


@pytest.mark.parametrize("precision", [pytest.param(capi.PREC_F64, id="fp64"), pytest.param(capi.PREC_F32, id="fp32")])
@pytest.mark.parametrize("K", [5, 10])
@pytest.mark.parametrize("floor", [0.25, 0.0])
def test_set_target_mi(precision, K, floor):
    """phi_k of eea_set_target_mi is BITWISE that of eea_spatial_coeff_rows (whole grid) + eea_set_phik_from_sums fed the
    host-built value grid of the restated field; the optional d_mi is the field call's; a call without d_mi gives the same bits;
    a second call on a changed `known` follows it; a control pass enqueued on the same stream behind the call, with nothing in
    between, equals one behind the two entries"""
    xs, ys, R, stride, p_unknown = 64, 41, 9, 3, 0.2
    g, known = ms.graded(xs, ys)
    npt, tt = (np.float32, torch.float32) if precision == capi.PREC_F32 else (np.float64, torch.float64)
    lx, ly = (xs - 1) * g.resolution, (ys - 1) * g.resolution
    changed = np.where(known < 0, 0, known).astype(np.int8)       # the map after everything unknown turned out free
    changed[:, :xs // 3] = known[:, :xs // 3]                     # ... but for the left third
    eng = _engine(K, g.resolution, precision)
    st = torch.cuda.Stream()
    for grid in (known, changed):
        dev = _Device(g, grid)
        mi = dev.restated(R, stride, p_unknown) if grid is changed else _restated(xs, ys, R, stride, p_unknown)
        v = mr.value_grid(g, stride, grid, mi, floor, npt)
        assert v.sum() > 0 and (v[::stride, ::stride] == 0).any()      # (blocking candidates: no floor there)
        # the two existing entries, and a control pass behind them
        d_v = torch.as_tensor(v).cuda()
        sums = torch.empty(K * K, dtype=tt, device="cuda")
        d_pose, d_ut, d_u0 = _control(eng, npt, tt)
        eng.spatial_coeff_rows(xs, ys, 0, ys, d_v, lx, ly, sums, stream=st.cuda_stream)
        eng.set_phik_from_sums(sums, lx, ly, stream=st.cuda_stream)
        eng.control_batch(4, d_pose, d_ut, d_u0, stream=st.cuda_stream)
        torch.cuda.synchronize()
        want, want_u0, want_ut = eng.phik(), d_u0.cpu().numpy(), d_ut.cpu().numpy()
        assert np.isfinite(want).all() and np.isfinite(want_u0).all()
        # something else in between, so that the call below has a phi_k to replace
        eng.set_target_gain(dev.cfg, 2, 4, dev.d_known, lx, ly, floor=1.0, stream=st.cuda_stream)
        torch.cuda.synchronize()
        assert not np.array_equal(eng.phik(), want)
        # the call, with d_mi, and the control pass right behind it
        _, buf, d_mi = dev.mi_buffer()
        d_pose, d_ut, d_u0 = _control(eng, npt, tt)
        eng.set_target_mi(dev.cfg, R, stride, dev.d_known, lx, ly, p_unknown=p_unknown, floor=floor, mi=d_mi, stream=st.cuda_stream)
        eng.control_batch(4, d_pose, d_ut, d_u0, stream=st.cuda_stream)
        torch.cuda.synchronize()
        _same(dev.checked(buf), mi)
        got = eng.phik()
        assert np.array_equal(got, want), np.abs(got - want).max()
        assert np.array_equal(d_u0.cpu().numpy(), want_u0) and np.array_equal(d_ut.cpu().numpy(), want_ut)
        # without d_mi: the engine's own workspace
        eng.set_target_gain(dev.cfg, 2, 4, dev.d_known, lx, ly, floor=1.0, stream=st.cuda_stream)
        eng.set_target_mi(dev.cfg, R, stride, dev.d_known, lx, ly, p_unknown=p_unknown, floor=floor, stream=st.cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(eng.phik(), want)
        dev.checked(buf)
    eng.close()


def test_mi_argument_errors_write_nothing():
    g, known = ms.graded(23, 19)
    dev = _Device(g, known)
    _, buf, d_mi = dev.mi_buffer()
    eng = _engine(5, g.resolution)
    before = eng.phik()
    lx, ly = 22 * g.resolution, 18 * g.resolution
    for kw, status in ((dict(R=0), capi.ERR_INVALID_ARGUMENT), (dict(stride=0), capi.ERR_INVALID_ARGUMENT),
                       (dict(R=1025), capi.ERR_UNSUPPORTED), (dict(known=None), capi.ERR_INVALID_ARGUMENT),
                       (dict(p=0.0), capi.ERR_INVALID_ARGUMENT), (dict(p=1.0), capi.ERR_INVALID_ARGUMENT),
                       (dict(p=float("nan")), capi.ERR_INVALID_ARGUMENT)):
        a = dict(dict(R=5, stride=2, known=dev.d_known, p=0.5), **kw)
        with pytest.raises(capi.EngineError) as ei:
            capi.sense_mi_field(dev.cfg, a["R"], a["stride"], a["known"], d_mi, p_unknown=a["p"])
        assert ei.value.status == status, kw
        with pytest.raises(capi.EngineError) as ei:
            eng.set_target_mi(dev.cfg, a["R"], a["stride"], a["known"], lx, ly, p_unknown=a["p"], floor=0.5, mi=d_mi)
        assert ei.value.status == status, kw
    for kw in (dict(floor=-1.0), dict(floor=float("nan")), dict(lx=0.0)):
        a = dict(dict(floor=0.5, lx=lx), **kw)
        with pytest.raises(capi.EngineError) as ei:
            eng.set_target_mi(dev.cfg, 5, 2, dev.d_known, a["lx"], ly, floor=a["floor"], mi=d_mi)
        assert ei.value.status == capi.ERR_INVALID_ARGUMENT, kw
    with pytest.raises(capi.EngineError) as ei:
        capi.sense_mi_field(dev.cfg, 5, 2, dev.d_known, None)
    assert ei.value.status == capi.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert (dev.checked(buf) == S_MI).all() and np.array_equal(eng.phik(), before)   # no refused call wrote anything
    eng.close()

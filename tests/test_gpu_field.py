"""Coverage fields on the device (include/ergodic_amd.h: eea_records_field; csrc/field_kernel.hip): sum records taken back to
the target grid as the band-limited visit density, the deficit against the target and the potential control() descends.

Checker: the float64 numpy restatement tests/field_restatement.py (held to the oracle's fourierBasis by tests/test_field.py)
with the engine's own phi_k / lamda_k from the getters.  Two-Gaussian target, a domain with xmin, ymin != 0.

Bounds per element, S = sum_m |a_m| of the record: fp64 1e-11 S (the project's fp64 tolerance for c_k / phi_k; the
rounding bound (K^2 + 4) 2^-53 S is about 1e-13 S at K = 30), fp32 1e-4 S (SURVEY 8d's fp32 tolerance).  Bitwise where the
entry point promises bits: row tiles, batches, the place of a record in a batch, the alignment of the output."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ergodic_exploration_amd import capi
from tests import field_restatement as fr
from tests.gpu_util import MAP_BOUNDS, MODELS, make_pair

pytestmark = pytest.mark.gpu

TOL, TOL_F32 = 1e-11, 1e-4
RES = 0.1
KINDS = (capi.FIELD_DENSITY, capi.FIELD_DEFICIT, capi.FIELD_POTENTIAL)
BIGGER = (-2.0, 13.0, -1.5, 7.0)   # the map after it has grown: another lx, ly (and grid: 151 x 86)
COUNTS = (0, 1, 37, -1)


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _random_records(rng, K, counts, dtype=np.float64):
    """random coefficient rows: sums of |count| cosine products would lie in [-|count|, |count|]; the rows with counts 0 and
    -1 carry coefficients too (the rule c = 0 is the entry point's, not the record's)"""
    L = (K * K + 2) // 2 * 2
    rec = np.zeros((len(counts), L))
    for j, n in enumerate(counts):
        rec[j, :K * K] = rng.uniform(-1.0, 1.0, K * K) * max(abs(n), 1)
        rec[j, K * K] = n
    return rec.astype(dtype)


def _real_record(eng, K):
    """the history record of one robot with 50 stored poses"""
    rng = np.random.default_rng(50)
    dtype = np.float64 if eng.real_size == 8 else np.float32
    poses = np.stack([rng.uniform(MAP_BOUNDS[0], MAP_BOUNDS[1], 50), rng.uniform(MAP_BOUNDS[2], MAP_BOUNDS[3], 50),
                      rng.uniform(-np.pi, np.pi, 50)], 1).astype(dtype)
    mem = capi.ReplayMemory(1, 64, 8, real_size=eng.real_size)
    d = _dev(poses)
    for t in range(50):
        mem.append(d[t:t + 1])
    rec = torch.empty((1, eng.ck_record_len), dtype=d.dtype, device="cuda")
    mem.history_records(eng, rec)
    torch.cuda.synchronize()
    out = rec.cpu().numpy()
    mem.close()
    assert out[0, K * K] == 50
    return out


def _field(eng, kind, rec, nx, ny, row0=0, nrows=None, fill=float("nan")):
    """the call on a NaN-filled output: every element has to be written"""
    nrows = ny - row0 if nrows is None else nrows
    n = 1 if rec.dim() == 1 else rec.shape[0]
    out = torch.full((n, nrows, nx), fill, dtype=rec.dtype, device="cuda")
    capi.records_field(eng, kind, rec, out, nx, ny, row0, nrows)
    torch.cuda.synchronize()
    return out


def _check(eng, kind, h_rec, got, K, lx, ly, nx, ny, tol, row0=0, nrows=None, res=RES):
    """|got - restatement| <= tol S per element; returns the largest |diff| / S over the records with S > 0"""
    want, S = fr.records_field(kind, h_rec.astype(np.float64), K, lx, ly, res, eng.phik(), eng.lamdak(), nx, ny, row0, nrows)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape
    assert np.isfinite(got).all(), "an element was not written, or a division reached the output"
    worst = 0.0
    for j in range(want.shape[0]):
        err = np.abs(got[j] - want[j]).max()
        assert err <= tol * S[j], (kind, j, err, S[j])
        if S[j] > 0:
            worst = max(worst, err / S[j])
    print("kind %d K = %d %d x %d rows %d+%d: max |diff| / S = %.3e (bound %.0e)" % (kind, K, nx, ny, row0, want.shape[1], worst, tol))
    return worst


@pytest.fixture(scope="module")
def base():
    """fp64, K = 10, the 121 x 61 grid of MAP_BOUNDS: the all-zero record, counts 1, 37, -1 and a real history record; the
    whole-grid fields of the three kinds, computed once"""
    K = 10
    eng, _ = make_pair("omni", K, 1.0)
    assert eng.target_grid_size == (121, 61)
    rng = np.random.default_rng(1)
    h_rec = np.concatenate([np.zeros((1, eng.ck_record_len)), _random_records(rng, K, (1, 37, -1)), _real_record(eng, K)])
    rec = _dev(h_rec)
    fields = {kind: _field(eng, kind, rec, 121, 61) for kind in KINDS}
    b = dict(K=K, eng=eng, h_rec=h_rec, rec=rec, fields=fields, lx=MAP_BOUNDS[1] - MAP_BOUNDS[0], ly=MAP_BOUNDS[3] - MAP_BOUNDS[2])
    yield b
    eng.close()


def test_three_kinds_on_the_shipped_grid(base):
    """1. K = 10, 121 x 61 (odd nx), 5 records, all three kinds against the restatement; the all-zero record: its DENSITY is
    exactly 0 and its DEFICIT is the band-limited target"""
    K, eng = base["K"], base["eng"]
    for kind in KINDS:
        _check(eng, kind, base["h_rec"], base["fields"][kind], K, base["lx"], base["ly"], 121, 61, TOL)
    dens, defi = base["fields"][capi.FIELD_DENSITY].cpu().numpy(), base["fields"][capi.FIELD_DEFICIT].cpu().numpy()
    assert (dens[0] == 0.0).all() and (dens[3] == 0.0).all()       # no count, a negative count
    w = np.where(np.arange(K) > 0, 2.0, 1.0)
    a_target = np.outer(w, w).reshape(-1) * eng.phik() / (base["lx"] * base["ly"])
    assert np.array_equal(defi[0], defi[3])
    zero = np.zeros((1, eng.ck_record_len))
    target, S = fr.records_field(fr.DEFICIT, zero, K, base["lx"], base["ly"], RES, eng.phik(), eng.lamdak(), 121, 61)
    assert S[0] == pytest.approx(np.abs(a_target).sum(), rel=1e-15)
    assert np.abs(defi[0] - target[0]).max() <= TOL * S[0]
    # the default arguments: the engine's target grid, all rows
    out = torch.full((5, 61, 121), float("nan"), dtype=torch.float64, device="cuda")
    capi.records_field(eng, capi.FIELD_POTENTIAL, base["rec"], out)
    torch.cuda.synchronize()
    assert torch.equal(out, base["fields"][capi.FIELD_POTENTIAL])


def _grid_engine(K, nx, ny, precision=capi.PREC_F64, seed=0):
    """an engine whose target is a random grid of nx x ny values on a domain sized to the grid"""
    _, em, rdiag, lim = MODELS["omni"]
    lim = np.array(lim)
    eng = capi.Engine(capi.make_config(em, 0.1, 1.0, RES, 1.0, K, np.diag(rdiag), -lim, lim, precision=precision))
    rng = np.random.default_rng(seed)
    phi = rng.uniform(0.0, 1.0, nx * ny)
    phi /= phi.sum()
    lx, ly = max(nx - 1, 1) * RES, max(ny - 1, 1) * RES
    eng.set_target_grid(nx, ny, phi.astype(np.float64 if precision == capi.PREC_F64 else np.float32), lx, ly)
    assert eng.target_grid_size == (nx, ny)
    return eng, lx, ly


SHAPES = [(5, 7, 5), (1, 3, 2), (20, 37, 19), (30, 66, 9), (32, 130, 3), (10, 5, 300), (10, 300, 3)]


@pytest.mark.parametrize("K,nx,ny", SHAPES)
def test_shapes_that_break_the_tiles(K, nx, ny):
    """2. grids smaller than a tile, one column past the 128-column tile, wide and tall ones, K from 1 to 32; 3 records"""
    eng, lx, ly = _grid_engine(K, nx, ny, seed=K + nx)
    h_rec = _random_records(np.random.default_rng(nx * ny), K, (37, 0, 1))
    rec = _dev(h_rec)
    for kind in KINDS:
        _check(eng, kind, h_rec, _field(eng, kind, rec, nx, ny), K, lx, ly, nx, ny, TOL)
    eng.close()


def _row_tiles(eng, rec, nx, ny, whole):
    for row0, nrows in ((0, 1), (1, 7), (ny - 3, 3), (17, ny - 17)):
        for kind in KINDS:
            tile = _field(eng, kind, rec, nx, ny, row0, nrows)
            assert torch.equal(tile, whole[kind][:, row0:row0 + nrows]), (kind, row0, nrows)


def test_row_tiles_are_slices_of_the_whole_grid(base):
    """3. 121 x 61 and 37 x 19: rows (0, 1), (1, 7), the last 3 and (17, ny - 17) -- bitwise the rows of the whole-grid call
    (the y table is indexed by row0 + r; the row tile's own tiling and alignment do not enter the arithmetic)"""
    _row_tiles(base["eng"], base["rec"], 121, 61, base["fields"])
    K, nx, ny = 20, 37, 19
    eng, lx, ly = _grid_engine(K, nx, ny, seed=3)
    h_rec = _random_records(np.random.default_rng(4), K, (37, 0, 1))
    rec = _dev(h_rec)
    whole = {kind: _field(eng, kind, rec, nx, ny) for kind in KINDS}
    _row_tiles(eng, rec, nx, ny, whole)
    _check(eng, capi.FIELD_DEFICIT, h_rec, _field(eng, capi.FIELD_DEFICIT, rec, nx, ny, 17, 2), K, lx, ly, nx, ny, TOL, 17, 2)
    eng.close()


def test_a_record_alone_is_its_field_in_a_batch(base):
    """4. record j alone, in the batch of 5 and in the batch reversed: the same bits; so is a field written to an output
    that starts 8 bytes past a 16-byte boundary (the wide stores follow the address, not the row index)"""
    eng, rec = base["eng"], base["rec"]
    back = torch.flip(rec, dims=[0]).contiguous()
    for kind in KINDS:
        whole = base["fields"][kind]
        assert torch.equal(torch.flip(_field(eng, kind, back, 121, 61), dims=[0]), whole)
        for j in range(5):
            assert torch.equal(_field(eng, kind, rec[j], 121, 61)[0], whole[j]), (kind, j)
    buf = torch.full((5 * 61 * 121 + 3,), float("nan"), dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    for shift in (1, 2):
        out = buf[shift:shift + 5 * 61 * 121].view(5, 61, 121)
        capi.records_field(eng, capi.FIELD_DENSITY, rec, out, 121, 61)
        torch.cuda.synchronize()
        assert torch.equal(out, base["fields"][capi.FIELD_DENSITY]), shift
        assert torch.isnan(buf[:shift]).all() and torch.isnan(buf[shift + 5 * 61 * 121:]).all()    # nothing outside
        buf.fill_(float("nan"))


def test_many_records_take_the_tall_row_tile_and_the_tile_stride():
    """the launch takes 64 rows per workgroup once there are enough tiles, and its workgroups stride over the tiles past
    65536: 600 records on 37 x 70 (a last row tile of 6 rows) against the same records alone (16 rows per workgroup) and
    the restatement; 70000 records on 3 x 2 at K = 1 against the restatement"""
    K, nx, ny = 5, 37, 70
    eng, lx, ly = _grid_engine(K, nx, ny, seed=9)
    rng = np.random.default_rng(10)
    h_rec = _random_records(rng, K, [int(n) for n in rng.integers(1, 40, 600)])
    rec = _dev(h_rec)
    many = _field(eng, capi.FIELD_DEFICIT, rec, nx, ny)
    for j in (0, 1, 299, 599):
        assert torch.equal(_field(eng, capi.FIELD_DEFICIT, rec[j], nx, ny)[0], many[j]), j
    _check(eng, capi.FIELD_DEFICIT, h_rec[::50], many[::50], K, lx, ly, nx, ny, TOL)
    eng.close()
    K, nx, ny = 1, 3, 2
    eng, lx, ly = _grid_engine(K, nx, ny, seed=11)
    h_rec = _random_records(rng, K, [int(n) for n in rng.integers(-1, 5, 70000)])
    for kind in (capi.FIELD_DENSITY, capi.FIELD_POTENTIAL):
        _check(eng, kind, h_rec, _field(eng, kind, _dev(h_rec), nx, ny), K, lx, ly, nx, ny, TOL)
    eng.close()


def test_no_count_gives_no_non_finite_value(base):
    """5. counts 0 and -1 with coefficients that would divide to inf / NaN or to garbage: every element of the NaN-filled
    output is overwritten with a finite value, and the fields are those of the all-zero record"""
    K, eng = base["K"], base["eng"]
    h_rec = _random_records(np.random.default_rng(5), K, (0, -1, 0, -1))
    h_rec[2, :K * K] = np.inf
    h_rec[3, :K * K] = 1e300
    rec = _dev(h_rec)
    for kind in KINDS:
        got = _field(eng, kind, rec, 121, 61)
        assert torch.isfinite(got).all(), kind
        for j in range(4):
            assert torch.equal(got[j], base["fields"][kind][0]), (kind, j)
    for row0, nrows in ((0, 1), (60, 1), (13, 17)):
        assert torch.isfinite(_field(eng, capi.FIELD_POTENTIAL, rec, 121, 61, row0, nrows)).all()


def test_fp32_engine():
    """6. K = 10, 121 x 61, fp32 engine and records: 1e-4 S; rows of 121 floats start on all four alignments"""
    K = 10
    eng, _ = make_pair("omni", K, 1.0, precision=capi.PREC_F32)
    h_rec = np.concatenate([_random_records(np.random.default_rng(6), K, COUNTS, np.float32), _real_record(eng, K)])
    rec = _dev(h_rec)
    lx, ly = MAP_BOUNDS[1] - MAP_BOUNDS[0], MAP_BOUNDS[3] - MAP_BOUNDS[2]
    whole = {}
    for kind in KINDS:
        whole[kind] = _field(eng, kind, rec, 121, 61)
        _check(eng, kind, h_rec, whole[kind], K, lx, ly, 121, 61, TOL_F32)
    _row_tiles(eng, rec, 121, 61, whole)
    for j in range(5):
        assert torch.equal(_field(eng, capi.FIELD_DEFICIT, rec[j], 121, 61)[0], whole[capi.FIELD_DEFICIT][j]), j
    eng.close()


def test_fields_follow_a_domain_change(base):
    """7. the fields, then eea_config_domain to a larger extent, then the fields of the same records: the second set is the
    restatement in the new lx, ly and phi_k on the new grid; the first set was the restatement in the old ones"""
    K = base["K"]
    eng, _ = make_pair("omni", K, 1.0)
    rec, h_rec = base["rec"], base["h_rec"]
    for kind in KINDS:
        before = _field(eng, kind, rec, 121, 61)
        assert torch.equal(before, base["fields"][kind])     # (another engine, the same domain: the same bits)
        _check(eng, kind, h_rec, before, K, base["lx"], base["ly"], 121, 61, TOL)
    assert eng.config_domain(BIGGER)
    nx, ny = eng.target_grid_size
    assert (nx, ny) == (151, 86)
    lx, ly = BIGGER[1] - BIGGER[0], BIGGER[3] - BIGGER[2]
    for kind in KINDS:
        after = torch.full((5, ny, nx), float("nan"), dtype=torch.float64, device="cuda")
        capi.records_field(eng, kind, rec, after)
        torch.cuda.synchronize()
        _check(eng, kind, h_rec, after, K, lx, ly, nx, ny, TOL)
        # the old grid size in the new domain: only the tables' key changed
        _check(eng, kind, h_rec, _field(eng, kind, rec, 121, 61), K, lx, ly, 121, 61, TOL)
    eng.close()


def test_fields_inside_the_fleet_loop_without_a_host_round_trip():
    """8. append_sample -> tick -> integrate_twist -> coverage() -> coverage_fields(fleet_only=True) for 20 ticks of 64 robots
    on ONE stream, nothing synchronising inside the loop (modelled on test_coverage_inside_the_fleet_loop_without_a_host_
    round_trip); then the last field against the restatement of the last fleet record, and the per-robot form"""
    from tests.test_gpu_fleet_tick import _engine
    from tests.test_gpu_replay_memory import _scenario
    from tests.test_host_mirror import COLL, DWA
    B, batch, ticks, cap, dt, model = 64, 8, 20, 32, 0.1, "omni"
    grid_a, _, bounds, poses0 = _scenario(B, np.random.default_rng(6))
    ccfg = capi.make_collision_cfg(bounds[0], bounds[2], 0.05, grid_a.xsize, grid_a.ysize, *COLL)
    dcfg = capi.DwaCfg(*DWA[model])
    eng = _engine(model)
    eng.config_domain(bounds)
    T, K = eng.T, 10
    nx, ny = eng.target_grid_size
    d_grid = _dev(grid_a.data, torch.int8)
    stream = torch.cuda.Stream()
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device="cuda")
    d_pose, d_vb = _dev(poses0), z(B, 3)
    d_ut, d_follow, d_count, d_u, d_traj = z(B, T, 3), z(B, dt=torch.int32), z(B, dt=torch.int32), z(B, 3), z(B, T, 3)
    d_valid, d_skip, d_source = z(B, dt=torch.int32), z(B, dt=torch.int32), z(B, dt=torch.int32)
    d_cols, d_n = z(B, batch, 3), z(B, dt=torch.int32)
    mem = capi.ReplayMemory(B, cap, batch, seed=99)
    with pytest.raises(capi.EngineError):
        mem.coverage_fields(eng, capi.FIELD_DEFICIT)     # (no coverage() yet)
    torch.cuda.synchronize()
    seen = []
    with torch.cuda.stream(stream):
        for t in range(ticks):
            mem.append_sample(d_pose, t, d_cols, d_n, stream=stream.cuda_stream)
            eng.tick_batch(B, d_pose, d_ut, d_follow, d_count, d_u, d_vb, d_grid, d_traj, d_valid, d_skip, ccfg, dcfg, 0.1, 0.5,
                           source=d_source, mem_cols=d_cols, n_mem=d_n, mem_stride=batch, stream=stream.cuda_stream, grid_epoch=1)
            capi.integrate_twist_batch(d_pose, d_u, dt, stream=stream.cuda_stream)
            d_vb.copy_(d_u)
            mem.coverage(eng, stream=stream.cuda_stream)
            robots, fleet = mem.coverage_fields(eng, capi.FIELD_DEFICIT, stream=stream.cuda_stream)
            assert robots is None and fleet.shape == (ny, nx)
            seen.append(fleet)
            if t == 0:
                first = fleet.clone()
    stream.synchronize()
    assert all(f is seen[0] for f in seen)                 # the object's own tensor, allocated once
    assert mem._field_ws[capi.FIELD_DEFICIT][2] is None    # no [B][ny][nx] without fleet_only=False
    h_rec = mem.coverage_records[1].cpu().numpy()
    assert h_rec[K * K] == B * ticks
    lx, ly = bounds[1] - bounds[0], bounds[3] - bounds[2]
    _check(eng, capi.FIELD_DEFICIT, h_rec[None, :], seen[-1][None], K, lx, ly, nx, ny, TOL)
    assert not torch.equal(first, seen[-1])                # (the fleet moved: its deficit changed)
    robots, fleet = mem.coverage_fields(eng, capi.FIELD_DENSITY, fleet_only=False)
    torch.cuda.synchronize()
    assert robots.shape == (B, ny, nx)
    _check(eng, capi.FIELD_DENSITY, mem.coverage_records[0].cpu().numpy()[:4], robots[:4], K, lx, ly, nx, ny, TOL)
    _check(eng, capi.FIELD_DENSITY, h_rec[None, :], fleet[None], K, lx, ly, nx, ny, TOL)
    mem.close()
    eng.close()


def test_argument_errors_with_live_handles(base):
    """9. a row range past ny_total, an unknown kind, n_rec = 0, a misaligned output: EEA_ERR_INVALID_ARGUMENT and nothing
    written; an engine without phi_k: EEA_ERR_NO_TARGET"""
    eng, rec = base["eng"], base["rec"]
    out = torch.full((5, 61, 121), -7.0, dtype=torch.float64, device="cuda")
    for kw in (dict(row0=60, nrows=2), dict(row0=61, nrows=1), dict(row0=0, nrows=62), dict(row0=0, nrows=0)):
        with pytest.raises(capi.EngineError) as ei:
            capi.records_field(eng, capi.FIELD_DENSITY, rec, out, 121, 61, **kw)
        assert ei.value.status == capi.ERR_INVALID_ARGUMENT, kw
    with pytest.raises(capi.EngineError) as ei:
        capi.records_field(eng, 3, rec, out, 121, 61)
    assert ei.value.status == capi.ERR_INVALID_ARGUMENT and "kind" in str(ei.value)
    with pytest.raises(capi.EngineError) as ei:
        capi.records_field(eng, capi.FIELD_DENSITY, rec[:0], out, 121, 61)
    assert ei.value.status == capi.ERR_INVALID_ARGUMENT
    with pytest.raises(capi.EngineError) as ei:
        capi.records_field(eng, capi.FIELD_DENSITY, rec, None, 121, 61)
    assert ei.value.status == capi.ERR_INVALID_ARGUMENT and "null" in str(ei.value)
    with pytest.raises(capi.EngineError) as ei:
        capi.records_field(eng, capi.FIELD_DENSITY, rec, out, 2 ** 16, 2 ** 15 + 1, 0, 1)
    assert ei.value.status == capi.ERR_UNSUPPORTED
    L = capi.lib()
    import ctypes as C
    st = L.eea_records_field(eng.h, 0, 5, C.c_void_p(rec.data_ptr()), 121, 61, 0, 61, C.c_void_p(out.data_ptr() + 4), None)
    assert st == capi.ERR_INVALID_ARGUMENT and b"aligned" in L.eea_last_error()
    _, em, rdiag, lim = MODELS["omni"]
    bare = capi.Engine(capi.make_config(em, 0.1, 1.0, RES, 1.0, 10, np.diag(rdiag), -np.array(lim), np.array(lim)))
    with pytest.raises(capi.EngineError) as ei:
        capi.records_field(bare, capi.FIELD_DENSITY, rec, out, 121, 61)
    assert ei.value.status == capi.ERR_NO_TARGET
    bare.close()
    torch.cuda.synchronize()
    assert (out == -7.0).all()

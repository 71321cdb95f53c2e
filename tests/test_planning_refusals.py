"""The complete text of every refusal the planning entries give before they select a device, in each entry's order: the three
dynamic-window batch entries, the two validate_control entries of the polygon base, eea_footprint_check_batch,
eea_body_collision_check_batch and the two layer constructors.  No GPU: every buffer is a host array that nothing may touch,
and no call below passes all of its entry's refusals with work to do.

A walk lists the refusals of one entry from first to last; every row is a call that is good up to the refusal it names.  The
rows marked "+" have a second fault that a later refusal would name: the earlier one wins.  The texts are those of the library
as it was before the entries were gathered behind shared helpers (csrc/entry_util.hpp); they are compared whole."""
import ctypes as C

import numpy as np
import pytest

from ergodic_exploration_amd import capi

OK, INV, UNS = 0, capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED
XS, YS, P = 80, 60, 4
COLL = (0.7, 1.0, 0.2, 0.8)
# dt, horizon, acc_dt, acc_lim x/y/th, max/min vx, max/min vy, max/min w, samples: the field order of capi.DwaCfg
DWA = (0.1, 1.0, 0.2, 1.0, 1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 2.0, -2.0, 3, 8, 5)
RECT = [(0.45, -0.25), (0.45, 0.25), (-0.45, 0.25), (-0.45, -0.25)]


def _cfg(res=0.1, xs=XS, ys=YS, bnd=COLL[0], search=COLL[1], obst=COLL[2], thr=COLL[3]):
    return capi.make_collision_cfg(-2.0, -1.0, res, xs, ys, bnd, search, obst, thr)


def _dwa(horizon=DWA[1], ns=DWA[12:]):
    return capi.DwaCfg(*(DWA[:1] + (horizon,) + DWA[2:12] + tuple(ns)))


def _fp(vertices, n=None):
    fp = capi.Footprint.of(vertices)
    if n is not None:
        fp.n = n
    return fp


GOOD, OMNI, FP = _cfg(), _dwa(), _fp(RECT)
R_OUT = float(np.hypot(0.45, 0.25))
FINE = R_OUT / 1024.5                        # the rectangle's circumscribed radius is 1024.5 cells
MANY = dict(xs=1 << 16, ys=(1 << 15) + 1)    # 2^31 + 65536 cells
WIDE, LONG = _dwa(ns=(17, 17, 29)), _dwa(horizon=2.0)   # 8381 samples; 20 steps

NULL_ARG = "null argument"
NULL_CFG = "null collision config"
RADII = "Search radius must be at least the same size as the boundary radius"
THRESHOLD = "Occupied threshold must be between 0 and 100"
CELLS = "the grid's xsize and ysize must be positive"
RESOLUTION = "the grid's resolution must be positive"
TOO_MANY = "xsize * ysize above 2^31"
VERTICES = "a footprint has 3 to 16 vertices"
NOT_FINITE = "a footprint vertex is not finite"
CONVEX = "the footprint must be strictly convex and counter-clockwise"
ORIGIN = "the body origin must lie strictly inside the footprint"
RADIUS = "the footprint's circumscribed radius is above 1024 cells"
EITHER = "give either d_vref or d_xt_ref"
EMPTY = "empty reference trajectory"
SAMPLES = "more than 8192 DWA samples"
NO_TIME = "the reference trajectory needs n_ref * dt_ref > 0"
# 20 steps of 0.1 s along 18 columns every 0.1 s: t = 1.9 s asks for column round(17 * 1.9 / 1.8) = 18
PAST = "the DWA rollout runs past the reference trajectory (step 19 reads column 18.000000 of 18)"
NO_LAYER = "null body layer"


class _Buffers:
    """host arrays in the place of every device buffer, filled with 7"""

    def __init__(self):
        self.arrays = {
            "grid": np.full(XS * YS, 7, dtype=np.int8), "sq": np.full(XS * YS, 7, dtype=np.int32), "pose": np.full((P, 3), 7.0),
            "u": np.full((P, 3), 7.0), "vb": np.full((P, 3), 7.0), "vref": np.full((P, 3), 7.0), "xt": np.full((P, 20, 3), 7.0),
            "self_": np.full(P, 7, dtype=np.int32), "hit": np.full(P, 7, dtype=np.int32), "valid": np.full(P, 7, dtype=np.int32),
            "found": np.full(P, 7, dtype=np.int32), "u_opt": np.full((P, 3), 7.0),
        }

    def __getattr__(self, name):
        return C.c_void_p(self.arrays[name].ctypes.data)

    def untouched(self):
        return all((a == 7).all() for a in self.arrays.values())


def _ref(s):
    return None if s is None else C.byref(s)


def _walk(call, rows):
    """every row (what, arguments of call, status, the whole message -- None where the call succeeds) holds"""
    L = capi.lib()
    for what, kw, status, text in rows:
        got = call(**kw)
        assert got == status, (what, got, L.eea_last_error())
        assert text is None or L.eea_last_error() == text.encode(), (what, L.eea_last_error())


def _footprint_rows(inp, out, prefix=""):
    """footprint_call_refusal's, for an entry whose input and output buffers are the arguments `inp` and `out`: the required
    pointers, the footprint, the cells, the resolution, the number of cells, the radius in cells.  The radii and the threshold
    are not looked at"""
    t = lambda text: prefix + text
    return [
        ("no configuration", dict(cfg=None), INV, t(NULL_ARG)), ("no footprint", dict(fp=None), INV, t(NULL_ARG)),
        ("no grid", dict(grid=None), INV, t(NULL_ARG)), ("no input", {inp: None}, INV, t(NULL_ARG)),
        ("no output", {out: None}, INV, t(NULL_ARG)),
        ("+ no footprint, no cells", dict(fp=None, cfg=_cfg(xs=0)), INV, t(NULL_ARG)),
        ("two vertices", dict(fp=_fp(RECT[:2])), INV, t(VERTICES)), ("17 vertices", dict(fp=_fp(RECT, n=17)), INV, t(VERTICES)),
        ("a NaN vertex", dict(fp=_fp([(0.6, 0.0), (float("nan"), 0.35), (-0.3, -0.35)])), INV, t(NOT_FINITE)),
        ("+ two vertices, one NaN", dict(fp=_fp([(float("nan"), 0.0), (-0.5, 0.0)])), INV, t(VERTICES)),
        ("clockwise", dict(fp=_fp(RECT[::-1])), INV, t(CONVEX)),
        ("the origin outside", dict(fp=_fp([(0.9, -0.2), (0.9, 0.2), (0.1, 0.2), (0.1, -0.2)])), INV, t(ORIGIN)),
        ("+ clockwise, no cells", dict(fp=_fp(RECT[::-1]), cfg=_cfg(xs=0)), INV, t(CONVEX)),
        ("xsize 0", dict(cfg=_cfg(xs=0)), INV, t(CELLS)), ("ysize 0", dict(cfg=_cfg(ys=0)), INV, t(CELLS)),
        ("+ no cells, resolution 0", dict(cfg=_cfg(xs=0, res=0.0)), INV, t(CELLS)),
        ("resolution 0", dict(cfg=_cfg(res=0.0)), INV, t(RESOLUTION)), ("resolution -0.1", dict(cfg=_cfg(res=-0.1)), INV, t(RESOLUTION)),
        ("resolution NaN", dict(cfg=_cfg(res=float("nan"))), INV, t(RESOLUTION)),
        ("+ resolution 0, 2^31 cells", dict(cfg=_cfg(res=0.0, **MANY)), INV, t(RESOLUTION)),
        ("2^31 + 65536 cells", dict(cfg=_cfg(**MANY)), UNS, t(TOO_MANY)),
        ("+ 2^31 cells, 1024.5 cells of radius", dict(cfg=_cfg(res=FINE, **MANY)), UNS, t(TOO_MANY)),
        ("1024.5 cells of radius", dict(cfg=_cfg(res=FINE)), UNS, t(RADIUS)),
    ]


# the shared part of the three dynamic-window entries, behind each one's own null checks
def _window_rows(prefix=""):
    t = lambda text: prefix + text
    traj = lambda **kw: dict(dict(vref=None, xt="xt", n_ref=20, dt_ref=0.1), **kw)
    return [
        ("neither reference", dict(vref=None), INV, t(EITHER)), ("both references", dict(xt="xt", n_ref=20, dt_ref=0.1), INV, t(EITHER)),
        ("+ neither reference, 8381 samples", dict(vref=None, dcfg=WIDE), INV, t(EITHER)),
        ("no column", traj(n_ref=0), INV, t(EMPTY)), ("+ no column, 8381 samples", traj(n_ref=0, dcfg=WIDE), INV, t(EMPTY)),
        ("8381 samples", dict(dcfg=WIDE), UNS, t(SAMPLES)), ("+ 8381 samples, dt_ref 0", traj(dcfg=WIDE, dt_ref=0.0), UNS, t(SAMPLES)),
        ("dt_ref 0", traj(dt_ref=0.0), INV, t(NO_TIME)), ("dt_ref -0.1", traj(dt_ref=-0.1), INV, t(NO_TIME)),
        ("dt_ref NaN", traj(dt_ref=float("nan")), INV, t(NO_TIME)),
        ("20 steps along 18 columns", traj(dcfg=LONG, n_ref=18), INV, t(PAST)),
    ]


def _entries(L, b):
    """name -> (call, its walk).  An argument that names a buffer is given as that buffer's name"""
    p = lambda name: None if name is None else getattr(b, name)

    def check(cfg=GOOD, fp=FP, grid="grid", pose="pose", hit="hit", n=P):
        return L.eea_footprint_check_batch(0, _ref(cfg), _ref(fp), p(grid), b.sq, p(pose), n, p(hit), None)

    def validate(cfg=GOOD, fp=FP, grid="grid", x0="pose", u="u", valid="valid", n=P):
        return L.eea_footprint_validate_control_batch(0, _ref(cfg), _ref(fp), p(grid), b.sq, p(x0), p(u), 0.1, 1.0, n, p(valid), None)

    def foot_dwa(cfg=GOOD, dcfg=OMNI, fp=FP, grid="grid", x0="pose", vb="vb", vref="vref", xt=None, n_ref=0, dt_ref=0.0, n=P,
                 u_opt="u_opt", found="found"):
        return L.eea_footprint_dwa_control_batch(0, _ref(cfg), _ref(dcfg), _ref(fp), p(grid), b.sq, p(x0), p(vb), p(vref), p(xt), n_ref,
                                                 dt_ref, n, p(u_opt), p(found), None)

    def disc_dwa(cfg=GOOD, dcfg=OMNI, grid="grid", x0="pose", vb="vb", vref="vref", xt=None, n_ref=0, dt_ref=0.0, u_opt="u_opt",
                 found="found"):
        return L.eea_dwa_control_batch(0, _ref(cfg), _ref(dcfg), p(grid), p(x0), p(vb), p(vref), p(xt), n_ref, dt_ref, P, p(u_opt),
                                       p(found), None)

    def body_check(grid="grid", pose="pose", hit="hit", n=P):
        return L.eea_body_collision_check_batch(None, p(grid), b.sq, p(pose), b.self_, n, p(hit), None)

    def body_validate(grid="grid", x0="pose", u="u", valid="valid", n=P):
        return L.eea_body_validate_control_batch(None, p(grid), b.sq, p(x0), p(u), b.self_, 0.1, 1.0, n, p(valid), None)

    def body_dwa(dcfg=OMNI, grid="grid", x0="pose", vb="vb", vref="vref", xt=None, n_ref=0, dt_ref=0.0, n=P, u_opt="u_opt", found="found"):
        return L.eea_body_dwa_control_batch(None, _ref(dcfg), p(grid), b.sq, p(x0), p(vb), p(vref), p(xt), n_ref, dt_ref, b.self_, n,
                                            p(u_opt), p(found), None)

    nulls = lambda names, text, also=None: [("no " + n, dict({n: None}, **(also or {})), INV, text) for n in names]
    unread = _cfg(bnd=1.0, search=0.7, thr=101.0)   # the polygon entries read neither the radii nor the threshold's range
    BC, BV, BD = ("eea_body_collision_check_batch: ", "eea_body_validate_control_batch: ", "eea_body_dwa_control_batch: ")
    return {
        "eea_footprint_check_batch": (check, _footprint_rows("pose", "hit") + [
            ("no pose to check", dict(n=0), OK, None), ("no pose, radii and threshold unread", dict(n=0, cfg=unread), OK, None)]),
        "eea_footprint_validate_control_batch": (validate, _footprint_rows("x0", "valid") + [
            ("+ 1024.5 cells of radius, no twist", dict(cfg=_cfg(res=FINE), u=None), UNS, RADIUS),
            ("no twist", dict(u=None), INV, NULL_ARG), ("+ no twist, no robot", dict(u=None, n=0), INV, NULL_ARG),
            ("no robot", dict(n=0), OK, None), ("no robot, radii and threshold unread", dict(n=0, cfg=unread), OK, None)]),
        "eea_footprint_dwa_control_batch": (foot_dwa, _footprint_rows("x0", "u_opt") + [
            ("+ 1024.5 cells of radius, no window", dict(cfg=_cfg(res=FINE), dcfg=None), UNS, RADIUS)] +
            nulls(("dcfg", "vb", "found"), NULL_ARG) + nulls(("found",), NULL_ARG, dict(vref=None)) + _window_rows() + [
            ("+ dt_ref 0, no robot", dict(vref=None, xt="xt", n_ref=20, dt_ref=0.0, n=0), INV, NO_TIME),
            ("no robot", dict(n=0), OK, None), ("no robot, radii and threshold unread", dict(n=0, cfg=unread), OK, None),
            ("no robot, 20 steps along 19 columns", dict(n=0, dcfg=LONG, vref=None, xt="xt", n_ref=19, dt_ref=0.1), OK, None)]),
        "eea_dwa_control_batch": (disc_dwa, [
            ("no configuration", dict(cfg=None), INV, NULL_CFG), ("+ no configuration, no grid", dict(cfg=None, grid=None), INV, NULL_CFG),
            ("swapped radii", dict(cfg=_cfg(bnd=1.0, search=0.7)), INV, RADII),
            ("+ swapped radii, threshold 101", dict(cfg=_cfg(bnd=1.0, search=0.7, thr=101.0)), INV, RADII),
            ("threshold 101", dict(cfg=_cfg(thr=101.0)), INV, THRESHOLD), ("threshold -1", dict(cfg=_cfg(thr=-1.0)), INV, THRESHOLD),
            ("+ threshold 101, no window", dict(cfg=_cfg(thr=101.0), dcfg=None), INV, THRESHOLD)] +
            nulls(("dcfg", "grid", "x0", "vb", "u_opt", "found"), NULL_ARG) + nulls(("grid",), NULL_ARG, dict(vref=None)) + _window_rows()),
        "eea_body_collision_check_batch": (body_check, nulls(("pose", "hit"), BC + NULL_ARG) + [
            ("no layer", {}, INV, BC + NO_LAYER), ("no layer, no grid", dict(grid=None), INV, BC + NO_LAYER),
            ("+ no layer, no pose to check", dict(n=0), INV, BC + NO_LAYER)]),
        "eea_body_validate_control_batch": (body_validate, nulls(("grid", "x0", "valid", "u"), BV + NULL_ARG) + [
            ("no layer", {}, INV, BV + NO_LAYER), ("+ no layer, no robot", dict(n=0), INV, BV + NO_LAYER)]),
        "eea_body_dwa_control_batch": (body_dwa, nulls(("grid", "x0", "u_opt", "dcfg", "vb", "found"), BD + NULL_ARG) +
                                       nulls(("dcfg",), BD + NULL_ARG, dict(vref=None)) + _window_rows(BD) + [
            ("no layer", {}, INV, BD + NO_LAYER), ("+ no layer, no robot", dict(n=0), INV, BD + NO_LAYER),
            ("no layer, 20 steps along 19 columns", dict(dcfg=LONG, vref=None, xt="xt", n_ref=19, dt_ref=0.1), INV, BD + NO_LAYER)]),
    }


ENTRY_NAMES = ["eea_footprint_check_batch", "eea_footprint_validate_control_batch", "eea_footprint_dwa_control_batch",
               "eea_dwa_control_batch", "eea_body_collision_check_batch", "eea_body_validate_control_batch",
               "eea_body_dwa_control_batch"]


@pytest.mark.parametrize("entry", ENTRY_NAMES)
def test_a_batch_entry_names_its_refusals_in_order(entry):
    b = _Buffers()
    call, rows = _entries(capi.lib(), b)[entry]
    _walk(call, rows)
    assert b.untouched()


def test_a_fleet_layer_names_its_refusals_in_order():
    L = capi.lib()

    def create(cfg=GOOD, body=4, B=3, out=True):
        h = C.c_void_p(0x7)
        st = L.eea_fleet_layer_create(0, _ref(cfg), body, B, C.byref(h) if out else None)
        assert not out or h.value is None, "a refused creation hands out no layer"
        return st

    _walk(create, [
        ("no handle", dict(out=False), INV, NULL_ARG), ("+ no handle, no configuration", dict(out=False, cfg=None), INV, NULL_ARG),
        ("no configuration", dict(cfg=None), INV, NULL_CFG), ("swapped radii", dict(cfg=_cfg(bnd=1.0, search=0.7)), INV, RADII),
        ("+ swapped radii, threshold 101", dict(cfg=_cfg(bnd=1.0, search=0.7, thr=101.0)), INV, RADII),
        ("threshold 101", dict(cfg=_cfg(thr=101.0)), INV, THRESHOLD), ("+ threshold 101, no robot", dict(cfg=_cfg(thr=101.0), B=0), INV, THRESHOLD),
        ("no robot", dict(B=0), INV, "a fleet layer needs at least one robot"),
        ("+ no robot, a negative body", dict(B=0, body=-1), INV, "a fleet layer needs at least one robot"),
        ("a negative body", dict(body=-1), INV, "the body radius of a fleet layer must be >= 0 cells"),
        ("+ a negative body, no cells", dict(body=-1, cfg=_cfg(xs=0)), INV, "the body radius of a fleet layer must be >= 0 cells"),
        ("xsize 0", dict(cfg=_cfg(xs=0)), INV, CELLS), ("+ no cells, resolution 0", dict(cfg=_cfg(ys=0, res=0.0)), INV, CELLS),
        ("resolution 0", dict(cfg=_cfg(res=0.0)), INV, RESOLUTION), ("resolution NaN", dict(cfg=_cfg(res=float("nan"))), INV, RESOLUTION),
        ("a negative boundary radius", dict(cfg=_cfg(bnd=-0.5)), INV, "the collision radii must not be negative"),
        ("+ a negative boundary radius, a body of 125 cells", dict(cfg=_cfg(bnd=-0.5), body=125), INV, "the collision radii must not be negative"),
        ("a body of 125 cells", dict(body=125), UNS, "a fleet layer's reach r_col + body above 127 cells"),
        ("+ a body of 128 cells, 2^31 cells", dict(body=128, cfg=_cfg(**MANY)), UNS, "a fleet layer's reach r_col + body above 127 cells"),
        ("2^31 cells", dict(cfg=_cfg(**MANY)), UNS, "a fleet layer of more than 2^31 centres or robots"),
        ("2^31 robots", dict(B=1 << 31), UNS, "a fleet layer of more than 2^31 centres or robots"),
    ])


def test_a_body_layer_names_its_refusals_in_order():
    L = capi.lib()

    def create(cfg=GOOD, fp=FP, B=4, flags=0, out=True):
        h = C.c_void_p(0x7)
        st = L.eea_body_layer_create(0, _ref(cfg), _ref(fp), B, flags, C.byref(h) if out else None)
        assert not out or h.value is None, "a refused creation hands out no layer"
        return st

    N = "eea_body_layer_create: "
    # footprint_on_grid_refusal's rows of the batch entries (the pointers are this entry's own)
    shared = [r for r in _footprint_rows("-", "-", N) if r[3] != N + NULL_ARG]
    _walk(create, [
        ("no handle", dict(out=False), INV, N + NULL_ARG), ("no configuration", dict(cfg=None), INV, N + NULL_ARG),
        ("no footprint", dict(fp=None), INV, N + NULL_ARG), ("+ no footprint, no robot", dict(fp=None, B=0), INV, N + NULL_ARG)] + shared + [
        ("+ 1024.5 cells of radius, no robot", dict(cfg=_cfg(res=FINE), B=0), UNS, N + RADIUS),
        ("no robot", dict(B=0), INV, N + "a body layer needs at least one robot"),
        ("+ no robot, unknown flags", dict(B=0, flags=2), INV, N + "a body layer needs at least one robot"),
        ("flag bit 1", dict(flags=2), INV, N + "unknown flag bits"), ("flag bit 31", dict(flags=0x80000001), INV, N + "unknown flag bits"),
        ("+ unknown flags, a near map of 2^31 cells", dict(flags=2, cfg=_cfg(xs=1 << 16, ys=1 << 15)), INV, N + "unknown flag bits"),
        # the grid fits, the near map (the grid and 2 * box = 14 cells more either way) does not
        ("a near map of 2^31 cells", dict(cfg=_cfg(xs=1 << 16, ys=1 << 15)), UNS, N + "a body layer of more than 2^31 near cells or robots"),
        ("2^31 robots", dict(B=1 << 31), UNS, N + "a body layer of more than 2^31 near cells or robots"),
    ])

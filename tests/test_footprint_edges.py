"""The scenes of tests/footprint_edge_scenes.py against themselves, without a device: every pose is decided by the 50-digit
reference alone (exact_signed itself on the cells that decide a pose: exact_verdicts, whose count of evaluations is asserted),
footprint_restatement.brute and .filtered give its verdict, and the scenes reach what they claim to (both verdicts, poses
`classify` calls ambiguous, boxes of two and more words, every listed seam and height residue, a window that fits the LDS at
0.0017 m and one that does not at 0.0013 m)."""
import numpy as np
import pytest

from tests import footprint_edge_scenes as es
from tests import footprint_plan_restatement as pr
from tests import footprint_restatement as fr


@pytest.fixture(scope="module")
def scenes():
    cache = {}

    def get(family, res):
        if (family, res) not in cache:
            cache[family, res] = es.families(family, res)
        return cache[family, res]
    return get


def test_the_polygons_and_the_launch_geometry():
    for name in es.NAMES:
        assert fr.valid(es.POLYGONS[name]), name
    assert len(es.POLYGONS["gon16"]) == fr.MAX_VERTICES
    r_in, r_out = es.radii("tiny")
    assert r_in / 0.1 < 0.7072 and fr.thresholds(r_in, r_out, 0.1)[0] == -1
    # one word per box row at 0.1 and 0.05 m; 107 columns at 0.01 m; near the largest window at 0.0017 m; none at 0.0013 m
    assert max(2 * es.box_of(n, 0.1) + 1 for n in es.NAMES) <= 64 and 2 * es.box_of("rect", 0.05) + 1 <= 64
    assert es.box_of("rect", 0.01) == 53 and es.box_of("rect", 0.0017) == 304
    assert 302.5 < es.radii("rect")[1] / 0.0017 < 303.5
    assert es.window_bytes(304, es.W_DEFAULT) <= es.LDS_LIMIT < es.window_bytes(304 + 48, es.W_DEFAULT)
    assert es.fits("rect", 0.0017) and not es.fits("rect", es.RES_NO_WINDOW, W=1)
    assert all(not es.fits(n, r, W=es.W_MEMORY) for n in es.NAMES for r in es.RES)
    assert set(es.names_at(0.0017)) == {"rect", "oct", "gon16", "tiny"}
    # the limits of dwa_cfg reserve exactly W cells, one step, and the robot's own reach is no larger
    for res in es.RES:
        for W in (2, 6, 9, 63, 128, es.W_MEMORY):
            d = es.dwa_cfg(res, W)
            assert pr.steps_of(d) == 1 and pr.limits_reach(d, res) == float(W) and pr.reach(d, np.zeros(3), res) <= W
            assert np.array_equal(pr.samples(d, np.zeros(3)), np.zeros((1, 3)))


def _agree(sc):
    """the 50-digit verdict of every pose against the scene's record, brute and filtered"""
    w, poses = sc.w, sc.poses
    hit, margin, n = es.exact_verdicts(w, sc.verts, poses)
    n_occ = int(fr.cr.occupied(w.data, w.threshold).sum())
    assert n >= len(poses) * min(n_occ, es.NEAREST) > 0, (sc.tag, n)          # mpmath was asked, about every pose
    if "cell" in sc.info:          # a hollow block's added cell is the one inside, at 50 digits
        i, j = sc.info["cell"]
        inside = es.exact_signed(w.res, w.xmin, w.ymin, i, j, sc.verts, poses[0])
        assert inside <= -es.MARGIN and sc.hit[0], sc.tag
    assert np.array_equal(hit, sc.hit), sc.tag
    assert (margin >= es.MARGIN).all() and np.allclose(margin, sc.margin, rtol=0, atol=1e-12), (sc.tag, margin.min())
    b_hit, b_margin = fr.brute(w.res, w.xmin, w.ymin, w.data, w.threshold, sc.verts, poses)
    assert np.array_equal(b_hit, sc.hit), (sc.tag, np.nonzero(b_hit != sc.hit)[0][:5])
    assert np.abs(b_margin - margin).max() < 1e-12, sc.tag
    f_hit, cls = fr.filtered(w.res, w.xmin, w.ymin, w.data, w.threshold, sc.verts, poses, sq=sc.sparse_sq())
    assert np.array_equal(f_hit, sc.hit) and (cls == fr.AMBIGUOUS).all(), sc.tag
    assert sc.ambiguous().all(), sc.tag


@pytest.mark.parametrize("family,res", es.CASES)
def test_every_pose_is_decided_and_the_restatement_agrees(scenes, family, res):
    got = scenes(family, res)
    assert len(got) > 0
    for sc in got:
        assert len(sc.x0) > 0, sc.tag
        _agree(sc)
    hits = sum(int(sc.hit.sum()) for sc in got)
    total = sum(len(sc.hit) for sc in got)
    assert 0.15 * total <= hits <= 0.85 * total, (hits, total)          # both verdicts, neither of them rare


@pytest.mark.parametrize("res", es.RES)
def test_single_cell_probes_reach_every_vertex_and_edge(scenes, res):
    """A: of the twelve probes per vertex-and-edge at least four are kept on average (a probe leaves when the field alone
    decides its pose, or the polygon is thinner than the pull); B: every near-parallel value of a_k occurs with both verdicts"""
    for sc in scenes("A", res):
        n = len(sc.verts)
        assert len(sc.x0) >= (4 * n if res != es.RES_NO_WINDOW else n), (sc.tag, len(sc.x0))
        assert sc.hit.any() and not sc.hit.all()
        assert sc.margin.min() < 1.01e-6          # (the 1e-6 m probes are there)
    for sc in scenes("B", res):
        a = es.a_of_edge(sc)
        for eps in es.EPS_PARALLEL:
            sel = np.abs(a - eps) < 1e-9
            assert sel.sum() >= 4 and sc.hit[sel].any() and not sc.hit[sel].all(), (sc.tag, eps, sel.sum())
        assert (np.abs(a) < 1.0e-3).any() and (np.abs(a) > 1.0e-3).any()          # either side of the kernel's branch


@pytest.mark.parametrize("res", es.RES)
def test_hollow_blocks_surround_the_polygon(scenes, res):
    got = scenes("C", res)
    names = set(sc.name for sc in got)
    assert names == set(es.hollow_names(res))
    for sc in got:
        x0, x1, y0, y1 = sc.info["box"]
        box = es.box_of(sc.name, res)
        assert (x1 - x0 + 1, y1 - y0 + 1) == (2 * box + 1, 2 * box + 1)          # unclipped
        # occupied cells beside the polygon in the rows it crosses: most of the box is occupied
        assert sc.info["occupied"] > 0.15 * (2 * box + 1) ** 2, sc.tag
    seen = set(sc.info.get("position") for sc in got)
    assert {None, "first", "last", "top", "bottom"} <= seen
    if "needle" in names:
        assert any(sc.info.get("position") == "narrow" and sc.name == "needle" for sc in got)
    widths = [sc.info["box"][1] - sc.info["box"][0] + 1 for sc in got if sc.name == "rect"]
    words = [(sc.boxes()[0, 1] - sc.window_x0()[0]) // 64 - (sc.boxes()[0, 0] - sc.window_x0()[0]) // 64 + 1 for sc in got if sc.name == "rect"]
    if res == 0.01:
        assert widths[0] == 107 and min(words) >= 2
    if res == 0.0017:
        assert widths[0] == 609 and min(words) >= 10
        assert max(sc.w.xs for sc in got) <= 720 + 16


@pytest.mark.parametrize("res", es.SEAM_RES)
def test_seams_and_clips_occur(scenes, res):
    got = scenes("D", res)
    c0s, heights, upper = set(), set(), 0
    for sc in got:
        b, wx0 = sc.boxes(), sc.window_x0()
        assert len(set(map(tuple, b))) == 1 and len(set(wx0)) == 1          # the poses of a scene share a cell
        x0, x1, y0, y1 = b[0]
        if "-ur" in sc.tag:
            assert x1 == sc.w.xs - 1 and y1 == sc.w.ys - 1 and x0 > 0 and y0 > 0
            upper += 1
        else:
            assert wx0[0] == 0 and y0 == 0
            c0s.add(int(x0 - wx0[0]))
        heights.add(int(y1 - y0 + 1) % 4)
    assert c0s == set(es.C0_LIST) and heights == {0, 1, 2, 3} and upper >= 8
    assert sum("-cell" in sc.tag for sc in got) >= len(es.SEAM_NAMES) * (len(es.C0_LIST) + 2)


@pytest.mark.parametrize("res", es.FAN_RES)
@pytest.mark.parametrize("name", es.FAN_NAMES)
def test_fans_are_decided(name, res):
    for N in es.FAN_N:
        f = es.fan(name, res, N)
        assert pr.steps_of(f.dwa) == 1 and pr.limits_reach(f.dwa, res) == 1.0 and len(f.robot.u) == N
        assert np.array_equal(f.robot.u[:, :2], np.zeros((N, 2)))
        turn = f.robot.u[:, 2] * es.DT
        assert turn[0] == -3.0 and abs(turn[-1] - 3.0) < 1e-12
        assert (f.margin >= fr.DECIDED).all() and f.free.any() and not f.free.all()
        # exact_signed itself on every cell and every heading against brute's verdicts and margins
        hit, margin, n = es.exact_verdicts(f.w, f.verts, f.poses)
        assert n == N * int((f.w.data != 0).sum())
        assert np.array_equal(~hit, f.free) and (margin >= fr.DECIDED).all() and np.abs(margin - f.margin).max() < 1e-12
        assert f.ambiguous() and es.fits(name, res, W=1, nsamp=N)          # every lane takes the exact test, from the window
        r_in, r_out = es.radii(name)
        oi, oj = np.nonzero(f.w.data)
        assert 2 <= len(oi) <= 3
        d = np.hypot(f.w.xmin + (oj + 0.5) * res - f.x0[0], f.w.ymin + (oi + 0.5) * res - f.x0[1])
        assert (d > r_in).all() and (d < r_out + res).all()


@pytest.mark.parametrize("res", es.BODY_RES)
def test_stamp_probes_are_decided(res):
    """the body layer's probes, where the occupied cells are a second robot's stamp: the restatement of the layer gives the
    50-digit verdicts, every margin is MARGIN or more, both verdicts occur at every polygon"""
    from tests import body_layer_restatement as br
    for name in es.BODY_NAMES:
        w, layer_poses, mask, x0, hit, margin = es.stamp_probes(res, name)
        ref = br.Layer(w, es.POLYGONS[name], layer_poses, mask)
        assert ref.flags.tolist() == [False, True] and ref.decided()[1] and not w.data.any()
        r_hit, r_margin = br.check(ref, es.judged(x0), np.zeros(len(x0), dtype=np.int64))
        assert np.array_equal(r_hit, hit) and (r_margin >= es.MARGIN).all() and np.abs(r_margin - margin).max() < 1e-12
        assert len(hit) >= 48 * len(es.POLYGONS[name]) and hit.any() and not hit.all()

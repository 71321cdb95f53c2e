"""eea_consensus_plan (ABI 6) in a world that CHANGES between launches: the header lets the caller rewrite the contents of the
groups' buffers -- d_skip among them, as eea_tick_batch does every tick -- and the engine's target between launches.
  * Skip sets: a skipped agent writes no record (pinned in tests/test_gpu_packed_exchange.py), and the plan owns the rotating
    record slots, so the plan has to empty a slot before the pass that writes it: an agent that was live when the slot was last
    written and is skipped now must not count again.  Bar: BITWISE the call-by-call sequence whose record buffer is zeroed
    before every pass, after EVERY launch of a schedule that skips single agents, whole and part wavefronts, a whole group and
    everybody, and brings them back; plus one check that does not share the record path: the last pass's d_ck rows of the live
    agents added in long double against the plan's sum record (1e-12 relative, the bar of test_packed_wavefront_records for the
    same sum) and the agent count exactly.
  * Target and domain: the captured kernel nodes hold lx, ly and the map origin BY VALUE and read phi_k through a pointer.  A new
    target on the same domain is picked up by the next replay; a changed domain makes eea_consensus_plan_launch refuse
    (EEA_ERR_UNSUPPORTED, nothing enqueued) until the plan is re-created or the old values are back.
Reference semantics: decentralised ergodic control shares c_k (README.md:225-227); ergodic_control.hpp:418-436 with c_bar."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ergodic_exploration_amd import capi
from tests.gpu_util import MAP_BOUNDS, make_pair, random_poses
from tests.test_gpu_control_parity import dev

pytestmark = pytest.mark.gpu

# the smallest batches that reach each record form (the forms of test_plan_is_bitwise_the_call_by_call_sequence); two groups,
# split at B // 2 - 2: uneven, and not on a wavefront boundary of the packed forms (17 = 4 * 4 + 1, 19 = 2 * 8 + 3)
FORMS = {
    "wavefront": ("simple_cart", 10, 20.0, 0, 70),          # one wavefront per agent, T = 200
    "packed16": ("omni", 10, 5.0, 16, 4 * 9 + 2),           # 4 agents per wavefront
    "packed8": ("simple_cart", 10, 2.0, 8, 8 * 5 + 3),      # 8 agents per wavefront
    "workgroup": ("omni", 30, 6.0, 0, 20),                  # one workgroup per agent
}
U0_FILL, STATUS_FILL = 9.0, -1


@pytest.fixture
def scene():
    made = []

    def _make(form):
        model, K, horizon, lanes, B = FORMS[form]
        capi.set_option(capi.OPT_AGENT_LANES, lanes)
        eng, _ = make_pair(model, K, horizon, n_oracles=0)
        made.append(eng)
        gb = [0, B // 2 - 2, B]
        A = 64 // lanes if lanes else 4    # agents per wavefront (where none is shared: only the size of the skipped runs)
        if lanes:
            assert eng.agent_lanes(gb[1]) == lanes and eng.agent_lanes(B - gb[1]) == lanes
            assert gb[1] % A != 0 and [eng.record_count(n) for n in (gb[1], B - gb[1])] == [-(-gb[1] // A), -(-(B - gb[1]) // A)]
        rng = np.random.default_rng(700 + K + lanes)
        ut0 = rng.uniform(-0.3, 0.3, (B, eng.T, 3))
        bad = ()
        if model == "simple_cart":
            ut0[:, :, 1] = 0.0
            bad = (gb[1] + 2 * A + 1,)     # SimpleCart rejects it (cart.hpp:167-170); inside the wavefront S1 skips partly
            ut0[bad[0], 5, 1] = 0.3
        return eng, gb, A, dev(random_poses(rng, B)), ut0, bad

    yield _make
    for eng in made:
        eng.close()
    capi.set_option(capi.OPT_AGENT_LANES, 0)


class _CallByCall:
    """the passes one call at a time with explicit synchronisation, the state kept between runs: pass i consumes the sum record
    of pass i - lag (an empty record before there is one); the record buffer is ZEROED before every pass -- what the owner of a
    record buffer that is reused under a changing skip set has to provide.  Records as the plan asks for them (one per wavefront
    where agents share one)."""

    def __init__(self, eng, gb, d_pose, ut, u0, status, lag):
        self.eng, self.gb, self.d_pose, self.lag = eng, gb, d_pose, lag
        self.ut, self.u0, self.status = ut.clone(), u0.clone(), status.clone()
        counts = [eng.record_count(gb[g + 1] - gb[g]) for g in range(len(gb) - 1)]
        self.roff = [0] + [int(x) for x in np.cumsum(counts)]
        RL = eng.ck_record_len
        self.arec = torch.zeros((self.roff[-1], RL), dtype=torch.float64, device="cuda")
        self.empty = torch.zeros((RL,), dtype=torch.float64, device="cuda")
        self.sums = []

    def run(self, passes, skip=None, ck=None):
        """`passes` more passes; skip [B] int32 or None; ck [B][K^2]: the LAST pass also writes the agents' own c_k there"""
        eng, gb = self.eng, self.gb
        for k in range(passes):
            src = len(self.sums) - self.lag
            out = torch.zeros_like(self.empty)
            self.arec.zero_()
            torch.cuda.synchronize()
            for g in range(len(gb) - 1):
                sl = slice(gb[g], gb[g + 1])
                eng.control_batch(gb[g + 1] - gb[g], self.d_pose[sl], self.ut[sl], self.u0[sl],
                                  ck=ck[sl] if ck is not None and k == passes - 1 else None,
                                  ck_rec=self.arec[self.roff[g]:self.roff[g + 1]], rec_per_wavefront=True, status=self.status[sl],
                                  skip=None if skip is None else skip[sl],
                                  ck_shared=self.sums[src] if src >= 0 else self.empty, ck_shared_parts=1)
            torch.cuda.synchronize()
            eng.ck_records_sum(self.roff[-1], self.arec, out)
            torch.cuda.synchronize()
            self.sums.append(out)


def _groups(gb, d_pose, ut, u0, status, skip=None):
    return [dict(B=gb[g + 1] - gb[g], pose=d_pose[gb[g]:gb[g + 1]], ut=ut[gb[g]:gb[g + 1]], u0=u0[gb[g]:gb[g + 1]],
                 status=status[gb[g]:gb[g + 1]], **({} if skip is None else dict(skip=skip[gb[g]:gb[g + 1]])))
            for g in range(len(gb) - 1)]


def _skip_sets(gb, A, B, bad, lag):
    """the schedule of the launches (agents of the whole batch; wavefronts are aligned to A within their group)"""
    g1 = gb[1]
    s1 = {1, g1 + 1} | set(range(A, 2 * A)) | {g1 + 2 * A, g1 + 2 * A + 2}    # singles, a whole wavefront, a partly skipped one
    s2 = {0, 2, 3, g1, B - 1} | set(range(g1 + A, g1 + 2 * A))                # the same kinds in the other groups
    group = set(range(gb[lag - 1], gb[lag]))                                   # one whole group
    assert not (s1 & s2) and not (s1 | s2) & set(bad) and max(s1 | s2) < B and 2 * A <= g1
    return [set(), s1, s2, group, set(range(B)), set()]


@pytest.mark.parametrize("form,lag,rccl", [(f, lag, False) for f in FORMS for lag in (1, 2)] + [("wavefront", 2, True)])
def test_plan_under_a_changing_skip_set(scene, form, lag, rccl):
    """Launch 2 is where a plan that never empties its slots shows: the agents S1 skips were live when every slot was last
    written, so the count element of the sum record comes out above the number of live agents.  Launches 3-4: agents come back
    and count again.  Launch 5 (everybody skipped): an all-zero sum record, count 0, nothing moves.  Launch 6: `lag` passes
    consume a count-0 record and use their own c_k, as the header says of the first passes ever."""
    eng, gb, A, d_pose, ut0, bad = scene(form)
    B, K2 = gb[-1], eng.K2
    slots = lag + 2
    d_skip = torch.zeros((B,), dtype=torch.int32, device="cuda")
    ut_b, u0_b = dev(ut0), torch.full((B, 3), U0_FILL, dtype=torch.float64, device="cuda")
    st_b = torch.full((B,), STATUS_FILL, dtype=torch.int32, device="cuda")
    ref = _CallByCall(eng, gb, d_pose, ut_b, u0_b, st_b, lag)
    comm = capi.Comm(0, 1, 0, capi.comm_unique_id() if rccl else None)
    plan = capi.ConsensusPlan(eng, comm, _groups(gb, d_pose, ut_b, u0_b, st_b, d_skip), lag=lag, passes_per_launch=slots)
    assert plan.passes_per_launch == slots
    stream = torch.cuda.Stream()
    try:
        for n, skipped in enumerate(_skip_sets(gb, A, B, bad, lag), start=1):
            idx = sorted(skipped)
            live = [b for b in range(B) if b not in skipped and b not in bad]
            h_skip = np.zeros(B, dtype=np.int32)
            h_skip[idx] = 1
            d_skip.copy_(torch.as_tensor(h_skip))
            for u0, st in ((ref.u0, ref.status), (u0_b, st_b)):   # what a skipped agent must leave alone
                u0.fill_(U0_FILL)
                st.fill_(STATUS_FILL)
            ut_before = ut_b.clone()
            d_ck = torch.full((B, K2), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            ref.run(slots, d_skip, d_ck)
            plan.launch(stream.cuda_stream)
            torch.cuda.synchronize()
            last, want = plan.last_sum(eng), ref.sums[-1].cpu().numpy()
            # the agent count first: an exact integer, and the figure a stale record shows in
            assert last[K2] == len(live), "launch %d: count element %r of the sum record, %d live agents" % (n, last[K2], len(live))
            # not through the record path: the live agents' own c_k of the last pass, added in long double
            own = d_ck.cpu().numpy()[live].astype(np.longdouble).sum(0) if live else np.zeros(K2, dtype=np.longdouble)
            assert not np.isnan(own).any()
            assert np.abs(last[:K2] - own).max() <= 1e-12 * max(1.0, float(np.abs(own).max())), n
            assert want[K2] == len(live) and np.array_equal(last, want), n
            assert torch.equal(ref.ut, ut_b) and torch.equal(ref.u0, u0_b) and torch.equal(ref.status, st_b), n
            # skipped agents: warm start, first control and status as they were; the rejected agent says so; the others ran
            assert torch.equal(ut_b[idx], ut_before[idx]) and (u0_b[idx] == U0_FILL).all(), n
            status = st_b.cpu().numpy()
            assert (status[idx] == STATUS_FILL).all() and (status[live] == capi.OK).all(), n
            assert all(status[b] == (STATUS_FILL if b in skipped else capi.ERR_INVALID_TWIST) for b in bad), n
            if live:
                assert not torch.equal(ut_b[live], ut_before[live]) and (u0_b[live] != U0_FILL).any(), n
            else:
                assert not last.any() and torch.equal(ut_b, ut_before)
    finally:
        plan.close()
        comm.close()


def _occupancy(frac, lx, ly, res=0.1):
    """int8 cells (OccupancyGrid.data layout) of a grid that spans (lx, ly) at the engine's resolution: unknown left of
    frac * lx, free right of it, a few uncertain cells"""
    nx, ny = int(round(lx / res)) + 1, int(round(ly / res)) + 1
    occ = np.zeros((ny, nx), dtype=np.int8)
    occ[:, :int(frac * nx)] = -1
    occ[::7, ::5] = 30
    return nx, ny, torch.as_tensor(occ).cuda()


class _Pair:
    """a plan and its call-by-call reference on buffers of their own, stepped together and compared after every launch"""

    def __init__(self, eng, gb, d_pose, ut, u0, status, lag=2):
        self.eng, self.per = eng, lag + 2
        self.ut, self.u0, self.status = ut, u0, status
        self.ref = _CallByCall(eng, gb, d_pose, ut, u0, status, lag)
        self.comm = capi.Comm(0, 1, 0, None)
        self.plan = capi.ConsensusPlan(eng, self.comm, _groups(gb, d_pose, ut, u0, status), lag=lag, passes_per_launch=self.per)
        self.stream = torch.cuda.Stream()

    def state(self):
        torch.cuda.synchronize()
        return self.ut.clone(), self.u0.clone(), self.status.clone(), torch.as_tensor(self.plan.last_sum(self.eng))

    def step(self):
        self.ref.run(self.per)
        self.plan.launch(self.stream.cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(self.plan.last_sum(self.eng), self.ref.sums[-1].cpu().numpy())
        assert torch.equal(self.ref.ut, self.ut) and torch.equal(self.ref.u0, self.u0) and torch.equal(self.ref.status, self.status)
        assert (self.status == capi.OK).all()

    def refused(self):
        """the launch is refused and enqueues nothing"""
        before = self.state()
        import ctypes as C
        rc = capi.lib().eea_consensus_plan_launch(self.plan.h, C.c_void_p(self.stream.cuda_stream))
        why = capi.lib().eea_last_error().decode() if rc != capi.OK else ""
        after = self.state()
        same = [torch.equal(a, b) for a, b in zip(before, after)]
        assert rc == capi.ERR_UNSUPPORTED, ("a launch on a changed domain returned status %d; unchanged after it (ut, u0, status, "
                                            "last sum): %s; max |ut moved| = %g" % (rc, same, float((after[0] - before[0]).abs().max())))
        assert "domain changed since the plan was created" in why and "must be re-created" in why, why
        assert all(same), same
        with pytest.raises(capi.EngineError) as ei:      # and through the wrapper
            self.plan.launch(self.stream.cuda_stream)
        assert ei.value.status == capi.ERR_UNSUPPORTED

    def close(self):
        self.plan.close()
        self.comm.close()


def _plain(scene, form):
    eng, gb, _, d_pose, ut0, _ = scene(form)
    B = gb[-1]
    if FORMS[form][0] == "simple_cart":
        ut0[:, :, 1] = 0.0     # nobody rejected here
    return (eng, gb, d_pose, dev(ut0), torch.zeros((B, 3), dtype=torch.float64, device="cuda"),
            torch.full((B,), STATUS_FILL, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("form", ["wavefront", "packed16"])
def test_plan_picks_up_a_new_target_on_the_same_domain(scene, form):
    """phi_k is read through a pointer at replay time: a target set between two launches, on the domain of plan_create, is the
    target of the next launch -- bitwise the call-by-call sequence that makes the same update at the same point"""
    args = _plain(scene, form)
    eng = args[0]
    lx, ly = MAP_BOUNDS[1] - MAP_BOUNDS[0], MAP_BOUNDS[3] - MAP_BOUNDS[2]
    pair = _Pair(*args)
    try:
        pair.step()
        phik = eng.phik()
        eng.set_target_occupancy(*_occupancy(0.3, lx, ly), lx, ly)
        assert np.abs(eng.phik() - phik).max() > 1e-3      # (otherwise this proves nothing)
        pair.step()
        phik = eng.phik()
        eng.set_target_occupancy(*_occupancy(0.7, lx, ly), lx, ly)
        assert np.abs(eng.phik() - phik).max() > 1e-3
        pair.step()
    finally:
        pair.close()


@pytest.mark.parametrize("form", ["wavefront", "packed16"])
def test_plan_refuses_a_changed_domain(scene, form):
    """lx, ly and the map origin sit BY VALUE in the captured kernel nodes: after a domain change a replay would run the old
    scalars against the new phi_k.  eea_consensus_plan_launch refuses (EEA_ERR_UNSUPPORTED, nothing enqueued) while the values
    differ from those of plan_create -- values, not generations: the old values back make the old plan launchable again.  A plan
    created after the change is the call-by-call sequence started afresh on the new domain."""
    eng, gb, d_pose, ut, u0, status = _plain(scene, form)
    x0, x1, y0, y1 = MAP_BOUNDS
    pair = _Pair(eng, gb, d_pose, ut, u0, status)
    fresh = None
    try:
        pair.step()
        # the origin alone (no rebuild, phi_k as it was); the extent (phi_k rebuilt from the Gaussians); the extent through a
        # target entry that brings its own domain
        for change in (lambda: eng.config_domain((x0 - 0.5, x1 - 0.5, y0, y1)),
                       lambda: eng.config_domain((x0, x1, y0 - 0.25, y1 - 0.25)),
                       lambda: eng.config_domain((x0, x1 + 2.0, y0, y1)),
                       lambda: eng.config_domain((x0, x1, y0, y1 + 1.0)),
                       lambda: eng.set_target_occupancy(*_occupancy(0.4, 14.0, 7.0), 14.0, 7.0)):
            change()
            pair.refused()
            eng.config_domain(MAP_BOUNDS)    # the old values (a rebuild from the Gaussians where the extent had changed)
            pair.step()
        # after a refusal: a new plan on the same buffers, on the new domain
        new = (x0 - 1.0, x1 + 1.0, y0, y1 + 1.0)
        eng.config_domain(new)
        eng.set_target_occupancy(*_occupancy(0.6, new[1] - new[0], new[3] - new[2]), new[1] - new[0], new[3] - new[2])
        pair.refused()
        pair.close()
        fresh = _Pair(eng, gb, d_pose, ut, u0, status)     # empty sum records for the first `lag` passes, on both sides
        fresh.step()
        fresh.step()
        eng.config_domain(MAP_BOUNDS)
        fresh.refused()
    finally:
        pair.close()
        if fresh is not None:
            fresh.close()

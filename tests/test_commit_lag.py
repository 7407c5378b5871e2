"""The header's commit lag field (gr_layout.h H_CL): committed kept as
lastIndex - lag in the header word while the SR_COMMITTED row goes stale.

Every case compares the full exported state (committed included), every
message and every result with the oracle after every pass. The CPU cases run
the lane code's host build (tests/simulate.HostlaneBackend: records -> rows
through host::header_of, one pass, rows -> records through host::resolve_sync);
the device twins keep their rows in HBM from pass to pass (devsim.DeviceLockstep,
the schedule bench.py times), so there a row stays stale for as long as the
field stands for it."""
import numpy as np
import pytest

from dragonboat_amd import abi, populations as P
import simulate as SIM

H_CL_MAX_LAG = 6  # gr_layout.h


def _lag(state, G):
    """lastIndex - committed of the G leaders (replica block 0)."""
    return (state["last_index"][:G] - state["committed"][:G]).astype(np.int64)


class _AckNet:
    """The network between passes. P.drop_acks drops HeartbeatResps (config 3);
    the lag moves with the ReplicateResps, so this drops or delays those.
    drop: every ReplicateResp is lost; stagger: those of follower slot 2 arrive
    one pass late (ahead of nothing else from that slot: the whole batch waits)."""

    def __init__(self):
        self.drop = False
        self.stagger = False
        self.held = np.zeros(0, abi.MESSAGE)
        self.dropped = 0
        self.changed = False  # the last call delivered something other than what was sent

    def __call__(self, k, msgs):
        ack = msgs["type"] == abi.REPLICATE_RESP
        if self.drop:
            self.dropped += int(ack.sum())
            msgs = msgs[~ack]
            ack = msgs["type"] == abi.REPLICATE_RESP
        late = ack & (msgs["slot"] == 2) if self.stagger else np.zeros(len(msgs), bool)
        self.changed = self.drop or bool(late.any()) or len(self.held) > 0
        out = np.concatenate([self.held, msgs[~late]])
        self.held = msgs[late].copy()
        order = np.lexsort((np.arange(len(out)), out["slot"], out["peer"]))  # held ones first in their mailbox
        return out[order]


# ---------------------------------------------------------------- drivers
class _HostDriver:
    """simulate.Lockstep over the host lane, with the device's wave hints."""

    def __init__(self, peers, G, R):
        from oracle.pyoracle import hostlane_lib
        self.G, self.R, self.n = G, R, R * G
        self.topo = P.Topology(G, R)
        self.hl = hostlane_lib()
        self.hl.hl_true_hints(1)
        self.ls = SIM.Lockstep(SIM.HostlaneBackend, peers, R)
        self.msgs = np.zeros(0, abi.MESSAGE)

    def export(self):
        return self.ls.export()

    def step(self, loc, net=None, k=0):
        out, res = self.ls.step(self.msgs, loc)
        self.msgs = self.topo.route_messages(out)
        if net is not None:
            self.msgs = net(k, self.msgs)
        return res

    def inject(self, idx, recs):
        self.ls.reload(idx, recs)

    def apply_all(self):
        self.ls.apply_all()

    @property
    def escalations(self):
        return self.ls.stats["escalations"]

    def close(self):
        self.hl.hl_true_hints(0)
        self.ls.close()


class _DevDriver:
    """devsim.DeviceLockstep: gr_step_device over loopback spaces."""

    def __init__(self, peers, G, R, lib_path=None):
        import devsim
        self.G, self.R, self.n = G, R, R * G
        self.ls = devsim.DeviceLockstep(peers, G, R, lib_path=lib_path)

    def export(self):
        return self.ls.export()

    def step(self, loc, net=None, k=0):
        res = self.ls.step(loc, drop_fn=net)
        # DeviceLockstep re-encodes the next inbox only when the count of messages
        # changed; a delayed batch swaps messages at the same count. Untouched
        # passes keep the mailboxes the kernels wrote (uniform, shared).
        if net is not None and net.changed:
            self.ls.override_inbox(self.ls.msgs)
        return res

    def inject(self, idx, recs):
        self.ls.inject(idx, recs)

    def apply_all(self):
        """simulate.Lockstep.apply_all on the device: the host persisted and
        applied everything (gr_commit_update + gr_notify_applied)."""
        import parity
        pop, eng = self.ls.pop, self.ls.eng
        keep = np.arange(self.n)
        uc = parity.update_commits(pop.export())
        pop.commit_all()
        rc, st = eng.commit_update(keep.astype(np.uint32), uc)
        assert rc == 0, (rc, st[st != 0][:5])
        eng.notify_applied(keep.astype(np.uint32), np.asarray(pop.export()["committed"], np.uint64))

    @property
    def escalations(self):
        return self.ls.stats["escalations"]

    def close(self):
        self.ls.close()


# ---------------------------------------------------------------- scenarios
def _steady(drv, passes, k0=0):
    G, R = drv.G, drv.R
    for k in range(passes):
        drv.step(P.propose_locals(R * G, np.arange(G), pass_index=k0 + k))


def _scenario_lag_range(drv):
    """The lag moves through and past the field's range: 2 -> 10 with every ack
    dropped for 8 proposing passes (the row is materialised past 6), back down
    when the acks resume (the field is set again), one follower's acks a pass
    late, then to 0 without proposals, and an idle pass."""
    G, R = drv.G, drv.R
    n = R * G
    net = _AckNet()
    k = 0
    for _ in range(4):
        drv.step(P.propose_locals(n, np.arange(G), pass_index=k), net, k)
        k += 1
    assert np.all(_lag(drv.export(), G) == 2)
    net.drop = True  # takes effect on the acks this pass sends
    peak = 0
    for _ in range(9):
        drv.step(P.propose_locals(n, np.arange(G), pass_index=k), net, k)
        k += 1
        peak = max(peak, int(_lag(drv.export(), G).max()))
    assert net.dropped > 0 and peak >= 10 > H_CL_MAX_LAG, peak
    net.drop = False
    for _ in range(4):
        drv.step(P.propose_locals(n, np.arange(G), pass_index=k), net, k)
        k += 1
    assert np.all(_lag(drv.export(), G) <= H_CL_MAX_LAG)
    net.stagger = True
    for _ in range(4):
        drv.step(P.propose_locals(n, np.arange(G), pass_index=k), net, k)
        k += 1
    net.stagger = False
    for _ in range(5):  # no proposals: the acks in flight drain, the lag falls to 0
        drv.step(P.propose_locals(n, [], pass_index=k), net, k)
        k += 1
    cur = drv.export()
    assert np.all(cur["last_index"] == cur["committed"])
    drv.step(P.propose_locals(n, [], pass_index=k), net, k)  # idle
    assert drv.escalations == 0


def _scenario_leader_changes(drv):
    """General lane, term adoption, truncation over set fields (config 5's churn)."""
    G, R = drv.G, drv.R
    topo = P.Topology(G, R)
    rng = np.random.default_rng(77)
    _steady(drv, 4)
    injected = 0
    for k in range(4, 10):
        cur = drv.export()
        ch = P.inject_leader_change(cur, topo, 0.1, rng)
        drv.inject(ch, cur[ch])
        injected += len(ch)
        drv.step(P.propose_locals(R * G, P.current_leaders(drv.export(), topo), pass_index=k))
    assert injected > 0


def _scenario_ticks_read_index(drv):
    """The tick lane over set fields: a Tick on every replica (heartbeats carry
    Commit to the followers) and a ReadIndex on every other leader, alone and
    beside proposals."""
    G, R = drv.G, drv.R
    n = R * G
    _steady(drv, 4)
    ready = 0
    for k in range(4, 10):
        loc = P.propose_locals(n, np.arange(G) if k % 2 else [], pass_index=k, ticks=1)
        lead = np.zeros(n, bool)
        lead[:G:2] = True
        loc["read_index"] = lead
        loc["read_ctx_low"] = np.where(lead, np.arange(n) + 1000 * k + 1, 0)
        loc["read_ctx_high"] = np.where(lead, k + 1, 0)
        res = drv.step(loc)
        ready += int(res["n_ready"].sum())
    assert ready > 0


def _scenario_commit_update(drv):
    """gr_commit_update (commit_marks reads committed) and gr_notify_applied
    between steady passes whose rows are stale."""
    _steady(drv, 4)
    for k in range(4, 10):
        drv.apply_all()
        _steady(drv, 1, k0=k)
    assert drv.escalations == 0


SCENARIOS = {"lag_range": (_scenario_lag_range, 128), "leader_changes": (_scenario_leader_changes, 192),
             "ticks_read_index": (_scenario_ticks_read_index, 192), "commit_update": (_scenario_commit_update, 192)}


def _peers(G, R, seed):
    return P.make_groups(G, R, seed=seed, election=10, heartbeat=1)


# ---------------------------------------------------------------- CPU cases
@pytest.mark.parametrize("R", [3, 5])
def test_steady_state_stays_closed_form(built, R):
    """128 x 3 and 128 x 5 with the device's hints, one proposal per leader per
    pass: after warm-up every lane that has a closed form is a steady lane in
    every pass and nothing escalates. R = 3: all R * G lanes. R = 5: the
    (R - 1) * G followers; SteadyLeader is the median of three voters
    (gr_steady.h static_assert S == 3), so a five-replica leader was FastLane's
    before this field existed and still is. A wrong steady lag would keep parity
    green and silently send these lanes through FastLane (the trap the H_MP
    comment in gr_layout.h records)."""
    from oracle.pyoracle import hostlane_steady_lanes
    G, passes, warm = 128, 10, 4
    drv = _HostDriver(_peers(G, R, 11), G, R)
    try:
        counts = [hostlane_steady_lanes()]
        for k in range(passes):
            drv.step(P.propose_locals(R * G, np.arange(G), pass_index=k))
            counts.append(hostlane_steady_lanes())
        assert drv.escalations == 0
        per_pass = np.diff(counts)[warm:]
        print("steady lanes per pass:", per_pass)
        assert np.all(per_pass == (R if R == 3 else R - 1) * G), per_pass
        assert np.all(_lag(drv.export(), G) == 2)
    finally:
        drv.close()


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_scenarios_host(built, name):
    fn, G = SCENARIOS[name]
    drv = _HostDriver(_peers(G, 3, 31), G, 3)
    try:
        fn(drv)
    finally:
        drv.close()


def test_steady_again_after_lag_returns(built):
    """After the lag left the field's range and came back, the steady lanes take
    every lane again (the field was set again; a lane that had to load the row
    each pass would still be steady, one that bailed would not)."""
    from oracle.pyoracle import hostlane_steady_lanes
    G, R = 128, 3
    n = R * G
    drv = _HostDriver(_peers(G, R, 13), G, R)
    net = _AckNet()
    try:
        k = 0
        for phase, passes in ((False, 4), (True, 8), (False, 8)):
            net.drop = phase
            for _ in range(passes):
                drv.step(P.propose_locals(n, np.arange(G), pass_index=k), net, k)
                k += 1
        s0 = hostlane_steady_lanes()
        for _ in range(3):
            drv.step(P.propose_locals(n, np.arange(G), pass_index=k), net, k)
            k += 1
        assert hostlane_steady_lanes() - s0 == 3 * n
        assert np.all(_lag(drv.export(), G) == 2)
    finally:
        drv.close()


def _lag_records(S, role):
    """One group per (lag 0..8, last_index 0..11 and two large ones) with the
    lag no larger than last_index: steady-state records (make_groups) edited."""
    cases = [(lag, last) for lag in range(9) for last in list(range(12)) + [2**32 + 5, 2**40] if lag <= last]
    G = len(cases)
    peers = P.make_groups(G, S, seed=17, base_index=64, spread=1)
    blk = slice(0, G) if role == "leader" else slice(G, 2 * G)
    for g, (lag, last) in enumerate(cases):
        for r in range(S):
            rec = peers[r * G + g:r * G + g + 1]
            lo = min(int(rec["first_index_m1"][0]), last)
            rec["last_index"], rec["committed"] = last, last - lag
            rec["applied"] = min(int(rec["applied"][0]), last - lag)
            rec["first_index_m1"] = lo
            rec["n_runs"] = 1
            rec["run_start"][0, 0] = lo
            rec["run_term"][0, 0] = rec["term"][0]
            rec["saved_to"], rec["marker_index"], rec["log_applied"] = 0, 0, 0  # fresh (gr_host.h get_u64_row)
            rem = rec["remotes"]
            rem["next"][0, :S] = last + 1
            rem["match"][0, :S] = last - lag
    return peers, G, blk


@pytest.mark.parametrize("S", [3, 5])
def test_record_round_trip_host(built, S):
    """Lags 0..8 over last_index from 0 up: a pass without input returns every
    record unchanged (load sets the field where the lag fits, sync resolves it),
    then one steady pass (a proposal per leader) equals the oracle, leaders and
    followers."""
    import parity
    peers, G, _ = _lag_records(S, "leader")
    ls = SIM.Lockstep(SIM.HostlaneBackend, peers, S)
    try:
        before = ls.eng.sync()
        ls.step(None, None)
        after = ls.eng.sync()
        assert not parity.compare_states(after, before, S)
        assert np.array_equal(after["committed"], peers["committed"])
        out, _ = ls.step(None, P.propose_locals(S * G, np.arange(G), pass_index=0))
        ls.step(P.Topology(G, S).route_messages(out), P.propose_locals(S * G, np.arange(G), pass_index=1))
    finally:
        ls.close()


# ---------------------------------------------------------------- device twins
def _split(monkeypatch):
    monkeypatch.setenv("GR_SPLIT_MIN_LANES", "1")  # read at gr_create
    monkeypatch.setenv("GR_SMALL_BLOCKS", "0")     # the split schedule, not the fused small-pass kernel


@pytest.mark.gpu
@pytest.mark.parametrize("G", [128, 192])
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_scenarios_device_split(gpu, monkeypatch, name, G):
    """The scenarios over the split schedule (steady kernel, role instances, tick
    and general kernels), 128 groups per replica block (route_wu = 1) and 192."""
    _split(monkeypatch)
    drv = _DevDriver(_peers(G, 3, 31), G, 3)
    try:
        SCENARIOS[name][0](drv)
    finally:
        drv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("G,R", [(128, 3), (192, 3), (128, 5)])
def test_steady_device_split(gpu, monkeypatch, G, R):
    """Ten steady passes on the split schedule: parity every pass, no escalation,
    the lag 2 throughout once the pipeline is full."""
    _split(monkeypatch)
    drv = _DevDriver(_peers(G, R, 11), G, R)
    try:
        _steady(drv, 10)
        assert drv.escalations == 0 and np.all(_lag(drv.export(), G) == 2)
    finally:
        drv.close()


@pytest.mark.gpu
def test_lag_range_device_small_kernel(gpu):
    """The lag scenario through gr_small_kernel (the default thresholds)."""
    drv = _DevDriver(_peers(128, 3, 31), 128, 3)
    try:
        _scenario_lag_range(drv)
    finally:
        drv.close()


@pytest.mark.gpu
def test_lag_range_device_checked_build(gpu, monkeypatch):
    """The lag scenario under the GR_COVERAGE build: GR_CHECK_STATE's invariants
    (committed <= lastIndex through the resolved field) count no violation."""
    import ctypes
    from dragonboat_amd import build
    from dragonboat_amd.engine import load_library
    _split(monkeypatch)
    lib = load_library(build.COVER_LIB)
    names = [x for x in lib.gr_coverage_names().decode().split(",") if x]
    before, after = np.zeros(len(names), np.uint64), np.zeros(len(names), np.uint64)
    assert lib.gr_coverage_read(before.ctypes.data_as(ctypes.c_void_p), len(names)) == len(names)
    drv = _DevDriver(_peers(128, 3, 31), 128, 3, lib_path=build.COVER_LIB)
    try:
        _scenario_lag_range(drv)
        lib.gr_coverage_read(after.ctypes.data_as(ctypes.c_void_p), len(names))
        hits = dict(zip(names, (after - before).tolist()))
        bad = {x: h for x, h in hits.items() if x.startswith("BAD_") and h}
        assert not bad, bad
        assert hits["STEADY_LEADER"] > 0 and hits["STEADY_FOLLOWER"] > 0, hits
    finally:
        drv.close()


@pytest.mark.gpu
def test_compact_log_keeps_field(gpu, monkeypatch):
    """gr_compact_log rewrites the header between steady passes: committed (the
    field, the row stale) is what it was, and the next passes equal the oracle
    stepping from the same firstIndex."""
    import parity
    _split(monkeypatch)
    G, R = 192, 3
    drv = _DevDriver(_peers(G, R, 19), G, R)
    try:
        _steady(drv, 4)
        drv.apply_all()
        ls = drv.ls
        cur = ls.pop.export()
        idx = np.arange(0, R * G, 2, dtype=np.uint32)
        new_lo = cur["committed"][idx] - np.uint64(1)
        rc, st = ls.eng.compact_log(idx, new_lo)
        assert rc == 0 and (st == 0).all()
        dev = ls.eng.sync(R * G)
        assert np.array_equal(dev["committed"], cur["committed"])
        assert np.array_equal(dev["first_index_m1"][idx], new_lo)
        want = dev.copy()  # the oracle continues from the compacted records
        ls.pop.reload(np.arange(R * G), want)
        assert not parity.compare_states(dev, ls.pop.export(), R)
        _steady(drv, 3, k0=4)
        assert drv.escalations == 0
    finally:
        drv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["GpuBackend", "GpuCompactBackend"])
def test_host_record_passes_after_steady(gpu, monkeypatch, backend):
    """gr_step / gr_step_compact (FastLane without the steady kernel) on an
    engine whose rows four steady device passes left stale: load the device's
    own records into a host-record engine state and step on."""
    _split(monkeypatch)
    G, R = 192, 3
    n = R * G
    topo = P.Topology(G, R)
    drv = _DevDriver(_peers(G, R, 23), G, R)
    try:
        _steady(drv, 4)
        dls = drv.ls
        eng = dls.eng

        class Reuse(getattr(SIM, backend)):  # the Lockstep's backend over the same engine
            def __init__(self, peers, slots, max_entry_size=abi.MAX_ENTRY_SIZE):
                self.eng, self.n = eng, n

            def close(self):
                pass
        ls = SIM.Lockstep(Reuse, dls.pop.export(), R)
        msgs = dls.msgs
        for k in range(4, 8):
            out, _ = ls.step(msgs, P.propose_locals(n, np.arange(G), pass_index=k))
            msgs = topo.route_messages(out)
        assert ls.stats["escalations"] == 0 and ls.stats["commits"] > 0
    finally:
        drv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("S", [3, 5])
def test_record_round_trip_device(gpu, S):
    """load -> sync returns every record unchanged, lags 0..8 (gr_io.h
    peers_to_rows / rows_to_peers), then a steady pass equals the oracle."""
    import parity
    peers, G, _ = _lag_records(S, "leader")
    ls = SIM.Lockstep(SIM.GpuBackend, peers, S)
    try:
        got = ls.eng.sync()
        assert not parity.compare_states(got, parity.normalize_marks(peers), S)
        assert np.array_equal(got["committed"], peers["committed"])
        out, _ = ls.step(None, P.propose_locals(S * G, np.arange(G), pass_index=0))
        ls.step(P.Topology(G, S).route_messages(out), P.propose_locals(S * G, np.arange(G), pass_index=1))
    finally:
        ls.close()

"""The quiesce manager on the device, on the GPU (-m gpu): gr_quiesce_kernel and
the general lane's Quiesce sends against tests/quiesce_model.py and the oracle
after every pass (quiesce_common.QuiesceLockstep). The managers run with
electionTick = 2, so the quiesce threshold is 20 ticks; raft itself runs with
election_timeout = 3, the smallest the reference's config check (ElectionRTT >
2 * HeartbeatRTT), and with it the oracle, accepts."""
import ctypes

import numpy as np
import pytest

from dragonboat_amd import abi, populations as P
from dragonboat_amd.engine import Engine, decode_space
import quiesce_common as QC

pytestmark = pytest.mark.gpu

ET = 2  # the managers' electionTick: threshold 20 ticks, new-to-quiesce window 2
RT = 3  # raft's election_timeout (heartbeat_timeout 1)


def _schedule(monkeypatch, split):
    """The fused small kernel (default at these sizes) or the forced split
    schedule: steady kernel, role instances, tick kernel, general kernel."""
    if split:
        monkeypatch.setenv("GR_SMALL_BLOCKS", "0")
        monkeypatch.setenv("GR_SPLIT_MIN_LANES", "1")


def _calm(peers):
    """With so short a timeout a follower is a late heartbeat or two from a
    campaign: start every election tick at 0 and take the largest timeout of
    [3, 6), so a healthy group never campaigns around a pass without a message."""
    peers["election_tick"] = 0
    peers["randomized_election_timeout"] = 2 * RT - 1
    return peers


def _burst_locals(n, leaders, k):
    return P.propose_locals(n, leaders, seed=77, pass_index=k, ticks=1)


def _notice_then_noop(targets, G, R):
    """Two inbox records for each target from one other replica: a Quiesce notice,
    then a NoOP (no raft handler, but activity: node.go:736-743), so the manager
    enters quiesce, raises its new-state flag and is awake again for the ticks."""
    m = np.zeros(2 * len(targets), abi.MESSAGE)
    m["peer"] = np.repeat(targets, 2)
    m["slot"] = (m["peer"] // G + 1) % R
    m["type"] = np.tile([abi.QUIESCE, abi.NOOP], len(targets))
    return m


# ---- idle -> quiesce -> burst -> re-quiesce
@pytest.mark.parametrize("split", [False, True], ids=["small", "split"])
@pytest.mark.parametrize("G,R", [(200, 3), (320, 3), (100, 5)])
def test_idle_quiesce_burst_requiesce(gpu, monkeypatch, G, R, split):
    _schedule(monkeypatch, split)
    n = G * R
    peers = _calm(P.make_groups(G, R, seed=31, election=RT))
    ls = QC.QuiesceLockstep(peers, G, R, QC.quiesce_records(n, ET))
    try:
        assert ls.eng.get_quiesce()
        third = np.arange(0, G, 3)  # leaders are replica 0: slots 0..G-1
        first_all = None
        for k in range(70):
            if k in (30, 36):  # the second burst falls inside the just-exited window
                ls.step(_burst_locals(n, third, k))
            else:
                ls.step(tick_all=(1, 1000 + k))
            if first_all is None and ls.all_quiesced():
                first_all = k
            if k == 29:
                assert ls.all_quiesced()
            if k == 32:
                assert not ls.all_quiesced()
        assert first_all is not None and first_all <= 22, first_all
        assert ls.all_quiesced(), "the burst's groups did not go back to sleep"
        q = ls.qstats
        assert q["quiesce_msgs"] >= n * (R - 1) and q["exited"] >= len(third) * R, q
        assert ls.stats["escalations"] == 0, ls.stats
        assert ls.stats["commits"] > 0
    finally:
        ls.close()


# ---- mixed population: disabled peers, random records, ReadIndex locals, dropped acks
def test_mixed_population(gpu):
    """30% of the peers disabled and random initial records, both by group: a
    leader asleep under awake followers (or the reverse) is an election, which
    test_escalation_prefix covers; here the managers' traffic is under test."""
    G, R = 200, 3
    n = G * R
    rng = np.random.default_rng(9)
    peers = _calm(P.make_groups(G, R, seed=32, election=RT))
    qg = QC.quiesce_records(G, ET)
    qg["enabled"] = rng.random(G) >= 0.3
    warm = rng.random(G) < 0.6
    qg["tick"][warm] = rng.integers(1, 60, warm.sum())
    qg["no_activity_since"][warm] = qg["tick"][warm] - np.minimum(qg["tick"][warm], rng.integers(0, 25, warm.sum()))
    qd = warm & (rng.random(G) < 0.4)
    qg["quiesced_since"][qd] = np.maximum(1, qg["tick"][qd] - rng.integers(0, 4, qd.sum()))
    ex = warm & ~qd & (rng.random(G) < 0.5)
    qg["exit_quiesce_tick"][ex] = qg["tick"][ex] - np.minimum(qg["tick"][ex], rng.integers(0, 30, ex.sum()))
    ls = QC.QuiesceLockstep(peers, G, R, np.tile(qg, R))
    try:
        for k in range(36):
            loc = P.propose_locals(n, np.zeros(0, np.int64), seed=5, pass_index=k, ticks=0)
            # at most two LocalTicks, the same for a group's replicas: a mailbox holds six
            # messages (a notice, two heartbeats, a ReadIndex heartbeat and two Replicates fill it)
            loc["ticks"] = np.tile(rng.choice([0, 1, 1, 1, 2], G), R)
            ri = np.zeros(n, bool)
            ri[:G] = rng.random(G) < 0.08  # on leaders, asleep or awake: their heartbeats carry the hint
            loc["read_index"] = ri
            loc["read_ctx_low"] = np.where(ri, 1 + k * n + np.arange(n), 0)
            loc["read_ctx_high"] = np.where(ri, 7, 0)
            if k % 9 == 4:
                loc["propose_entries"][rng.choice(G, G // 4, replace=False)] = 1
            ls.step(loc, drop_fn=lambda kk, m: P.drop_acks(m, 0.3, rng))
        qs = ls.qstats
        assert qs["entered"] > 0 and qs["exited"] > 0 and qs["split"] > 0 and qs["quiesce_msgs"] > 0, qs
        assert ls.stats["escalations"] == 0, ls.stats
    finally:
        ls.close()


# ---- escalation prefix: elections off, followers whose timeout fires on a tick
@pytest.mark.parametrize("split", [False, True], ids=["small", "split"])
def test_escalation_prefix(gpu, monkeypatch, split):
    monkeypatch.delenv("GR_ELECTIONS", raising=False)
    _schedule(monkeypatch, split)
    G, R = 100, 3
    n = G * R
    peers = P.cold_start(G, R, seed=33, election=RT)
    q = QC.quiesce_records(n, ET)
    q["tick"] = 100  # outside the just-exited window: a notice is taken
    q["no_activity_since"] = 100
    ls = QC.QuiesceLockstep(peers, G, R, q)
    try:
        # a Quiesce notice (and a NoOP that wakes the peer again) for every third
        # peer, then two LocalTicks: the entry lies below the tick whose election
        # timeout escalates; every sixth peer only gets the notice and sleeps
        notice = _notice_then_noop(np.arange(0, n, 3), G, R)
        notice = notice[~((notice["type"] == abi.NOOP) & (notice["peer"] % 6 == 0))]
        ls.override_inbox(notice)
        for k in range(8):
            loc = P.propose_locals(n, np.zeros(0, np.int64), seed=6, pass_index=k, ticks=2)
            ls.step(loc)
        assert ls.stats["esc_reasons"].get("election", 0) > 0, ls.stats
        assert ls.qstats["prefix_sends"] > 0, ls.qstats
    finally:
        ls.close()


# ---- switch off: the same inputs leave the records untouched, results as before
def test_switch_off_leaves_records_alone(gpu, monkeypatch):
    monkeypatch.delenv("GR_QUIESCE_ON_DEVICE", raising=False)
    G, R = 100, 3
    n = G * R
    peers = _calm(P.make_groups(G, R, seed=34, election=RT))
    q = QC.quiesce_records(n, ET)
    q["tick"], q["no_activity_since"] = 100, 80  # the next tick would enter quiesce
    ls = QC.QuiesceLockstep(peers, G, R, q, quiesce=False)
    try:
        assert not ls.eng.get_quiesce()
        notice = np.zeros(G, abi.MESSAGE)
        notice["peer"], notice["slot"], notice["type"] = np.arange(G, 2 * G), 0, abi.QUIESCE
        ls.override_inbox(notice)
        for k in range(4):  # the harness checks the records against the untouched model every pass
            ls.step(P.propose_locals(n, np.arange(G), seed=7, pass_index=k, ticks=1, quiesced=k % 2))
        assert ls.qstats["quiesce_msgs"] == 0
        assert np.array_equal(ls.eng.sync_quiesce(n), q)
    finally:
        ls.close()


# ---- a checkQuorum leader steps down on a tick_all tick: the documented draws
def test_step_down_on_broadcast_tick(gpu):
    G, R = 100, 3
    n = G * R
    peers = _calm(P.make_groups(G, R, seed=35, election=RT, check_quorum=True))
    peers["remotes"]["active"] = 0  # nobody has answered since the last check
    ls = QC.QuiesceLockstep(peers, G, R, QC.quiesce_records(n, ET))
    try:
        for k in range(4):  # every message to a leader is lost: its quorum check fails on the third tick
            ls.step(tick_all=(1, 50 + k), drop_fn=lambda kk, m: m[m["peer"] >= G])
        st = ls.export()
        assert np.all(st["state"][:G] == abi.FOLLOWER), "a leader did not step down"
        # reset() took gr_tick_all's draw of that pass (raft.go:704-720 with the documented splitmix64)
        draw = np.array([abi.splitmix64(52 + p) for p in range(G)], np.uint64)
        assert np.array_equal(st["randomized_election_timeout"][:G], RT + draw % np.uint64(RT))
    finally:
        ls.close()


# ---- graph: two captured passes with tick_all bound, replayed 20 times
def test_graph_replay_with_broadcast_tick(gpu):
    import torch
    from oracle.pyoracle import OraclePopulation
    from quiesce_model import QuiesceManager
    import devsim
    import parity
    G, R = 100, 3
    n, S = G * R, R
    peers = _calm(P.make_groups(G, R, seed=36, election=RT))
    q = QC.quiesce_records(n, ET)
    topo = P.Topology(G, R)
    in_pos, out_pos = topo.loopback_routes(S)
    eng = Engine(n, S, quiesce=True)
    try:
        eng.load(peers)
        eng.load_quiesce(q)
        eng.bind_routes(in_pos, out_pos)
        eng.tick_all(1, 99)
        nb = eng.space_bytes(1, n * S)
        a, b = (torch.zeros(nb, dtype=torch.uint8, device="cuda") for _ in range(2))
        g = eng.graph_capture(a.data_ptr(), b.data_ptr(), 1, n * S, n, 2)
        for _ in range(20):
            eng.graph_replay(g, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        eng.graph_destroy(g)
        # the same 40 passes on the oracle, split by the model
        pop = OraclePopulation(peers, S)
        model = [QuiesceManager.from_record(r) for r in q]
        loc = QC.tick_locals(peers, 1, 99)
        msgs = np.zeros(0, abi.MESSAGE)
        for k in range(40):
            per = [[] for _ in range(n)]
            for x in np.lexsort((np.arange(len(msgs)), msgs["slot"], msgs["peer"])):
                per[int(msgs["peer"][x])].append((int(msgs["type"][x]), int(msgs["hint"][x])))
            eff, senders = loc.copy(), []
            for p, m in enumerate(model):
                eff["ticks"][p], eff["quiesced_ticks"][p], send = m.run_pass(False, per[p], 1)
                if send:
                    senders.append(p)
            o = pop.step(msgs, eff)
            qm = np.zeros((len(senders), R - 1), abi.MESSAGE)
            for x, p in enumerate(senders):
                qm[x]["peer"], qm[x]["type"] = p, abi.QUIESCE
                qm[x]["slot"] = [j for j in range(R) if j != p // G]
            msgs = devsim.route(np.concatenate([qm.reshape(-1), o["msgs"]]), None, G, R)
        assert all(m.quiesced() for m in model)
        want_q = np.zeros(n, abi.QUIESCE_STATE)
        for p, m in enumerate(model):
            m.to_record(want_q[p])
        assert np.array_equal(eng.sync_quiesce(n), want_q)
        assert not parity.compare_states(eng.sync(n), pop.export(), S)
    finally:
        eng.close()


def _about_to_quiesce(n, tick):
    q = QC.quiesce_records(n, ET)
    q["tick"] = tick  # threshold 20: tick 21 enters
    return q


# ---- boundaries: gr_step and gr_step_compact return the Quiesce messages
def test_host_paths_return_quiesce_messages(gpu):
    G, R = 64, 3
    n = G * R
    peers = _calm(P.make_groups(G, R, seed=37, election=RT))
    loc = P.propose_locals(n, np.zeros(0, np.int64), seed=8, ticks=2)  # a Tick (leaders' heartbeats), then the entry
    outs = []
    for compact in (False, True):
        eng = Engine(n, R, quiesce=True)
        try:
            eng.load(peers)
            eng.load_quiesce(_about_to_quiesce(n, 19))
            bad = loc.copy()
            bad["quiesced_ticks"][5] = 1  # a host-chosen split is refused before anything is written
            with pytest.raises(Exception):
                eng.step(None, bad) if not compact else eng.step_compact(
                    np.zeros(0, abi.CMSG), np.zeros(0, abi.MESSAGE), *eng.pack_locals(bad))
            assert np.array_equal(eng.sync_quiesce(n), _about_to_quiesce(n, 19))
            if compact:
                c, ext, cres, xres = eng.step_compact(np.zeros(0, abi.CMSG), np.zeros(0, abi.MESSAGE),
                                                      *eng.pack_locals(loc))
                out = eng.unpack_messages(c, ext)
                assert len(cres) == n
            else:
                out, res = eng.step(None, loc)
                assert not res["escalation"].any()
            qs = eng.sync_quiesce(n)
            assert np.all(qs["quiesced_since"] == 21) and np.all(qs["tick"] == 21)
            st = eng.sync(n)
            assert np.all(st["election_tick"][G:] == 2)  # one Tick, one QuiescedTick
        finally:
            eng.close()
        outs.append(out)
        qm = out[out["type"] == abi.QUIESCE]
        assert len(qm) == n * (R - 1) and not qm["term"].any()
        # first in its mailbox: every leader -> follower mailbox is [Quiesce, Heartbeat]
        for p in range(G):
            for j in (1, 2):
                mb = out[(out["peer"] == p) & (out["slot"] == j)]
                assert mb["type"].tolist() == [abi.QUIESCE, abi.HEARTBEAT], (p, j, mb["type"])
    key = lambda m: np.sort(m, order=["peer", "slot", "type"])
    assert np.array_equal(key(outs[0]), key(outs[1]))


# ---- boundaries: a Quiesce frame through gr_step_wire quiesces its peer
def test_wire_quiesce_frame(gpu):
    import wirefeed
    G, R = 64, 3
    n = G * R
    peers = P.make_groups(G, R, seed=38, election=RT)
    cl = (np.arange(n) % G) + 1
    eng = Engine(n, R, quiesce=True)
    feed = wirefeed.WireFeed(peers, cl)
    try:
        eng.load(peers)
        q = QC.quiesce_records(n, ET)
        q["tick"], q["no_activity_since"] = 100, 100
        eng.load_quiesce(q)
        eng.bind_nodes(cl, peers["node_id"])
        m = np.zeros(2, abi.MESSAGE)
        m["peer"], m["slot"], m["type"] = [G + 3, 2 * G + 9], [0, 1], abi.QUIESCE
        d_msgs, nm, d_ents, ne, keep = feed.decode(m)
        out, res, idx, why = eng.step_wire(d_msgs, nm, d_ents, ne)
        assert len(idx) == 0, (idx, why)
        got = eng.sync_quiesce(n)
        want = q.copy()
        want["quiesced_since"][[G + 3, 2 * G + 9]] = 100
        assert np.array_equal(got, want)
        # both announce it in turn (node.go:643-645), to the other two voters
        assert sorted(out["peer"][out["type"] == abi.QUIESCE].tolist()) == [G + 3, G + 3, 2 * G + 9, 2 * G + 9]
    finally:
        feed.close()
        eng.close()


# ---- boundaries: a mailbox with a Quiesce message and a heartbeat crosses the compact exchange
def test_quiesce_message_survives_cx(gpu):
    import torch
    from dragonboat_amd import exchange as X
    eng = Engine(64, 3)
    try:
        positions, depth = 256, abi.GR_C
        pc = X.pad_positions(positions)
        nb = eng.space_bytes(1, positions, depth)
        m = np.zeros(3, abi.MESSAGE)
        m["peer"] = [7, 7, 130]
        m["type"] = [abi.QUIESCE, abi.HEARTBEAT, abi.QUIESCE]
        m["term"] = [0, 5, 0]
        m["commit"][1], m["hint"][1], m["hint_high"][1] = 1234, 11, 12
        pos = np.array([7, 7, 130], np.uint32)
        src = np.zeros(nb, np.uint8)
        assert eng.lib.gr_space_encode(src.ctypes.data, 1, positions, depth, m.ctypes.data, 3, pos.ctypes.data) == 0
        want = decode_space(src, 1, positions, depth)
        cb = eng.cx_bytes(1, positions, depth, pc, pc)
        d_src = torch.from_numpy(src).cuda()
        d_cx = torch.zeros(cb, dtype=torch.uint8, device="cuda")
        d_dst = torch.full((nb,), 0xA5, dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        eng.cx_pack(d_src.data_ptr(), 1, positions, depth, d_cx.data_ptr(), pc, pc, s)
        eng.cx_unpack(d_dst.data_ptr(), 1, positions, depth, d_cx.data_ptr(), pc, pc, s)
        torch.cuda.synchronize()
        got = decode_space(d_dst.cpu().numpy(), 1, positions, depth)
        assert len(got) == 3 and np.array_equal(got, want)
        assert got["type"].tolist() == [abi.QUIESCE, abi.HEARTBEAT, abi.QUIESCE]
    finally:
        eng.close()


# ---- load / sync over ranges and slot lists, refusals as gr_load_peers
def test_load_sync_and_refusals(gpu):
    from dragonboat_amd.engine import GpuRaftError
    eng = Engine(300, 3)
    try:
        assert not eng.sync_quiesce().view(np.uint8).any()  # never loaded: disabled, all zero
        rng = np.random.default_rng(4)
        q = np.zeros(100, abi.QUIESCE_STATE)
        for f in ("tick", "quiesced_since", "no_activity_since", "exit_quiesce_tick"):
            q[f] = rng.integers(0, 1 << 32, 100, dtype=np.uint64)
        q["election_tick"] = rng.integers(0, 1 << 31, 100, dtype=np.uint64)
        q["enabled"] = rng.integers(0, 2, 100)
        eng.load_quiesce(q, first=50)
        assert np.array_equal(eng.sync_quiesce(100, first=50), q)
        slots = rng.permutation(300)[:100].astype(np.uint32)
        eng.load_quiesce(q, slots=slots)
        assert np.array_equal(eng.sync_quiesce(slots=slots), q)
        before = eng.sync_quiesce()
        for f, v in (("tick", 1 << 32), ("election_tick", 1 << 31), ("enabled", 2)):
            bad = q.copy()
            bad[f][17] = v
            with pytest.raises(GpuRaftError, match="invalid"):
                eng.load_quiesce(bad, first=0)
        with pytest.raises(GpuRaftError, match="range"):
            eng.load_quiesce(q, first=250)
        with pytest.raises(GpuRaftError, match="range"):
            eng.load_quiesce(q[:2], slots=[5, 5])
        with pytest.raises(GpuRaftError, match="range"):
            eng.sync_quiesce(slots=[1, 300])
        assert np.array_equal(eng.sync_quiesce(), before)  # nothing was written
        peers = P.make_groups(100, 3, seed=1)
        eng.load(peers)  # loading groups leaves the quiesce records alone
        assert np.array_equal(eng.sync_quiesce(), before)
        assert eng.lib.gr_splitmix64(12345) == abi.splitmix64(12345)
    finally:
        eng.close()


# ---- the third coverage table: every id reached on the device, no BAD_* id hit
def test_quiesce_coverage(gpu, monkeypatch):
    from dragonboat_amd import build
    from dragonboat_amd.engine import load_library
    monkeypatch.delenv("GR_ELECTIONS", raising=False)
    lib = load_library(build.COVER_LIB)

    def read(fn_read, fn_names):
        names = [x for x in fn_names().decode().split(",") if x]
        buf = (ctypes.c_uint64 * len(names))()
        assert fn_read(buf, len(names)) == len(names)
        return dict(zip(names, list(buf)))

    q0 = read(lib.gr_coverage_quiesce_read, lib.gr_coverage_quiesce_names)
    b0 = read(lib.gr_coverage_read, lib.gr_coverage_names)
    G, R = 70, 3
    n = G * R
    # idle -> quiesce with two LocalTicks a pass (a pass that splits), a ReadIndex, a burst
    ls = QC.QuiesceLockstep(_calm(P.make_groups(G, R, seed=39, election=RT)), G, R, _about_to_quiesce(n, 9),
                            lib_path=build.COVER_LIB)
    try:
        for k in range(12):
            if k == 9:
                loc = P.propose_locals(n, np.arange(0, G, 2), seed=3, pass_index=k, ticks=1)
                loc["read_index"][1], loc["read_ctx_low"][1] = 1, 99  # a quiesced leader's ReadIndex
                ls.step(loc)
            else:
                ls.step(tick_all=(1 if k < 4 else 2, k))
        for k in range(12, 15):  # proposals alone: the lean lane's uniform mailboxes
            ls.step(P.propose_locals(n, np.arange(G), seed=3, pass_index=k))
    finally:
        ls.close()
    # a notice below an escalating tick (elections off)
    q = QC.quiesce_records(n, ET)
    q["tick"], q["no_activity_since"] = 100, 100
    ls = QC.QuiesceLockstep(P.cold_start(G, R, seed=40, election=RT), G, R, q, lib_path=build.COVER_LIB)
    try:
        ls.override_inbox(_notice_then_noop(np.arange(0, n, 2), G, R))
        for k in range(3):
            ls.step(P.propose_locals(n, np.zeros(0, np.int64), seed=4, pass_index=k, ticks=2))
        assert ls.qstats["prefix_sends"] > 0
    finally:
        ls.close()
    q1 = read(lib.gr_coverage_quiesce_read, lib.gr_coverage_quiesce_names)
    b1 = read(lib.gr_coverage_read, lib.gr_coverage_names)
    missed = [x for x in q1 if q1[x] == q0[x]]
    assert not missed, missed
    bad = {x: b1[x] - b0[x] for x in b1 if x.startswith("BAD_") and b1[x] != b0[x]}
    assert not bad, bad

"""gr_collect_updates after passes of every device switch: campaigns, votes and
promotions, InstallSnapshot restores, config-change entries, the quiesce manager
with gr_tick_all, an escalation hand-off and a real gr_graph_replay, on the fused
small kernel and on the split schedule forced onto a small population (where the
steady, role, tick and general kernels each write LR_RFLAGS in their own way).

The reference of every collect but the graph replay's owes nothing to the
engine: the oracle's results and records of the pass (devsim.DeviceLockstep's
collect callback, updates_common.LockstepCollect) or the reference side of
all_switches_common.Population, through the Python restatement of Peer.HasUpdate
in updates_common.ref_classes. Every comparison is exact."""
import numpy as np
import pytest

from dragonboat_amd import abi, populations as P
from dragonboat_amd.engine import Engine
import devsim
import elections_common as EC
import parity
import quiesce_common as QC
import updates_common as UC
from test_all_switches import check_live_all, check_update_counts, live_all
from test_quiesce_gpu import ET, RT, _burst_locals, _calm, _notice_then_noop, _schedule
from test_updates import COLD_EXT, COLD_REPORTED, cold_locals

pytestmark = pytest.mark.gpu
U32 = np.uint32
SCHEDULES = pytest.mark.parametrize("split", [False, True], ids=["small", "split"])


@pytest.fixture(autouse=True)
def _no_env_switch(monkeypatch):
    for v in ("GR_SNAPSHOTS", "GR_CONFIG_ENTRIES", "GR_ELECTIONS", "GR_QUIESCE_ON_DEVICE"):
        monkeypatch.delenv(v, raising=False)


# ---------------------------------------------------------------- every switch at once
@pytest.mark.parametrize("G,drain_after", [(192, False), (200, True)])  # route_wu = 1 / 0
def test_live_all_updates(gpu, monkeypatch, G, drain_after):
    """test_all_switches.live_all on the split schedule with the host driven by
    gr_collect_updates alone (all_switches_common.Population, updates=True): every
    collect against the reference side's own results and records, commits and
    applied indexes to the reported slots only, from the records; the reference
    side commits every peer, so a lost update shows in the next pass's comparison.
    The engine's counts per pass equal the reference's, which equal the table of
    test_all_switches. G = 192 drains gr_restored_snapshots and gr_promotions
    before the collect, G = 200 after it: both give the reference's lists."""
    monkeypatch.setenv("GR_SPLIT_MIN_LANES", "1")
    monkeypatch.setenv("GR_SMALL_BLOCKS", "0")
    pop, committed = live_all("dev", G, updates=True, drain_after=drain_after)
    try:
        check_live_all(pop, committed, G)
        check_update_counts(pop, G)
    finally:
        pop.close()


# ---------------------------------------------------------------- elections
@SCHEDULES
@pytest.mark.parametrize("G", [200, 320])  # route_wu = 0 / 1
def test_cold_start_collect(gpu, monkeypatch, G, split):
    """The cold start of test_cold_start_split_schedule (40 passes of one tick,
    seed 21) with a collect against the oracle's records after every pass and the
    reported peers committed on both sides. A peer whose term or vote moved
    arrives EXT with that term and vote; every promotion is reported. The counts
    per pass are those of the oracle alone (test_updates.COLD_REPORTED, derived
    without a device): all 3 G peers after pass 0, a peak of 213 of 600 at pass 9
    (320 of 960 at pass 8), nothing in passes 20..25 and 32..39 (20 and 27..39)."""
    monkeypatch.setenv("GR_ELECTIONS", "1")
    _schedule(monkeypatch, split)
    R, n = 3, 3 * G
    peers = EC.cold_peers(G, R, 21)
    ds = devsim.DeviceLockstep(peers, G, R)
    try:
        assert ds.eng.get_elections()
        col = UC.LockstepCollect(ds, peers)
        promoted = 0
        for k in range(40):
            before = ds.export()
            ds.step(cold_locals(G, k), collect=col)
            turned = (before["state"] != abi.LEADER) & (col.state["state"] == abi.LEADER)
            assert col.classes[turned].all(), f"pass {k}: the reference does not report a promotion"
            pr = ds.eng.promotions()  # after the collect: it takes nothing from the list
            assert sorted(pr["peer"].tolist()) == np.nonzero(turned)[0].tolist(), f"pass {k}"
            assert np.all(col.at[pr["peer"].astype(np.int64)] >= 0), f"pass {k}: a promotion was not reported"
            promoted += len(pr)
        got = [c[0] for c in col.counts]
        print("cold start collect", G, split, col.counts)
        assert 0 in got and max(got[1:]) > n // 4
        assert got == COLD_REPORTED[G] and [c[1] for c in col.counts] == COLD_EXT[G]
        assert promoted >= G and np.all(EC.leaders_per_group(ds.export(), G, R) == 1)
    finally:
        ds.close()


# ---------------------------------------------------------------- quiesce on the device
@SCHEDULES
def test_quiesce_collect(gpu, monkeypatch, split):
    """test_idle_quiesce_burst_requiesce at 200 x 3 (70 passes, gr_tick_all, two
    bursts) with a collect against the oracle after every pass, the reported
    peers committed. While every manager sleeps (pass 29 and the last) the
    reference reports no peer, and the engine returns no record and copies 8
    bytes down. A burst pass reports at least the proposing leaders.

    This case first showed the engine's race at the update states' allocation
    (DESIGN.md §3): gr_set_update_states as the first call on them lost its first
    slots to the zero fill, so the first collect classified against the empty
    State. check_collect now reads the update states before every collect."""
    _schedule(monkeypatch, split)
    G, R = 200, 3
    n = G * R
    peers = _calm(P.make_groups(G, R, seed=31, election=RT))
    ls = QC.QuiesceLockstep(peers, G, R, QC.quiesce_records(n, ET))
    try:
        col = UC.LockstepCollect(ls, peers)
        third = np.arange(0, G, 3)
        for k in range(70):
            col.want_none = k in (29, 69)
            if k in (30, 36):
                loc = _burst_locals(n, third, k)
                col.propose = loc["propose_entries"]
                ls.step(loc, collect=col)
                assert col.classes[third].all() and np.all(col.at[third] >= 0), f"pass {k}: a proposing leader"
                col.propose = None
            else:
                ls.step(tick_all=(1, 1000 + k), collect=col)
            if col.want_none:
                assert ls.all_quiesced(), k
        print("quiesce collect", split, col.counts)
        assert ls.stats["escalations"] == 0 and ls.stats["commits"] > 0
    finally:
        ls.close()


# ---------------------------------------------------------------- escalation hand-off
@SCHEDULES
def test_escalation_handoff(gpu, monkeypatch, split):
    """test_escalation_prefix's cold start with elections off (100 x 3, two ticks
    a pass, 8 passes). In the callback every escalated peer arrives EXT with the
    reason and item it stopped at and its State at the device prefix. The harness
    then reloads it with the record of its whole pass and the test sets its update
    state to that State, as a host that ran the suffix has handed it on; a second
    collect before the next pass reports the peer only for what it still has to
    save or apply, and the next pass's record carries no escalation of the last."""
    _schedule(monkeypatch, split)
    G, R = 100, 3
    n = G * R
    peers = P.cold_start(G, R, seed=33, election=RT)
    q = QC.quiesce_records(n, ET)
    q["tick"], q["no_activity_since"] = 100, 100
    ls = QC.QuiesceLockstep(peers, G, R, q)
    every = np.arange(n, dtype=U32)
    try:
        col = UC.LockstepCollect(ls, peers)
        notice = _notice_then_noop(np.arange(0, n, 3), G, R)
        ls.override_inbox(notice[~((notice["type"] == abi.NOOP) & (notice["peer"] % 6 == 0))])
        handed, last = 0, np.zeros(0, np.int64)
        for k in range(8):
            res = ls.step(P.propose_locals(n, np.zeros(0, np.int64), seed=6, pass_index=k, ticks=2), collect=col)
            esc = res[res["escalation"] != 0]
            idx = esc["peer"].astype(np.int64)
            c = col.cr[col.at[idx]]
            assert np.all(col.at[idx] >= 0) and np.all(c["flags"] & abi.CR_EXT), f"pass {k}"
            x, mid = col.rx[c["aux"].astype(np.int64)], col.state[idx]
            assert np.array_equal(x["escalation"], esc["escalation"]) and np.array_equal(x["esc_item"], esc["esc_item"])
            assert np.array_equal(x["esc_item"], col.dense["esc_item"][idx])
            for f, g in (("term", "term"), ("vote", "vote"), ("committed", "committed"), ("last_index", "last_index")):
                assert np.array_equal(x[f], mid[g]), (k, f)
            # the last pass's escalated peers: nothing of it in this pass's records
            again = np.isin(last, idx)
            old = col.at[last[~again]]
            assert not col.cr["escalation"][old[old >= 0]].any()
            assert not col.dense["escalation"][last[~again]].any()
            # reloaded: the State the host handed on, then a collect before the next pass
            full = ls.export()
            hs = np.zeros(len(idx), abi.UPDATE_STATE)
            hs["term"], hs["vote"], hs["commit"] = full["term"][idx], full["vote"][idx], full["committed"][idx]
            col.ref.prev[idx] = hs
            ls.eng.set_update_states(idx.astype(U32), hs)
            now = parity.normalize_marks(full)
            dense = np.zeros(n, abi.RESULT)  # the first collect took the per-pass fields: State and the log's marks
            dense["peer"] = every
            for f in ("term", "vote", "committed", "last_index"):
                dense[f] = now[f]
            dense["save_from"] = UC.ref_save_from(now["saved_to"], now["marker_index"], now["last_index"])
            cr, rx, _, _ = UC.check_collect(ls.eng, col.ref, n, dense=dense, state=now)
            owes = (dense["save_from"] != 0) | (dense["committed"] > np.maximum(now["log_applied"], now["first_index_m1"]))
            assert np.array_equal(cr["peer"].astype(np.int64), np.nonzero(owes)[0]) and len(rx) == 0
            assert not cr["escalation"].any()
            UC.commit_reported(ls, now, cr["peer"])
            handed += len(idx)
            last = idx
        print("escalation hand-off", split, ls.stats["esc_reasons"], handed, col.counts)
        assert ls.stats["esc_reasons"].get("election", 0) > 0 and handed > 0, ls.stats
    finally:
        ls.close()


# ---------------------------------------------------------------- graph replay
@SCHEDULES
def test_graph_replay_collect(gpu, monkeypatch, split):
    """Elections on, a cold start of 100 x 3 with gr_tick_all(1, 99) bound, a
    two-pass graph replayed 20 times, a collect after each replay against the
    dense collect and sync of that moment (no oracle holds per-pass records of a
    replay). Every peer whose term or vote differs from the mirrored prev
    arrives EXT, those included that the first pass of the pair moved and the
    second left alone, which the same inputs stepped pass by pass through
    DeviceLockstep name. The final state equals the oracle's after 40 passes."""
    import torch
    monkeypatch.setenv("GR_ELECTIONS", "1")
    _schedule(monkeypatch, split)
    G, R = 100, 3
    n, S = G * R, R
    peers = EC.cold_peers(G, R, 21)
    loc = QC.tick_locals(peers, 1, 99)
    every = np.arange(n, dtype=U32)
    # pass by pass beside the oracle: term and vote after every pass
    ds = devsim.DeviceLockstep(peers, G, R)
    try:
        tv = [np.stack([peers["term"], peers["vote"]])]
        for k in range(40):
            ds.step(loc)
            st = ds.export()
            tv.append(np.stack([st["term"], st["vote"]]))
        assert ds.stats["escalations"] == 0, ds.stats
        want = ds.export()
    finally:
        ds.close()
    assert np.all(EC.leaders_per_group(want, G, R) == 1)
    eng = Engine(n, S, elections=True)
    try:
        eng.load(peers)
        in_pos, out_pos = P.Topology(G, R).loopback_routes(S)
        eng.bind_routes(in_pos, out_pos)
        ref = UC.RefUpdates(n)
        eng.set_update_states(every, ref.launch(peers))
        eng.tick_all(1, 99)
        nb = eng.space_bytes(1, n * S)
        a, b = (torch.zeros(nb, dtype=torch.uint8, device="cuda") for _ in range(2))
        g = eng.graph_capture(a.data_ptr(), b.data_ptr(), 1, n * S, n, 2)
        first_only = 0
        for i in range(20):
            eng.graph_replay(g, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            before = ref.prev.copy()
            cr, rx, dense, _ = UC.check_collect(eng, ref, n)
            assert np.array_equal(np.stack([dense["term"], dense["vote"]]), tv[2 * i + 2]), f"replay {i}"
            moved = np.nonzero((dense["term"] != before["term"]) | (dense["vote"] != before["vote"]))[0]
            at = np.full(n, -1, np.int64)
            at[cr["peer"].astype(np.int64)] = np.arange(len(cr))
            c = cr[at[moved]]
            assert np.all(at[moved] >= 0) and np.all(c["flags"] & abi.CR_EXT), f"replay {i}"
            x = rx[c["aux"].astype(np.int64)]
            assert np.array_equal(x["term"], tv[2 * i + 2][0][moved]) and np.array_equal(x["vote"], tv[2 * i + 2][1][moved])
            only = (tv[2 * i] != tv[2 * i + 1]).any(axis=0) & (tv[2 * i + 1] == tv[2 * i + 2]).all(axis=0)
            assert np.isin(np.nonzero(only)[0], moved).all()
            first_only += int(only.sum())
        eng.graph_destroy(g)
        assert first_only > 0  # (153 on the host lane with these inputs)
        assert not parity.compare_states(eng.sync(n), want, S)
    finally:
        eng.close()

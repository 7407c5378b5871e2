"""Snapshots on the device (gpuraft.h gr_set_snapshots): a leader's
InstallSnapshot to a compacted follower (raft.go:500-532), a peer's restore from
one (raft.go:303-325, 933-951) and Peer.RestoreRemotes (gr_restore_remotes).

Every case runs on two backends, the host lane built with snapshots compiled on
(`not gpu`) and the engine with the switch on (`-m gpu`), beside the reference
side: the oracle's raft object built from the same records and driven through
the same items (snapshot_common.py, tests/native/snapshot_ref.cpp). After every
pass the peer records, the snapshot records, the messages, the results and the
restored list must agree field for field; an escalation must be the one the case
names and leave exactly the items below it applied. After a restore two more
ordinary passes (a heartbeat, a Replicate) run the same way, so a header summary
bit left stale by the restore shows up as a mismatch. With the switch off the
escalations are what they always were (test_switch_off).
"""
import numpy as np
import pytest

from dragonboat_amd import abi, populations as P
import snapshot_common as C
from test_config_change import _group, _member

BACKENDS = [pytest.param("cpu", id="host"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
APPLIED, HOST, NO_SLOT = abi.CC_APPLIED, abi.CC_HOST, abi.CC_NO_SLOT
VOTER, OBS, EMPTY = abi.SLOT_VOTER, abi.SLOT_OBSERVER, abi.SLOT_EMPTY
ENTS = [(i, 5) for i in range(1, 11)]  # a log 1..10 at term 5


@pytest.fixture(autouse=True)
def _no_env_switch(monkeypatch):
    monkeypatch.delenv("GR_SNAPSHOTS", raising=False)
    monkeypatch.delenv("GR_ELECTIONS", raising=False)


def _need(be, request):
    request.getfixturevalue("gpu" if be == "gpu" else "built")


def _snap(index, term, n=1):
    s = np.zeros(n, abi.SNAPSHOT_REC)
    s["index"], s["term"] = index, term
    return s


def _loc(propose=0, ticks=0, rand=77):
    loc = np.zeros(1, abi.LOCAL)
    loc["propose_entries"], loc["ticks"], loc["rand"] = propose, ticks, rand
    return loc


def _msg(type_, slot, term, log_index=0, log_term=0, commit=0, reject=0, ents=0, ent_term=0, hint=0):
    m = np.zeros(1, abi.MESSAGE)
    m["type"], m["slot"], m["term"], m["log_index"], m["log_term"] = type_, slot, term, log_index, log_term
    m["commit"], m["reject"], m["hint"] = commit, reject, hint
    if ents:
        m["n_entries"], m["n_runs"] = ents, 1
        m["run_term"][0, 0] = ent_term
    return m


def _window(p, runs):
    """Replace the record's term-run window."""
    g = p[0]
    g["n_runs"], g["run_start"], g["run_term"] = len(runs), 0, 0
    for k, (s, t) in enumerate(runs):
        g["run_start"][k], g["run_term"][k] = s, t


def _install(slot, term, index, sterm, reject=0):
    """An InstallSnapshot record by gpuraft.h's convention."""
    return _msg(C.INSTALL_SNAPSHOT, slot, term, log_index=index, log_term=sterm, reject=reject)


# ---------------------------------------------------------------- the leader
def _leader(S, next2, state2=abi.RETRY, active2=1, snap2=0, state1=abi.REPLICATE_ST):
    """Node 1 leads voters 1..3 at term 5 with the log 1..10 compacted to
    firstIndex - 1 = 6; node 2 follows closely, node 3 (slot 2) lags at next2."""
    p = _group(S, 1, abi.LEADER, [10, 8, 3])
    p[0]["first_index_m1"] = 6
    _window(p, [(6, 5)])  # as gr_compact_log leaves it
    _member(p, 1, 2, VOTER, match=8, next_=11, state=state1, active=1)
    _member(p, 2, 3, VOTER, match=3, next_=next2, state=state2, active=active2)
    p[0]["remotes"][2]["snapshot_index"] = snap2
    return p


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_leader_sends_install_snapshot(be, S, request):
    """next = firstIndex - 1 on an active remote in Retry, one proposal as the
    trigger: the InstallSnapshot carries the record (6, 5) and Commit 0, the remote
    is in Snapshot state with snapshotIndex 6; the ack ReplicateResp{6} leaves
    that state and the next send starts at 7."""
    _need(be, request)
    side = C.Side(be, _leader(S, 6), S, _snap(6, 5))
    st, out, _, rest = side.step(loc=_loc(propose=1))
    to3 = out[out["slot"] == 2]
    assert len(to3) == 1 and to3[0]["type"] == C.INSTALL_SNAPSHOT
    assert [int(to3[0][f]) for f in ("log_index", "log_term", "commit", "term")] == [6, 5, 0, 5]
    r = st[0]["remotes"][2]
    assert [int(r[f]) for f in ("state", "snapshot_index", "next", "match")] == [abi.SNAPSHOT_ST, 6, 6, 3]
    assert len(rest) == 0
    st, out, _, _ = side.step(loc=_loc(propose=1))  # paused: nothing more goes to node 3
    assert not np.any(out["slot"] == 2)
    st, out, _, _ = side.step(_msg(abi.REPLICATE_RESP, 2, 5, log_index=6))
    r = st[0]["remotes"][2]
    assert int(r["match"]) == 6 and int(r["snapshot_index"]) == 0 and int(r["state"]) != abi.SNAPSHOT_ST
    to3 = out[out["slot"] == 2]
    assert len(to3) == 1 and to3[0]["type"] == abi.REPLICATE and int(to3[0]["log_index"]) == 6
    assert int(to3[0]["n_entries"]) == 6  # 7..12
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_leader_inactive_remote_and_boundary(be, S, request):
    """An inactive remote gets no message and does not change (raft.go:516-520);
    next = firstIndex is an ordinary Replicate; a remote already in Snapshot state
    is paused."""
    _need(be, request)
    side = C.Side(be, _leader(S, 6, active2=0), S, _snap(6, 5))
    before = side.state[0]["remotes"][2].copy()
    st, out, _, _ = side.step(loc=_loc(propose=1))
    assert not np.any(out["slot"] == 2) and st[0]["remotes"][2].tobytes() == before.tobytes()
    side.close()
    side = C.Side(be, _leader(S, 7), S, _snap(6, 5))
    _, out, _, _ = side.step(loc=_loc(propose=1))
    to3 = out[out["slot"] == 2]
    assert len(to3) == 1 and to3[0]["type"] == abi.REPLICATE
    assert [int(to3[0][f]) for f in ("log_index", "log_term", "n_entries")] == [6, 5, 5]
    side.close()
    side = C.Side(be, _leader(S, 6, state2=abi.SNAPSHOT_ST, snap2=6), S, _snap(6, 5))
    _, out, _, _ = side.step(loc=_loc(propose=1))
    assert not np.any(out["slot"] == 2)
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_leader_escalations(be, S, request):
    """An empty snapshot record is the reference's panic("got an empty snapshot"):
    GR_ESC_PANIC at the proposal. A full mailbox (six heartbeats already queued
    for node 3, node 2 paused) is GR_ESC_CAPACITY at the proposal, item 6."""
    _need(be, request)
    side = C.Side(be, _leader(S, 6), S, _snap(0, 0))
    _, _, res, _ = side.step(loc=_loc(propose=1), esc={0: "panic"})
    assert int(res[0]["esc_item"]) == 0
    side.close()
    side = C.Side(be, _leader(S, 6, state1=abi.WAIT), S, _snap(6, 5))
    st, out, res, _ = side.step(loc=_loc(propose=1, ticks=6), esc={0: "capacity"})
    assert int(res[0]["esc_item"]) == 6 and int(np.sum(out["slot"] == 2)) == 6
    assert int(st[0]["remotes"][2]["state"]) == abi.RETRY
    side.close()


# ---------------------------------------------------------------- the receiver
def _follower(S, ents=ENTS, committed=8, term=5, state=abi.FOLLOWER, self_id=2):
    """Node self_id of voters 1..3, led by node 1 (slot 0)."""
    p = _group(S, self_id, state, [10 if j + 1 == self_id else 0 for j in range(3)], committed=committed, term=term,
               ents=ents)
    p[0]["remotes"]["match"][self_id - 1] = p[0]["last_index"]
    return p


def _after_restore(side, index, sterm, term, leader_slot=0):
    """The restored log, then two ordinary passes under the reference."""
    g = side.state[0]
    assert [int(g[f]) for f in ("last_index", "committed", "first_index_m1", "saved_to", "marker_index",
                                "log_applied")] == [index, index, index, index, index + 1, index]
    assert int(g["n_runs"]) == 1 and (int(g["run_start"][0]), int(g["run_term"][0])) == (index, sterm)
    assert side.snap[0]["index"] == index and side.snap[0]["term"] == sterm
    side.step(_msg(abi.HEARTBEAT, leader_slot, term, commit=index))
    st, out, res, _ = side.step(_msg(abi.REPLICATE, leader_slot, term, log_index=index, log_term=sterm,
                                     commit=index, ents=1, ent_term=term))
    assert int(st[0]["last_index"]) == index + 1 and int(res[0]["append_from"]) == index + 1
    assert int(res[0]["save_from"]) == index + 1
    assert len(out) == 1 and int(out[0]["log_index"]) == index + 1 and not out[0]["reject"]


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_receiver_not_restored(be, S, request):
    """Index <= committed: ignored, the ack carries committed. matchTerm hit:
    commitTo(Index), the ack carries the new committed. Neither restores."""
    _need(be, request)
    side = C.Side(be, _follower(S), S)
    st, out, _, rest = side.step(_install(0, 5, 7, 5))
    assert len(rest) == 0 and int(st[0]["committed"]) == 8 and int(st[0]["election_tick"]) == 0
    assert len(out) == 1 and out[0]["type"] == abi.REPLICATE_RESP and int(out[0]["log_index"]) == 8
    st, out, _, rest = side.step(_install(0, 5, 9, 5))
    assert len(rest) == 0 and int(st[0]["committed"]) == 9 and int(st[0]["last_index"]) == 10
    assert int(out[0]["log_index"]) == 9 and side.snap[0]["index"] == 0
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
def test_receiver_term_window(be, request):
    """matchTerm's lookup falls below the device's term-run window (index 7, the
    window starts at 9): GR_ESC_TERM_WINDOW, nothing applied."""
    _need(be, request)
    p = _follower(3, committed=5)
    _window(p, [(9, 5)])
    side = C.Side(be, p, 3)
    before = side.state.copy()
    st, out, res, rest = side.step(_install(0, 5, 7, 5), esc={0: "term_window"})
    assert int(res[0]["esc_item"]) == 0 and len(out) == 0 and len(rest) == 0
    assert st.tobytes() == before.tobytes()
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_restore_onto_shorter_log(be, S, request):
    _need(be, request)
    side = C.Side(be, _follower(S), S)
    st, out, res, rest = side.step(_install(0, 5, 20, 5))
    assert C._rest_key(rest) == [(0, 20, 5)]
    assert len(out) == 1 and out[0]["type"] == abi.REPLICATE_RESP and int(out[0]["log_index"]) == 20
    assert int(res[0]["committed"]) == 20 and int(res[0]["last_index"]) == 20 and int(res[0]["save_from"]) == 0
    assert int(res[0]["append_from"]) == 0 and int(st[0]["applied"]) == 8  # raft.applied is the RSM's to move
    _after_restore(side, 20, 5, 5)
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_restore_onto_longer_log_with_term_mismatch(be, S, request):
    """Three runs (terms 3, 4, 5 over 1..12), committed 6; the snapshot (10, 6)
    disagrees with the local term 5 at 10: the log becomes the single run (10, 6)."""
    _need(be, request)
    ents = [(i, 3) for i in range(1, 5)] + [(i, 4) for i in range(5, 9)] + [(i, 5) for i in range(9, 13)]
    p = _follower(S, ents=ents, committed=6, term=6)
    _window(p, [(1, 3), (5, 4), (9, 5)])
    side = C.Side(be, p, S)
    _, out, _, rest = side.step(_install(0, 6, 10, 6))
    assert C._rest_key(rest) == [(0, 10, 6)] and int(out[0]["log_index"]) == 10
    _after_restore(side, 10, 6, 6)
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_reject_is_the_observer_list(be, S, request):
    """reject = 1: the receiver is in Snapshot.Membership.Observers. A voter
    panics ("converting to observer"); an observer restores."""
    _need(be, request)
    side = C.Side(be, _follower(S), S)
    before = side.state.copy()
    st, out, res, rest = side.step(_install(0, 5, 20, 5, reject=1), esc={0: "panic"})
    assert len(out) == 0 and len(rest) == 0 and st.tobytes() == before.tobytes() and side.snap[0]["index"] == 0
    side.close()
    p = _follower(S, state=abi.OBSERVER, self_id=3)
    _member(p, 2, 3, OBS, match=10)
    side = C.Side(be, p, S)
    _, out, _, rest = side.step(_install(0, 5, 20, 5, reject=1))
    assert C._rest_key(rest) == [(0, 20, 5)] and int(out[0]["log_index"]) == 20
    _after_restore(side, 20, 5, 5)
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_term_rules(be, S, request):
    """Lane::handle's term rules apply unchanged: a higher-term snapshot makes a
    follower and a leader step down with the pass's draw and then restore; a
    lower-term one is dropped; a leader at the same term ignores it."""
    _need(be, request)
    for p in (_follower(S), _leader(S, 11)):
        src = 1 if p[0]["state"] == abi.LEADER else 0
        side = C.Side(be, p, S, _snap(6, 5))
        st, out, res, rest = side.step(_install(src, 7, 20, 6), loc=_loc(rand=12345))
        g = st[0]
        assert g["state"] == abi.FOLLOWER and int(g["term"]) == 7 and int(g["leader_id"]) == src + 1
        assert int(g["randomized_election_timeout"]) == 10 + 12345 % 10 and int(res[0]["term"]) == 7
        assert C._rest_key(rest) == [(0, 20, 6)] and int(out[0]["log_index"]) == 20 and int(out[0]["term"]) == 7
        _after_restore(side, 20, 6, 7, leader_slot=src)
        side.close()
    side = C.Side(be, _follower(S), S)
    before = side.state.copy()
    st, out, _, rest = side.step(_install(0, 4, 20, 4))
    assert len(out) == 0 and len(rest) == 0 and st.tobytes() == before.tobytes()
    side.close()
    side = C.Side(be, _leader(S, 11), S, _snap(6, 5))
    before = side.state.copy()
    st, out, _, rest = side.step(_install(1, 5, 20, 5))
    assert len(out) == 0 and len(rest) == 0 and st.tobytes() == before.tobytes()
    side.close()


def _candidate(S):
    p = _group(S, 2, abi.CANDIDATE, [0, 10, 0], leader_id=0)
    p[0]["vote"] = 2  # its own granted bit comes with the load (gpuraft.h votes_granted)
    return p


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_candidate(be, S, request):
    """With elections on too: becomeFollower(term, From) with the pass's draw,
    then the follower's handler. With elections off the candidate escalates
    GR_ESC_UNSUPPORTED as it always did."""
    _need(be, request)
    side = C.Side(be, _candidate(S), S, elect=True)
    st, out, _, rest = side.step(_install(0, 5, 20, 5), loc=_loc(rand=4321))
    g = st[0]
    assert g["state"] == abi.FOLLOWER and int(g["leader_id"]) == 1 and int(g["vote"]) == 2
    assert int(g["randomized_election_timeout"]) == 10 + 4321 % 10
    assert C._rest_key(rest) == [(0, 20, 5)] and int(out[0]["log_index"]) == 20
    _after_restore(side, 20, 5, 5)
    side.close()
    side = C.Side(be, _candidate(S), S)
    before = side.state.copy()
    st, out, _, rest = side.step(_install(0, 5, 20, 5), loc=_loc(rand=4321), esc={0: "unsupported"})
    assert len(out) == 0 and len(rest) == 0 and st.tobytes() == before.tobytes()
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_items_after_a_restore_in_the_same_pass(be, S, request):
    """A Replicate with one entry at LogIndex = Index behind the snapshot in the
    same mailbox appends to the restored log (append_from, a window push at the
    new term); two snapshots with rising indexes leave two list records and a
    third is GR_ESC_CAPACITY (a lane stages two restores per pass)."""
    _need(be, request)
    p = _follower(S, term=6)
    side = C.Side(be, p, S)
    msgs = np.concatenate([_install(0, 6, 20, 5),
                           _msg(abi.REPLICATE, 0, 6, log_index=20, log_term=5, commit=20, ents=1, ent_term=6)])
    st, out, res, rest = side.step(msgs)
    g = st[0]
    assert C._rest_key(rest) == [(0, 20, 5)] and [int(m["log_index"]) for m in out] == [20, 21]
    assert int(res[0]["append_from"]) == 21 and int(res[0]["save_from"]) == 21 and int(g["last_index"]) == 21
    assert int(g["n_runs"]) == 2 and (int(g["run_start"][1]), int(g["run_term"][1])) == (21, 6)
    side.close()
    side = C.Side(be, _follower(S), S)
    st, out, _, rest = side.step(np.concatenate([_install(0, 5, 20, 5), _install(0, 5, 30, 5)]))
    assert C._rest_key(rest) == [(0, 20, 5), (0, 30, 5)] and [int(m["log_index"]) for m in out] == [20, 30]
    _after_restore(side, 30, 5, 5)
    side.close()
    side = C.Side(be, _follower(S), S)
    three = np.concatenate([_install(0, 5, 20, 5), _install(0, 5, 30, 5), _install(0, 5, 40, 5)])
    st, out, res, rest = side.step(three, esc={0: "capacity"})
    assert int(res[0]["esc_item"]) == 2 and C._rest_key(rest) == [(0, 20, 5), (0, 30, 5)]
    assert int(st[0]["last_index"]) == 30 and side.snap[0]["index"] == 30
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_escalation_leaves_no_trace(be, S, request):
    """The snapshot record and the list belong to the run that stands. Node 3
    (slot 2) leads; node 1 sends six ReadIndex requests, which the follower
    forwards to the leader and which fill that mailbox. The snapshot behind them
    restores in the first attempt and its ack then finds no place:
    GR_ESC_CAPACITY at item 6. The prefix that stands holds no restore: no list
    record, the snapshot record untouched, the log as it was.
    The other way round, a restore at item 0 and an escalation at item 1 (a
    RequestVote with elections off): the restore stands and is listed once."""
    _need(be, request)
    p = _follower(S)
    p[0]["leader_id"] = 3
    side = C.Side(be, p, S, _snap(4, 5))
    reads = np.concatenate([_msg(abi.READ_INDEX, 0, 0, hint=100 + k) for k in range(6)])
    st, out, res, rest = side.step(np.concatenate([reads, _install(2, 5, 20, 5)]), esc={0: "capacity"})
    assert int(res[0]["esc_item"]) == 6 and len(rest) == 0 and len(out) == 6
    assert (int(side.snap[0]["index"]), int(side.snap[0]["term"])) == (4, 5)
    assert int(st[0]["last_index"]) == 10 and int(st[0]["committed"]) == 8 and int(st[0]["first_index_m1"]) == 0
    assert side.restored == []
    side.close()
    side = C.Side(be, _follower(S), S)
    msgs = np.concatenate([_install(0, 5, 20, 5), _msg(abi.REQUEST_VOTE, 2, 5, log_index=20, log_term=5)])
    st, out, res, rest = side.step(msgs, esc={0: "unsupported"})
    assert int(res[0]["esc_item"]) == 1 and C._rest_key(rest) == [(0, 20, 5)] and side.snap[0]["index"] == 20
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_nonmember_sender(be, S, request):
    """An InstallSnapshot from a slot that holds no member keeps escalating."""
    _need(be, request)
    p = _follower(S)
    _member(p, 2, 3, EMPTY)
    side = C.Side(be, p, S)
    side.step(_install(2, 5, 20, 5), esc={0: "unsupported"})
    side.close()


# ---------------------------------------------------------------- the switch
@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_switch_off(be, S, request):
    """Off (the default): the leader escalates GR_ESC_SNAPSHOT and every receiver
    GR_ESC_UNSUPPORTED, with nothing of the item applied."""
    _need(be, request)
    side = C.Side(be, _leader(S, 6), S, _snap(6, 5), on=False)
    _, out, res, _ = side.step(loc=_loc(propose=1), esc={0: "snapshot"})
    assert int(res[0]["esc_item"]) == 0 and len(out) == 0
    side.close()
    obs = _follower(S, state=abi.OBSERVER, self_id=3)
    _member(obs, 2, 3, OBS, match=10)
    for p in (_follower(S), obs, _candidate(S)):
        side = C.Side(be, p, S, on=False)
        before = side.state.copy()
        st, out, _, _ = side.step(_install(0, 5, 20, 5), loc=_loc(), esc={0: "unsupported"})
        assert len(out) == 0 and st.tobytes() == before.tobytes()
        side.close()


@pytest.mark.gpu
def test_switch_and_records_api(gpu, monkeypatch):
    """gr_set_snapshots / gr_get_snapshots, GR_SNAPSHOTS=1 at gr_create, the
    snapshot records' slot rules, and loads and syncs leaving the records alone."""
    from dragonboat_amd.engine import Engine, GpuRaftError
    eng = Engine(8, 3)
    try:
        assert not eng.get_snapshots()
        eng.set_snapshots(True)
        assert eng.get_snapshots()
        eng.set_snapshots(False)
        assert not eng.get_snapshots()
        assert not eng.get_snapshot_recs(np.arange(8)).view(np.uint64).any()  # zeroed
        recs = np.zeros(3, abi.SNAPSHOT_REC)
        recs["index"], recs["term"] = [5, 6, 7], [1, 2, 3]
        eng.set_snapshot_recs([6, 0, 3], recs)
        assert eng.get_snapshot_recs([3, 6, 0, 1]).tolist() == [(7, 3), (5, 1), (6, 2), (0, 0)]
        for bad in ([0, 8], [1, 1]):
            with pytest.raises(GpuRaftError):
                eng.set_snapshot_recs(bad, recs[:2])
            with pytest.raises(GpuRaftError):
                eng.get_snapshot_recs(bad)
        eng.load(P.make_groups(2, 3, seed=1))
        eng.sync(6)
        assert eng.get_snapshot_recs([3, 6, 0, 1]).tolist() == [(7, 3), (5, 1), (6, 2), (0, 0)]
        assert len(eng.restored_snapshots()) == 0
    finally:
        eng.close()
    monkeypatch.setenv("GR_SNAPSHOTS", "1")
    eng = Engine(8, 3)
    try:
        assert eng.get_snapshots()
    finally:
        eng.close()


# ---------------------------------------------------------------- gr_restore_remotes
def _rr(be, p, S, members, want, rand=0):
    side = C.Side(be, p, S)
    st = side.restore([0], C.membership(members, rand))
    assert int(st[0]) == want, (int(st[0]), want)
    return side


def _fresh(g, j, match, kind=VOTER):
    r = g["remotes"][j]
    return [int(r[f]) for f in ("kind", "match", "next", "state", "active", "snapshot_index")] == \
        [kind, match, int(g["last_index"]) + 1, abi.RETRY, 0, 0]


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_restore_remotes_membership(be, S, request):
    """The same membership: every remote fresh (match 0, or lastIndex for the peer
    itself; next lastIndex + 1; Retry, inactive). One id dropped: its slot empties
    and keeps the id. One new id: the free slot (S = 5), or no slot (S = 3)."""
    _need(be, request)
    lead = _group(S, 1, abi.LEADER, [10, 8, 8])
    lead[0]["remotes"][2]["state"], lead[0]["remotes"][2]["snapshot_index"] = abi.SNAPSHOT_ST, 9
    side = _rr(be, lead, S, [(1, VOTER), (2, VOTER), (3, VOTER)], APPLIED)
    g = side.state[0]
    assert g["state"] == abi.LEADER and all(_fresh(g, j, m) for j, m in [(0, 10), (1, 0), (2, 0)])
    side.step(loc=_loc(propose=1))  # the leader's next pass sends from lastIndex + 1
    side.close()
    side = _rr(be, _group(S, 2, abi.FOLLOWER, [0, 10, 0]), S, [(2, VOTER), (1, VOTER)], APPLIED)
    g = side.state[0]
    assert g["remotes"][2]["kind"] == EMPTY and g["remote_id"][2] == 3 and g["self_slot"] == 1
    assert [int(g["remotes"][2][f]) for f in ("match", "next", "state", "active")] == [0] * 4
    assert _fresh(g, 0, 0) and _fresh(g, 1, 10)
    side.close()
    side = _rr(be, _group(S, 2, abi.FOLLOWER, [0, 10, 0]), S, [(1, VOTER), (2, VOTER), (3, VOTER), (9, OBS)],
               APPLIED if S == 5 else NO_SLOT)
    if S == 5:
        g = side.state[0]
        assert g["remote_id"][3] == 9 and _fresh(g, 3, 0, OBS)
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_restore_remotes_readd_gets_its_old_slot(be, S, request):
    """Slots: node 1, an empty slot, and an empty slot that still carries id 3.
    Node 3 comes back to its old slot, not the lower empty one, which a new id
    takes; self removed by the membership ends with no slot of its own."""
    _need(be, request)
    p = _group(S, 1, abi.FOLLOWER, [10, 0, 0], leader_id=2)
    _member(p, 1, 0, EMPTY)
    _member(p, 2, 3, EMPTY)
    side = _rr(be, p, S, [(1, VOTER), (3, VOTER)], APPLIED)
    g = side.state[0]
    assert g["remotes"][1]["kind"] == EMPTY and g["remote_id"][2] == 3 and _fresh(g, 2, 0)
    assert int(side.restore([0], C.membership([(1, VOTER), (3, VOTER), (8, VOTER)]))[0]) == APPLIED
    assert side.state[0]["remote_id"][1] == 8 and _fresh(side.state[0], 1, 0)
    assert int(side.restore([0], C.membership([(3, VOTER), (8, VOTER)]))[0]) == APPLIED
    assert side.state[0]["self_slot"] == abi.GR_SLOT_NONE and side.state[0]["remote_id"][0] == 1
    side.close()


def _observer_peer(S, other_obs=False):
    """Node 3 as an observer of voters 1, 2 (and, other_obs, observer 4 in slot 3)."""
    p = _group(S, 3, abi.OBSERVER, [4, 6], committed=10)
    _member(p, 2, 3, OBS, match=9, next_=3, state=abi.WAIT, active=1)
    if other_obs:
        _member(p, 3, 4, OBS, match=2)
    g = p[0]
    g["vote"], g["election_tick"], g["heartbeat_tick"] = 2, 4, 1
    g["flags"] |= abi.F_PENDING_CONFIG_CHANGE
    return p


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_restore_remotes_promotion(be, S, request):
    """A listed voter that this peer holds as an observer: becomeFollower(term,
    leaderID) with `rand` as the draw, whichever id it is (raft.go:329-333): the
    peer itself, or another node on a leader, which steps down. Two such ids need
    two draws: GR_CC_HOST. So does a candidate, whatever the list."""
    _need(be, request)
    side = _rr(be, _observer_peer(S), S, [(1, VOTER), (2, VOTER), (3, VOTER)], APPLIED, rand=12345)
    g = side.state[0]
    assert g["state"] == abi.FOLLOWER and g["self_slot"] == 2 and int(g["leader_id"]) == 1 and int(g["vote"]) == 2
    assert int(g["randomized_election_timeout"]) == 10 + 12345 % 10
    assert int(g["election_tick"]) == 0 and int(g["heartbeat_tick"]) == 0
    assert not g["flags"] & abi.F_PENDING_CONFIG_CHANGE
    assert all(_fresh(g, j, m) for j, m in [(0, 0), (1, 0), (2, 10)])
    side.step(loc=_loc(ticks=3))  # a follower now: its election clock runs
    side.close()
    lead = _group(S, 1, abi.LEADER, [10, 10], committed=10)
    _member(lead, 2, 3, OBS, match=7, next_=8, state=abi.REPLICATE_ST, active=1)
    side = _rr(be, lead, S, [(1, VOTER), (2, VOTER), (3, VOTER)], APPLIED, rand=99)
    g = side.state[0]
    assert g["state"] == abi.FOLLOWER and int(g["leader_id"]) == 1
    assert int(g["randomized_election_timeout"]) == 10 + 99 % 10 and _fresh(g, 2, 0)
    side.close()
    if S == 5:
        side = _rr(be, _observer_peer(S, other_obs=True), S, [(1, VOTER), (2, VOTER), (3, VOTER), (4, VOTER)], HOST)
        side.close()
    cand = _group(S, 1, abi.CANDIDATE, [10, 0, 0], leader_id=0)
    cand[0]["vote"] = 1
    side = _rr(be, cand, S, [(1, VOTER), (2, VOTER), (3, VOTER)], HOST)
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
def test_restore_remotes_ack_bit_restriction(be, request):
    """A leader holds a ReadIndex request that node 3 (slot 2) confirmed; the
    membership drops node 3 and brings node 9. The bit stays node 3's: node 9
    takes slot 3 (S = 5), or finds no slot (S = 3)."""
    _need(be, request)
    for S, want in [(5, APPLIED), (3, NO_SLOT)]:
        p = _group(S, 1, abi.LEADER, [10, 10, 10], committed=10)
        g = p[0]
        g["read_index_count"] = 1
        rs = g["read_index"][0]
        rs["index"], rs["ctx_low"], rs["from_slot"], rs["ack_bits"] = 10, 7, abi.GR_SLOT_NONE, 1 << 2
        side = _rr(be, p, S, [(1, VOTER), (2, VOTER), (9, VOTER)], want)
        if want == APPLIED:
            g = side.state[0]
            assert g["remote_id"][3] == 9 and g["remotes"][2]["kind"] == EMPTY
            assert int(g["read_index"][0]["ack_bits"]) == 1 << 2
        side.close()


@pytest.mark.parametrize("be", BACKENDS)
def test_restore_remotes_refusals_write_nothing(be, request):
    """Refused peers are bit-identical (Side.restore checks every status-1 and
    status-2 peer), and so is every peer of a call refused as a whole: a slot
    out of range or listed twice, a kind that is no gr_slot_kind."""
    _need(be, request)
    peers = np.concatenate([_group(3, 1, abi.LEADER, [10, 8, 8]), _group(3, 1, abi.CANDIDATE, [10, 0, 0], leader_id=0),
                            _group(3, 2, abi.FOLLOWER, [0, 10, 0]), _group(3, 3, abi.FOLLOWER, [0, 0, 10])])
    side = C.Side(be, peers, 3)
    same = C.membership([(1, VOTER), (2, VOTER), (3, VOTER)])
    four = C.membership([(1, VOTER), (2, VOTER), (3, VOTER), (4, VOTER)])
    st = side.restore([3, 1, 2, 0], np.concatenate([same, same, four, same]))
    assert list(st) == [APPLIED, HOST, NO_SLOT, APPLIED]
    bad_kind = np.concatenate([same, same])
    bad_kind[1]["kind"][1] = 3
    for idx, ms, err in [([0, 4], np.concatenate([same, same]), -4), ([2, 2], np.concatenate([same, same]), -4),
                         ([0, 1], bad_kind, -1)]:
        rc, _, new = side.restore_raw(np.asarray(idx, np.uint32), ms)
        assert rc == err, (idx, rc)
        assert new.tobytes() == side.state.tobytes()
    side.close()


@pytest.mark.gpu
def test_restore_remotes_refused_while_a_pass_is_pending(gpu):
    """Between gr_step_compact_begin and _end the call is refused exactly as
    gr_apply_config_change is: GR_ESTATE, no status written, no peer changed."""
    import ctypes
    from dragonboat_amd.engine import Engine, GpuRaftError
    G = 64
    eng = Engine(G * 3, 3)
    try:
        eng.load(P.make_groups(G, 3, seed=1))
        sl = np.arange(4, dtype=np.uint32)
        ms = np.concatenate([C.membership([(1, VOTER), (2, VOTER)])] * 4)
        cm, xm = eng.pack_messages(np.zeros(0, abi.MESSAGE))
        cl, xl = eng.pack_locals(P.propose_locals(G * 3, np.arange(G), pass_index=0))
        ib, ob = abi.cinbox_of(cm, xm, cl, xl), abi.COutbox()
        assert eng.lib.gr_step_compact_begin(eng._h, ctypes.byref(ib)) == 0
        st = np.full(4, -1, np.int32)
        assert eng.lib.gr_restore_remotes(eng._h, sl.ctypes.data, ms.ctypes.data, 4, st.ctypes.data) == -6
        assert np.all(st == -1)
        with pytest.raises(GpuRaftError):
            eng.restore_remotes(sl, ms)
        assert eng.lib.gr_step_compact_end(eng._h, ctypes.byref(ob)) == 0
        assert eng.lib.gr_release_coutbox(eng._h, ctypes.byref(ob)) == 0
        assert np.all(eng.sync_peers(sl)["remotes"]["kind"][:, 2] == VOTER)  # nobody was dropped
        rc, st = eng.restore_remotes(sl, ms)  # after _end the call is taken
        assert rc == 0 and list(st) == [APPLIED] * 4
        assert np.all(eng.sync_peers(sl)["remotes"]["kind"][:, 2] == EMPTY)
    finally:
        eng.close()


# ---------------------------------------------------------------- a live population
# Chosen on the host lane: the groups with an active remote restore in pass 1, the others in
# pass 3 (a heartbeat ack activates the remote first), and by pass 7 every laggard follows
# its leader at the steady state's distance; five more passes show it stays there.
PASSES = 12


def _live(be, monkeypatch, split):
    """200 groups x 3 through gr_step. Replica 2 of every group lags below its
    leader's firstIndex - 1; its remote is active in 150 groups and inactive in
    50, where a heartbeat ack activates it first. Proposals every pass, a
    heartbeat tick every pass: InstallSnapshot -> restore and ack -> Replicates
    resume. The restored list is drained every pass and gr_restore_remotes called
    on the restored peers. Every pass is compared with the reference-driven run.
    "Caught up" is the steady state's own distance: a follower learns its leader's
    commit index from the next pass's Replicate, so with one proposal per pass it
    ends every pass exactly one entry behind, as replica 1, which never lagged, does."""
    if split:
        monkeypatch.setenv("GR_SPLIT_MIN_LANES", "1")  # read at gr_create
        monkeypatch.setenv("GR_SMALL_BLOCKS", "0")     # the split schedule, not the fused small kernel
    G, R, S = 200, 3, 3
    n = R * G
    topo = P.Topology(G, R)
    peers = P.make_groups(G, R, seed=31, term_lo=2, term_hi=5)
    lead, lag = peers[:G], peers[2 * G:]
    hi = lead["last_index"].copy()
    cut = hi - np.uint64(16)  # the leaders compacted up to here and took their snapshot there
    for v in (peers[:G], peers[G:2 * G]):
        v["first_index_m1"] = cut
        v["run_start"][:, 0] = cut
    old = cut - np.uint64(40)  # where the laggards stopped
    for f in ("committed", "applied", "last_index"):
        lag[f] = old
    lag["n_runs"] = 1
    lag["run_start"][:, 1], lag["run_term"][:, 1] = 0, 0
    lag["remotes"]["match"][:, 2] = old
    lag["remotes"]["next"][:, :3] = (old + np.uint64(1))[:, None]
    r2 = lead["remotes"][:, 2]
    r2["match"], r2["next"], r2["state"] = old, old + np.uint64(1), abi.RETRY
    r2["active"] = np.where(np.arange(G) < 150, 1, 0)
    lead["remotes"][:, 2] = r2
    snap = np.zeros(n, abi.SNAPSHOT_REC)
    snap["index"][:2 * G] = np.tile(cut, 2)
    snap["term"][:2 * G] = np.tile(lead["run_term"][:, 0], 2)
    side = C.Side(be, peers, S, snap)
    same = np.concatenate([C.membership([(1, VOTER), (2, VOTER), (3, VOTER)])] * n)
    msgs = np.zeros(0, abi.MESSAGE)
    try:
        committed = []
        for k in range(PASSES):
            loc = P.propose_locals(n, np.arange(G), pass_index=k)
            loc["ticks"][:G] = 1  # heartbeat_timeout 1: a heartbeat broadcast every pass
            st, out, res, rest = side.step(msgs, loc)  # no escalation of any kind, or Side.step fails
            msgs = topo.route_messages(out)
            if len(rest):  # the host: the RSM recovers, then RestoreRemotes on those peers
                who = np.unique(rest["peer"]).astype(np.uint32)
                rst = side.restore(who, same[:len(who)])
                assert not rst.any()
            committed.append(st["committed"].copy())
        assert sorted(p for p, _, _ in side.restored) == list(range(2 * G, 3 * G))  # exactly the 200 laggards, once each
        got = {p: (i, t) for p, i, t in side.restored}
        assert all(got[2 * G + g] == (int(cut[g]), int(lead["run_term"][g, 0])) for g in range(G))
        last = committed[-1]
        assert np.all(last[2 * G:] == last[G:2 * G]) and np.all(last[2 * G:] + np.uint64(1) == last[:G])  # caught up
        assert np.all(committed[-1] > committed[-3])  # and still advancing, every replica
    finally:
        side.close()


def test_live_population_host(built, monkeypatch):
    _live("cpu", monkeypatch, False)


@pytest.mark.gpu
@pytest.mark.parametrize("split", [False, True], ids=["fused", "split"])
def test_live_population_gpu(gpu, monkeypatch, split):
    _live("gpu", monkeypatch, split)

"""Every device switch on at once: elections, snapshots (gr_set_snapshots) and
config-change entries (gr_set_config_entries), the configuration a deployment
runs. test_snapshots.py and test_config_entries.py each turn on one of the two
side arrays; here a restore meets a live gr_cc_index record, a promotion follows
a restore, and a leader sends an InstallSnapshot and a marked Replicate in one
broadcast.

Every case runs on two backends, the host lane built with the three switches
compiled on (`not gpu`) and the engine with them set (`-m gpu`), beside one
reference side: the oracle's raft object built from the same records, with typed
in-memory entries and both message conventions (all_switches_common.py,
tests/native/all_switches_ref.cpp). After every pass the peer records, the
snapshot records, the gr_cc_index records, the messages, the results and the
restored list must agree; an escalation must be the one the case names and leave
exactly the items below it applied.
"""
import numpy as np
import pytest

from dragonboat_amd import abi
import all_switches_common as C
import config_change_common as CC
import config_entries_common as CE
from test_config_change import _group, _member
from test_snapshots import _install, _snap, _window

BACKENDS = [pytest.param("cpu", id="host"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
VOTER = abi.SLOT_VOTER
REQUEST_VOTE_RESP = 15
SAME = [(1, VOTER), (2, VOTER), (3, VOTER)]


@pytest.fixture(autouse=True)
def _no_env_switch(monkeypatch):
    for v in ("GR_SNAPSHOTS", "GR_CONFIG_ENTRIES", "GR_ELECTIONS"):
        monkeypatch.delenv(v, raising=False)


def _need(be, request):
    request.getfixturevalue("gpu" if be == "gpu" else "built")


def _in_memory(p):
    """Every uncommitted entry in memory, everything saved (the typed
    reference's precondition: marker_index = committed + 1)."""
    g = p[0]
    g["marker_index"], g["saved_to"], g["log_applied"] = int(g["committed"]) + 1, g["last_index"], g["committed"]
    return p


def _loc(propose=0, cc=0, ticks=0, rand=77):
    loc = np.zeros(1, abi.LOCAL)
    loc["propose_entries"], loc["propose_has_config_change"], loc["ticks"], loc["rand"] = propose, cc, ticks, rand
    return loc


def _msg(type_, slot, term, log_index=0, log_term=0, commit=0, reject=0, ents=0, ent_term=0, hint=0, hint_high=0):
    m = np.zeros(1, abi.MESSAGE)
    m["type"], m["slot"], m["term"], m["log_index"], m["log_term"] = type_, slot, term, log_index, log_term
    m["commit"], m["reject"], m["hint"], m["hint_high"] = commit, reject, hint, hint_high
    if ents:
        m["n_entries"], m["n_runs"] = ents, 1
        m["run_term"][0, 0] = ent_term
    return m


def _rec(cc):
    return int(cc[0]["last"]), int(cc[0]["prev"])


def _live(side):
    """The record as it counts: values at or below committed are 0."""
    return _rec(C.norm_cc(side.cc, side.state["committed"]))


def _marks(out, slot):
    m = out[(out["slot"] == slot) & (out["type"] == abi.REPLICATE)]
    return [(int(x["reject"]), int(x["hint"]), int(x["hint_high"]), int(x["log_index"]), int(x["n_entries"])) for x in m]


def _follower(S, ents=None, committed=8, term=5, state=abi.FOLLOWER, self_id=2, leader_id=1):
    """Node self_id of voters 1..3 over the log 1..10 at term 5 (or `ents`)."""
    ents = ents or [(i, 5) for i in range(1, 11)]
    last = ents[-1][0]
    p = _group(S, self_id, state, [last if j + 1 == self_id else 0 for j in range(3)], committed=committed, term=term,
               ents=ents, leader_id=leader_id)
    return _in_memory(p)


def _long_follower(S):
    """test_restore_onto_longer_log_with_term_mismatch's peer: runs (1,3) (5,4)
    (9,5) over 1..12, committed 6, term 6."""
    ents = [(i, 3) for i in range(1, 5)] + [(i, 4) for i in range(5, 9)] + [(i, 5) for i in range(9, 13)]
    p = _follower(S, ents=ents, committed=6, term=6)
    _window(p, [(1, 3), (5, 4), (9, 5)])
    return p


def _restored(side, index, sterm):
    g = side.state[0]
    assert [int(g[f]) for f in ("last_index", "committed", "first_index_m1", "saved_to", "marker_index",
                                "log_applied")] == [index, index, index, index, index + 1, index]
    assert int(g["n_runs"]) == 1 and (int(g["run_start"][0]), int(g["run_term"][0])) == (index, sterm)
    assert side.snap[0]["index"] == index and side.snap[0]["term"] == sterm


def _two_passes(side, index, lterm, term, leader_slot=0, ents=1, commit=None):
    """Two ordinary passes under the reference: a heartbeat, then an unmarked
    Replicate of `ents` entries of `term` after (index, lterm), both with
    `commit` (default: index)."""
    commit = index if commit is None else commit
    side.step(_msg(abi.HEARTBEAT, leader_slot, term, commit=commit))
    st, out, res, _, _ = side.step(_msg(abi.REPLICATE, leader_slot, term, log_index=index, log_term=lterm,
                                        commit=commit, ents=ents, ent_term=term))
    assert int(st[0]["last_index"]) == index + ents and int(res[0]["append_from"]) == index + 1
    assert len(out) == 1 and int(out[0]["log_index"]) == index + ents and not out[0]["reject"]


def _campaigning(side, term, **kw):
    """The peer made a candidate at `term` with its own vote, on a fresh Side
    with the records as they stand."""
    p = side.state.copy()
    g = p[0]
    g["state"], g["term"], g["vote"], g["leader_id"], g["election_tick"] = abi.CANDIDATE, term, g["node_id"], 0, 0
    new = C.Side(side.be, p, side.S, side.snap, side.cc, **kw)
    side.close()
    return new


def _win(side, term, slot=0, **kw):
    return side.step(_msg(REQUEST_VOTE_RESP, slot, term), _loc(), **kw)


# ---------------------------------------------------------------- restore, then promotion
def scn_restore_then_promotion(be, S, cc, **kw):
    """The restore discards entries 11..12 and commits 10: whatever the record
    named, the log holds no config change above committed. The reference's
    getPendingConfigChangeCount over (10, 12] at the later promotion finds none."""
    side = C.Side(be, _long_follower(S), S, cc=C.cc_recs(1, *cc), **kw)
    _, out, _, rest, rec = side.step(_install(0, 6, 10, 6))
    assert C._rest_key(rest) == [(0, 10, 6)] and int(out[0]["log_index"]) == 10
    _restored(side, 10, 6)
    if side.config_entries:
        assert _live(side) == (0, 0)
    else:  # the switch off: the restore must not look at the array, let alone write it
        assert _rec(rec) == cc
    _two_passes(side, 10, 6, 6, ents=2)
    assert int(side.state[0]["last_index"]) == 12 and int(side.state[0]["committed"]) == 10
    if not side.config_entries:
        assert _rec(side.cc) == cc
        if be == "gpu":
            assert side.eng.get_cc_indexes(side.all).tobytes() == C.cc_recs(1, *cc).tobytes()
    return side


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
@pytest.mark.parametrize("cc", [(11, 0), (11, 8), (9, 8)], ids=["last_above", "last_above_prev_live", "both_below"])
def test_restore_onto_longer_log_then_promotion(be, S, cc, request):
    """A record with last > idx, with last > idx >= prev > committed, and with
    both in (committed, idx]: after the restore it normalises to (0, 0). The peer
    then takes two unmarked entries, campaigns at term 7 and wins: leader with
    the flag clear, and a config change proposed to it is appended and sets the
    flag. Before the restore moved the record, the first two variants failed
    here: the record (11, 0) outlived the restore and the new leader held
    GR_F_PENDING_CONFIG_CHANGE with no config change in its log."""
    _need(be, request)
    side = _campaigning(scn_restore_then_promotion(be, S, cc), 7)
    st, _, _, _, _ = _win(side, 7)
    g = st[0]
    assert g["state"] == abi.LEADER and int(g["last_index"]) == 13 and not int(g["flags"]) & C.PENDING
    assert _live(side) == (0, 0)
    st, out, res, _, cc2 = side.step(loc=_loc(propose=1, cc=1))
    assert int(res[0]["propose_result"]) == abi.PROP_APPENDED and int(res[0]["propose_first"]) == 14
    assert int(st[0]["flags"]) & C.PENDING and _rec(cc2) == (14, 0)
    side.close()


# ---------------------------------------------------------------- matchTerm hit
@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
@pytest.mark.parametrize("last", [9, 10], ids=["last_committed", "last_above"])
def test_match_term_commit_keeps_the_record(be, S, last, request):
    """Snapshot (9, 5) on the log 1..10 at term 5: matchTerm, commitTo(9), no
    restore, the entries survive. A later promotion sets the flag exactly when
    the recorded config change lies above 9."""
    _need(be, request)
    side = C.Side(be, _follower(S), S, cc=C.cc_recs(1, last))
    st, out, _, rest, _ = side.step(_install(0, 5, 9, 5))
    assert len(rest) == 0 and int(st[0]["committed"]) == 9 and int(st[0]["last_index"]) == 10
    assert int(out[0]["log_index"]) == 9 and side.snap[0]["index"] == 0
    assert _live(side) == ((10, 0) if last == 10 else (0, 0))
    _two_passes(side, 10, 5, 5, commit=9)
    side = _campaigning(side, 6)
    st, _, _, _, _ = _win(side, 6)
    assert st[0]["state"] == abi.LEADER and bool(int(st[0]["flags"]) & C.PENDING) == (last == 10)
    side.close()


# ---------------------------------------------------------------- shorter log
@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_restore_onto_shorter_log_with_live_record(be, S, request):
    """idx 20 > lastIndex 10 with the record (10, 0) live: committed passes it,
    so it is stale afterwards; the rest is test_restore_onto_shorter_log."""
    _need(be, request)
    side = C.Side(be, _follower(S), S, cc=C.cc_recs(1, 10))
    st, out, res, rest, _ = side.step(_install(0, 5, 20, 5))
    assert C._rest_key(rest) == [(0, 20, 5)] and int(out[0]["log_index"]) == 20
    assert int(res[0]["committed"]) == 20 and int(res[0]["save_from"]) == 0 and int(st[0]["applied"]) == 8
    _restored(side, 20, 5)
    assert _live(side) == (0, 0)
    _two_passes(side, 20, 5, 5)
    side.close()


# ---------------------------------------------------------------- candidate
@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_candidate_over_config_change_restores(be, S, request):
    """Lane::handle's GR_CANDIDATE branch for an InstallSnapshot of the
    candidate's own term, which needs snapshots and elections: becomeFollower
    with the pass's draw, then the restore, over uncommitted entries one of which
    is a config change. A later promotion counts 0."""
    _need(be, request)
    p = _follower(S, state=abi.CANDIDATE, leader_id=0)
    p[0]["vote"] = 2
    side = C.Side(be, p, S, cc=C.cc_recs(1, 10))
    st, out, _, rest, _ = side.step(_install(0, 5, 20, 5), loc=_loc(rand=4321))
    g = st[0]
    assert g["state"] == abi.FOLLOWER and int(g["leader_id"]) == 1 and int(g["vote"]) == 2
    assert int(g["randomized_election_timeout"]) == 10 + 4321 % 10
    assert C._rest_key(rest) == [(0, 20, 5)] and int(out[0]["log_index"]) == 20
    _restored(side, 20, 5)
    _two_passes(side, 20, 5, 5)
    side = _campaigning(side, 6)
    st, _, _, _, _ = _win(side, 6)
    assert st[0]["state"] == abi.LEADER and not int(st[0]["flags"]) & C.PENDING and _live(side) == (0, 0)
    side.close()


# ---------------------------------------------------------------- leader steps down
@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_leader_with_flag_steps_down_and_restores(be, S, request):
    """A leader with GR_F_PENDING_CONFIG_CHANGE and the record (10, 0) gets an
    InstallSnapshot of term 7: reset() clears the flag, then the restore."""
    _need(be, request)
    p = _in_memory(_group(S, 1, abi.LEADER, [10, 8, 8]))
    p[0]["flags"] |= C.PENDING
    side = C.Side(be, p, S, cc=C.cc_recs(1, 10))
    st, out, res, rest, _ = side.step(_install(1, 7, 20, 6), loc=_loc(rand=12345))
    g = st[0]
    assert g["state"] == abi.FOLLOWER and int(g["term"]) == 7 and int(g["leader_id"]) == 2
    assert not int(g["flags"]) & C.PENDING and int(g["randomized_election_timeout"]) == 10 + 12345 % 10
    assert C._rest_key(rest) == [(0, 20, 6)] and int(out[0]["log_index"]) == 20 and int(out[0]["term"]) == 7
    _restored(side, 20, 6)
    assert _live(side) == (0, 0)
    _two_passes(side, 20, 6, 7, leader_slot=1)
    side.close()


# ---------------------------------------------------------------- one pass, several items
@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_marked_replicate_restore_marked_replicate_in_one_pass(be, S, request):
    """A marked Replicate (entries 11..12, mark 12), an InstallSnapshot (20, 5)
    that restores, and a marked Replicate on top of the snapshot (entries 21..22,
    both marked) in one mailbox: the staging record is touched before the
    restore, cleared by it and merged after it, one restore is staged, and the
    record afterwards holds the second Replicate's marks alone."""
    _need(be, request)
    side = C.Side(be, _follower(S, term=6), S)
    msgs = np.concatenate([
        _msg(abi.REPLICATE, 0, 6, log_index=10, log_term=5, commit=8, reject=1, ents=2, ent_term=6, hint=12),
        _install(0, 6, 20, 5),
        _msg(abi.REPLICATE, 0, 6, log_index=20, log_term=5, commit=20, reject=1, ents=2, ent_term=6, hint=22,
             hint_high=21)])
    st, out, res, rest, cc = side.step(msgs)
    assert C._rest_key(rest) == [(0, 20, 5)] and [int(m["log_index"]) for m in out] == [12, 20, 22]
    assert int(st[0]["last_index"]) == 22 and int(st[0]["committed"]) == 20 and int(res[0]["append_from"]) == 11
    assert _rec(cc) == (22, 21)
    if be == "cpu":  # the staging record is what was copied back
        assert _rec(side.stage) == (22, 21)
    _two_passes(side, 22, 6, 6, commit=20)
    assert _live(side) == (22, 21)
    side.close()
    # the first Replicate alone leaves (12, 0): the restore above is what dropped it
    side = C.Side(be, _follower(S, term=6), S)
    _, _, _, _, cc = side.step(msgs[:1])
    assert _rec(cc) == (12, 0)
    side.close()


# ---------------------------------------------------------------- escalation after a restore
@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_escalation_after_restore_leaves_no_trace(be, S, request):
    """test_escalation_leaves_no_trace's item with a live record: six forwarded
    ReadIndex requests fill the leader's mailbox, the snapshot behind them
    restores in the first attempt (clearing the staging record) and its ack finds
    no place: GR_ESC_CAPACITY at item 6. The peer record, the snapshot record and
    the gr_cc_index record are bit for bit what they were."""
    _need(be, request)
    p = _follower(S, leader_id=3)
    side = C.Side(be, p, S, _snap(4, 5), C.cc_recs(1, 10, 9))
    before = side.state.copy()
    reads = np.concatenate([_msg(abi.READ_INDEX, 0, 0, hint=100 + k) for k in range(6)])
    st, out, res, rest, cc = side.step(np.concatenate([reads, _install(2, 5, 20, 5)]), esc={0: "capacity"})
    assert int(res[0]["esc_item"]) == 6 and len(rest) == 0 and len(out) == 6 and side.restored == []
    assert st.tobytes() == before.tobytes()
    assert side.snap.tobytes() == _snap(4, 5).tobytes() and cc.tobytes() == C.cc_recs(1, 10, 9).tobytes()
    side.close()


# ---------------------------------------------------------------- leader, one laggard
@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_leader_sends_snapshot_and_marked_replicate(be, S, request):
    """Node 1 leads the log 1..10 compacted to 6 with the flag set and the config
    change at 10 uncommitted. Node 2 is in Retry at next 9, node 3 lags at next 6
    = firstIndex - 1. One proposal's broadcast sends node 2 the entries 9..11
    marked 10 and node 3 the InstallSnapshot (6, 5). Node 3 acks at 6 and gets
    the entries 7..11, marked 10 as well."""
    _need(be, request)
    p = _group(S, 1, abi.LEADER, [10, 8, 3])
    p[0]["first_index_m1"] = 6
    _window(p, [(6, 5)])
    _member(p, 1, 2, VOTER, match=8, next_=9, state=abi.RETRY, active=1)
    _member(p, 2, 3, VOTER, match=3, next_=6, state=abi.RETRY, active=1)
    p[0]["flags"] |= C.PENDING
    side = C.Side(be, _in_memory(p), S, _snap(6, 5), C.cc_recs(1, 10))
    st, out, _, rest, cc = side.step(loc=_loc(propose=1))
    to3 = out[out["slot"] == 2]
    assert len(to3) == 1 and to3[0]["type"] == C.INSTALL_SNAPSHOT and len(rest) == 0
    assert [int(to3[0][f]) for f in ("log_index", "log_term", "commit", "term", "reject")] == [6, 5, 0, 5, 0]
    assert _marks(out, 1) == [(1, 10, 0, 8, 3)] and _rec(cc) == (10, 0)
    r = st[0]["remotes"][2]
    assert [int(r[f]) for f in ("state", "snapshot_index", "next", "match")] == [abi.SNAPSHOT_ST, 6, 6, 3]
    st, out, _, _, _ = side.step(_msg(abi.REPLICATE_RESP, 2, 5, log_index=6))
    r = st[0]["remotes"][2]
    assert int(r["match"]) == 6 and int(r["snapshot_index"]) == 0 and int(r["state"]) != abi.SNAPSHOT_ST
    assert _marks(out, 2) == [(1, 10, 0, 6, 5)]
    # two ordinary passes: node 3 acks the resend (8 commits with it), then another proposal goes out
    st, _, _, _, cc = side.step(_msg(abi.REPLICATE_RESP, 2, 5, log_index=11))
    assert int(st[0]["remotes"][2]["match"]) == 11 and _rec(cc) == (10, 0)
    st, out, _, _, _ = side.step(loc=_loc(propose=1))
    assert int(st[0]["last_index"]) == 12 and _marks(out, 2) == [(0, 0, 0, 11, 1)]
    side.close()


# ---------------------------------------------------------------- host calls on a restored peer
@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_restore_remotes_and_apply_on_a_restored_peer(be, S, request):
    """gr_restore_remotes after the restore and gr_apply_config_change on the
    later leader, all three switches on (gpu: the engine calls; cpu: the host
    builds of the same code). Neither moves the snapshot record or the
    gr_cc_index record; the apply clears the flag; the config change proposed
    next finds nothing above committed and records prev = 0."""
    _need(be, request)
    side = C.Side(be, _long_follower(S), S, cc=C.cc_recs(1, 11, 8))
    side.step(_install(0, 6, 10, 6))
    assert list(side.restore([0], C.membership(SAME))) == [abi.CC_APPLIED]
    _two_passes(side, 10, 6, 6, ents=2)
    side = _campaigning(side, 7)
    _win(side, 7)
    st, _, _, _, cc = side.step(loc=_loc(propose=1, cc=1))
    assert int(st[0]["flags"]) & C.PENDING and _rec(cc) == (14, 0)
    st, _, _, _, _ = side.step(_msg(abi.REPLICATE_RESP, 0, 7, log_index=14))
    assert int(st[0]["committed"]) == 14
    assert list(side.apply([0], CC.changes(1, abi.CC_ADD_NODE, 1))) == [abi.CC_APPLIED]
    assert not int(side.state[0]["flags"]) & C.PENDING
    st, _, res, _, cc = side.step(loc=_loc(propose=1, cc=1))
    assert int(res[0]["propose_result"]) == abi.PROP_APPENDED and int(st[0]["flags"]) & C.PENDING
    assert _rec(cc) == (15, 0)
    side.close()


# ---------------------------------------------------------------- switch independence
@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_switch_independence(be, S, request):
    """The first case with one switch off. Config entries off, over the live
    records (11, 0) and (11, 8): the restore and the two passes run as
    test_snapshots.py has them and the gr_cc_index array is never written: the
    engine allocates and binds it whatever the switch says, so a restore that
    cleared it regardless would show in its bytes (Side.step compares them after
    every pass, the scenario after the restore and after the two passes). The
    promotion over uncommitted entries escalates GR_ESC_UNSUPPORTED
    (test_promotion_switch_off). On the host lane this half runs the snapshots
    build, which has no array at all. Snapshots off: the InstallSnapshot escalates
    GR_ESC_UNSUPPORTED with nothing applied (test_switch_off)."""
    _need(be, request)
    for rec in ((11, 0), (11, 8)):
        side = _campaigning(scn_restore_then_promotion(be, S, rec, config_entries=False), 7, config_entries=False)
        st, _, res, _, cc = _win(side, 7, esc={0: "unsupported"})
        assert int(res[0]["esc_item"]) == 0 and st[0]["state"] == abi.CANDIDATE and _rec(cc) == rec
        side.close()
    side = C.Side(be, _long_follower(S), S, cc=C.cc_recs(1, 11), snapshots=False)
    before = side.state.copy()
    st, out, res, rest, cc = side.step(_install(0, 6, 10, 6), loc=_loc(), esc={0: "unsupported"})
    assert int(res[0]["esc_item"]) == 0 and len(out) == 0 and len(rest) == 0
    assert st.tobytes() == before.tobytes() and _rec(cc) == (11, 0)
    side.close()


# ---------------------------------------------------------------- live populations
PASSES, LAG = 20, 4          # replica LAG of every group starts below its leader's firstIndex - 1
CC_PASS, MUTE_PASS = 5, 7    # the scripted groups: a config change to one follower only, then the leader muted


def _kinds(G):
    """The scripted subset, by group: 1 the follower that holds the uncommitted
    config change wins (count 1); 2 another follower wins and later sends that
    follower a snapshot; 3 the restored laggard wins; 0 the rest."""
    g = np.arange(G)
    return np.where(g % 8 == 1, 1, np.where(g % 8 == 5, 2, np.where(g % 8 == 3, 3, 0)))


def _population(G, R, seed):
    """test_snapshots._live's start at R = 5: replica LAG stopped 56 entries
    below its leader's log, 40 below where replicas 0..3 compacted and took
    their snapshot; its remote is active in three groups of four."""
    from dragonboat_amd import populations as P
    peers = P.make_groups(G, R, seed=seed, term_lo=2, term_hi=5)
    peers["election_tick"] = 0  # every replica ticks from pass 0 on: nobody times out before the first heartbeat
    lead, lag = peers[:G], peers[LAG * G:]
    cut = lead["last_index"] - np.uint64(16)
    for r in range(LAG):
        v = peers[r * G:(r + 1) * G]
        v["first_index_m1"] = cut
        v["run_start"][:, 0] = cut
    old = cut - np.uint64(40)
    for f in ("committed", "applied", "last_index"):
        lag[f] = old
    lag["n_runs"] = 1
    lag["run_start"][:, 1], lag["run_term"][:, 1] = 0, 0
    lag["remotes"]["match"][:, LAG] = old
    lag["remotes"]["next"][:, :R] = (old + np.uint64(1))[:, None]
    r4 = lead["remotes"][:, LAG]
    r4["match"], r4["next"], r4["state"] = old, old + np.uint64(1), abi.RETRY
    r4["active"] = np.where(np.arange(G) % 4 != 2, 1, 0)
    lead["remotes"][:, LAG] = r4
    snap = np.zeros(R * G, abi.SNAPSHOT_REC)
    snap["index"][:LAG * G] = np.tile(cut, LAG)
    snap["term"][:LAG * G] = np.tile(lead["run_term"][:, 0], LAG)
    return peers, snap


def live_all(be, G, seed=31, updates=False, drain_after=False):
    """G groups x 5 with every switch on, scripted (see the tests' docstring).
    Returns the finished Population and the committed indexes after every pass.
    updates: the host is driven by gr_collect_updates alone
    (all_switches_common.Population); drain_after: it drains the restored and the
    promotion list after the collect, not before it."""
    from dragonboat_amd import populations as P
    R = 5
    n = R * G
    peers, snap = _population(G, R, seed)
    pop = C.Population(be, peers, snap, G, R, updates=updates, drain_after=drain_after)
    kind = _kinds(G)
    grp = np.arange(n) % G
    rep = np.arange(n) // G
    winner = {1: 1, 2: 2, 3: LAG}
    compacted = set()
    committed = []
    for k in range(PASSES):
        ref = pop.ref
        lead = np.nonzero((ref["state"] == abi.LEADER) & ~pop.muted)[0]
        loc = P.propose_locals(n, lead, seed=seed, pass_index=k, ticks=1)
        plain = lead[(kind[lead % G] == 0) & ((lead % G) % 3 == 0)]
        pop.propose_cc(loc, plain)  # a scripted third: a config change whenever the flag is clear
        if k == CC_PASS:
            pop.propose_cc(loc, lead[(kind[lead % G] == 1) | (kind[lead % G] == 2)])
        if k == MUTE_PASS:
            pop.muted[lead[kind[lead % G] != 0]] = True
        if k >= MUTE_PASS:  # the scripted winner's election clock runs ahead until it campaigns
            for kd, r in winner.items():
                w = np.nonzero((kind[grp] == kd) & (rep == r) & (ref["state"] == abi.FOLLOWER) &
                               (ref["leader_id"] == 1))[0]
                loc["ticks"][w] = 10
        # kind 2: the new leader (replica 2) compacts past what it would send replica 1
        # once it has committed that far, and takes its snapshot there
        for p in lead[(kind[lead % G] == 2) & (lead // G == 2)]:
            g = int(p) % G
            if g not in compacted and int(ref[p]["committed"]) >= int(ref[p]["remotes"][1]["next"]) + 1:
                compacted.add(g)
                i = int(ref[p]["committed"])
                pop.compact([p], [i], [CE._term_at(ref[p], i)])

        def keep(sender, receiver, m):
            ks, rs, rr = kind[sender % G], sender // G, receiver // G
            rep_ = m["type"] == abi.REPLICATE
            # kinds 1, 2: from CC_PASS on the old leader's Replicates reach replica 1 only
            cut1 = rep_ & ((ks == 1) | (ks == 2)) & (rs == 0) & (rr != 1) & (k >= CC_PASS)
            # kind 2: the new leader's Replicates do not reach replica 1 (its InstallSnapshot will)
            cut2 = rep_ & (ks == 2) & (rs == 2) & (rr == 1)
            return ~(cut1 | cut2)
        pop.step(loc, keep=keep)
        committed.append(pop.ref["committed"].copy())
    return pop, committed


def check_live_all(pop, committed, G):
    R, c = 5, pop.count
    print("all-switches population", pop.be, G, c, pop.esc)
    for name in ("restores_uncommitted", "promoted_flag", "promoted_clear", "promoted_restored",
                 "snapshots_sent_flagged", "marked_replicates"):
        assert c[name] > 0, (name, c)
    for why in ("unsupported", "election", "config_change", "snapshot"):
        assert pop.esc.get(why, 0) == 0, pop.esc
    ref = pop.ref
    live = ~pop.muted
    nl = ((ref["state"] == abi.LEADER) & live).reshape(R, G).sum(axis=0)
    assert np.all(nl == 1), f"groups without exactly one live leader: {np.nonzero(nl != 1)[0][:8]}"
    leader = np.argmax(((ref["state"] == abi.LEADER) & live).reshape(R, G), axis=0) * G + np.arange(G)
    lag = LAG * G + np.arange(G)
    follows = leader != lag
    last, prev = committed[-1], committed[-3]
    assert np.all(last[lag][follows] + np.uint64(1) == last[leader][follows]), \
        np.nonzero(last[lag] + np.uint64(1) != last[leader])[0][:8]
    assert np.all(last[lag] > prev[lag])  # and still advancing, the laggards that lead included


LIVE_DOC = """G groups x 5 replicas, every switch on, 20 scripted passes, each compared
    with the reference (peer, snapshot and gr_cc_index records, messages, results,
    the restored list). The leaders propose every pass with a tick each; the
    leaders of every third unscripted group propose a config change whenever
    their flag is clear; replica 4 of every group starts below its leader's
    firstIndex - 1 and is caught up by InstallSnapshot. In three groups of eight,
    at pass 5 the leader proposes a config change and from then on its Replicates
    reach replica 1 only; at pass 7 it is muted for good and one scripted
    follower's election clock runs ahead: replica 1 (it wins over its uncommitted
    config change: count 1), replica 2 (count 0; the host then compacts it past
    replica 1's next with a snapshot record, so replica 1 gets an InstallSnapshot
    while its gr_cc_index record is live), or replica 4 (a restored peer wins).
    Every pass the host drains the restored list, calls gr_restore_remotes on
    those peers, gr_commit_update and gr_notify_applied on all, and
    gr_apply_config_change where a change was committed.

    check_live_all requires every interaction counter, computed from the
    reference side's records, to be non-zero, no escalation of the kinds the
    handlers lifted, one live leader per group, and every laggard that follows a
    leader one entry behind its committed index and advancing. Observed, equal
    on the host lane, through gr_step and on the split schedule (G = 192 / 200):
    restores 216 / 225, of peers with last > committed 24 / 25; promotions
    72 / 75, over uncommitted entries with the flag set 24 / 25 and clear
    24 / 25, of previously restored peers 24 / 25; InstallSnapshot sent
    216 / 225, by a leader whose flag is set 40 / 42; marked Replicates
    1168 / 1223; escalations none."""


def test_live_all_hostlane_192(built):
    pop, committed = live_all("cpu", 192)
    check_live_all(pop, committed, 192)


def test_live_all_hostlane_200(built):
    pop, committed = live_all("cpu", 200)
    check_live_all(pop, committed, 200)


@pytest.mark.gpu
@pytest.mark.parametrize("G", [192, 200])  # route_wu = 1 / 0
@pytest.mark.parametrize("be", ["gpu", "dev"])
def test_live_all_gpu(gpu, monkeypatch, be, G):
    if be == "dev":
        monkeypatch.setenv("GR_SPLIT_MIN_LANES", "1")  # read at gr_create
        monkeypatch.setenv("GR_SMALL_BLOCKS", "0")     # the split schedule, not the fused small kernel
    pop, committed = live_all(be, G)
    try:
        check_live_all(pop, committed, G)
    finally:
        pop.close()


for _t in (test_live_all_hostlane_192, test_live_all_hostlane_200, test_live_all_gpu):
    _t.__doc__ = LIVE_DOC


# ---------------------------------------------------------------- the same, the host driven by the collect alone
# Per pass, from the reference side's records (ref_step's results and peer
# records through updates_common.ref_classes, prevState mirrored from the loaded
# State): reported peers, ext records, restored peers. Per 24 groups (G = 192: x 8)
# and per 25 (G = 200: x 8): of 120 / 125 peers.
UPD_REPORTED = {192: [960, 912, 768, 960, 768, 960, 864, 960, 696, 888, 672, 864, 672, 864, 864, 864, 888, 864, 864, 864],
                200: [1000, 950, 800, 1000, 800, 1000, 900, 1000, 725, 925, 700, 900, 700, 900, 900, 900, 925, 900, 900,
                      900]}
UPD_EXT = {192: {8: 72, 9: 288}, 200: {8: 75, 9: 300}}
UPD_RESTORED = {192: {1: 144, 3: 48, 16: 24}, 200: {1: 150, 3: 50, 16: 25}}


def check_update_counts(pop, G):
    """The reference's own counts per pass (Population._collect computes them
    from rres / rst alone) against the table; the engine's equal them pass by pass
    (asserted at every collect)."""
    got = pop.upd_counts
    print("updates per pass (reported, ext, restored)", pop.be, G, got)
    assert len(got) == PASSES
    assert [c[0] for c in got] == UPD_REPORTED[G]
    assert {k: c[1] for k, c in enumerate(got) if c[1]} == UPD_EXT[G]
    assert {k: c[2] for k, c in enumerate(got) if c[2]} == UPD_RESTORED[G]


@pytest.mark.parametrize("G", [192, 200])
def test_live_all_updates_hostlane(built, G):
    """live_all with the host driven by the collect alone, on the host lane (the
    collect emulated by gr_update_class over the host lane's results): after every
    pass the rule of updates_common.ref_classes runs over the reference side's own
    results and records, and gr_commit_update / gr_notify_applied go to the
    reported peers only, with stable_log_to and applied_to taken from the records.
    The reference side still commits every peer, so a peer the rule failed to
    report shows as a saved_to / log_applied difference in the next pass's
    comparison. Asserted of the reference in every pass: every restored peer,
    every promoted peer and every peer parity.update_commits has something to
    commit for is reported ("a restore moves committed, so the State condition
    reports it"; "a host that commits only the reported slots loses nothing").
    The counts per pass are the reference's, recomputed here, and equal the
    table derived on the reference side alone (UPD_REPORTED, UPD_EXT,
    UPD_RESTORED)."""
    pop, committed = live_all("cpu", G, updates=True)
    check_live_all(pop, committed, G)
    check_update_counts(pop, G)

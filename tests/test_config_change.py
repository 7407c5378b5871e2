"""Membership changes applied on the device: gr_apply_config_change, which is
Peer.ApplyConfigChange / RejectConfigChange (peer.go:153-174 -> raft.addNode /
addObserver / removeNode, raft.go:822-861) for a list of engine slots.

Every case runs on two backends, the host build of gr_config_change.h over
records (`not gpu`) and the engine (`-m gpu`), against the reference side: the
oracle's raft object built from the same record, changed by the oracle's
restatement of those functions and exported (config_change_common.py). State and
status must agree after the call, refused peers must be untouched bit for bit,
and later passes run under the usual oracle parity.
"""
import numpy as np
import pytest

from dragonboat_amd import abi, populations as P
import config_change_common as C
import simulate as SIM
from test_golden import _peer

BACKENDS = [pytest.param("cpu", id="host"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
ADD, REMOVE, OBSERVER = abi.CC_ADD_NODE, abi.CC_REMOVE_NODE, abi.CC_ADD_OBSERVER
APPLIED, HOST, NO_SLOT = abi.CC_APPLIED, abi.CC_HOST, abi.CC_NO_SLOT
ENTS = [(i, 5) for i in range(1, 11)]  # a log 1..10 at term 5


def _need(be, request):
    request.getfixturevalue("gpu" if be == "gpu" else "built")


def _member(p, j, node_id, kind, match=0, next_=None, state=abi.RETRY, active=0):
    g = p[0]
    g["remote_id"][j] = node_id
    r = g["remotes"][j]
    r["kind"], r["match"], r["state"], r["active"], r["snapshot_index"] = kind, match, state, active, 0
    r["next"] = (int(g["last_index"]) + 1 if next_ is None else next_) if kind != abi.SLOT_EMPTY else 0


def _group(S, self_id, state, matches, committed=8, term=5, ents=ENTS, leader_id=1):
    """A peer of the group with voters 1..len(matches) in slots 0.., node self_id,
    the other slots empty with no id; a leader's followers replicate actively."""
    p = _peer(S, len(matches), state, term, ents, committed)
    g = p[0]
    g["node_id"], g["self_slot"], g["leader_id"] = self_id, self_id - 1, leader_id
    for j in range(abi.GR_SMAX):
        if j < len(matches):
            lead = state == abi.LEADER and j != self_id - 1
            _member(p, j, j + 1, abi.SLOT_VOTER, matches[j], state=abi.REPLICATE_ST if lead else abi.RETRY,
                    active=1 if lead else 0)
        else:
            _member(p, j, 0, abi.SLOT_EMPTY)
    return p


def _one(be, p, S, type_, node_id, want, rand=0):
    side = C.Side(be, p, S)
    st = side.change([0], C.changes(1, type_, node_id, rand))
    assert int(st[0]) == want, (int(st[0]), want)
    return side


# ---------------------------------------------------------------- RemoveNode
@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_remove_follower_on_each_peer(be, S, request):
    """Node 3 leaves a three-voter group: on the leader its slot empties and
    nothing commits ({10, 8} -> 8 = committed); the removed peer itself ends with
    no slot of its own; the other follower keeps its leader."""
    _need(be, request)
    side = _one(be, _group(S, 1, abi.LEADER, [10, 8, 8]), S, REMOVE, 3, APPLIED)
    g = side.state[0]
    assert g["remotes"][2]["kind"] == abi.SLOT_EMPTY and g["remote_id"][2] == 3 and g["self_slot"] == 0
    assert [int(g["remotes"][2][f]) for f in ("match", "next", "snapshot_index", "state", "active")] == [0] * 5
    side.close()
    side = _one(be, _group(S, 3, abi.FOLLOWER, [0, 0, 10]), S, REMOVE, 3, APPLIED)
    assert side.state[0]["self_slot"] == abi.GR_SLOT_NONE and side.state[0]["state"] == abi.FOLLOWER
    side.step(loc=_tick(3))  # selfRemoved: ticks on without campaigning
    side.close()
    side = _one(be, _group(S, 2, abi.FOLLOWER, [0, 10, 0]), S, REMOVE, 3, APPLIED)
    assert side.state[0]["self_slot"] == 1 and side.state[0]["leader_id"] == 1
    side.close()


def _tick(n, rand=77):
    loc = np.zeros(1, abi.LOCAL)
    loc["ticks"], loc["rand"] = n, rand
    return loc


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_remove_leader_on_follower(be, S, request):
    """The leader's id leaves: the follower keeps leaderID (removeNode does not
    touch it) and its later ticks run under parity."""
    _need(be, request)
    side = _one(be, _group(S, 2, abi.FOLLOWER, [0, 10, 0]), S, REMOVE, 1, APPLIED)
    g = side.state[0]
    assert g["leader_id"] == 1 and g["remotes"][0]["kind"] == abi.SLOT_EMPTY and g["self_slot"] == 1
    side.step(loc=_tick(2))
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_remove_transfer_target_and_absent_id(be, S, request):
    """abortLeaderTransfer only when the target is the removed id and the peer
    leads; an absent id still clears the pending flag and runs that check."""
    _need(be, request)
    for target, removed, left in [(3, 3, 0), (2, 3, 2), (77, 77, 0)]:
        p = _group(S, 1, abi.LEADER, [10, 8, 8])
        p[0]["leader_transfer_target"] = target
        p[0]["flags"] |= abi.F_PENDING_CONFIG_CHANGE
        side = _one(be, p, S, REMOVE, removed, APPLIED)
        g = side.state[0]
        assert int(g["leader_transfer_target"]) == left and not g["flags"] & abi.F_PENDING_CONFIG_CHANGE
        if removed == 77:
            assert list(g["remotes"]["kind"][:3]) == [abi.SLOT_VOTER] * 3
        side.close()
    p = _group(S, 2, abi.FOLLOWER, [0, 10, 0])  # not leading: leaderTransfering() is false
    p[0]["leader_transfer_target"] = 3
    side = _one(be, p, S, REMOVE, 3, APPLIED)
    assert int(side.state[0]["leader_transfer_target"]) == 3
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_remove_last_voter_skips_try_commit(be, S, request):
    """len(r.remotes) == 0 after the removal: tryCommit is not evaluated
    (raft.go:856), although match 10 is above committed 8."""
    _need(be, request)
    side = _one(be, _group(S, 1, abi.LEADER, [10]), S, REMOVE, 1, APPLIED)
    g = side.state[0]
    assert g["self_slot"] == abi.GR_SLOT_NONE and int(g["committed"]) == 8
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
def test_remove_that_would_commit_goes_to_host(be, request):
    """Four voters with matches {10, 10, 8, 8}, committed 8. Removing an 8 makes
    the quorum match 10: at the current term the reference commits and
    broadcasts, so GR_CC_HOST and the peer untouched; with entry 10 at an older
    term tryCommit refuses and the change applies with committed unchanged."""
    _need(be, request)
    side = _one(be, _group(5, 1, abi.LEADER, [10, 10, 8, 8]), 5, REMOVE, 4, HOST)
    assert side.state[0]["remotes"][3]["kind"] == abi.SLOT_VOTER and int(side.state[0]["committed"]) == 8
    side.close()
    old = [(i, 4) for i in range(1, 11)]
    side = _one(be, _group(5, 1, abi.LEADER, [10, 10, 8, 8], ents=old), 5, REMOVE, 4, APPLIED)
    assert side.state[0]["remotes"][3]["kind"] == abi.SLOT_EMPTY and int(side.state[0]["committed"]) == 8
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_follower_left_as_only_voter_goes_to_host(be, S, request):
    """removeNode's tryCommit has no leader check: a follower left alone with
    committed 8 < lastIndex 10 at its term would commit 10."""
    _need(be, request)
    side = _one(be, _group(S, 1, abi.FOLLOWER, [10, 0], leader_id=2), S, REMOVE, 2, HOST)
    assert side.state[0]["remotes"][1]["kind"] == abi.SLOT_VOTER
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
def test_term_lookup_below_window_goes_to_host(be, request):
    """The quorum match after the removal (7) is above committed (5) and below
    the record's oldest run (9): its term is LogReader's to give. The oracle's
    log is rebuilt from the same window and cannot tell, so only the engine side
    runs here: GR_CC_HOST, untouched."""
    _need(be, request)
    p = _group(3, 1, abi.LEADER, [10, 7, 5], committed=5)
    p[0]["run_start"][0] = 9
    side = C.Side(be, p, 3)
    rc, st, new = side.apply_raw(np.zeros(1, np.uint32), C.changes(1, REMOVE, 3))
    assert rc == -6 and list(st) == [HOST] and new.tobytes() == side.state.tobytes()
    side.close()


# ---------------------------------------------------------------- AddNode
@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_add_voter(be, S, request):
    """A new id takes the lowest free slot as setRemote(id, 0, lastIndex + 1)
    leaves it and the leader's next pass sends to it; an id that is a voter
    changes nothing but the pending flag; a full table is GR_CC_NO_SLOT."""
    _need(be, request)
    p = _group(S, 1, abi.LEADER, [10, 10], committed=10)
    p[0]["flags"] |= abi.F_PENDING_CONFIG_CHANGE
    side = _one(be, p, S, ADD, 99, APPLIED)
    g = side.state[0]
    assert g["remote_id"][2] == 99 and g["remotes"][2]["kind"] == abi.SLOT_VOTER
    assert [int(g["remotes"][2][f]) for f in ("match", "next", "state", "active")] == [0, 11, abi.RETRY, 0]
    assert not g["flags"] & abi.F_PENDING_CONFIG_CHANGE
    loc = _tick(0)
    loc["propose_entries"] = 1
    _, out, _ = side.step(loc=loc)
    to_new = out[out["slot"] == 2]
    assert len(to_new) == 1 and to_new[0]["type"] == abi.REPLICATE and int(to_new[0]["log_index"]) == 10
    before = side.state.copy()
    assert int(side.change([0], C.changes(1, ADD, 2))[0]) == APPLIED
    assert side.state.tobytes() == before.tobytes()
    side.close()
    full = _group(S, 1, abi.LEADER, [10] * S, committed=10)
    side = _one(be, full, S, ADD, 99, NO_SLOT)
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_readd_gets_its_old_slot(be, S, request):
    """Slots: node 1, an empty slot, node 3. Node 3 leaves and comes back: its old
    slot, not the lower empty one, which the next new id takes."""
    _need(be, request)
    p = _group(S, 1, abi.LEADER, [10, 10, 10], committed=10)
    _member(p, 1, 0, abi.SLOT_EMPTY)
    side = _one(be, p, S, REMOVE, 3, APPLIED)
    assert int(side.change([0], C.changes(1, ADD, 3))[0]) == APPLIED
    g = side.state[0]
    assert g["remote_id"][2] == 3 and g["remotes"][2]["kind"] == abi.SLOT_VOTER and int(g["remotes"][2]["next"]) == 11
    assert g["remotes"][1]["kind"] == abi.SLOT_EMPTY
    assert int(side.change([0], C.changes(1, ADD, 8))[0]) == APPLIED
    assert side.state[0]["remote_id"][1] == 8 and side.state[0]["remotes"][1]["kind"] == abi.SLOT_VOTER
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_promote_observer(be, S, request):
    """Another peer's observer becomes a voter with its progress kept. The peer's
    own: becomeFollower(term, leaderID) with the record's draw, so the timeout is
    electionTimeout + rand % electionTimeout, the ticks are 0, the vote and the
    leader stay and every remote is as resetRemotes leaves it."""
    _need(be, request)
    p = _group(S, 1, abi.LEADER, [10, 10], committed=10)
    _member(p, 2, 3, abi.SLOT_OBSERVER, match=7, next_=8, state=abi.REPLICATE_ST, active=1)
    side = _one(be, p, S, ADD, 3, APPLIED)
    r = side.state[0]["remotes"][2]
    assert [int(r[f]) for f in ("kind", "match", "next", "state", "active")] == [abi.SLOT_VOTER, 7, 8,
                                                                                  abi.REPLICATE_ST, 1]
    side.close()
    p = _group(S, 3, abi.OBSERVER, [4, 6], committed=10)
    _member(p, 2, 3, abi.SLOT_OBSERVER, match=9, next_=3, state=abi.WAIT, active=1)
    g = p[0]
    g["vote"], g["election_tick"], g["heartbeat_tick"] = 2, 4, 1
    g["flags"] |= abi.F_PENDING_CONFIG_CHANGE
    side = _one(be, p, S, ADD, 3, APPLIED, rand=12345)
    g = side.state[0]
    assert g["state"] == abi.FOLLOWER and g["self_slot"] == 2 and int(g["leader_id"]) == 1 and int(g["vote"]) == 2
    assert int(g["randomized_election_timeout"]) == 10 + 12345 % 10
    assert int(g["election_tick"]) == 0 and int(g["heartbeat_tick"]) == 0
    for j, m in [(0, 0), (1, 0), (2, 10)]:
        r = g["remotes"][j]
        assert [int(r[f]) for f in ("kind", "match", "next", "state", "active")] == [abi.SLOT_VOTER, m, 11,
                                                                                      abi.RETRY, 0]
    side.step(loc=_tick(3))  # a follower now: its election clock runs
    side.close()


# ---------------------------------------------------------------- AddObserver
@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_add_observer(be, S, request):
    """A new observer takes a free slot; one that exists changes nothing; an id
    that is a voter would be in both of the reference's maps: GR_CC_HOST."""
    _need(be, request)
    side = _one(be, _group(S, 1, abi.LEADER, [10, 10], committed=10), S, OBSERVER, 9, APPLIED)
    r = side.state[0]["remotes"][2]
    assert side.state[0]["remote_id"][2] == 9
    assert [int(r[f]) for f in ("kind", "match", "next", "state")] == [abi.SLOT_OBSERVER, 0, 11, abi.RETRY]
    before = side.state.copy()
    assert int(side.change([0], C.changes(1, OBSERVER, 9))[0]) == APPLIED
    assert side.state.tobytes() == before.tobytes()
    assert int(side.change([0], C.changes(1, OBSERVER, 2))[0]) == HOST
    side.close()


# ---------------------------------------------------------------- the rest of the table
@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_reject_and_candidate(be, S, request):
    """node_id 0 is RejectConfigChange: only the pending flag goes. A candidate's
    tally is kept by slot: GR_CC_HOST whatever the change."""
    _need(be, request)
    p = _group(S, 1, abi.LEADER, [10, 8, 8])
    p[0]["flags"] |= abi.F_PENDING_CONFIG_CHANGE | abi.F_CHECK_QUORUM
    side = _one(be, p, S, REMOVE, 0, APPLIED)
    assert int(side.state[0]["flags"]) == abi.F_CHECK_QUORUM
    assert list(side.state[0]["remotes"]["kind"][:3]) == [abi.SLOT_VOTER] * 3
    side.close()
    p = _group(S, 1, abi.CANDIDATE, [10, 0, 0], leader_id=0)
    p[0]["vote"] = 1
    for type_, node in [(REMOVE, 3), (ADD, 9), (OBSERVER, 9)]:
        side = _one(be, p, S, type_, node, HOST)
        side.close()


def _ack(term, slot, ctx):
    m = np.zeros(1, abi.MESSAGE)
    m["type"], m["slot"], m["term"], m["hint"] = abi.HEARTBEAT_RESP, slot, term, ctx
    return m


@pytest.mark.parametrize("be", BACKENDS)
def test_new_node_does_not_inherit_a_removed_nodes_ack(be, request):
    """A leader holds a ReadIndex request that node 3 (slot 2) confirmed. Node 3
    leaves: readStatus.confirmed is keyed by node id, so its ack still counts and
    the bit stays. A new node must not land in slot 2 (S = 5: it takes slot 3);
    with slot 2 the only empty one (S = 3) there is no slot. Node 2's heartbeat ack
    then confirms the read: the engine and the oracle release it in the same pass."""
    _need(be, request)
    for S, want, slot in [(5, APPLIED, 3), (3, NO_SLOT, None)]:
        p = _group(S, 1, abi.LEADER, [10, 10, 10], committed=10)
        g = p[0]
        g["read_index_count"] = 1
        rs = g["read_index"][0]
        rs["index"], rs["ctx_low"], rs["from_slot"], rs["ack_bits"] = 10, 7, abi.GR_SLOT_NONE, 1 << 2
        side = _one(be, p, S, REMOVE, 3, APPLIED)
        assert int(side.state[0]["read_index"][0]["ack_bits"]) == 1 << 2
        assert int(side.change([0], C.changes(1, ADD, 9))[0]) == want
        if slot is not None:
            assert side.state[0]["remote_id"][slot] == 9 and side.state[0]["remotes"][2]["kind"] == abi.SLOT_EMPTY
        _, _, res = side.step(_ack(5, 1, 7))
        assert int(res[0]["n_ready"]) == 1 and int(res[0]["ready"][0]["ctx_low"]) == 7
        assert int(side.state[0]["read_index_count"]) == 0
        side.close()


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("be", BACKENDS)
def test_refused_calls_write_nothing(be, request):
    """A slot out of range, a slot listed twice and a type that is no
    ConfigChangeType (the reference panics) are errors, and every peer, the
    validly listed ones too, is as it was."""
    _need(be, request)
    peers = np.concatenate([_group(3, 1, abi.LEADER, [10, 8, 8]) for _ in range(4)])
    peers["flags"] |= abi.F_PENDING_CONFIG_CHANGE
    side = C.Side(be, peers, 3)
    bad_type = C.changes(3, REMOVE, 3)
    bad_type["type"][2] = 3
    for idx, cc, err in [([0, 4, 1], C.changes(3, REMOVE, 3), -4), ([0, 1, 0], C.changes(3, REMOVE, 3), -4),
                         ([0, 1, 2], bad_type, -1)]:
        rc, _, new = side.apply_raw(np.asarray(idx, np.uint32), cc)
        assert rc == err, (idx, rc)
        assert new.tobytes() == side.state.tobytes()
    assert list(side.change([3, 0], C.changes(2, REMOVE, 3))) == [APPLIED, APPLIED]  # the engine still works
    side.close()


@pytest.mark.gpu
def test_refused_while_a_pass_is_pending(gpu):
    """Between gr_step_compact_begin and _end the call is refused as gr_compact_log
    is: GR_ESTATE, whether its types are good or not (a bad type alone is
    GR_EINVAL), no status written and no peer changed. The wrapper, which fills
    the statuses with -1 first, raises instead of handing back statuses that
    nobody wrote."""
    import ctypes
    from dragonboat_amd.engine import Engine, GpuRaftError
    G = 64
    eng = Engine(G * 3, 3)
    try:
        eng.load(P.make_groups(G, 3, seed=1))
        sl = np.arange(4, dtype=np.uint32)
        good, bad = C.changes(4, REMOVE, 3), C.changes(4, REMOVE, 3)
        bad["type"][1] = 3
        call = lambda cc, st: eng.lib.gr_apply_config_change(eng._h, sl.ctypes.data, cc.ctypes.data, 4, st.ctypes.data)
        assert call(bad, np.zeros(4, np.int32)) == -1
        cm, xm = eng.pack_messages(np.zeros(0, abi.MESSAGE))
        cl, xl = eng.pack_locals(P.propose_locals(G * 3, np.arange(G), pass_index=0))
        ib, ob = abi.cinbox_of(cm, xm, cl, xl), abi.COutbox()
        assert eng.lib.gr_step_compact_begin(eng._h, ctypes.byref(ib)) == 0
        idx = np.zeros(4, np.uint64)
        for cc in (good, bad):
            st = np.full(4, -1, np.int32)
            assert call(cc, st) == -6 and np.all(st == -1)
            assert eng.lib.gr_compact_log(eng._h, sl.ctypes.data, idx.ctypes.data, 4, None) == -6  # the same code
        with pytest.raises(GpuRaftError):
            eng.apply_config_change(sl, good)
        assert eng.lib.gr_step_compact_end(eng._h, ctypes.byref(ob)) == 0
        assert eng.lib.gr_release_coutbox(eng._h, ctypes.byref(ob)) == 0
        assert np.all(eng.sync_peers(sl)["remotes"]["kind"][:, 2] == abi.SLOT_VOTER)  # nobody was removed
        rc, st = eng.apply_config_change(sl, C.changes(4, ADD, 3))  # after _end the call is taken (a voter: no more)
        assert rc == 0 and list(st) == [APPLIED] * 4
    finally:
        eng.close()


# ---------------------------------------------------------------- the header's summaries
def test_header_summaries_after_a_change(built):
    """The device-only header bits (gr_layout.h). A loaded steady leader carries
    H_NX for every slot, H_MS and H_MP; a change clears them (the rows beside the
    header are written exact, as the state comparison of every other test shows)
    and keeps H_CL, H_GE_LO and the run bits. A follower whose leader is removed
    forgets the leader's slot (F_LSLOT) and no other flag."""
    p = _group(3, 1, abi.LEADER, [10, 8, 8])
    p[0]["first_index_m1"] = 0
    rc, before, after = C.headers(p, C.changes(1, REMOVE, 3), 3)
    assert rc == APPLIED
    assert before & C.H_SYNC_MASK == (7 << 56) | (1 << 59) | (6 << 40)
    assert after & C.H_SYNC_MASK == 0
    keep = C.H_CL_MASK | C.H_RUN_MASK | C.H_GE_LO
    assert before & C.H_CL_MASK == 3 << 21 and after & keep == before & keep
    p = _group(3, 2, abi.FOLLOWER, [0, 10, 0])
    rc, before, after = C.headers(p, C.changes(1, REMOVE, 1), 3)
    assert rc == APPLIED and before & C.H_F_LSLOT == 1 << 13 and after & C.H_F_LSLOT == 0
    rc, before, after = C.headers(p, C.changes(1, REMOVE, 3), 3)
    assert rc == APPLIED and after & C.H_F_LSLOT == 1 << 13  # the leader stayed
    rc, before, after = C.headers(_group(3, 1, abi.CANDIDATE, [10, 0, 0]), C.changes(1, REMOVE, 3), 3)
    assert rc == HOST and after == before


# ---------------------------------------------------------------- a live population
def _live(be, monkeypatch, split):
    """200 groups x 3 replicas through gr_step: steady passes until the leaders
    hold their remote summaries, node 3 removed on every peer in one call, six
    more passes, a new node added, more passes, all under oracle parity."""
    from oracle.pyoracle import hostlane_steady_leaders
    if split:
        monkeypatch.setenv("GR_SPLIT_MIN_LANES", "1")  # read at gr_create
        monkeypatch.setenv("GR_SMALL_BLOCKS", "0")     # the split schedule, not the fused small kernel
    G, R, S = 200, 3, 3
    n = R * G
    topo = P.Topology(G, R)
    rng = np.random.default_rng(5)
    ls = SIM.Lockstep(SIM.GpuBackend if be == "gpu" else SIM.HostlaneBackend, P.make_groups(G, R, seed=23), S)
    leaders = np.arange(G)
    msgs = np.zeros(0, abi.MESSAGE)
    k = 0

    def step(live_slots):
        nonlocal msgs, k
        out, res = ls.step(msgs, P.propose_locals(n, leaders, pass_index=k))
        k += 1
        keep = np.isin(out["slot"], live_slots)  # the transport knows no other node
        msgs = topo.route_messages(out[keep])
        return out, res

    def change(idx, cc):
        """The call on the engine and on the reference side, the same slot list."""
        idx = np.asarray(idx, np.uint32)
        if be == "gpu":
            rc, st = ls.eng.eng.apply_config_change(idx, cc)
        else:
            rc, st = C.host_apply(ls.eng.state, idx, cc, S)
        ref = ls.pop.export()
        rrc, rst = C.ref_apply(ref, idx, cc, S)
        assert rc == rrc == 0 and not st.any() and not rst.any(), (rc, rrc, st[st != 0][:5], rst[rst != 0][:5])
        ls.pop.reload(idx, ref[idx])
        bad = parity_states(ls)
        assert not bad, bad[:3]

    def parity_states(ls):
        import parity
        return parity.compare_states(ls.eng.sync(), ls.pop.export(), S)

    try:
        lean0 = hostlane_steady_leaders() if be == "cpu" else 0
        for _ in range(4):  # warm-up: the pipeline fills, the waves get their hints
            step([0, 1, 2])
        # the last two steady passes, bracketed: which lane finished the leaders
        if be == "gpu":
            t0 = ls.eng.eng.stats()
            ls.eng.eng.timing_begin()
        for _ in range(2):
            step([0, 1, 2])
        # The leaders' remote summaries are live. A lean lane that finishes a leader
        # sets H_NX_j, H_MS and H_MP_j exactly for the rows that hold next =
        # lastIndex + 1, own match = lastIndex and a follower's match = lastIndex - 2,
        # and leaves those rows stale (gr_fast.h, the leader's sync bits;
        # gr_steady.h requires and keeps them). So two things are asserted: those
        # values hold on every leader (the sync resolves bits and exact rows alike),
        # and no lane left the lean kernels in the bracketed passes, so it was a
        # lean lane that wrote them, as bits (tests/test_steady_wu_gpu.py counts the
        # same way). The host build draws its wave hints, so only some waves try the
        # closed form in a pass; there SteadyLeader, which requires the bits, must
        # have finished leaders G times over the six passes.
        if be == "cpu":
            assert hostlane_steady_leaders() - lean0 >= G
        else:
            t = ls.eng.eng.timing_end()
            commits = ls.eng.eng.stats()["leader_commits"] - t0["leader_commits"]
            print("bracketed passes:", t, "leader commits", commits)
            assert t["passes"] == 2 and t["bailed_lanes"] == 0, t
            assert commits >= G  # and the leaders were at work in them
        dev = ls.eng.sync()[:G]
        hi = dev["last_index"]
        assert np.all(dev["remotes"]["next"][:, :3] == (hi + np.uint64(1))[:, None])
        assert np.all(dev["remotes"]["match"][:, 0] == hi)
        assert np.all(dev["remotes"]["match"][:, 1:3] == (hi - np.uint64(2))[:, None])
        assert ls.stats["escalations"] == 0
        # node 3 leaves, on every peer of every group, one call
        change(rng.permutation(n), C.changes(n, REMOVE, 3))
        assert np.all(ls.eng.sync()[2 * G:]["self_slot"] == abi.GR_SLOT_NONE)
        # what was in flight to and from node 3 is dropped (Peer.Handle drops a
        # non-member's responses, peer.go:200-209; its host is gone)
        msgs = msgs[(msgs["peer"] < 2 * G) & (msgs["slot"] != 2)]
        commits = ls.stats["commits"]
        for _ in range(7):
            step([0, 1])
        assert ls.stats["commits"] - commits >= 4 * 2 * G  # the two-voter groups go on committing
        # node 9 joins, on the two members left
        last = ls.pop.export()["last_index"][:G].copy()
        change(rng.permutation(2 * G), C.changes(2 * G, ADD, 9, rand=1))
        out, _ = step([0, 1])
        first = out[(out["slot"] == 2) & (out["peer"] < G)]
        first = first[np.unique(first["peer"], return_index=True)[1]]  # each leader's first message to the new node
        assert len(first) == G and np.all(first["type"] == abi.REPLICATE)
        assert np.all(first["log_index"] == last[first["peer"]])  # next was lastIndex + 1 when it joined
        for _ in range(3):
            step([0, 1])
        assert ls.stats["escalations"] == 0  # Lockstep fails any escalation the oracle does not justify
        assert not parity_states(ls)
    finally:
        ls.close()


def test_live_population_host(built, monkeypatch):
    _live("cpu", monkeypatch, False)


@pytest.mark.gpu
@pytest.mark.parametrize("split", [False, True], ids=["fused", "split"])
def test_live_population_gpu(gpu, monkeypatch, split):
    _live("gpu", monkeypatch, split)

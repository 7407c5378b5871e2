"""Elections on the device, on the CPU: the host build of the lane code with
elections compiled on (tests/_build/libhostlane_elect.so) against the oracle,
bit-exact after every pass through simulate.Lockstep and network.Net. The
reference's vote tables (tests/golden/election_tables.json) run as table ==
oracle == lane; its election known-answer tests run over the in-memory network;
cold starts elect a leader in every group without one escalation to the host."""
import json
import os

import numpy as np
import pytest

from dragonboat_amd import abi
from network import Net, node_records
import elections_common as EC
import simulate as SIM

TABLES = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "election_tables.json")))
STATES = {"follower": abi.FOLLOWER, "candidate": abi.CANDIDATE, "leader": abi.LEADER}
BE = EC.ElectHostlaneBackend


@pytest.fixture(autouse=True)
def _libs(built):
    EC.hostlane_elect_lib()


def with_log(rec, terms, term=None, committed=0):
    """Give record(s) `rec` a persisted log whose entry i + 1 has term terms[i]."""
    runs = [(0, 0)]
    for i, t in enumerate(terms):
        if runs[-1][1] != t:
            runs.append((i + 1, t))
    assert len(runs) <= abi.GR_K
    rec["last_index"] = len(terms)
    rec["committed"] = committed
    rec["applied"] = committed
    rec["n_runs"] = len(runs)
    for k, (s, t) in enumerate(runs):
        rec["run_start"][..., k] = s
        rec["run_term"][..., k] = t
    S = rec["remotes"].shape[-1]
    for j in range(S):
        rec["remotes"][..., j]["next"] = len(terms) + 1
        own = rec["self_slot"] == j
        rec["remotes"][..., j]["match"] = np.where(own, len(terms), 0)
    if term is not None:
        rec["term"] = term
    return rec


def vote_request(peer, slot, **f):
    m = np.zeros(1, abi.MESSAGE)
    m["peer"], m["slot"], m["type"] = peer, slot, abi.REQUEST_VOTE
    for k, v in f.items():
        m[k] = v
    return m


def run_vote_rows(peers, msgs, slots):
    """One pass: every peer gets its RequestVote; returns the engine's replies by
    peer. Lockstep checks state, messages and results against the oracle, and
    no row may go to the host."""
    ls = SIM.Lockstep(BE, peers, slots)
    try:
        _, res = ls.step(np.concatenate(msgs), None)
        assert not res["escalation"].any(), res["escalation"]
        out = ls.last_out
        assert np.all(out["type"] == abi.REQUEST_VOTE_RESP)
        return {int(m["peer"]): bool(m["reject"]) for m in out}
    finally:
        ls.close()


# ---- raft_etcd_test.go:1426-1459 TestRecvMsgVote
def test_table_recv_msg_vote():
    rows = TABLES["recv_msg_vote"]["rows"]
    assert len(rows) == 20
    peers = node_records([1, 2], {1, 2}, copies=len(rows))[:len(rows)]  # node 1 of {1, 2}, one per row
    with_log(peers, [2, 2])
    msgs = []
    for k, (state, i, term, vote, _) in enumerate(rows):
        peers[k]["state"] = STATES[state]
        peers[k]["vote"] = vote
        if state == "leader":
            peers[k]["leader_id"] = 1
        msgs.append(vote_request(k, 1, log_index=i, log_term=term))
    got = run_vote_rows(peers, msgs, 2)
    assert [got[k] for k in range(len(rows))] == [r[4] for r in rows]


# ---- raft_etcd_paper_test.go:806-825 TestVoter
def test_table_voter():
    rows = TABLES["voter"]["rows"]
    peers = node_records([1, 2], {1, 2}, copies=len(rows))[:len(rows)]
    msgs = []
    for k, (terms, logterm, index, _) in enumerate(rows):
        with_log(peers[k:k + 1], terms)
        msgs.append(vote_request(k, 1, term=3, log_term=logterm, log_index=index))
    got = run_vote_rows(peers, msgs, 2)
    assert [got[k] for k in range(len(rows))] == [r[3] for r in rows]


# ---- raft_test.go:1145-1171 TestCanGrantVote: the sender's log is up to date
# (both logs empty), so the reply rejects exactly when canGrantVote is false
def test_table_can_grant_vote():
    rows = TABLES["can_grant_vote"]["rows"]
    peers = node_records([1, 2, 3], {1, 2, 3}, copies=len(rows))[:len(rows)]
    peers["term"] = 1
    msgs = []
    for k, (vote, mt, _) in enumerate(rows):
        peers[k]["vote"] = vote
        msgs.append(vote_request(k, 1, term=mt))
    got = run_vote_rows(peers, msgs, 3)
    assert [not got[k] for k in range(len(rows))] == [r[2] for r in rows]


# ---- raft_test.go:1134-1143 TestHandleVoteResp, on a candidate of five voters
# (quorum 3), so that the table's four responses decide nothing
def test_table_handle_vote_resp():
    rows = TABLES["handle_vote_resp"]["rows"]
    peers = node_records([1, 2, 3, 4, 5], {1, 2, 3, 4, 5})[:1]
    ls = SIM.Lockstep(BE, peers, 5)
    try:
        for frm, rejected, count in rows:
            m = np.zeros(1, abi.MESSAGE)
            if frm == 1:  # node 1's own vote is its campaign's (raft.go:783)
                m["peer"], m["slot"], m["type"] = 0, 0, abi.ELECTION
            else:
                m["peer"], m["slot"], m["type"], m["term"], m["reject"] = 0, frm - 1, abi.REQUEST_VOTE_RESP, 1, rejected
            _, res = ls.step(m, None)
            assert not res["escalation"].any()
            dev = ls.eng.sync().view(abi.PEER_VOTES)[0]
            assert dev["state"] == abi.CANDIDATE
            assert bin(int(dev["votes_granted"])).count("1") == count, (frm, rejected, dev["votes_granted"])
        assert int(dev["votes_granted"]) == 0b101 and int(dev["votes_rejected"]) == 0b010
    finally:
        ls.close()


# ---------------------------------------------------------------- network KATs
def _election(net, nid):
    net.send(net.msg(nid, nid, abi.ELECTION))


def _no_host_elections(net):
    r = net.ls.stats["esc_reasons"]
    assert r.get("election", 0) == 0 and r.get("unsupported", 0) == 0, r


# ---- raft_etcd_test.go:425-460 TestLeaderElection (nopStepper = a node that
# neither receives nor sends)
@pytest.mark.parametrize("n,dead,logs,wstate,wterm", [
    (3, (), {}, abi.LEADER, 1),
    (3, (3,), {}, abi.LEADER, 1),
    (3, (2, 3), {}, abi.CANDIDATE, 1),
    (4, (2, 3), {}, abi.CANDIDATE, 1),
    (5, (2, 3), {}, abi.LEADER, 1),
    (5, (), {2: [1], 3: [1], 4: [1, 1]}, abi.FOLLOWER, 1),
])
def test_leader_election(n, dead, logs, wstate, wterm):
    ids = list(range(1, n + 1))
    recs = node_records(ids, set(ids))
    for nid, terms in logs.items():
        with_log(recs[nid - 1:nid], terms, term=terms[-1])
    net = Net(BE, ids, records=recs)
    for d in dead:
        net.isolate(d)
    _election(net, 1)
    st = net.state(1)
    assert (int(st["state"]), int(st["term"])) == (wstate, wterm)
    _no_host_elections(net)
    net.close()


# ---- raft_etcd_test.go:781-844 TestDuelingCandidates
def dueling_candidates(backend):
    net = Net(backend, [1, 2, 3])
    net.cut(1, 3)
    _election(net, 1)
    _election(net, 3)
    assert int(net.state(1)["state"]) == abi.LEADER
    assert int(net.state(3)["state"]) == abi.CANDIDATE
    net.recover()
    _election(net, 3)
    for nid, last in ((1, 1), (2, 1), (3, 0)):
        st = net.state(nid)
        assert (int(st["state"]), int(st["term"]), int(st["last_index"])) == (abi.FOLLOWER, 2, last), nid
    assert int(net.state(1)["committed"]) == 1
    _no_host_elections(net)
    net.close()


def test_dueling_candidates():
    dueling_candidates(BE)


# ---- raft_etcd_test.go:917-959 TestCandidateConcede
def kat_candidate_concede(backend):
    net = Net(backend, [1, 2, 3])
    net.isolate(1)
    _election(net, 1)
    _election(net, 3)
    net.recover()
    net.send(net.msg(3, 3, abi.LEADER_HEARTBEAT))
    net.send(net.msg(3, 3, abi.PROPOSE, entries=1))
    net.send(net.msg(3, 3, abi.LEADER_HEARTBEAT))
    a = net.state(1)
    assert (int(a["state"]), int(a["term"])) == (abi.FOLLOWER, 1)
    for nid in (1, 2, 3):
        st = net.state(nid)
        assert (int(st["last_index"]), int(st["committed"])) == (2, 2), nid
    _no_host_elections(net)
    net.close()


def test_candidate_concede():
    kat_candidate_concede(BE)


# ---- raft_etcd_test.go:498-557 TestLeaderElectionOverwriteNewerLogs. Node 1 wins
# with an uncommitted entry in its log: that promotion is the host's.
def kat_leader_election_overwrite_newer_logs(backend):
    ids = [1, 2, 3, 4, 5]
    recs = node_records(ids, set(ids))
    with_log(recs[0:1], [1], term=1)
    with_log(recs[1:2], [1], term=1)
    with_log(recs[2:3], [2], term=2)
    recs[3:5]["term"], recs[3:5]["vote"] = 2, 3
    net = Net(backend, ids, records=recs)
    _election(net, 1)
    st = net.state(1)
    assert (int(st["state"]), int(st["term"])) == (abi.FOLLOWER, 2)
    _election(net, 1)
    st = net.state(1)
    assert (int(st["state"]), int(st["term"])) == (abi.LEADER, 3)
    for nid in ids:
        st = net.state(nid)
        runs = [(int(st["run_start"][k]), int(st["run_term"][k])) for k in range(int(st["n_runs"]))]
        assert int(st["last_index"]) == 2 and runs[-2:] == [(1, 1), (2, 3)], (nid, runs)
    r = net.ls.stats["esc_reasons"]
    assert r.get("election", 0) == 0 and r.get("unsupported", 0) == 1, r
    net.close()


def test_leader_election_overwrite_newer_logs():
    kat_leader_election_overwrite_newer_logs(BE)


# ---- raft_etcd_test.go:1740-1810 TestFreeStuckCandidateWithCheckQuorum
def kat_free_stuck_candidate_with_check_quorum(backend):
    recs = node_records([1, 2, 3], {1, 2, 3}, check_quorum=True)
    recs[1]["randomized_election_timeout"] = 11
    net = Net(backend, [1, 2, 3], records=recs)
    net.tick(2, 10)
    _election(net, 1)
    net.isolate(1)
    _election(net, 3)
    b, c = net.state(2), net.state(3)
    assert int(b["state"]) == abi.FOLLOWER and int(c["state"]) == abi.CANDIDATE
    assert int(c["term"]) == int(b["term"]) + 1
    _election(net, 3)
    b, c = net.state(2), net.state(3)
    assert int(b["state"]) == abi.FOLLOWER and int(c["state"]) == abi.CANDIDATE
    assert int(c["term"]) == int(b["term"]) + 2
    net.recover()
    net.send(net.msg(1, 3, abi.HEARTBEAT, term=int(net.state(1)["term"])))
    a, c = net.state(1), net.state(3)
    assert int(a["state"]) == abi.FOLLOWER and int(a["term"]) == int(c["term"])
    _election(net, 3)
    assert int(net.state(3)["state"]) == abi.LEADER
    _no_host_elections(net)
    net.close()


def test_free_stuck_candidate_with_check_quorum():
    kat_free_stuck_candidate_with_check_quorum(BE)


# ---- raft_etcd_test.go:136-151 TestLeaderTransferToUpToDateNode (TimeoutNow)
def kat_leader_transfer_to_up_to_date_node(backend):
    net = Net(backend, [1, 2, 3])
    _election(net, 1)
    assert int(net.state(1)["leader_id"]) == 1
    net.send(net.msg(2, 1, abi.LEADER_TRANSFER, hint=2))
    st = net.state(1)
    assert (int(st["state"]), int(st["leader_id"])) == (abi.FOLLOWER, 2)
    net.send(net.msg(1, 1, abi.PROPOSE, entries=1))
    net.send(net.msg(1, 2, abi.LEADER_TRANSFER, hint=1))
    st = net.state(1)
    assert (int(st["state"]), int(st["leader_id"])) == (abi.LEADER, 1)
    _no_host_elections(net)
    net.close()


def test_leader_transfer_to_up_to_date_node():
    kat_leader_transfer_to_up_to_date_node(BE)


# ---- raft_etcd_test.go:961-969 TestSingleNodeCandidate: becomeCandidate and
# becomeLeader in one item need two draws, so this campaign is the host's
def test_single_node_candidate():
    net = Net(BE, [1])
    _election(net, 1)
    assert int(net.state(1)["state"]) == abi.LEADER
    assert net.ls.stats["esc_reasons"] == {"election": 1}
    net.close()


# ---------------------------------------------------------------- cold start
@pytest.mark.parametrize("R,check_quorum,seed", [(3, False, 11), (5, False, 12), (3, True, 13)])
def test_cold_start(R, check_quorum, seed):
    G = 70
    stats, elected, final = EC.cold_start(BE, G, R, seed, check_quorum=check_quorum)
    EC.assert_cold_start(stats, elected, final, G, R)


def test_cold_start_elections_off_escalates():
    """The same run through the default host lane: every campaign goes to the host."""
    stats, elected, final = EC.cold_start(SIM.HostlaneBackend, 70, 3, 11)
    assert stats["esc_reasons"].get("election", 0) >= 70


# ---------------------------------------------------------------- promotion with uncommitted entries
def test_promotion_with_uncommitted_entries_is_the_hosts():
    """A candidate whose log ends past its commit point wins: the device cannot
    rule out a pending config change (getPendingConfigChangeCount, raft.go:903-917),
    so the deciding RequestVoteResp escalates UNSUPPORTED at that item and the
    items before it stand (Lockstep compares the prefix with the oracle)."""
    peers = node_records([1, 2, 3], {1, 2, 3})[:1]
    with_log(peers, [1], term=1, committed=0)
    ls = SIM.Lockstep(BE, peers, 3)
    try:
        m = np.zeros(1, abi.MESSAGE)
        m["peer"], m["slot"], m["type"] = 0, 0, abi.ELECTION
        _, res = ls.step(m, None)  # the campaign itself runs on the device
        assert not res["escalation"].any() and int(ls.eng.sync()[0]["state"]) == abi.CANDIDATE
        m = np.zeros(2, abi.MESSAGE)
        m["peer"], m["type"], m["term"] = 0, abi.REQUEST_VOTE_RESP, 2
        m["slot"] = [1, 2]
        m["reject"] = [1, 0]  # item 0: a rejection, recorded on the device; item 1 wins
        _, res = ls.step(m, None)
        assert int(res[0]["escalation"]) == abi.ESC_NAMES.index("unsupported") and int(res[0]["esc_item"]) == 1
        assert int(ls.export()[0]["state"]) == abi.LEADER  # the host finished the pass
    finally:
        ls.close()


# ---------------------------------------------------------------- candidate reload guard
def test_candidate_reload_guard_reports_a_lost_tally():
    peers = node_records([1, 2, 3, 4, 5], {1, 2, 3, 4, 5})[:1]
    peers["state"], peers["term"], peers["vote"] = abi.CANDIDATE, 1, 1
    be = BE(peers, 5)
    m = np.zeros(1, abi.MESSAGE)
    m["peer"], m["slot"], m["type"], m["term"] = 0, 1, abi.REQUEST_VOTE_RESP, 1
    be.step(m, np.zeros(0, abi.LOCAL))
    assert int(be.sync().view(abi.PEER_VOTES)[0]["votes_granted"]) == 0b11
    with pytest.raises(EC.TallyLost, match="device tally holds remote votes"):
        be.load(np.array([0]), peers)
    # a record of a later campaign starts a fresh tally: nothing is lost
    later = peers.copy()
    later["term"] = 2
    be.load(np.array([0]), later)


def crafted_candidate_messages(backend):
    """A candidate's handlers the network tests do not reach: a Replicate at its
    own term (handleCandidateReplicate, raft.go:1433-1437) and a RequestVoteResp
    from an observer (:1450-1454). Node 1 of voters {1, 2} and observer 3."""
    peers = node_records([1, 2, 3], {1, 2}, copies=2)[:2]
    ls = SIM.Lockstep(backend, peers, 3)
    try:
        m = np.zeros(2, abi.MESSAGE)
        m["peer"], m["slot"], m["type"] = [0, 1], 0, abi.ELECTION
        _, res = ls.step(m, None)
        assert not res["escalation"].any()
        m = np.zeros(2, abi.MESSAGE)
        m["peer"], m["term"] = [0, 1], 1
        m["slot"] = [1, 2]
        m["type"] = [abi.REPLICATE, abi.REQUEST_VOTE_RESP]
        _, res = ls.step(m, None)
        assert not res["escalation"].any()
        st = ls.eng.sync().view(abi.PEER_VOTES)
        assert (int(st[0]["state"]), int(st[0]["leader_id"])) == (abi.FOLLOWER, 2)
        assert (int(st[1]["state"]), int(st[1]["votes_granted"])) == (abi.CANDIDATE, 0b001)
    finally:
        ls.close()


def test_crafted_candidate_messages():
    crafted_candidate_messages(BE)

"""Elections on the device, on the GPU (-m gpu): the kernels against the oracle,
bit-exact after every pass, with GR_ELECTIONS=1 set for the engines the existing
harnesses create (simulate.Lockstep over gr_step, devsim.DeviceLockstep over the
device-resident split schedule, network.Net)."""
import numpy as np
import pytest

from dragonboat_amd import abi
import elections_common as EC
import simulate as SIM
import test_elections_hostlane as H

pytestmark = pytest.mark.gpu


@pytest.fixture
def elect(gpu, monkeypatch):
    monkeypatch.setenv("GR_ELECTIONS", "1")


def _check_promotions(ls, k, before, res):
    """Engine.promotions() after a pass: exactly the peers whose device state
    turned leader in it, each with the empty entry's index = its last_index."""
    after = ls.eng.sync()
    turned = (before["state"] != abi.LEADER) & (after["state"] == abi.LEADER)
    pr = ls.eng.eng.promotions()
    assert sorted(pr["peer"].tolist()) == np.nonzero(turned)[0].tolist(), f"pass {k}"
    p = pr["peer"].astype(np.int64)
    assert np.all(pr["noop_index"] == after["last_index"][p]) and np.all(pr["term"] == after["term"][p]), f"pass {k}"
    ls.promoted = getattr(ls, "promoted", 0) + len(pr)


# ---- cold start through gr_step (the fused small kernel)
@pytest.mark.parametrize("G,R,seed", [(70, 3, 11), (64, 5, 12)])
def test_cold_start_gr_step(elect, G, R, seed):
    seen = []
    def after(ls, k, before, res):
        _check_promotions(ls, k, before, res)
        seen.append(ls.promoted)
    stats, elected, final = EC.cold_start(SIM.GpuBackend, G, R, seed, after_pass=after)
    EC.assert_cold_start(stats, elected, final, G, R)
    assert seen[-1] >= G  # every group's leader was promoted on the device


# ---- feature off: the same cold start hands every campaign to the host, as before
def test_cold_start_elections_off(gpu, monkeypatch):
    monkeypatch.delenv("GR_ELECTIONS", raising=False)
    stats, elected, final = EC.cold_start(SIM.GpuBackend, 70, 3, 11, passes=30, propose_passes=0)
    assert stats["esc_reasons"].get("election", 0) >= 70, stats["esc_reasons"]


# ---- cold start on the split schedule: the steady kernel's listing, the tick
# kernel's hand-over at the election timeout, and gr_step_kernel
@pytest.mark.parametrize("G", [200, 320])  # route_wu = 0 / 1 (320 % 64 == 0)
def test_cold_start_split_schedule(elect, monkeypatch, G):
    from dragonboat_amd import populations as P
    import devsim
    monkeypatch.setenv("GR_SMALL_BLOCKS", "0")
    monkeypatch.setenv("GR_SPLIT_MIN_LANES", "1")
    R, seed = 3, 21
    ds = devsim.DeviceLockstep(EC.cold_peers(G, R, seed), G, R)
    try:
        assert ds.eng.get_elections()
        promoted = 0
        for k in range(40):
            ds.step(P.propose_locals(R * G, np.zeros(0, np.int64), seed=seed, pass_index=k, ticks=1))
            promoted += len(ds.eng.promotions())
        st = ds.export()
        nl = EC.leaders_per_group(st, G, R)
        # 40 passes cover every first timeout (at most 20 ticks), the vote round
        # trip and, with this seed, the second round of the groups whose first split
        assert np.all(nl == 1), np.nonzero(nl != 1)[0][:8]
        assert promoted >= G
        r = ds.stats["esc_reasons"]
        assert r.get("election", 0) == 0 and r.get("unsupported", 0) == 0, r
    finally:
        ds.close()


# ---- one network KAT on the device: raft_etcd_test.go:781-844 TestDuelingCandidates
def test_dueling_candidates_gpu(elect):
    H.dueling_candidates(SIM.GpuBackend)


# ---- the vote bytes cross the boundary
def test_vote_bytes_round_trip(gpu):
    from dragonboat_amd.engine import Engine
    from network import node_records
    peers = node_records([1, 2, 3, 4, 5], {1, 2, 3, 4, 5})  # five records, self slots 0..4
    peers["term"] = 3
    peers["state"][:3] = abi.CANDIDATE
    peers["vote"][:3] = peers["node_id"][:3]
    v = peers.view(abi.PEER_VOTES)  # the tally bytes by name, in place
    v["votes_granted"] = [0b00100, 0b10000, 0, 0b00110, 0b11111]
    v["votes_rejected"] = [0b01000, 0, 0, 0b01000, 0b11111]
    peers["state"][4], peers["leader_id"][4] = abi.LEADER, 5
    eng = Engine(5, 5)
    try:
        eng.load(peers)
        got = eng.sync(5).view(abi.PEER_VOTES)
    finally:
        eng.close()
    # candidates keep their bytes, with their own granted bit ORed in
    assert got["votes_granted"][:3].tolist() == [0b00101, 0b10010, 0b00100]
    assert got["votes_rejected"][:3].tolist() == [0b01000, 0, 0]
    # any other state exports 0
    assert got["votes_granted"][3:].tolist() == [0, 0] and got["votes_rejected"][3:].tolist() == [0, 0]
    assert not got["read_index"]["ack_bits"].any() and not got["read_index_count"].any()


# ---- the election coverage table: every new id reached on the device, no BAD_* id hit
def test_election_coverage(elect):
    import ctypes
    from dragonboat_amd import build
    from dragonboat_amd.engine import load_library
    lib = load_library(build.COVER_LIB)

    class Cover(SIM.GpuBackend):
        lib_path = build.COVER_LIB

    def read(fn_read, fn_names):
        names = [n for n in fn_names().decode().split(",") if n]
        buf = (ctypes.c_uint64 * len(names))()
        assert fn_read(buf, len(names)) == len(names)
        return dict(zip(names, list(buf)))

    e0 = read(lib.gr_coverage_elect_read, lib.gr_coverage_elect_names)
    b0 = read(lib.gr_coverage_read, lib.gr_coverage_names)
    EC.cold_start(Cover, 70, 3, 11, passes=45, propose_passes=2)
    H.dueling_candidates(Cover)
    H.kat_candidate_concede(Cover)
    H.kat_leader_election_overwrite_newer_logs(Cover)
    H.kat_free_stuck_candidate_with_check_quorum(Cover)
    H.kat_leader_transfer_to_up_to_date_node(Cover)
    H.crafted_candidate_messages(Cover)
    e1 = read(lib.gr_coverage_elect_read, lib.gr_coverage_elect_names)
    b1 = read(lib.gr_coverage_read, lib.gr_coverage_names)
    missed = [n for n in e1 if e1[n] == e0[n]]
    assert not missed, missed
    bad = {n: b1[n] - b0[n] for n in b1 if n.startswith("BAD_") and b1[n] != b0[n]}
    assert not bad, bad

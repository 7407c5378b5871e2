"""The steady kernel's per-wave stats (gr_kernels.h steady_stats): the device
counters of every pass against the same totals counted from the oracle's
messages and states.

The steady lanes sum their counters as bit planes (one ballot per bit) instead
of block_stats' nine butterflies; the role instances, the tick and the general
kernels keep block_stats. The reference is independent of both: what the oracle
delivered, sent and committed in the pass. Split schedule as test_commit_lag.py
sets it, oracle parity of state, mailboxes and results after every pass
(devsim.DeviceLockstep.step asserts it).

Shapes (groups per replica block, R = 3): 64: every workgroup holds waves of
two roles and the last one a half-empty wave; 128: whole waves; 192: an odd
block count, as the headline has; 130: replica blocks that do not start on a
wave, so steady waves hold lanes of two roles' neighbours and the closed form
leaves some of them to FastLane."""
import numpy as np
import pytest

from dragonboat_amd import abi, populations as P
from test_commit_lag import _DevDriver, _peers, _split

FIELDS = ("leader_commits", "follower_commits", "escalations", "msgs_in", "msgs_out", "leader_msgs_in",
          "leader_msgs_out", "replicate_entries")


def _expected(inbox, sent, before, after):
    """One pass's totals from the oracle's side: inbox = the messages delivered,
    sent = the messages the pass produced (as the next inbox), states before and
    after. Leaders send Replicates and receive ReplicateResps; the followers the
    reverse (steady passes carry nothing else)."""
    adv = after["committed"] > before["committed"]
    lead = after["state"] == abi.LEADER
    rep_in = inbox["type"] == abi.REPLICATE
    assert np.all(np.isin(inbox["type"], (abi.REPLICATE, abi.REPLICATE_RESP)))
    assert np.all(np.isin(sent["type"], (abi.REPLICATE, abi.REPLICATE_RESP)))
    return {"leader_commits": int((adv & lead).sum()), "follower_commits": int((adv & ~lead).sum()),
            "escalations": 0, "msgs_in": len(inbox), "msgs_out": len(sent),
            "leader_msgs_in": int((~rep_in).sum()), "leader_msgs_out": int((sent["type"] == abi.REPLICATE).sum()),
            "replicate_entries": int(inbox["n_entries"][rep_in].sum())}


def _run(G, proposers, passes=10, entries=None, lib_path=None):
    """proposers(k) -> the leader slots proposing in pass k; entries(k) -> the
    per-proposer entry count (default 1)."""
    R = 3
    drv = _DevDriver(_peers(G, R, 11), G, R, lib_path=lib_path)
    try:
        eng = drv.ls.eng
        total = {f: 0 for f in FIELDS}
        for k in range(passes):
            inbox = drv.ls.msgs.copy()
            before = drv.export().copy()
            s0 = eng.stats()
            loc = P.propose_locals(R * G, proposers(k), entries=1 if entries is None else entries(k), pass_index=k)
            drv.step(loc)
            s1 = eng.stats()
            want = _expected(inbox, drv.ls.msgs, before, drv.export())
            got = {f: s1[f] - s0[f] for f in FIELDS}
            print("pass", k, got)
            assert got == want, (k, got, want)
            for f in FIELDS:
                total[f] += got[f]
        assert drv.escalations == 0
        return total
    finally:
        drv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("G", [64, 128, 192, 130])
def test_steady_passes_stats_match_oracle(gpu, monkeypatch, G):
    """Ten steady passes, a proposal per leader per pass: from the fourth pass
    on every leader commits and both followers commit in every pass."""
    _split(monkeypatch)
    t = _run(G, lambda k: np.arange(G))
    assert t["leader_commits"] >= 6 * G and t["follower_commits"] >= 2 * 6 * G
    assert t["leader_msgs_in"] > 0 and t["replicate_entries"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("G", [128, 192])
def test_odd_groups_only_stats_match_oracle(gpu, monkeypatch, G):
    """Only odd groups propose, then nobody: waves whose lanes differ in every
    counter (0 or 1 commits, 0 to 4 acks, 0 to 2 Replicates out), then idle
    lanes that count nothing."""
    _split(monkeypatch)
    t = _run(G, lambda k: np.arange(1, G, 2) if k < 7 else np.zeros(0, np.int64))
    assert 0 < t["leader_commits"] <= 7 * (G // 2)


@pytest.mark.gpu
@pytest.mark.parametrize("G", [128, 192])
def test_two_entry_proposals_stats_match_oracle(gpu, monkeypatch, G):
    """Every third leader proposes two entries in some passes: the closed form
    takes one proposal of one entry at most, so those lanes of a steady wave go
    to FastLane (block_stats in the role instances) while their wave-mates are
    counted by the steady kernel; the row totals are the sum of both."""
    _split(monkeypatch)
    two = np.arange(0, G, 3)

    def proposers(k):
        return two if k in (4, 5, 7) else np.arange(G)

    def entries(k):
        return 2 if k in (4, 5, 7) else 1
    t = _run(G, proposers, entries=entries)
    assert t["replicate_entries"] > 0


@pytest.mark.gpu
def test_checked_build_counts_no_lane_outside_the_bit_planes(gpu, monkeypatch):
    """The GR_COVERAGE build: both closed forms run, the totals match, and no
    finished lane counted more than the bit planes hold
    (BAD_STEADY_STATS_RANGE, gr_steady.h kSteady*Bits)."""
    import ctypes
    from dragonboat_amd import build
    from dragonboat_amd.engine import load_library
    _split(monkeypatch)
    lib = load_library(build.COVER_LIB)
    names = [x for x in lib.gr_coverage_names().decode().split(",") if x]
    assert "BAD_STEADY_STATS_RANGE" in names
    before, after = np.zeros(len(names), np.uint64), np.zeros(len(names), np.uint64)
    assert lib.gr_coverage_read(before.ctypes.data_as(ctypes.c_void_p), len(names)) == len(names)
    _run(192, lambda k: np.arange(192) if k != 6 else np.arange(0, 192, 2), lib_path=build.COVER_LIB)
    lib.gr_coverage_read(after.ctypes.data_as(ctypes.c_void_p), len(names))
    hits = dict(zip(names, (after - before).tolist()))
    bad = {x: h for x, h in hits.items() if x.startswith("BAD_") and h}
    assert not bad, bad
    assert hits["STEADY_LEADER"] > 0 and hits["STEADY_FOLLOWER"] > 0, hits

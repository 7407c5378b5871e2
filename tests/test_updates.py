"""gr_update_class, the host form of the rule gr_collect_updates runs on the
device (gr_host.h update_class), against the Python restatement of
Peer.HasUpdate in tests/updates_common.py. No GPU: the function takes records.
Struct layouts and exports are covered by tests/test_abi.py."""
import numpy as np
import pytest

from dragonboat_amd import abi
from dragonboat_amd.engine import update_class
import updates_common as UC

U = np.uint64
FLAG_SETS = [0, UC.MORE, UC.EVERY, UC.MORE | UC.EVERY]


def _random_cases(n, seed):
    """Result records, (log_applied, first_index_m1) and update states around the
    rule's edges: fields are drawn from a few values close to each other so that
    every comparison of the rule goes both ways often."""
    rng = np.random.default_rng(seed)
    res = np.zeros(n, abi.RESULT)
    prev = np.zeros(n, abi.UPDATE_STATE)
    base = rng.choice(np.array([0, 1, 5, 2**32 - 1, 2**32, 2**40, 2**63], U), n)
    last = base + rng.integers(0, 4, n).astype(U)
    res["peer"] = np.arange(n)
    res["last_index"] = last
    # committed: at, just below, far below (commit_lag >= 2^32) or above last_index
    lag = rng.choice(np.array([0, 1, 2, 6, 7, 2**32 - 1, 2**32, 2**33], U), n)
    res["committed"] = np.where(lag <= last, last - lag, last)
    above = rng.random(n) < 0.03
    res["committed"] = np.where(above, last + U(1), res["committed"])
    # save_from through inMemory.entriesToSave, the wrapping marker test included:
    # 0..300 entries to save (255 and 256 are the compact record's edge)
    cnt = rng.choice(np.array([0, 0, 1, 2, 254, 255, 256, 300], U), n)
    cnt = np.minimum(cnt, last)
    saved_to = last - cnt
    marker = np.where(rng.random(n) < 0.2, saved_to + U(2) + rng.integers(0, 3, n).astype(U),  # idx - marker wraps
                      saved_to + U(1) - np.minimum(rng.integers(0, 3, n).astype(U), saved_to + U(1)))
    res["save_from"] = UC.ref_save_from(saved_to, marker, last)
    res["term"] = rng.choice(np.array([0, 1, 2, 2**32 + 1], U), n)
    res["vote"] = rng.choice(np.array([0, 1, 3], U), n)
    empty = rng.random(n) < 0.1  # the empty State, with every kind of prev
    for f in ("term", "vote", "committed"):
        res[f] = np.where(empty, U(0), res[f])
    same = rng.random(n) < 0.6  # prev equal to State, or off in one field
    prev["term"] = np.where(same, res["term"], rng.choice(np.array([0, 1, 2], U), n))
    prev["vote"] = np.where(same | (rng.random(n) < 0.5), res["vote"], rng.choice(np.array([0, 1, 3], U), n))
    prev["commit"] = np.where(same | (rng.random(n) < 0.5), res["committed"], res["committed"] - U(1))
    quiet = rng.random(n) < 0.7  # per-pass fields mostly clear
    res["escalation"] = np.where(quiet, 0, rng.integers(0, 13, n))
    res["propose_result"] = np.where(rng.random(n) < 0.7, 0, rng.integers(0, 4, n))
    res["n_ready"] = np.where(rng.random(n) < 0.85, 0, rng.integers(0, abi.GR_Q + 1, n))
    res["n_forwarded"] = np.where(rng.random(n) < 0.85, 0, rng.integers(0, 4, n))
    # applied / firstIndex-1 at, below and above committed (committed at or below first_index_m1)
    c = res["committed"]
    la = np.where(rng.random(n) < 0.5, c, c - np.minimum(rng.integers(0, 3, n).astype(U), c))
    la = np.where(rng.random(n) < 0.1, c + U(1), la)
    lo = np.where(rng.random(n) < 0.3, c + rng.integers(0, 2, n).astype(U), la - np.minimum(U(1), la))
    wrap = rng.random(n) < 0.02  # applied + 1 wraps to 0 in Go as well
    la = np.where(wrap, U(2**64 - 1), la)
    return res, la, lo, prev


@pytest.mark.parametrize("flags", FLAG_SETS)
def test_update_class_matches_restatement(built, flags):
    n = 20_000
    res, la, lo, prev = _random_cases(n, seed=40 + flags)
    want = UC.ref_classes(res, la, lo, prev, flags)
    got = update_class(res, la, lo, prev, more_to_apply=bool(flags & UC.MORE), every=bool(flags & UC.EVERY))
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(int(k), int(got[k]), int(want[k]), res[k], int(la[k]), int(lo[k]), prev[k])
                           for k in bad[:3]]
    # the cases do reach every class and every corner they are meant to
    if not flags & UC.EVERY:
        assert {0, 1, 2} <= set(want.tolist())
    assert np.any((res["last_index"] - res["committed"] >= U(2**32)) & (res["committed"] <= res["last_index"]))
    save = np.where(res["save_from"] != 0, res["last_index"] - res["save_from"] + U(1), U(0))
    assert np.any(save == 255) and np.any(save == 256)
    assert np.any((res["term"] == 0) & (res["vote"] == 0) & (res["committed"] == 0) & (prev["term"] != 0))
    assert np.any(res["committed"] <= lo)


def _one(**kw):
    r = np.zeros(1, abi.RESULT)
    for k, v in kw.items():
        r[k] = v
    return r


def test_update_class_corners(built):
    """Each condition and each EXT rule on its own, on a peer that is otherwise quiet:
    State {term 3, vote 1, commit 100} equal to prev, nothing to save or apply."""
    quiet = dict(term=3, vote=1, committed=100, last_index=100)
    prev = np.zeros(1, abi.UPDATE_STATE)
    prev["term"], prev["vote"], prev["commit"] = 3, 1, 100

    def cls(r, la=100, lo=50, p=prev, **fl):
        return int(update_class(r, la, lo, p, **fl)[0])
    assert cls(_one(**quiet)) == abi.UPD_NONE
    assert cls(_one(**quiet), more_to_apply=False) == abi.UPD_NONE
    # each flag on its own
    assert cls(_one(**quiet), more_to_apply=False, every=True) == abi.UPD_COMPACT
    assert cls(_one(**quiet), la=99, more_to_apply=False) == abi.UPD_NONE
    assert cls(_one(**quiet), la=99, more_to_apply=True) == abi.UPD_COMPACT
    # committed at or below first_index_m1: nothing to apply whatever applied says
    assert cls(_one(**quiet), la=10, lo=100) == abi.UPD_NONE
    assert cls(_one(**quiet), la=10, lo=99) == abi.UPD_COMPACT
    # State changed: commit alone is compact, term or vote is EXT
    assert cls(_one(**dict(quiet, committed=99)), la=99) == abi.UPD_COMPACT
    assert cls(_one(**dict(quiet, term=4))) == abi.UPD_EXT
    assert cls(_one(**dict(quiet, vote=2))) == abi.UPD_EXT
    # the empty State never counts as changed, and a new node's prev is empty
    zero = np.zeros(1, abi.UPDATE_STATE)
    assert cls(_one(), la=0, lo=0) == abi.UPD_NONE
    assert cls(_one(), la=0, lo=0, p=zero) == abi.UPD_NONE
    assert cls(_one(**quiet), p=zero) == abi.UPD_EXT
    # entries to save; 255 fit the compact record, 256 do not
    assert cls(_one(**dict(quiet, last_index=101, save_from=101))) == abi.UPD_COMPACT
    assert cls(_one(**dict(quiet, last_index=354, save_from=100))) == abi.UPD_COMPACT
    assert cls(_one(**dict(quiet, last_index=355, save_from=100))) == abi.UPD_EXT
    # commit_lag at 2^32 needs the full record
    big = dict(quiet, committed=100, last_index=100 + 2**32 - 1, save_from=100 + 2**32 - 1)
    assert cls(_one(**big)) == abi.UPD_COMPACT
    big = dict(quiet, committed=100, last_index=100 + 2**32, save_from=100 + 2**32)
    assert cls(_one(**big)) == abi.UPD_EXT
    # ready to read, the engine's conditions
    assert cls(_one(**dict(quiet, n_ready=1))) == abi.UPD_EXT
    assert cls(_one(**dict(quiet, n_forwarded=1))) == abi.UPD_EXT
    assert cls(_one(**dict(quiet, escalation=6))) == abi.UPD_EXT
    assert cls(_one(**dict(quiet, propose_result=abi.PROP_DROPPED))) == abi.UPD_COMPACT


def test_update_class_refuses_unknown_flags(built):
    from dragonboat_amd.engine import load_library
    lib = load_library()
    r, p = _one(), np.zeros(1, abi.UPDATE_STATE)
    assert lib.gr_update_class(r.ctypes.data, 0, 0, p.ctypes.data, 4) == -1
    assert lib.gr_update_class(None, 0, 0, p.ctypes.data, 0) == -1
    assert lib.gr_update_class(r.ctypes.data, 0, 0, None, 0) == -1
    assert lib.gr_update_class(r.ctypes.data, 0, 0, p.ctypes.data, 3) == abi.UPD_COMPACT


def test_expand_updates_follows_cresult_rules():
    from dragonboat_amd.engine import expand_updates
    cr = np.zeros(3, abi.CRESULT)
    cr["peer"] = [2, 5, 7]
    cr["last_index"] = [10, 2**32 + 9, 40]
    cr["commit_lag"] = [2, 0, 0]
    cr["save_count"] = [0, 3, 0]
    cr["propose_result"] = [0, abi.PROP_APPENDED, 0]
    cr["flags"][2], cr["aux"][2] = abi.CR_EXT, 0
    rx = np.zeros(1, abi.RESULT)
    rx["peer"], rx["term"], rx["n_ready"] = 7, 9, 2
    term, vote, prop = np.arange(8) + 100, np.arange(8) + 200, np.full(8, 2)
    res = expand_updates(cr, rx, term, vote, prop)
    assert res["committed"].tolist() == [8, 2**32 + 9, 0] and res["save_from"].tolist() == [0, 2**32 + 7, 0]
    assert res["term"].tolist() == [102, 105, 9] and res["vote"].tolist() == [202, 205, 0]
    assert res["propose_first"].tolist() == [0, 2**32 + 8, 0] and res["n_ready"].tolist() == [0, 0, 2]


# The cold start of tests/test_elections_gpu.py (elections_common.cold_peers(G, 3,
# 21), 40 passes of one tick) through the oracle alone, the rule over its records,
# the reported peers committed after every pass: reported peers and ext records
# per pass. tests/test_updates_switches_gpu.py requires the same of the device.
COLD_REPORTED = {
    200: [600, 21, 49, 72, 99, 160, 179, 207, 197, 213, 177, 146, 101, 76, 47, 23, 15, 3, 3, 2, 0, 0, 0, 0, 0, 0, 1, 2,
          1, 2, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0],
    320: [960, 42, 70, 120, 164, 220, 265, 308, 320, 317, 306, 241, 204, 123, 94, 34, 19, 8, 5, 2, 0, 1, 2, 1, 2, 1, 2,
          0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]}
COLD_EXT = {
    200: [4, 21, 45, 51, 50, 90, 84, 71, 60, 56, 28, 21, 10, 1, 6, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 0,
          0, 0, 0, 0, 0, 0, 0],
    320: [12, 42, 58, 79, 94, 100, 113, 129, 113, 92, 78, 25, 13, 6, 4, 2, 0, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0,
          0, 0, 0, 0, 0, 0, 0, 0, 0]}


def cold_locals(G, k):
    from dragonboat_amd import populations as P
    return P.propose_locals(3 * G, np.zeros(0, np.int64), seed=21, pass_index=k, ticks=1)


@pytest.mark.parametrize("G", [200, 320])
def test_cold_start_counts_of_the_oracle(built, G):
    """What the device's collects are held to in test_updates_switches_gpu.py,
    of the reference alone: the counts per pass, a pass that reports nothing and
    one that reports more than a quarter of the peers. Pass 0 reports every peer
    (the loaded groups have entries to apply); the update states are the loaded
    State, so only the peers whose term moves in it are EXT."""
    import elections_common as EC
    counts = UC.oracle_collect_counts(EC.cold_peers(G, 3, 21), G, 3, 40, lambda k: cold_locals(G, k))
    assert [c[0] for c in counts] == COLD_REPORTED[G] and [c[1] for c in counts] == COLD_EXT[G]
    assert 0 in COLD_REPORTED[G][1:] and max(COLD_REPORTED[G][1:]) > 3 * G // 4

"""Config-change entries on the device (gpuraft.h gr_set_config_entries): a
config change proposed, replicated with its marks, merged and truncated on a
follower, and counted at a promotion over uncommitted entries.

Every case runs on two backends, the host lane built with config entries
compiled on (`not gpu`) and the engine with the switch on (`-m gpu`), beside the
reference side: the oracle's raft object built from the same records, with the
in-memory entries at the recorded indexes typed ConfigChangeEntry, driven through
the same items (config_entries_common.py, tests/native/config_entries_ref.cpp).
After every pass the peer records, the gr_cc_index records, the messages and the
results must agree field for field (stale record values and marks at or below a
message's commit compare as 0); an escalation must be the one the case names and
leave exactly the items below it applied. With the switch off the escalations
and the bytes are what they always were.
"""
import ctypes

import numpy as np
import pytest

from dragonboat_amd import abi
import config_entries_common as C
from test_config_change import _group, _member

BACKENDS = [pytest.param("cpu", id="host"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
VOTER = abi.SLOT_VOTER
REQUEST_VOTE_RESP = 15
HEARTBEAT_RESP = 18


@pytest.fixture(autouse=True)
def _no_env_switch(monkeypatch):
    monkeypatch.delenv("GR_CONFIG_ENTRIES", raising=False)
    monkeypatch.delenv("GR_ELECTIONS", raising=False)


def _need(be, request):
    request.getfixturevalue("gpu" if be == "gpu" else "built")


def _peer(S, self_id, state, matches, committed=8, term=5, leader_id=1, flags=0):
    """A peer of voters 1..3 with the log 1..10 at term 5, every uncommitted
    entry in memory (marker_index = committed + 1), everything saved."""
    p = _group(S, self_id, state, matches, committed=committed, term=term, leader_id=leader_id)
    g = p[0]
    g["marker_index"], g["saved_to"], g["log_applied"] = committed + 1, g["last_index"], committed
    g["flags"] |= flags
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


def _fwd_cc(slot, ents=1):
    """A forwarded Propose holding a ConfigChangeEntry, as Lane::propose forwards it."""
    return _msg(abi.PROPOSE, slot, 0, reject=1, ents=ents)


def _rec(cc):
    return int(cc[0]["last"]), int(cc[0]["prev"])


def _marks(out, slot):
    m = out[(out["slot"] == slot) & (out["type"] == abi.REPLICATE)]
    return [(int(x["reject"]), int(x["hint"]), int(x["hint_high"]), int(x["log_index"]), int(x["n_entries"])) for x in m]


def _leader(S, flags=0):
    return _peer(S, 1, abi.LEADER, [10, 8, 8], flags=flags)


# ---------------------------------------------------------------- 1. propose
def scn_propose(be, S=3, **kw):
    side = C.Side(be, _leader(S), S, **kw)
    st, out, res, cc = side.step(loc=_loc(propose=1, cc=1))
    assert int(res[0]["propose_result"]) == abi.PROP_APPENDED and int(res[0]["propose_first"]) == 11
    assert int(st[0]["flags"]) & C.PENDING and int(st[0]["last_index"]) == 11
    assert _rec(cc) == (11, 0)
    # followers in Replicate state at next = 11: the new entry alone, marked
    assert _marks(out, 1) == [(1, 11, 0, 10, 1)] and _marks(out, 2) == [(1, 11, 0, 10, 1)]
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_propose(be, S, request):
    """A CC proposal is appended on the device: flag set, record (hi, 0), both
    Replicates marked."""
    _need(be, request)
    scn_propose(be, S)


@pytest.mark.parametrize("be", BACKENDS)
def test_propose_switch_off(be, request):
    """The same input with the switch off escalates config_change, as ever."""
    _need(be, request)
    side = C.Side(be, _leader(3), 3, on=False)
    st, cc, out, res = side.raw(loc=_loc(propose=1, cc=1))
    assert int(res[0]["escalation"]) == C.ESC["config_change"] and int(res[0]["esc_item"]) == 0
    assert int(st[0]["last_index"]) == 10 and not int(st[0]["flags"]) & C.PENDING and len(out) == 0
    side.close()


# ---------------------------------------------------------------- 2. still escalates
def scn_still_escalates(be, S=3, **kw):
    # a CC proposal while one is pending
    side = C.Side(be, _leader(S, flags=C.PENDING), S, C.cc_recs(1, 10), **kw)
    st, _, res, cc = side.step(loc=_loc(propose=1, cc=1), esc={0: "config_change"})
    assert int(res[0]["esc_item"]) == 0 and int(st[0]["last_index"]) == 10 and _rec(cc) == (10, 0)
    side.close()
    # a CC in a two-entry batch
    side = C.Side(be, _leader(S), S, **kw)
    st, _, _, cc = side.step(loc=_loc(propose=2, cc=1), esc={0: "config_change"})
    assert int(st[0]["last_index"]) == 10 and _rec(cc) == (0, 0)
    side.close()
    # a forwarded CC is taken
    side = C.Side(be, _leader(S), S, **kw)
    st, out, res, cc = side.step(_fwd_cc(1))
    assert int(res[0]["n_forwarded"]) == 1 and int(res[0]["forwarded_entries"]) == 1
    assert int(st[0]["flags"]) & C.PENDING and _rec(cc) == (11, 0) and _marks(out, 2) == [(1, 11, 0, 10, 1)]
    # ... and the next one meets the flag
    st, _, res, cc = side.step(_fwd_cc(2), esc={0: "config_change"})
    assert int(res[0]["esc_item"]) == 0 and int(st[0]["last_index"]) == 11 and _rec(cc) == (11, 0)
    side.close()
    # a forwarded CC in a batch of two
    side = C.Side(be, _leader(S), S, **kw)
    side.step(_fwd_cc(1, ents=2), esc={0: "config_change"})
    side.close()
    # a forwarded CC and a local one in a single pass: the local one escalates
    # at its own item and the prefix stands
    side = C.Side(be, _leader(S), S, **kw)
    st, out, res, cc = side.step(_fwd_cc(1), _loc(propose=1, cc=1), esc={0: "config_change"})
    assert int(res[0]["esc_item"]) == 1 and int(res[0]["n_forwarded"]) == 1
    assert int(st[0]["last_index"]) == 11 and int(st[0]["flags"]) & C.PENDING and _rec(cc) == (11, 0)
    side.close()
    # two forwarded CCs in one pass: the second escalates at its own item
    side = C.Side(be, _leader(S), S, **kw)
    st, _, res, cc = side.step(np.concatenate([_fwd_cc(1), _fwd_cc(2)]), esc={0: "config_change"})
    assert int(res[0]["esc_item"]) == 1 and int(st[0]["last_index"]) == 11 and _rec(cc) == (11, 0)
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
def test_still_escalates(be, request):
    _need(be, request)
    scn_still_escalates(be)


# ---------------------------------------------------------------- 3. follower
def _follower(S, term=5):
    return _peer(S, 2, abi.FOLLOWER, [0, 10, 0], term=term)


def scn_follower(be, S=3, **kw):
    side = C.Side(be, _follower(S), S, **kw)
    # a marked three-entry Replicate is merged
    rep = _msg(abi.REPLICATE, 0, 5, log_index=10, log_term=5, commit=8, reject=1, ents=3, ent_term=5, hint=13,
               hint_high=11)
    st, _, _, cc = side.step(rep)
    assert int(st[0]["last_index"]) == 13 and _rec(cc) == (13, 11)
    # a duplicate changes nothing
    st2, _, _, cc = side.step(rep)
    assert _rec(cc) == (13, 11) and st2.tobytes() == st.tobytes()
    # a reject (no entry 20 here) and an early ack (below committed) merge nothing
    side.step(_msg(abi.REPLICATE, 0, 5, log_index=20, log_term=5, commit=8, reject=1, ents=2, ent_term=5, hint=22))
    assert _rec(side.cc) == (13, 11)
    side.step(_msg(abi.REPLICATE, 0, 5, log_index=5, log_term=5, commit=8, reject=1, ents=2, ent_term=5, hint=7))
    assert _rec(side.cc) == (13, 11)
    side.close()
    # one mark merged above an existing one; a mark at or below the commit is ignored
    side = C.Side(be, _follower(S), S, C.cc_recs(1, 10), **kw)
    _, _, _, cc = side.step(_msg(abi.REPLICATE, 0, 5, log_index=10, log_term=5, commit=8, reject=1, ents=1, ent_term=5,
                                 hint=11))
    assert _rec(cc) == (11, 10)
    side.close()
    side = C.Side(be, _follower(S), S, **kw)
    st, _, _, cc = side.step(_msg(abi.REPLICATE, 0, 5, log_index=8, log_term=5, commit=10, reject=1, ents=3,
                                  ent_term=5, hint=11, hint_high=9))
    assert int(st[0]["committed"]) == 10 and C.norm_cc(cc, st["committed"])[0]["last"] == 11
    assert C.norm_cc(cc, st["committed"])[0]["prev"] == 0
    side.close()
    # a truncating Replicate drops `last`: entry 10 (a config change at term 5)
    # gives way to the new leader's entry at term 6
    trunc = _msg(abi.REPLICATE, 0, 6, log_index=9, log_term=5, commit=8, ents=1, ent_term=6)
    side = C.Side(be, _follower(S, term=6), S, C.cc_recs(1, 10), **kw)
    st, _, res, cc = side.step(trunc)
    assert int(res[0]["append_from"]) == 10 and C.norm_cc(cc, st["committed"]).tobytes() == C.cc_recs(1).tobytes()
    side.close()
    # ... and keeps one below the conflict index
    side = C.Side(be, _follower(S, term=6), S, C.cc_recs(1, 9), **kw)
    _, _, _, cc = side.step(trunc)
    assert _rec(cc) == (9, 0)
    side.close()
    # (last, prev) both above committed: escalates, and the item leaves no trace
    side = C.Side(be, _follower(S, term=6), S, C.cc_recs(1, 10, 9), **kw)
    before = side.state.copy()
    st, out, res, cc = side.step(trunc, esc={0: "config_change"})
    assert int(res[0]["esc_item"]) == 0 and len(out) == 0 and _rec(cc) == (10, 9)
    assert st.tobytes() == before.tobytes()
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_follower(be, S, request):
    _need(be, request)
    scn_follower(be, S)


# ---------------------------------------------------------------- 4. promotion
def _candidate(S):
    """Node 1 campaigns at term 6 over the log 1..10 with committed = 8."""
    p = _peer(S, 1, abi.CANDIDATE, [10, 0, 0], term=6, leader_id=0)
    p[0]["vote"] = 1
    return p


def _win():
    return _msg(REQUEST_VOTE_RESP, 1, 6)


def scn_promotion(be, S=3, **kw):
    # count 0: leader, flag clear, one gr_promotions record
    side = C.Side(be, _candidate(S), S, elect=True, **kw)
    st, out, _, _ = side.step(_win(), _loc())
    assert int(st[0]["state"]) == abi.LEADER and not int(st[0]["flags"]) & C.PENDING and int(st[0]["last_index"]) == 11
    assert _marks(out, 1) == [(0, 0, 0, 10, 1)]  # the empty entry alone, from next = 11
    if be == "gpu":
        pr = side.eng.promotions()
        assert len(pr) == 1 and (int(pr[0]["peer"]), int(pr[0]["term"]), int(pr[0]["noop_index"])) == (0, 6, 11)
    side.close()
    # count 1: the flag is set
    side = C.Side(be, _candidate(S), S, C.cc_recs(1, 10), elect=True, **kw)
    st, _, _, cc = side.step(_win(), _loc())
    assert int(st[0]["state"]) == abi.LEADER and int(st[0]["flags"]) & C.PENDING and _rec(cc) == (10, 0)
    # the follower's reject brings next back to 9: the resend carries the mark
    st, out, _, _ = side.step(_msg(abi.REPLICATE_RESP, 1, 6, log_index=10, reject=1, hint=8))
    assert _marks(out, 1) == [(1, 10, 0, 8, 3)]
    side.close()
    # a stale record counts 0
    side = C.Side(be, _candidate(S), S, C.cc_recs(1, 8, 7), elect=True, **kw)
    st, _, _, _ = side.step(_win(), _loc())
    assert int(st[0]["state"]) == abi.LEADER and not int(st[0]["flags"]) & C.PENDING
    side.close()
    # count 2: the reference panics there
    side = C.Side(be, _candidate(S), S, C.cc_recs(1, 10, 9), elect=True, **kw)
    _, _, _, _, panic = C.ref_step(side.ref, side.cc, _win(), _loc(), S)
    assert int(panic[0]) == 0
    st, _, res, cc = side.step(_win(), _loc(), esc={0: "panic"})
    assert int(res[0]["esc_item"]) == 0 and int(st[0]["state"]) == abi.CANDIDATE and _rec(cc) == (10, 9)
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_promotion(be, S, request):
    _need(be, request)
    scn_promotion(be, S)


@pytest.mark.parametrize("be", BACKENDS)
def test_promotion_switch_off(be, request):
    """The same input with the switch off escalates unsupported, as today."""
    _need(be, request)
    side = C.Side(be, _candidate(3), 3, elect=True, on=False)
    st, _, _, res = side.raw(_win(), _loc())
    assert int(res[0]["escalation"]) == C.ESC["unsupported"] and int(res[0]["esc_item"]) == 0
    assert int(st[0]["state"]) == abi.CANDIDATE
    side.close()


# ---------------------------------------------------------------- 5. resend
def _lagging_leader(S, state2, next2):
    """Node 1 leads with pendingConfigChange set; node 2 (slot 1) lags at match 8."""
    p = _leader(S, flags=C.PENDING)
    _member(p, 1, 2, VOTER, match=8, next_=next2, state=state2, active=1)
    return p


def scn_resend(be, S=3, **kw):
    # a follower in Retry with next <= last: the heartbeat response's resend is marked
    side = C.Side(be, _lagging_leader(S, abi.RETRY, 9), S, C.cc_recs(1, 10), **kw)
    _, out, _, _ = side.step(_msg(HEARTBEAT_RESP, 1, 5))
    assert _marks(out, 1) == [(1, 10, 0, 8, 2)]
    side.close()
    # two uncommitted config changes in the record: both marks
    side = C.Side(be, _lagging_leader(S, abi.RETRY, 9), S, C.cc_recs(1, 10, 9), **kw)
    _, out, _, _ = side.step(_msg(HEARTBEAT_RESP, 1, 5))
    assert _marks(out, 1) == [(1, 10, 9, 8, 2)]
    side.close()
    # a follower in Wait whose ack moves the commit: the lean leader would send
    # entry 10 from next = 10 and hands the lane over, the general lane marks it
    side = C.Side(be, _lagging_leader(S, abi.WAIT, 9), S, C.cc_recs(1, 10), **kw)
    st, out, _, _ = side.step(_msg(abi.REPLICATE_RESP, 1, 5, log_index=9))
    assert int(st[0]["committed"]) == 9 and _marks(out, 1) == [(1, 10, 0, 9, 1)]
    side.close()
    # a config change that is committed but not applied needs no mark
    p = _lagging_leader(S, abi.RETRY, 9)
    side = C.Side(be, p, S, C.cc_recs(1, 8), **kw)
    _, out, _, _ = side.step(_msg(HEARTBEAT_RESP, 1, 5))
    assert _marks(out, 1) == [(0, 0, 0, 8, 2)]
    side.close()


@pytest.mark.parametrize("be", BACKENDS)
@pytest.mark.parametrize("S", [3, 5])
def test_resend(be, S, request):
    _need(be, request)
    scn_resend(be, S)


def test_resend_every_wave_hint(built):
    """The host lane draws another wave hint, and the fused or the split
    schedule, with every call: the resend cases under sixteen of them."""
    for _ in range(16):
        scn_resend("cpu", 3)


# ---------------------------------------------------------------- 8. ABI
def test_marks_validated_hostlane(built):
    """GR_EINVAL for marks out of range (the host packer's validate_msg)."""
    p = _follower(3)
    for hint, high in ((10, 0), (14, 0), (0, 0), (12, 12), (12, 13), (12, 10)):
        m = _msg(abi.REPLICATE, 0, 5, log_index=10, log_term=5, commit=8, reject=1, ents=3, ent_term=5, hint=hint,
                 hint_high=high)
        assert C.host_step(p, C.cc_recs(1), m, None, 3, rc_ok=(-1,)) == -1
    m = _msg(abi.REPLICATE, 0, 5, log_index=10, log_term=5, commit=8, reject=1, ents=3, ent_term=5, hint=13, hint_high=11)
    assert len(C.host_step(p, C.cc_recs(1), m, None, 3)) == 4


@pytest.mark.gpu
def test_abi(gpu):
    """A set / get round trip; GR_ERANGE on a duplicate or a slot out of range
    before anything is written; GR_ESTATE between _begin and _end; GR_EINVAL for
    marks out of range with the switch on, through gr_step and gr_step_compact."""
    from dragonboat_amd.engine import Engine, GpuRaftError
    eng = Engine(8, 3, config_entries=True)
    assert eng.get_config_entries() is True
    assert eng.get_cc_indexes(np.arange(8)).tobytes() == C.cc_recs(8).tobytes()  # zeroed at gr_create
    recs = C.cc_recs(3)
    recs["last"], recs["prev"] = [11, 22, 2 ** 40], [10, 0, 7]
    eng.set_cc_indexes([5, 0, 2], recs)
    assert eng.get_cc_indexes([2, 5, 0]).tobytes() == recs[[2, 0, 1]].tobytes()
    for bad in ([1, 1], [8]):
        with pytest.raises(GpuRaftError) as ei:
            eng.set_cc_indexes(bad, C.cc_recs(len(bad), 99))
        assert "(-4)" in str(ei.value)
        with pytest.raises(GpuRaftError) as ei:
            eng.get_cc_indexes(bad)
        assert "(-4)" in str(ei.value)
    assert eng.get_cc_indexes([1]).tobytes() == C.cc_recs(1).tobytes()  # nothing written
    eng.load(np.concatenate([_follower(3)] * 8))
    eng.set_cc_indexes(np.arange(8), C.cc_recs(8))
    good = _msg(abi.REPLICATE, 0, 5, log_index=10, log_term=5, commit=8, reject=1, ents=3, ent_term=5, hint=13, hint_high=11)
    pack = eng.lib

    def compact(m):
        cm, ext = np.zeros(len(m), abi.CMSG), np.zeros(len(m), abi.MESSAGE)
        n_ext = ctypes.c_size_t()
        assert pack.gr_pack_messages(m.ctypes.data, len(m), cm.ctypes.data, ext.ctypes.data, ctypes.byref(n_ext)) == 0
        return cm, ext[:n_ext.value]

    for hint, high in ((10, 0), (14, 0), (0, 0), (12, 12), (12, 10)):
        m = good.copy()
        m["hint"], m["hint_high"] = hint, high
        before = eng.sync(8)
        with pytest.raises(GpuRaftError) as ei:
            eng.step(m)
        assert "(-1)" in str(ei.value)
        cm, ext = compact(m)
        with pytest.raises(GpuRaftError) as ei:
            eng.step_compact(cm, ext, np.zeros(0, abi.CLOCAL), np.zeros(0, abi.LOCAL))
        assert "(-1)" in str(ei.value)
        assert eng.sync(8).tobytes() == before.tobytes()  # before anything is written
    # GR_ESTATE between _begin and _end
    cm, ext = compact(good)
    assert len(ext) == 1  # a marked Replicate with both marks travels as an ext record
    ib = abi.cinbox_of(cm, ext, np.zeros(0, abi.CLOCAL), np.zeros(0, abi.LOCAL))
    assert eng.lib.gr_step_compact_begin(eng._h, ctypes.byref(ib)) == 0
    one = C.cc_recs(1, 5)
    idx = np.zeros(1, np.uint32)
    assert eng.lib.gr_set_cc_indexes(eng._h, idx.ctypes.data, one.ctypes.data, 1) == -6
    assert eng.lib.gr_get_cc_indexes(eng._h, idx.ctypes.data, one.ctypes.data, 1) == -6
    assert eng.lib.gr_set_config_entries(eng._h, 0) == -6
    ob = abi.COutbox()
    assert eng.lib.gr_step_compact_end(eng._h, ctypes.byref(ob)) == 0
    eng._take_coutbox(ob)
    assert (int(eng.get_cc_indexes([0])[0]["last"]), int(eng.get_cc_indexes([0])[0]["prev"])) == (13, 11)
    # the switch off: the same out-of-range marks are taken as the parent took them
    eng.set_config_entries(False)
    assert eng.get_config_entries() is False
    m = good.copy()
    m["hint"], m["log_index"] = 3, 13
    eng.step(m)
    eng.close()


# ---------------------------------------------------------------- 9. switch off
def _random_replicates(rng, n, with_marks):
    """Replicates to eight followers of the log 1..10 at term 5: appends,
    duplicates, rejects and early acks, their reject / hint / hint_high random."""
    m = np.zeros(n, abi.MESSAGE)
    m["type"], m["slot"], m["term"], m["log_term"] = abi.REPLICATE, 0, 5, 5
    m["peer"] = rng.integers(0, 8, n)
    m["log_index"] = rng.integers(5, 13, n)
    m["commit"] = rng.integers(0, 12, n)
    ne = rng.integers(0, 4, n)
    m["n_entries"], m["n_runs"] = ne, ne > 0
    m["run_term"][:, 0] = np.where(ne > 0, 5, 0)
    if with_marks:
        m["reject"] = rng.integers(0, 2, n)
        m["hint"] = rng.integers(0, 2 ** 40, n)
        m["hint_high"] = rng.integers(0, 2 ** 40, n)
    return m


@pytest.mark.parametrize("be", BACKENDS)
def test_switch_off_bytes(be, request):
    """Replicates with random reject / hint / hint_high and the same Replicates
    with all three zeroed give byte-identical state, outbox and results."""
    _need(be, request)
    peers = np.concatenate([_follower(3)] * 8)
    rng = np.random.default_rng(20)
    a = C.Side(be, peers, 3, on=False)
    b = C.Side(be, peers, 3, on=False)
    for _ in range(6):
        m = _random_replicates(rng, 24, True)
        z = m.copy()
        z["reject"], z["hint"], z["hint_high"] = 0, 0, 0
        sa, _, oa, ra = a.raw(m)
        sb, _, ob, rb = b.raw(z)
        assert sa.tobytes() == sb.tobytes() and oa.tobytes() == ob.tobytes() and ra.tobytes() == rb.tobytes()
        assert not np.any(oa["reject"] & (oa["type"] == abi.REPLICATE))
        a.state, b.state = sa, sb
    a.close()
    b.close()


# ---------------------------------------------------------------- 10. coverage
SCENARIOS = (scn_propose, scn_still_escalates, scn_follower, scn_promotion, scn_resend)


def _names(raw):
    return [n for n in raw.decode().split(",") if n]


def _check_cover(cc_counts, cc_names, counts, names):
    missing = [n for n, c in zip(cc_names, cc_counts) if c == 0]
    assert not missing, f"config-change-entry branches never reached: {missing}"
    bad = {n: int(c) for n, c in zip(names, counts) if c and n.startswith("BAD_")}
    assert not bad, f"invariants violated: {bad}"


def test_coverage_hostlane(built):
    """Every id of the config-change-entry coverage table is reached by the
    scenarios on the host lane, and no BAD_* id of the main table moves."""
    def read():
        out = []
        for elect in (False, True):
            l = C.lib(elect)
            ncc, nmain = _names(l.hl_coverage_cc_names()), _names(l.hl_coverage_names())
            a, b = np.zeros(len(ncc), np.uint64), np.zeros(len(nmain), np.uint64)
            l.hl_coverage_cc(a.ctypes.data, len(a))
            l.hl_coverage(b.ctypes.data, len(b))
            out.append((a, b, ncc, nmain))
        return out
    before = read()
    for _ in range(8):  # the lean hand-over needs a wave hint that takes the lean leader
        for s in SCENARIOS:
            s("cpu")
    after = read()
    cc = sum(x[0] - y[0] for x, y in zip(after, before))
    main = sum(x[1] - y[1] for x, y in zip(after, before))
    _check_cover(cc, after[0][2], main, after[0][3])


@pytest.mark.gpu
def test_coverage_gpu(gpu):
    """The same on the device, from the engine built with -DGR_COVERAGE."""
    from dragonboat_amd import build
    from dragonboat_amd.engine import load_library
    lib = load_library(build.COVER_LIB)
    ncc, nmain = _names(lib.gr_coverage_cc_names()), _names(lib.gr_coverage_names())

    def read():
        a, b = np.zeros(len(ncc), np.uint64), np.zeros(len(nmain), np.uint64)
        assert lib.gr_coverage_cc_read(a.ctypes.data_as(ctypes.c_void_p), len(a)) == len(a)
        assert lib.gr_coverage_read(b.ctypes.data_as(ctypes.c_void_p), len(b)) == len(b)
        return a, b
    a0, b0 = read()
    for s in SCENARIOS:
        s("gpu", lib_path=build.COVER_LIB)
    a1, b1 = read()
    _check_cover(a1 - a0, ncc, b1 - b0, nmain)


# ---------------------------------------------------------------- 7. wire
@pytest.mark.gpu
def test_wire_marks(gpu):
    """A frame with a Replicate whose entries have type 1 goes through
    gr_step_wire: the router sets the marks from the entries' types, and state,
    outbox and record equal those of the host-marked gr_step."""
    import wirefeed
    from dragonboat_amd import wire as W
    from dragonboat_amd.engine import Engine

    class TypedFeed(wirefeed.WireFeed):
        """WireFeed whose marked Replicates travel as the reference sends them:
        no Reject, no Hint, the entries at the marks typed ConfigChangeEntry."""

        def decode(self, msgs):
            torch = self.torch
            batches, wm, we, payload = wirefeed.to_wire(msgs, self.node_id, self.remote_id, self.cluster_of)
            first = wm["first_entry"].astype(np.int64)
            for k, m in enumerate(msgs):
                if m["type"] != abi.REPLICATE or not m["reject"]:
                    continue
                for idx in (int(m["hint"]), int(m["hint_high"])):
                    if idx:
                        we["type"][first[k] + idx - int(m["log_index"]) - 1] = 1
                wm["reject"][k], wm["hint"][k], wm["hint_high"][k] = 0, 0, 0
            frames = self.codec.marshal(payload, batches, wm, we)
            table = W.frames_table(batches["frame_off"], batches["frame_len"])
            d_buf = torch.from_numpy(frames).cuda()
            d_bat = torch.from_numpy(table.view(np.uint8)).cuda()
            d_msgs = torch.empty(len(wm) * W.WMESSAGE.itemsize, dtype=torch.uint8, device="cuda")
            d_ents = torch.empty(max(1, len(we)) * W.WENTRY.itemsize, dtype=torch.uint8, device="cuda")
            nm, ne = self.codec.unmarshal_device(d_buf.data_ptr(), len(frames), d_bat.data_ptr(), len(table),
                                                 d_msgs.data_ptr(), len(wm), d_ents.data_ptr(), max(1, len(we)))
            assert nm == len(wm) and ne == len(we)
            return d_msgs.data_ptr(), nm, d_ents.data_ptr(), ne, (d_buf, d_bat, d_msgs, d_ents)

    peers = np.concatenate([_follower(3)] * 3)
    msgs = np.concatenate([
        _msg(abi.REPLICATE, 0, 5, log_index=10, log_term=5, commit=8, reject=1, ents=3, ent_term=5, hint=13, hint_high=11),
        _msg(abi.REPLICATE, 0, 5, log_index=10, log_term=5, commit=9, ents=2, ent_term=5),
        _msg(abi.REPLICATE, 0, 5, log_index=10, log_term=5, commit=8, reject=1, ents=1, ent_term=5, hint=11)])
    msgs["peer"] = [0, 1, 2]
    cl = np.arange(3, dtype=np.uint64) + 1
    got = []
    for wire in (False, True):
        eng = Engine(3, 3, config_entries=True)
        eng.load(peers)
        if wire:
            feed = TypedFeed(peers, cl)
            eng.bind_nodes(cl, np.asarray(peers["node_id"], np.uint64))
            dm, nm, de, ne, keep = feed.decode(msgs)
            out, res, idx, why = eng.step_wire(dm, nm, de, ne)
            assert len(idx) == 0
            feed.close()
        else:
            out, res = eng.step(msgs)
        got.append((eng.sync(3), out, res, eng.get_cc_indexes(np.arange(3))))
        eng.close()
    for a, b in zip(*got):
        assert a.tobytes() == b.tobytes()
    cc = got[1][3]
    assert [(int(r["last"]), int(r["prev"])) for r in cc] == [(13, 11), (0, 0), (11, 0)]
    # the switch off: the router leaves a Replicate's reject / hint as the frame has them
    eng = Engine(3, 3)
    eng.load(peers)
    feed = TypedFeed(peers, cl)
    eng.bind_nodes(cl, np.asarray(peers["node_id"], np.uint64))
    dm, nm, de, ne, keep = feed.decode(msgs)
    out, res, idx, why = eng.step_wire(dm, nm, de, ne)
    assert eng.get_cc_indexes(np.arange(3)).tobytes() == C.cc_recs(3).tobytes()
    feed.close()
    eng.close()


# ---------------------------------------------------------------- 6. live populations
CC_PASS, MUTE_PASS, PASSES = 44, 46, 96


def live_population(be, G, seed, lib_path=None):
    """Cold start with a tick every pass and a proposal on every leader. At
    CC_PASS the leaders of the even groups propose a config change; from
    MUTE_PASS on the messages of the leaders of every third group are dropped
    for good, so those groups re-elect over uncommitted entries, the groups of
    both kinds with a config change among them. Returns the finished Population."""
    from dragonboat_amd import populations as P
    R = 3
    pop = C.Population(be, P.cold_start(G, R, seed=seed), G, R, lib_path=lib_path)
    for k in range(PASSES):
        lead = np.nonzero((pop.ref["state"] == abi.LEADER) & ~pop.muted)[0]
        loc = P.propose_locals(R * G, lead, seed=seed, pass_index=k, ticks=1)
        if k == CC_PASS or k == PASSES - 12:  # the second round: on the re-elected leaders too
            pop.propose_cc(loc, lead[(lead % G) % 2 == 0])
        if k == MUTE_PASS:
            pop.muted[lead[(lead % G) % 3 == 0]] = True
        pop.step(loc)
    return pop


def check_live_population(pop, G):
    R = 3
    live = ~pop.muted
    nl = ((pop.ref["state"] == abi.LEADER) & live).reshape(R, G).sum(axis=0)
    assert np.all(nl == 1), f"groups without exactly one live leader: {np.nonzero(nl != 1)[0][:8]}"
    assert pop.muted.sum() >= G // 3 - 1 and pop.promoted_pending >= 1, (int(pop.muted.sum()), pop.promoted_pending)
    for why in ("unsupported", "election", "config_change"):
        assert pop.esc.get(why, 0) == 0, pop.esc
    # the config changes of the second round were committed and applied everywhere live
    assert not np.any((pop.ref["flags"][live] & C.PENDING) != 0)


def test_live_population_hostlane(built):
    """70 x 3 on the host lane (waves straddle replica blocks)."""
    pop = live_population("cpu", 70, 11)
    check_live_population(pop, 70)


@pytest.mark.gpu
def test_live_population_gr_step(gpu):
    """70 x 3 through gr_step (the fused small kernel)."""
    pop = live_population("gpu", 70, 11)
    try:
        check_live_population(pop, 70)
    finally:
        pop.close()


@pytest.mark.gpu
@pytest.mark.parametrize("G,seed", [(200, 12), (320, 11)])  # route_wu = 0 / 1 (320 % 64 == 0)
def test_live_population_split_schedule(gpu, monkeypatch, G, seed):
    """200 x 3 and 320 x 3 on the device-resident split schedule. The seeds were
    picked on the host lane (every pass is under parity, so the run is the same
    there): with them every muted group re-elects within the pass budget (200 x 3
    with seed 11 leaves one group's second round past it)."""
    monkeypatch.setenv("GR_SMALL_BLOCKS", "0")
    monkeypatch.setenv("GR_SPLIT_MIN_LANES", "1")
    pop = live_population("dev", G, seed)
    try:
        check_live_population(pop, G)
    finally:
        pop.close()

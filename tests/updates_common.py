"""Updates out of the device-resident path (gpuraft.h gr_collect_updates): the
reference side of tests/test_updates.py, tests/test_updates_gpu.py,
tests/test_updates_switches_gpu.py and the updates mode of
all_switches_common.Population.

The rule is restated here from the reference's Go, not from the engine:
Peer.HasUpdate (internal/raft/peer.go:218-241), entryLog.hasEntriesToApply
(logentry.go:245-255), Peer.Commit's prevState half (peer.go:246-248) and
gpuraft.h's gr_cresult limits. It runs over result and peer records of the
moment of the collect, with the update states kept in Python: records that owe
nothing to the engine where a harness holds them (the oracle's pass in
devsim.DeviceLockstep, ref_step's in all_switches_common), else the dense
gr_collect_results records and the gr_sync_groups_to_host state, which
tests/devsim.py keeps under oracle parity. All arithmetic is uint64 and wraps,
as Go's does."""
import numpy as np

from dragonboat_amd import abi
from dragonboat_amd.engine import expand_updates
import parity

U = np.uint64
MORE, EVERY = abi.UPD_MORE_TO_APPLY, abi.UPD_EVERY


def ref_save_from(saved_to, marker, last):
    """inMemory.entriesToSave (inmemory.go:101-108): its first index, 0 when empty."""
    saved_to, marker, last = (np.asarray(x, U) for x in (saved_to, marker, last))
    idx = saved_to + U(1)
    nothing = (idx - marker) > (last + U(1) - marker)
    return np.where(~nothing & (idx <= last), idx, U(0))


def ref_classes(res, log_applied, first_index_m1, prev, flags):
    """abi.UPD_NONE / UPD_COMPACT / UPD_EXT per dense result record."""
    term, vote, commit = res["term"], res["vote"], res["committed"]
    last, sf = res["last_index"], res["save_from"]
    log_applied, lo = np.asarray(log_applied, U), np.asarray(first_index_m1, U)
    # pst := r.raftState(); !IsEmptyState(pst) && !IsStateEqual(pst, prevState)
    empty = (term == 0) & (vote == 0) & (commit == 0)
    equal = (term == prev["term"]) & (vote == prev["vote"]) & (commit == prev["commit"])
    rep = ~empty & ~equal
    rep |= sf != 0  # len(entriesToSave()) > 0
    if flags & MORE:  # hasEntriesToApply: committed + 1 > max(applied + 1, firstIndex())
        rep |= (commit + U(1)) > np.maximum(log_applied + U(1), lo + U(1))
    rep |= res["n_ready"] != 0  # len(readyToRead) != 0
    rep |= (res["escalation"] != 0) | (res["propose_result"] != abi.PROP_NONE) | (res["n_forwarded"] != 0)
    if flags & EVERY:
        rep |= True
    # gr_cresult: committed = last - commit_lag (32 bits), save_from = last - save_count + 1 (8 bits)
    save = np.where(sf != 0, last - sf + U(1), U(0))
    fits = (res["escalation"] == 0) & (commit <= last) & ((last - commit) < U(1 << 32)) & (sf <= last + U(1)) & \
        (save <= U(255))
    ext = ~fits | (res["n_ready"] != 0) | (res["n_forwarded"] != 0) | (term != prev["term"]) | (vote != prev["vote"])
    return np.where(rep, np.where(ext, abi.UPD_EXT, abi.UPD_COMPACT), abi.UPD_NONE).astype(np.int32)


COMPACT_FIELDS = [f for f in parity.RESULT_FIELDS if f != "append_from"]


class RefUpdates:
    """The Python side of gr_collect_updates for one engine: the update states
    (zero = emptyState, LaunchPeer's prevState for a new node) and the Commit rule."""

    def __init__(self, n):
        self.prev = np.zeros(n, abi.UPDATE_STATE)

    def launch(self, peers):
        """LaunchPeer with lastIndex > 0: prevState = the loaded raftState()."""
        st = np.zeros(len(peers), abi.UPDATE_STATE)
        st["term"], st["vote"], st["commit"] = peers["term"], peers["vote"], peers["committed"]
        self.prev = st
        return st

    def collect(self, dense, state, first, n, flags):
        """(reported slots ascending, their classes); advances prev by the Commit rule."""
        sl = slice(first, first + n)
        cls = ref_classes(dense[sl], state["log_applied"][sl], state["first_index_m1"][sl], self.prev[sl], flags)
        rep = np.nonzero(cls)[0] + first
        d = dense[rep]
        nonempty = (d["term"] != 0) | (d["vote"] != 0) | (d["committed"] != 0)
        for f, g in (("term", "term"), ("vote", "vote"), ("commit", "committed")):
            self.prev[f][rep[nonempty]] = d[g][nonempty]
        return rep, cls[rep - first]


def check_collect(eng, ref, n_slots, first=0, n=None, flags=MORE, propose_entries=None, dense=None, state=None):
    """One gr_collect_updates against the reference taken at the same moment.
    dense / state: result and peer records of that moment that do not come from
    the engine (the oracle's, or the reference side's of all_switches_common);
    where given, the reported set, the classes, the ext order and the update states
    after the collect are derived from them alone, and the engine's dense collect
    serves only the byte-for-byte check of ext records and the field check of
    expanded compact records (the harness has compared it with the same reference
    in the same pass). Returns (cresults, ext results, dense records, state): the
    records the rule ran over."""
    n = n_slots - first if n is None else n
    eng_dense = eng.collect_results(n_slots)
    dense = eng_dense if dense is None else dense
    state = eng.sync(n_slots) if state is None else state
    assert len(dense) >= n_slots and len(state) >= n_slots
    before = ref.prev.copy()
    ust = eng.get_update_states(np.arange(n_slots, dtype=np.uint32))
    assert ust.tobytes() == before.tobytes(), \
        f"update states before the collect: slots {np.nonzero(ust != before)[0][:8]}"
    cr, rx = eng.collect_updates_flags(first, n, flags)
    rep, cls = ref.collect(dense, state, first, n, flags)
    if n:  # device to host: the two totals, then the records and nothing else
        last = eng.updates_last()
        assert (last["n_results"], last["n_ext_results"]) == (len(cr), len(rx))
        assert last["bytes_down"] == 8 + abi.CRESULT.itemsize * len(cr) + abi.RESULT.itemsize * len(rx)
    assert np.array_equal(cr["peer"].astype(np.int64), rep), \
        f"reported slots: engine {len(cr)} reference {len(rep)}, first differences " \
        f"{sorted(set(cr['peer'].tolist()) ^ set(rep.tolist()))[:8]}"
    isx = (cr["flags"] & abi.CR_EXT) != 0
    bad = rep[isx != (cls == abi.UPD_EXT)]
    assert len(bad) == 0, \
        f"which records are EXT: {len(bad)} differ, engine EXT {int(isx.sum())} reference {int(np.sum(cls == abi.UPD_EXT))}; " \
        f"(slot, engine record, reference record, engine dense record, prev) " \
        f"{[(int(p), cr[cr['peer'] == p][0], dense[p], eng_dense[p], before[p]) for p in bad[:3]]}"
    assert len(rx) == int(isx.sum())
    assert np.array_equal(cr["aux"][isx], np.arange(len(rx), dtype=np.uint32)), "ext records in record order"
    want = eng_dense[rep]
    assert rx.tobytes() == want[isx].tobytes(), "an EXT record equals the dense record byte for byte"
    got = expand_updates(cr, rx, before["term"], before["vote"], propose_entries)
    for f in COMPACT_FIELDS:
        assert np.array_equal(got[f][~isx], want[f][~isx]), f"compact records: {f}"
    assert np.array_equal(got["peer"], want["peer"]) and not got["escalation"][~isx].any()
    ust = eng.get_update_states(np.arange(n_slots, dtype=np.uint32))
    assert ust.tobytes() == ref.prev.tobytes(), "update states after the collect"
    return cr, rx, dense, state


# tests/native/hostlane.hip hl_update_fields: UpdateFields' members in order, and
# the result-flag forms (gr_layout.h RF_*; HDR_LAG: the header carries the commit lag)
UF_FIELDS = ["term", "vote", "committed", "last_index", "save_from", "escalation", "propose_result", "n_ready",
             "n_forwarded"]
RF_ESCALATED, RF_PROPOSE, RF_READY, RF_APPEND, RF_FORWARDED, RF_HARDSTATE, RF_APPEND_LAST, RF_PROP_OK = \
    (1 << k for k in range(8))
HDR_LAG = 0x100


def lane_update_fields(lib, n):
    """After an hl_step of `lib` (any host-lane build) over n peers:
    (rc, update_fields(make_result(..)) per lane, lane_update_fields(..) per
    lane, flag word per lane); rc = n, or GR_ESTATE (-6) unless lane l stepped
    peer l for all l."""
    import ctypes
    a, b = np.zeros((n, len(UF_FIELDS)), U), np.zeros((n, len(UF_FIELDS)), U)
    rf = np.zeros(n, np.uint16)
    lib.hl_update_fields.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    rc = lib.hl_update_fields(a.ctypes.data, b.ctypes.data, rf.ctypes.data, n)
    return rc, a, b, rf


class FieldsCheck:
    """lane_update_fields against make_result after every pass of a run: both
    equal for every lane, and the flag forms that occurred."""

    def __init__(self):
        self.seen, self.passes, self.by_field = 0, 0, np.zeros(len(UF_FIELDS), np.int64)

    def after(self, lib, n, results=None):
        rc, a, b, rf = lane_update_fields(lib, n)
        assert rc == n, f"pass {self.passes}: lane l did not step peer l for all l (rc {rc})"
        bad = np.nonzero((a != b).any(axis=1))[0]
        assert len(bad) == 0, \
            f"pass {self.passes}: lane_update_fields != make_result on lanes {bad[:4]}: " \
            f"{[(dict(zip(UF_FIELDS, a[k].tolist())), dict(zip(UF_FIELDS, b[k].tolist())), hex(rf[k])) for k in bad[:2]]}"
        if results is not None:  # the export's make_result is the pass's own
            for k, f in enumerate(UF_FIELDS):
                assert np.array_equal(a[:, k], results[f].astype(U)), f
        for bit in range(9):
            if np.any(rf & (1 << bit)):
                self.seen |= 1 << bit
        self.by_field += (a != 0).any(axis=0)
        self.passes += 1

    def saw(self, *forms):
        return all(self.seen & f for f in forms)


def oracle_records(o):
    """The result records of an oracle pass as a collect's reference (the `o` a
    devsim.DeviceLockstep hands its collect callback): the oracle's own results
    at the device prefix; the oracle does not escalate, so an escalated peer gets
    the reason and item the device stopped at, which the oracle's esc_mask must
    justify."""
    dense = o["results"].copy()
    assert np.array_equal(dense["peer"], np.arange(len(dense)))
    if "device_results" in o:
        e = o["device_results"]
        e = e[e["escalation"] != 0]
        p = e["peer"].astype(np.int64)
        assert np.all((o["esc_mask"][p] >> e["escalation"].astype(np.uint32)) & 1)
        assert np.array_equal(o["limits"][p], e["esc_item"])
        dense["escalation"][p], dense["esc_item"][p] = e["escalation"], e["esc_item"]
    return dense


def commit_reported(sim, state, slots):
    """Persist and apply everything the listed peers have outstanding, on the
    engine and in the oracle of a DeviceLockstep (stable_log_to = last_index,
    applied_to = committed), from the reference's records."""
    slots = np.asarray(slots, np.int64)
    if len(slots) == 0:
        return
    uc = parity.update_commits(state[slots])
    rc, st = sim.eng.commit_update(slots.astype(np.uint32), uc)
    assert rc == 0 and not st.any(), (rc, st[st != 0][:4])
    rc, st = sim.pop.commit_update(slots.astype(np.uint32), uc)
    assert rc == 0 and not st.any()


class LockstepCollect:
    """The collect callback of a DeviceLockstep / QuiesceLockstep: one
    gr_collect_updates per pass against the oracle's records of that pass
    (check_collect with dense = the oracle's results, state = its mid records),
    then the reported peers committed on both sides. peers: the loaded records
    (LaunchPeer with lastIndex > 0 sets the update states to their State)."""

    def __init__(self, sim, peers, commit=True):
        self.sim, self.commit = sim, commit
        self.ref = RefUpdates(sim.n)
        sim.eng.set_update_states(np.arange(sim.n, dtype=np.uint32), self.ref.launch(peers))
        self.counts = []       # per pass: (reported, ext records), the reference's
        self.propose = None    # the pass's bound ProposeEntries counts, when it has any
        self.want_none = False  # this pass the reference reports no peer: asserted of it, then of the engine

    def __call__(self, o):
        n = self.sim.n
        dense, state = oracle_records(o), o["mid"]
        prev = self.ref.prev.copy()
        cls = ref_classes(dense, state["log_applied"], state["first_index_m1"], prev, MORE)  # of the reference, first
        self.classes = cls
        if self.want_none:
            assert not cls.any(), f"the reference reports {np.nonzero(cls)[0][:8]}"
        try:
            cr, rx, _, _ = check_collect(self.sim.eng, self.ref, n, propose_entries=self.propose, dense=dense,
                                         state=state)
        except AssertionError as e:
            raise AssertionError(f"collect after pass {self.sim.k}: {e}") from None
        assert (len(cr), len(rx)) == (int(np.sum(cls != 0)), int(np.sum(cls == abi.UPD_EXT)))
        if self.want_none:  # nothing to pack: the two totals come down and nothing else
            assert len(cr) == 0 and self.sim.eng.updates_last()["bytes_down"] == 8
        # a term or vote that moved arrives in full, with that term and vote
        moved = np.nonzero(((dense["term"] != prev["term"]) | (dense["vote"] != prev["vote"])) &
                           ((dense["term"] | dense["vote"] | dense["committed"]) != 0))[0]
        at = np.full(n, -1, np.int64)
        at[cr["peer"].astype(np.int64)] = np.arange(len(cr))
        c = cr[at[moved]]
        assert np.all(at[moved] >= 0) and np.all(c["flags"] & abi.CR_EXT), "a moved term or vote not reported in full"
        x = rx[c["aux"].astype(np.int64)]
        assert np.array_equal(x["peer"], moved) and np.array_equal(x["term"], dense["term"][moved]) and \
            np.array_equal(x["vote"], dense["vote"][moved])
        self.counts.append((len(cr), len(rx)))
        self.cr, self.rx, self.dense, self.state, self.moved, self.at = cr, rx, dense, state, moved, at
        if self.commit:
            commit_reported(self.sim, state, cr["peer"])


def oracle_collect_counts(peers, G, R, passes, locals_fn):
    """The same inputs through the oracle alone (no engine, no GPU): per pass,
    (reported, ext records) by the rule over the oracle's records, the reported
    peers committed, as LockstepCollect does beside a device."""
    from dragonboat_amd import populations as P
    from oracle.pyoracle import OraclePopulation
    n = G * R
    pop, topo = OraclePopulation(peers, R), P.Topology(G, R)
    ref = RefUpdates(n)
    ref.launch(peers)
    msgs, counts = np.zeros(0, abi.MESSAGE), []
    for k in range(passes):
        o = pop.step(msgs, locals_fn(k))
        rep, cls = ref.collect(o["results"], o["mid"], 0, n, MORE)
        counts.append((len(rep), int(np.sum(cls == abi.UPD_EXT))))
        if len(rep):
            rc, st = pop.commit_update(rep.astype(np.uint32), parity.update_commits(o["mid"][rep]))
            assert rc == 0 and not st.any()
        msgs = topo.route_messages(o["msgs"])
    return counts


def commit_all(eng, state, slots):
    """gr_commit_update of everything the listed peers have outstanding:
    stable_log_to = last_index (at its term), applied_to = committed."""
    slots = np.asarray(slots, np.int64)
    if len(slots) == 0:
        return
    uc = parity.update_commits(state[slots])
    rc, st = eng.commit_update(slots.astype(np.uint32), uc)
    assert rc == 0 and not st.any(), (rc, st[st != 0][:4])

"""TEST INFRASTRUCTURE: bindings of tests/_build/libhostlane_all.so and the
driver of the tests that run every device switch at once (elections, snapshots,
config-change entries), the configuration a deployment runs.

host_step: the engine's lane code on the CPU with the three switches compiled on
(tests/native/hostlane_all.hip), over records plus the snapshot records, the
restored list and the gr_cc_index records. ref_step: the reference side, the
oracle's raft object built from the same records with typed in-memory entries,
speaking both message conventions (tests/native/all_switches_ref.cpp). Side runs
one backend (the host lane, or an Engine) beside the reference and compares
everything a pass leaves: peer records, snapshot records (byte-equal),
gr_cc_index records (norm_cc), messages (norm_marks), results and the restored
list. Population does the same for live groups on "cpu", "gpu" (gr_step) and
"dev" (the device-resident split schedule).
"""
import ctypes
import os

import numpy as np

from dragonboat_amd import abi
import config_entries_common as CE
import parity
import snapshot_common as SN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "_build", "libhostlane_all.so")
_lib = None

INSTALL_SNAPSHOT = SN.INSTALL_SNAPSHOT
ESC = CE.ESC
PENDING = CE.PENDING
norm_cc, norm_marks, cc_recs = CE.norm_cc, CE.norm_marks, CE.cc_recs
membership = SN.membership
_rest_key = SN._rest_key


def lib():
    """The host lane with elections, snapshots and config entries on."""
    global _lib
    if _lib is None:
        c = ctypes
        l = c.CDLL(LIB)
        l.hl_step_all.argtypes = [c.c_uint32, c.c_uint64, c.c_void_p, c.c_uint32, c.POINTER(abi.Inbox), c.c_void_p,
                                  c.c_size_t, c.POINTER(c.c_size_t), c.c_void_p, c.POINTER(c.c_size_t), c.c_void_p,
                                  c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t), c.c_void_p, c.c_void_p]
        l.asr_step.argtypes = [c.c_uint32, c.c_uint64, c.c_void_p, c.c_uint32, c.POINTER(abi.Inbox), c.c_void_p,
                               c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t), c.c_void_p,
                               c.POINTER(c.c_size_t), c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t), c.c_void_p]
        l.hl_restore_remotes.argtypes = [c.c_uint32, c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p, c.c_uint32,
                                         c.c_void_p]
        l.hl_commit_update.argtypes = [c.c_uint32, c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p, c.c_uint32,
                                       c.c_void_p]
        for t in ("snap", "cc"):
            getattr(l, f"hl_coverage_{t}").argtypes = [c.c_void_p, c.c_uint32]
            getattr(l, f"hl_coverage_{t}_names").restype = c.c_char_p
        l.hl_coverage.argtypes = [c.c_void_p, c.c_uint32]
        l.hl_coverage_names.restype = c.c_char_p
        _lib = l
    return _lib


def _inbox(msgs, loc):
    msgs = np.zeros(0, abi.MESSAGE) if msgs is None else np.ascontiguousarray(msgs, abi.MESSAGE)
    loc = np.zeros(0, abi.LOCAL) if loc is None else np.ascontiguousarray(loc, abi.LOCAL)
    return msgs, loc, abi.inbox_of(msgs, loc)


def host_step(peers, snap, cc, msgs, loc, S):
    """One pass of the host lane: (peers', snap', cc', messages, results,
    restored, the cc staging records as the pass left them)."""
    peers = np.array(peers, abi.PEER, copy=True)
    snap = np.array(snap, abi.SNAPSHOT_REC, copy=True)
    cc = np.array(cc, abi.CC_INDEX, copy=True)
    msgs, loc, ib = _inbox(msgs, loc)
    n = len(peers)
    cap = max(16, 8 * n * S)
    out, res, rest = np.zeros(cap, abi.MESSAGE), np.zeros(n, abi.RESULT), np.zeros(2 * n, abi.RESTORED)
    stage = np.zeros(n, abi.CC_INDEX)
    n_out, n_res, n_rest = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    rc = lib().hl_step_all(S, abi.MAX_ENTRY_SIZE, peers.ctypes.data, n, ctypes.byref(ib), out.ctypes.data, cap,
                           ctypes.byref(n_out), res.ctypes.data, ctypes.byref(n_res), snap.ctypes.data,
                           rest.ctypes.data, len(rest), ctypes.byref(n_rest), cc.ctypes.data, stage.ctypes.data)
    assert rc == 0, rc
    return peers, snap, cc, out[:n_out.value], res[:n_res.value], rest[:n_rest.value], stage


def ref_step(peers, snap, cc, msgs, loc, S, limits=None):
    """The same pass on the reference side, each peer stopped before item
    limits[p]: (peers', snap', cc', messages, results by peer, restored, the item
    at which the oracle panicked or -1, by peer)."""
    peers = np.array(peers, abi.PEER, copy=True)
    snap = np.array(snap, abi.SNAPSHOT_REC, copy=True)
    cc = np.array(cc, abi.CC_INDEX, copy=True)
    msgs, loc, ib = _inbox(msgs, loc)
    n = len(peers)
    cap = max(16, 8 * n * S)
    out, res, rest = np.zeros(cap, abi.MESSAGE), np.zeros(n, abi.RESULT), np.zeros(cap, abi.RESTORED)
    n_out, n_res, n_rest = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    panic = np.full(n, -1, np.int32)
    lim = None if limits is None else np.ascontiguousarray(limits, np.uint32)
    rc = lib().asr_step(S, abi.MAX_ENTRY_SIZE, peers.ctypes.data, n, ctypes.byref(ib),
                        None if lim is None else lim.ctypes.data, snap.ctypes.data, cc.ctypes.data, out.ctypes.data,
                        cap, ctypes.byref(n_out), res.ctypes.data, ctypes.byref(n_res), rest.ctypes.data, cap,
                        ctypes.byref(n_rest), panic.ctypes.data)
    assert rc == 0, rc
    by_peer = np.zeros(n, abi.RESULT)
    r = res[:n_res.value]
    by_peer[r["peer"]] = r
    return peers, snap, cc, out[:n_out.value], by_peer, rest[:n_rest.value], panic


def host_restore(peers, idx, ms, S):
    """gr_restore_remotes as the all-switches host build runs it, in place: (rc, status)."""
    idx, ms, st = SN._rr_args(peers, idx, ms)
    rc = lib().hl_restore_remotes(S, peers.ctypes.data, len(peers), idx.ctypes.data, ms.ctypes.data, len(idx),
                                  st.ctypes.data)
    return rc, st


def host_commit_update(peers, idx, uc, S):
    """gr_commit_update on records through the all-switches host build, in place."""
    idx = np.ascontiguousarray(idx, np.uint32)
    uc = np.ascontiguousarray(uc, abi.UPDATE_COMMIT)
    st = np.zeros(len(idx), np.int32)
    rc = lib().hl_commit_update(S, peers.ctypes.data, len(peers), idx.ctypes.data, uc.ctypes.data, len(idx),
                                st.ctypes.data)
    return rc, st


def compare_pass(S, got, want, where=""):
    """Everything a pass leaves, engine side against reference side:
    (state, snap, cc, messages, results, restored) each."""
    st, snap, cc, out, res, rest = got
    rst, rsnap, rcc, rout, rres, rrest = want
    bad = parity.compare_states(st, rst, S)
    assert not bad, f"{where}state {bad[:3]}"
    assert snap.tobytes() == rsnap.tobytes(), f"{where}snapshot records {np.nonzero(snap != rsnap)[0][:4]}"
    a, b = norm_cc(cc, st["committed"]), norm_cc(rcc, rst["committed"])
    assert a.tobytes() == b.tobytes(), \
        f"{where}cc records {[(int(p), cc[p].tolist(), rcc[p].tolist()) for p in np.nonzero(a != b)[0][:4]]}"
    bad = parity.compare_msgs(norm_marks(out), norm_marks(rout))
    assert not bad, f"{where}messages {bad[:3]}"
    bad = parity.compare_results(res, rres)
    assert not bad, f"{where}results {bad[:3]}"
    assert _rest_key(rest) == _rest_key(rrest), f"{where}restored {(_rest_key(rest)[:4], _rest_key(rrest)[:4])}"


class Side:
    """`peers` with their snapshot and gr_cc_index records on one backend (cpu:
    the host lane over records; gpu: an Engine) beside the reference side,
    stepped together, elections always on. snapshots / config_entries = False
    turns that one switch off: the host lane and the reference side are then the
    single-switch pair of the other (snapshot_common / config_entries_common,
    their elections builds)."""

    def __init__(self, be, peers, S, snap=None, cc=None, snapshots=True, config_entries=True):
        assert snapshots or config_entries
        self.be, self.S, self.n = be, S, len(peers)
        self.snapshots, self.config_entries = snapshots, config_entries
        self.snap = np.zeros(self.n, abi.SNAPSHOT_REC) if snap is None else np.array(snap, abi.SNAPSHOT_REC)
        self.cc = np.zeros(self.n, abi.CC_INDEX) if cc is None else np.array(cc, abi.CC_INDEX)
        self.all = np.arange(self.n, dtype=np.uint32)
        if be == "gpu":
            from dragonboat_amd.engine import Engine
            self.eng = Engine(self.n, S, elections=True, snapshots=snapshots, config_entries=config_entries)
            assert self.eng.get_elections() and self.eng.get_snapshots() == snapshots
            assert self.eng.get_config_entries() == config_entries
            self.eng.load(peers)
            self.eng.set_snapshot_recs(self.all, self.snap)
            self.eng.set_cc_indexes(self.all, self.cc)
            self.state = self.eng.sync(self.n)
        else:
            from oracle.pyoracle import hostlane_step
            self.state, _, _ = hostlane_step(peers, None, None, S)  # a load and a sync
        self.ref = self.state.copy()
        self.restored = []  # every record drained so far
        self.stage = None   # cpu: the cc staging records of the last pass

    def raw(self, msgs=None, loc=None):
        """One pass on the engine side alone: (state, snap, cc, messages, results, restored)."""
        if self.be == "gpu":
            out, res = self.eng.step(msgs, loc)
            return (self.eng.sync(self.n), self.eng.get_snapshot_recs(self.all), self.eng.get_cc_indexes(self.all),
                    out, res, self.eng.restored_snapshots())
        if self.snapshots and self.config_entries:
            st, snap, cc, out, res, rest, self.stage = host_step(self.state, self.snap, self.cc, msgs, loc, self.S)
            return st, snap, cc, out, res, rest
        if self.snapshots:
            st, snap, out, res, rest = SN.host_step(self.state, self.snap, msgs, loc, self.S, elect=True)
            return st, snap, self.cc.copy(), out, res, rest
        st, cc, out, res = CE.host_step(self.state, self.cc, msgs, loc, self.S, elect=True)
        return st, self.snap.copy(), cc, out, res, np.zeros(0, abi.RESTORED)

    def ref_raw(self, msgs, loc, lim):
        if self.snapshots and self.config_entries:
            return ref_step(self.ref, self.snap, self.cc, msgs, loc, self.S, lim)
        if self.snapshots:
            rst, rsnap, rout, rres, rrest, panic = SN.ref_step(self.ref, self.snap, msgs, loc, self.S, lim)
            return rst, rsnap, self.cc.copy(), rout, rres, rrest, panic
        rst, rcc, rout, rres, panic = CE.ref_step(self.ref, self.cc, msgs, loc, self.S, lim)
        return rst, self.snap.copy(), rcc, rout, rres, np.zeros(0, abi.RESTORED), panic

    def step(self, msgs=None, loc=None, esc=None):
        """One pass on both sides, compared field for field. esc: {peer: reason}
        the pass must escalate with, exactly (None: no escalation). Returns
        (state, messages, results, restored, cc)."""
        got = self.raw(msgs, loc)
        st, snap, cc, out, res, rest = got
        e = {int(r["peer"]): int(r["escalation"]) for r in res if r["escalation"]}
        want = {int(p): ESC[v] for p, v in (esc or {}).items()}
        assert e == want, (e, want, [(int(r["peer"]), int(r["esc_item"])) for r in res if r["escalation"]])
        lim = parity.limits_from(res, self.n)
        *ref, panic = self.ref_raw(msgs, loc, lim)
        assert np.all(panic < 0), panic  # every reference panic lies at or past an escalation
        if not self.config_entries:  # the reference has no record to compare: the array is never written
            assert cc.tobytes() == self.cc.tobytes(), (cc, self.cc)
        compare_pass(self.S, got, ref)
        self.state, self.ref, self.snap, self.cc = st, ref[0], snap, cc
        self.restored.extend(_rest_key(rest))
        return st, out, res, rest, cc

    def restore(self, idx, ms):
        """One gr_restore_remotes on both sides; returns the statuses. Refused and
        unlisted peers are untouched bit for bit, the others equal the reference;
        the snapshot and gr_cc_index records do not move."""
        idx = np.asarray(idx, np.uint32)
        old = self.state.copy()
        if self.be == "gpu":
            rc, st = self.eng.restore_remotes(idx, ms)
            new = self.eng.sync(self.n)
        else:
            new = self.state.copy()
            rc, st = host_restore(new, idx, ms, self.S)
        ref = self.ref.copy()
        # the reference's own export drops a removed node's ack (snapshot_common.Side.restore)
        for f in ("from_slot", "ack_bits"):
            ref["read_index"][f] = np.where(np.arange(abi.GR_Q)[None, :] < ref["read_index_count"][:, None],
                                            old["read_index"][f], ref["read_index"][f])
        rrc, rst = SN.ref_restore(ref, idx, ms, self.S)
        assert list(st) == list(rst), (st, rst)
        assert rc == rrc == (-6 if np.any(st != 0) else 0), (rc, rrc)
        touched = np.zeros(self.n, bool)
        touched[idx[st == 0]] = True
        assert new[~touched].tobytes() == old[~touched].tobytes(), "a refused or unlisted peer changed"
        bad = parity.compare_states(new, ref, self.S)
        assert not bad, bad[:3]
        self._records_unmoved()
        self.state, self.ref = new, ref
        return st

    def apply(self, idx, changes):
        """One gr_apply_config_change on both sides (the reference side of
        config_change_common); returns the statuses. The snapshot and gr_cc_index
        records do not move."""
        import config_change_common as CC
        idx = np.asarray(idx, np.uint32)
        if self.be == "gpu":
            rc, st = self.eng.apply_config_change(idx, changes)
            new = self.eng.sync(self.n)
        else:
            new = self.state.copy()
            rc, st = CC.host_apply(new, idx, changes, self.S)
        ref = self.ref.copy()
        rrc, rst = CC.ref_apply(ref, idx, changes, self.S)
        assert list(st) == list(rst) and rc == rrc, (rc, rrc, st, rst)
        bad = parity.compare_states(new, ref, self.S)
        assert not bad, bad[:3]
        self._records_unmoved()
        self.state, self.ref = new, ref
        return st

    def _records_unmoved(self):
        if self.be == "gpu":
            assert self.eng.get_snapshot_recs(self.all).tobytes() == self.snap.tobytes()
            assert self.eng.get_cc_indexes(self.all).tobytes() == self.cc.tobytes()
            assert len(self.eng.restored_snapshots()) == 0

    def close(self):
        if self.be == "gpu":
            self.eng.close()


# ---------------------------------------------------------------- live populations
def compact_records(recs, idx, index):
    """gr_compact_log on records, in place (gr_io.h compact_rows): firstIndex - 1
    becomes index[x], runs wholly below it drop out and the run covering it
    starts there."""
    for p, i in zip(np.asarray(idx, np.int64), np.asarray(index, np.uint64)):
        g = recs[p]
        i = int(i)
        assert int(g["first_index_m1"]) <= i <= int(g["saved_to"] if g["marker_index"] else g["last_index"])
        runs = [(int(g["run_start"][k]), int(g["run_term"][k])) for k in range(int(g["n_runs"]))]
        keep = [k for k, (s, _) in enumerate(runs) if s <= i]
        if keep:
            runs = [(i, runs[keep[-1]][1])] + runs[keep[-1] + 1:]
        g["first_index_m1"] = i
        g["n_runs"], g["run_start"], g["run_term"] = len(runs), 0, 0
        for k, (s, t) in enumerate(runs):
            g["run_start"][k], g["run_term"][k] = s, t


class Population:
    """G groups x R replicas (replica-major) on one backend beside the reference
    side with elections, snapshots and config entries on: "cpu" the host lane
    over records, "gpu" an Engine through gr_step, "dev" an Engine on the
    device-resident schedule (gr_step_device over loopback spaces, as
    config_entries_common.Population runs it). Every pass is compared at the
    device prefix (compare_pass); an escalated peer's pass is finished by the
    reference, as the host would, and the peer reloaded with its exact peer,
    gr_cc_index and snapshot records. After a pass the host drains the restored
    list and calls gr_restore_remotes on those peers, persists and applies
    everything (gr_commit_update, gr_notify_applied) and applies a committed
    config change on every replica that reached it (gr_apply_config_change; the
    change re-adds a voter, which only clears pendingConfigChange; the host build of
    gr_config_change.h on "cpu", the oracle's own addNode on the reference side).

    The counters (self.count) are computed from the reference side's records
    alone, so they do not depend on the code under test."""

    def __init__(self, be, peers, snap, G, R, updates=False, drain_after=False):
        from dragonboat_amd import populations as P
        self.be, self.G, self.R, self.S, self.n = be, G, R, R, G * R
        self.updates, self.drain_after = updates, drain_after
        self.topo = P.Topology(G, R)
        self.all = np.arange(self.n, dtype=np.uint32)
        self.msgs = np.zeros(0, abi.MESSAGE)  # the next inbox (receiver peer, sender slot)
        self.muted = np.zeros(self.n, bool)    # peers whose messages are dropped for good
        self.esc = {}                          # reason -> count
        self.pending = {}                      # group -> (index, term, replicas applied)
        self.ever_restored = np.zeros(self.n, bool)
        self.count = dict(restores=0, restores_uncommitted=0, promotions=0, promoted_flag=0, promoted_clear=0,
                          promoted_restored=0, snapshots_sent=0, snapshots_sent_flagged=0, marked_replicates=0)
        self.same = np.concatenate([membership([(j + 1, abi.SLOT_VOTER) for j in range(R)])] * self.n)
        self.k = 0
        self.refsnap = np.array(snap, abi.SNAPSHOT_REC, copy=True)
        self.refcc = np.zeros(self.n, abi.CC_INDEX)
        if be == "cpu":
            from oracle.pyoracle import hostlane_step
            self.state, _, _ = hostlane_step(peers, None, None, self.S)
            self.snap, self.cc = self.refsnap.copy(), self.refcc.copy()
            self.ref = self.state.copy()
            self._launch_updates()
            return
        from dragonboat_amd.engine import Engine
        self.eng = Engine(self.n, self.S, elections=True, snapshots=True, config_entries=True)
        assert self.eng.get_config_entries() and self.eng.get_elections() and self.eng.get_snapshots()
        self.eng.load(peers)
        self.eng.set_snapshot_recs(self.all, self.refsnap)
        self.ref = self.eng.sync(self.n)
        if be == "dev":
            import torch
            self.torch = torch
            self.in_pos, self.out_pos = self.topo.loopback_routes(self.S)
            self.positions, self.depth = self.n * self.S, abi.GR_C
            self.eng.bind_routes(self.in_pos, self.out_pos)
            nb = self.eng.space_bytes(1, self.positions, self.depth)
            self.spaces = [torch.zeros(nb, dtype=torch.uint8, device="cuda") for _ in range(2)]
            self.stream = torch.cuda.current_stream()
            peer = np.full(self.positions, -1, np.int64)
            slot = np.full(self.positions, -1, np.int64)
            for j in range(self.S):
                ok = self.in_pos[j] != 0xFFFFFFFF
                peer[self.in_pos[j, ok].astype(np.int64)] = np.nonzero(ok)[0]
                slot[self.in_pos[j, ok].astype(np.int64)] = j
            self.inv = (peer, slot)
            self.dirty = False  # the space the next pass reads must be re-encoded
        self._launch_updates()

    # -- updates=True: the host learns what to persist, apply and answer from
    # gr_collect_updates alone (INTEGRATION.md "Updates out of the device-resident path")
    def _launch_updates(self):
        """LaunchPeer with lastIndex > 0: the update states are the loaded
        raftState(); the host's applied index is the loaded one."""
        if not self.updates:
            return
        import updates_common as UC
        assert self.be in ("cpu", "dev"), "gr_collect_updates speaks for device-resident passes"
        self.upd = UC.RefUpdates(self.n)
        st = self.upd.launch(self.ref)
        if self.be == "dev":
            self.eng.set_update_states(self.all, st)
        self.happ = self.ref["log_applied"].copy()  # the applied index the host holds
        self.reported = np.zeros(0, abi.RESULT)    # the last collect's records, expanded
        self.upd_counts = []  # per pass, from the reference side's records: (reported, ext records, restored peers)

    def _collect(self, k, loc, before, res, st, rres, rst, rrest, rest):
        """The collect after pass k, before anything is reloaded. The reference
        for it is the reference side's own pass: rres / rst (ref_step), through the
        rule of updates_common. On "dev" gr_collect_updates with the default flags;
        on "cpu" the same call emulated by gr_update_class over the host lane's
        results. Leaves the reported peers' records in self.reported."""
        import updates_common as UC
        from dragonboat_amd.engine import expand_updates, update_class
        n = self.n
        assert len(res) == n and np.array_equal(res["peer"], self.all), "every peer takes a local input, in peer order"
        cls = UC.ref_classes(rres, rst["log_applied"], rst["first_index_m1"], self.upd.prev, UC.MORE)
        reported = cls != abi.UPD_NONE
        who = np.unique(rrest["peer"]).astype(np.int64)
        turned = (before["state"] != abi.LEADER) & (rst["state"] == abi.LEADER)
        uc = parity.update_commits(rst)
        owes = (uc["stable_log_to"] != 0) | (uc["applied_to"] != 0)
        restored = np.zeros(n, bool)
        restored[who] = True
        # of the reference itself: the rule, which leaves inmem.snapshot out, loses none of these
        for what, m in (("restored", restored), ("promoted", turned), ("with something to commit", owes)):
            assert reported[m].all(), f"pass {k}: {what} peers the rule does not report: {np.nonzero(m & ~reported)[0][:8]}"
        self.upd_counts.append((int(reported.sum()), int(np.sum(cls == abi.UPD_EXT)), len(who)))
        prev = self.upd.prev.copy()
        if self.be == "cpu":
            got = update_class(res, st["log_applied"], st["first_index_m1"], prev)
            rep, rcls = self.upd.collect(rres, rst, 0, n, UC.MORE)
            assert np.array_equal(np.nonzero(got)[0], rep), \
                f"pass {k}: reported {sorted(set(np.nonzero(got)[0].tolist()) ^ set(rep.tolist()))[:8]}"
            assert np.array_equal(got[rep], rcls), f"pass {k}: classes"
            self.reported = res[rep]
            return
        if not self.drain_after:
            prom = self.eng.promotions()
        cr, rx, _, _ = UC.check_collect(self.eng, self.upd, n, propose_entries=loc["propose_entries"], dense=rres,
                                        state=rst)
        assert len(cr) == int(reported.sum()) and len(rx) == self.upd_counts[-1][1]
        if self.drain_after:  # the collect cleared LR_RFLAGS; it takes nothing from the two lists
            prom, rest = self.eng.promotions(), self.eng.restored_snapshots()
        assert _rest_key(rest) == _rest_key(rrest), f"pass {k}: restored {(_rest_key(rest)[:4], _rest_key(rrest)[:4])}"
        assert sorted(prom["peer"].tolist()) == np.nonzero(turned)[0].tolist(), f"pass {k}: promotions"
        for r in prom:  # the empty entry: the first of the new leader's term
            g, i, t = rst[int(r["peer"])], int(r["noop_index"]), int(r["term"])
            assert t == int(g["term"]) and CE._term_at(g, i) == t and CE._term_at(g, i - 1) != t, (k, r)
        self.reported = expand_updates(cr, rx, prev["term"], prev["vote"], loc["propose_entries"])

    def _commit_reported(self, rrest):
        """gr_commit_update and gr_notify_applied from the records alone, to the
        reported slots and to no others. An escalated peer was reloaded with the
        record of its whole pass: the host commits what that record holds."""
        r = self.reported
        slots = r["peer"].astype(np.int64)
        # the RSM recovered from the snapshots of the restored list
        np.maximum.at(self.happ, rrest["peer"].astype(np.int64), rrest["index"])
        if len(slots) == 0:
            return
        own = self.ref[slots]  # the host's own log: the terms it persisted
        uc = np.zeros(len(slots), abi.UPDATE_COMMIT)
        save = r["save_from"] != 0
        uc["stable_log_to"] = np.where(save, r["last_index"], 0)
        uc["stable_log_term"] = np.where(
            save, own["run_term"][np.arange(len(own)), np.maximum(own["n_runs"].astype(np.int64) - 1, 0)], 0)
        committed = r["committed"].copy()
        esc = r["escalation"] != 0
        if esc.any():
            uc[esc] = parity.update_commits(own[esc])
            uc["applied_to"][esc] = 0
            committed[esc] = own["committed"][esc]
        above = committed > self.happ[slots]
        uc["applied_to"] = np.where(above, committed, 0)
        self.happ[slots] = np.where(above, committed, self.happ[slots])
        if self.be == "cpu":
            rc, stt = host_commit_update(self.state, slots, uc, self.S)
            assert rc == 0, (rc, stt[stt != 0][:4])
            self.state["applied"][slots] = committed
        else:
            rc, stt = self.eng.commit_update(slots.astype(np.uint32), uc)
            assert rc == 0, (rc, stt[stt != 0][:4])
            self.eng.notify_applied(slots.astype(np.uint32), committed)

    # -- one pass on the engine side: (state, snap, cc, the next inbox's records, results, restored)
    def _engine_pass(self, loc):
        if self.be == "cpu":
            st, snap, cc, out, res, rest, _ = host_step(self.state, self.snap, self.cc, self.msgs, loc, self.S)
            return st, snap, cc, self.topo.route_messages(out), res, rest
        eng = self.eng
        if self.be == "gpu":
            out, res = eng.step(self.msgs, loc)
            nxt = self.topo.route_messages(out)
        else:
            from dragonboat_amd.engine import decode_space
            src, dst = self.spaces[self.k % 2], self.spaces[(self.k + 1) % 2]
            if self.dirty:
                self._encode(self.msgs, src)
                self.dirty = False
            eng.set_locals(loc)
            eng.step_device(src.data_ptr(), dst.data_ptr(), 1, self.positions, 1, self.positions, self.n,
                            self.stream.cuda_stream, depth=self.depth)
            self.torch.cuda.synchronize()
            res = eng.collect_results(self.n)
            nxt = decode_space(dst.cpu().numpy(), 1, self.positions, self.depth)
            pos = nxt["peer"].astype(np.int64)
            nxt["peer"] = self.inv[0][pos].astype(np.uint32)
            nxt["slot"] = self.inv[1][pos].astype(np.uint8)
        rest = None if self.updates and self.drain_after else eng.restored_snapshots()  # None: drained after the collect
        return eng.sync(self.n), eng.get_snapshot_recs(self.all), eng.get_cc_indexes(self.all), nxt, res, rest

    def _encode(self, msgs, space):
        buf = np.zeros(self.eng.space_bytes(1, self.positions, self.depth), np.uint8)
        pos = self.in_pos[msgs["slot"].astype(np.int64), msgs["peer"].astype(np.int64)].astype(np.uint32)
        assert np.all(pos != 0xFFFFFFFF)
        order = np.argsort(pos, kind="stable")
        m, pos = np.ascontiguousarray(msgs[order]), np.ascontiguousarray(pos[order])
        rc = self.eng.lib.gr_space_encode(buf.ctypes.data, 1, self.positions, self.depth,
                                          m.ctypes.data if len(m) else None, len(m),
                                          pos.ctypes.data if len(pos) else None)
        assert rc == 0, rc
        space.copy_(self.torch.from_numpy(buf))

    def _load(self, idx, recs, cc, snap):
        idx = np.asarray(idx, np.int64)
        if self.be == "cpu":
            self.state[idx], self.cc[idx], self.snap[idx] = recs, cc, snap
        else:
            self.eng.load_peers(idx.astype(np.uint32), recs)
            self.eng.set_cc_indexes(idx.astype(np.uint32), cc)
            self.eng.set_snapshot_recs(idx.astype(np.uint32), snap)

    def step(self, loc, allowed=(), keep=None):
        """One pass. allowed: escalation reasons the script causes this pass;
        keep(sender, receiver, msgs) -> bool mask: the messages the script lets
        through (None: all)."""
        k, before = self.k, self.ref
        st, snap, cc, nxt, res, rest = self._engine_pass(loc)
        lim = parity.limits_from(res, self.n)
        rst, rsnap, rcc, rout, rres, rrest, panic = ref_step(self.ref, self.refsnap, self.refcc, self.msgs, loc,
                                                              self.S, lim)
        assert np.all(panic < 0), (k, np.nonzero(panic >= 0)[0][:4])
        compare_pass(self.S, (st, snap, cc, nxt, res, rrest if rest is None else rest),
                     (rst, rsnap, rcc, self.topo.route_messages(rout), rres, rrest), f"pass {k}: ")
        if self.updates:
            self._collect(k, loc, before, res, st, rres, rst, rrest, rest)
        esc = res[res["escalation"] != 0]
        for r in esc:
            nm = abi.ESC_NAMES[r["escalation"]]
            self.esc[nm] = self.esc.get(nm, 0) + 1
            assert nm in allowed or nm not in ("unsupported", "election", "config_change", "snapshot"), \
                (k, int(r["peer"]), nm)
        if self.be == "cpu":
            self.state, self.snap, self.cc = st, snap, cc
        if len(esc):  # the host runs their suffix and reloads them with exact records
            rst, rsnap, rcc, rout, _, rrest, panic = ref_step(self.ref, self.refsnap, self.refcc, self.msgs, loc, self.S)
            assert np.all(panic < 0), (k, "the reference panicked in an escalated suffix")
            idx = esc["peer"].astype(np.int64)
            self._load(idx, rst[idx], rcc[idx], rsnap[idx])
            if self.be == "dev":
                self.dirty = True
            if self.updates:  # reloaded: the update state is the State the host already handed on
                hs = np.zeros(len(idx), abi.UPDATE_STATE)
                hs["term"], hs["vote"], hs["commit"] = rst["term"][idx], rst["vote"][idx], rst["committed"][idx]
                self.upd.prev[idx] = hs
                if self.be == "dev":
                    self.eng.set_update_states(idx.astype(np.uint32), hs)
        self._count(before, rst, rout, rrest)
        self.ref, self.refsnap, self.refcc = rst, rsnap, rcc
        out = self.topo.route_messages(rout)
        # a sender's engine slot: replica (its slot at the receiver) * G + group
        sender = out["slot"].astype(np.int64) * self.G + out["peer"].astype(np.int64) % self.G
        ok = ~self.muted[sender]
        if keep is not None:
            ok &= keep(sender, out["peer"].astype(np.int64), out)
        if not ok.all() and self.be == "dev":
            self.dirty = True
        self.msgs = out[ok]
        self.k += 1
        self._host(rrest)
        return res

    def _count(self, before, after, rout, rrest):
        c = self.count
        who = rrest["peer"].astype(np.int64)
        c["restores"] += len(who)
        c["restores_uncommitted"] += int(np.sum(before["last_index"][who] > before["committed"][who]))
        turned = (before["state"] != abi.LEADER) & (after["state"] == abi.LEADER)
        over = turned & (before["last_index"] > before["committed"])
        flag = (after["flags"] & PENDING) != 0
        c["promotions"] += int(turned.sum())
        c["promoted_flag"] += int(np.sum(over & flag))
        c["promoted_clear"] += int(np.sum(over & ~flag))
        c["promoted_restored"] += int(np.sum(turned & self.ever_restored))
        inst = rout[rout["type"] == INSTALL_SNAPSHOT]
        c["snapshots_sent"] += len(inst)
        c["snapshots_sent_flagged"] += int(np.sum(flag[inst["peer"].astype(np.int64)]))
        m = norm_marks(rout)
        c["marked_replicates"] += int(np.sum((m["type"] == abi.REPLICATE) & (m["reject"] != 0)))
        self.ever_restored[who] = True

    def _host(self, rrest):
        # the RSM recovers from the snapshot, then RestoreRemotes on those peers
        who = np.unique(rrest["peer"]).astype(np.uint32)
        if len(who):
            ms = self.same[:len(who)]
            rrc, rst = SN.ref_restore(self.ref, who, ms, self.S)
            assert rrc == 0 and not rst.any(), (rrc, rst)
            if self.be == "cpu":
                rc, stt = host_restore(self.state, who, ms, self.S)
            else:
                rc, stt = self.eng.restore_remotes(who, ms)
                assert len(self.eng.restored_snapshots()) == 0
            assert rc == 0 and not stt.any(), (rc, stt)
        uc = parity.update_commits(self.ref)
        new = CE.ref_commit_all(self.ref, self.S)  # the reference side commits every peer, reported or not
        if self.updates:
            self._commit_reported(rrest)
        elif self.be == "cpu":
            rc, stt = host_commit_update(self.state, self.all, uc, self.S)
            assert rc == 0, (rc, stt[stt != 0][:4])
            self.state["applied"] = new["applied"]
        else:
            rc, stt = self.eng.commit_update(self.all, uc)
            assert rc == 0, (rc, stt[stt != 0][:4])
            self.eng.notify_applied(self.all, new["applied"])
        self.ref = new
        # committed config changes: every replica that reached one applies it
        import config_change_common as CC
        applied = []
        if self.be != "cpu" and self.pending:  # the side records as they stand before the calls
            side0 = self.eng.get_cc_indexes(self.all), self.eng.get_snapshot_recs(self.all)
        for g, (index, term, done) in list(self.pending.items()):
            for r in range(self.R):
                p = r * self.G + g
                if p in done or int(self.ref[p]["committed"]) < index:
                    continue
                done.add(p)
                if CE._term_at(self.ref[p], index) != term:
                    continue  # another entry was committed there, or a snapshot covers it: the proposal was lost
                ch = np.zeros(1, abi.CONFIG_CHANGE)
                ch["node_id"], ch["type"] = self.ref[p]["remote_id"][0], abi.CC_ADD_NODE
                rc, stt = CC.ref_apply(self.ref, [p], ch, self.S)
                assert rc == 0 and int(stt[0]) == abi.CC_APPLIED, (rc, stt)
                assert not int(self.ref[p]["flags"]) & PENDING
                if self.be == "cpu":  # gr_config_change.h's host build, as Side.apply runs it
                    rc, stt = CC.host_apply(self.state, [p], ch, self.S)
                else:
                    rc, stt = self.eng.apply_config_change([p], ch)
                assert rc == 0 and int(stt[0]) == abi.CC_APPLIED, (rc, stt)
                applied.append(p)
            if len(done) == self.R:
                del self.pending[g]
        if applied:  # the call moves the peer record alone: state under parity, side records untouched
            if self.be == "cpu":
                got = self.state[applied]
            else:
                got = self.eng.sync_peers(applied)
                assert self.eng.get_cc_indexes(self.all).tobytes() == side0[0].tobytes()
                assert self.eng.get_snapshot_recs(self.all).tobytes() == side0[1].tobytes()
            bad = parity.compare_states(got, self.ref[applied], self.S)
            assert not bad, f"pass {self.k - 1}: after gr_apply_config_change {bad[:3]}"

    def propose_cc(self, loc, leaders):
        """Mark a config change in the proposals of `leaders` whose
        pendingConfigChange is clear; remembers (index, term) per group."""
        for p in leaders:
            p = int(p)
            if int(self.ref[p]["flags"]) & PENDING or (p % self.G) in self.pending:
                continue
            loc["propose_has_config_change"][p] = 1
            self.pending[p % self.G] = (int(self.ref[p]["last_index"]) + 1, int(self.ref[p]["term"]), set())

    def compact(self, idx, index, term):
        """The host compacts peers idx up to index[x] (gr_compact_log) and
        records the snapshot it took there (gr_set_snapshot_recs)."""
        idx = np.asarray(idx, np.uint32)
        rec = np.zeros(len(idx), abi.SNAPSHOT_REC)
        rec["index"], rec["term"] = index, term
        compact_records(self.ref, idx, index)
        self.refsnap[idx] = rec
        if self.be == "cpu":
            compact_records(self.state, idx, index)
            self.snap[idx] = rec
        else:
            rc, stt = self.eng.compact_log(idx, index)
            assert rc == 0 and not stt.any(), (rc, stt)
            self.eng.set_snapshot_recs(idx, rec)

    def close(self):
        if self.be != "cpu":
            self.eng.close()

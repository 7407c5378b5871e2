"""TEST INFRASTRUCTURE: bindings of tests/_build/libhostlane_cc*.so and the
driver the config-change-entry tests share.

host_step: the engine's lane code on the CPU with config entries compiled on
(tests/native/hostlane_cc.hip), over records plus the gr_cc_index records.
ref_step: the reference side, the oracle's raft object built from the same
records with typed in-memory entries (tests/native/config_entries_ref.cpp).
Side runs one backend (the host lane, or an Engine) beside the reference and
compares everything a pass leaves: peer records, messages, results and the
records. Marks at or below a message's commit and record values at or below
committed are stale (gpuraft.h) and compare as 0.
"""
import ctypes
import os

import numpy as np

from dragonboat_amd import abi
import parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = {False: os.path.join(ROOT, "tests", "_build", "libhostlane_cc.so"),
        True: os.path.join(ROOT, "tests", "_build", "libhostlane_cc_elect.so")}
_libs = {}

ESC = {"term_window": 1, "random": 2, "unsupported": 3, "election": 4, "panic": 5, "capacity": 6, "snapshot": 7,
       "config_change": 11}
PENDING = 0x04  # GR_F_PENDING_CONFIG_CHANGE


def lib(elect=False):
    """The host lane with config entries on; elect: with elections on too."""
    if elect not in _libs:
        c = ctypes
        l = c.CDLL(LIBS[elect])
        l.hl_step_cc.argtypes = [c.c_uint32, c.c_uint64, c.c_void_p, c.c_uint32, c.POINTER(abi.Inbox), c.c_void_p,
                                 c.c_size_t, c.POINTER(c.c_size_t), c.c_void_p, c.POINTER(c.c_size_t), c.c_void_p]
        l.ccr_step.argtypes = [c.c_uint32, c.c_uint64, c.c_void_p, c.c_uint32, c.POINTER(abi.Inbox), c.c_void_p,
                               c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t), c.c_void_p,
                               c.POINTER(c.c_size_t), c.c_void_p]
        l.hl_coverage_cc.argtypes = [c.c_void_p, c.c_uint32]
        l.hl_coverage_cc_names.restype = c.c_char_p
        l.hl_coverage.argtypes = [c.c_void_p, c.c_uint32]
        l.hl_coverage_names.restype = c.c_char_p
        _libs[elect] = l
    return _libs[elect]


def _inbox(msgs, loc):
    msgs = np.zeros(0, abi.MESSAGE) if msgs is None else np.ascontiguousarray(msgs, abi.MESSAGE)
    loc = np.zeros(0, abi.LOCAL) if loc is None else np.ascontiguousarray(loc, abi.LOCAL)
    return msgs, loc, abi.inbox_of(msgs, loc)


def host_step(peers, cc, msgs, loc, S, elect=False, rc_ok=(0,)):
    """One pass of the host lane: (peers', cc', messages, results), or the
    return code when it is not 0 (and listed in rc_ok)."""
    peers = np.array(peers, abi.PEER, copy=True)
    cc = np.array(cc, abi.CC_INDEX, copy=True)
    msgs, loc, ib = _inbox(msgs, loc)
    cap = max(16, 8 * len(peers) * S)
    out, res = np.zeros(cap, abi.MESSAGE), np.zeros(len(peers), abi.RESULT)
    n_out, n_res = ctypes.c_size_t(), ctypes.c_size_t()
    rc = lib(elect).hl_step_cc(S, abi.MAX_ENTRY_SIZE, peers.ctypes.data, len(peers), ctypes.byref(ib),
                               out.ctypes.data, cap, ctypes.byref(n_out), res.ctypes.data, ctypes.byref(n_res),
                               cc.ctypes.data)
    assert rc in rc_ok, rc
    if rc:
        return rc
    return peers, cc, out[:n_out.value], res[:n_res.value]


def ref_step(peers, cc, msgs, loc, S, limits=None):
    """The same pass on the reference side, each peer stopped before item
    limits[p]: (peers', cc', messages, results by peer, the item at which the
    oracle panicked or -1, by peer)."""
    peers = np.array(peers, abi.PEER, copy=True)
    cc = np.array(cc, abi.CC_INDEX, copy=True)
    msgs, loc, ib = _inbox(msgs, loc)
    n = len(peers)
    cap = max(16, 8 * n * S)
    out, res = np.zeros(cap, abi.MESSAGE), np.zeros(n, abi.RESULT)
    n_out, n_res = ctypes.c_size_t(), ctypes.c_size_t()
    panic = np.full(n, -1, np.int32)
    lim = None if limits is None else np.ascontiguousarray(limits, np.uint32)
    rc = lib().ccr_step(S, abi.MAX_ENTRY_SIZE, peers.ctypes.data, n, ctypes.byref(ib),
                        None if lim is None else lim.ctypes.data, cc.ctypes.data, out.ctypes.data, cap,
                        ctypes.byref(n_out), res.ctypes.data, ctypes.byref(n_res), panic.ctypes.data)
    assert rc == 0, rc
    by_peer = np.zeros(n, abi.RESULT)
    r = res[:n_res.value]
    by_peer[r["peer"]] = r
    return peers, cc, out[:n_out.value], by_peer, panic


def norm_cc(cc, committed):
    """Record values at or below committed are stale: they compare as 0."""
    cc = np.array(cc, abi.CC_INDEX, copy=True)
    for f in ("last", "prev"):
        cc[f] = np.where(cc[f] > committed, cc[f], 0)
    # a stale `last` above a live `prev` cannot be (last > prev); a stale pair is (0, 0)
    return cc


def norm_marks(msgs):
    """A Replicate's marks at or below its own commit may be omitted: they
    compare as 0, and a message left without a mark as unmarked."""
    m = np.array(msgs, abi.MESSAGE, copy=True)
    rep = (m["type"] == abi.REPLICATE) & (m["reject"] != 0)
    for f in ("hint_high", "hint"):
        m[f] = np.where(rep & (m[f] <= m["commit"]), 0, m[f])
    m["reject"] = np.where(rep & (m["hint"] == 0), 0, m["reject"])
    return m


def cc_recs(n, last=0, prev=0):
    r = np.zeros(n, abi.CC_INDEX)
    r["last"], r["prev"] = last, prev
    return r


class Side:
    """`peers` and their gr_cc_index records on one backend (cpu: the host lane
    over records; gpu: an Engine) beside the reference side, stepped together.
    on = False: the switch off (the default host lane, a default Engine); the
    reference side is then not consulted."""

    def __init__(self, be, peers, S, cc=None, elect=False, on=True, lib_path=None):
        self.be, self.S, self.n, self.elect, self.on = be, S, len(peers), elect, on
        self.cc = np.zeros(self.n, abi.CC_INDEX) if cc is None else np.array(cc, abi.CC_INDEX)
        self.all = np.arange(self.n, dtype=np.uint32)
        if be == "gpu":
            from dragonboat_amd.engine import Engine
            self.eng = Engine(self.n, S, config_entries=on, elections=elect, lib_path=lib_path)
            assert self.eng.get_config_entries() == on
            self.eng.load(peers)
            self.eng.set_cc_indexes(self.all, self.cc)
            self.state = self.eng.sync(self.n)
        else:
            from oracle.pyoracle import hostlane_step
            self.state, _, _ = hostlane_step(peers, None, None, S)  # a load and a sync
        self.ref = self.state.copy()

    def raw(self, msgs=None, loc=None):
        """One pass on the engine side alone: (state, cc, messages, results)."""
        if self.be == "gpu":
            out, res = self.eng.step(msgs, loc)
            return self.eng.sync(self.n), self.eng.get_cc_indexes(self.all), out, res
        if self.on:
            return host_step(self.state, self.cc, msgs, loc, self.S, self.elect)
        if self.elect:  # the elections build of the default host lane (elections_common.py)
            import elections_common as EC
            be = EC.ElectHostlaneBackend(self.state, self.S)
            m, l, _ = _inbox(msgs, loc)
            out, res = be.step(m, l)
            return be.state, self.cc.copy(), out, res
        from oracle.pyoracle import hostlane_step
        st, out, res = hostlane_step(self.state, msgs, loc, self.S)
        return st, self.cc.copy(), out, res

    def step(self, msgs=None, loc=None, esc=None):
        """One pass on both sides, compared field for field. esc: {peer: reason}
        the pass must escalate with, exactly (None: no escalation). Returns
        (state, messages, results, cc)."""
        st, cc, out, res = self.raw(msgs, loc)
        got = {int(r["peer"]): int(r["escalation"]) for r in res if r["escalation"]}
        want = {int(p): ESC[v] for p, v in (esc or {}).items()}
        assert got == want, (got, want, [(int(r["peer"]), int(r["esc_item"])) for r in res if r["escalation"]])
        lim = parity.limits_from(res, self.n)
        rst, rcc, rout, rres, panic = ref_step(self.ref, self.cc, msgs, loc, self.S, lim)
        assert np.all(panic < 0), panic  # every reference panic lies at or past an escalation
        bad = parity.compare_states(st, rst, self.S)
        assert not bad, bad[:3]
        a, b = norm_cc(cc, st["committed"]), norm_cc(rcc, rst["committed"])
        assert a.tobytes() == b.tobytes(), (cc, rcc)
        bad = parity.compare_msgs(norm_marks(out), norm_marks(rout))
        assert not bad, bad[:3]
        bad = parity.compare_results(res, rres)
        assert not bad, bad[:3]
        self.state, self.ref, self.cc = st, rst, cc
        return st, out, res, cc

    def close(self):
        if self.be == "gpu":
            self.eng.close()


# ---------------------------------------------------------------- live populations
def ref_commit_all(peers, S):
    """The host persists and applies everything (the oracle's commit_peer) on records."""
    peers = np.array(peers, abi.PEER, copy=True)
    l = lib()
    l.ccr_commit_all.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32]
    rc = l.ccr_commit_all(S, abi.MAX_ENTRY_SIZE, peers.ctypes.data, len(peers))
    assert rc == 0, rc
    return peers


def _term_at(rec, idx):
    t = 0
    for k in range(int(rec["n_runs"])):
        if int(rec["run_start"][k]) <= idx:
            t = int(rec["run_term"][k])
    return t


class Population:
    """G groups x R replicas (replica-major) on one backend beside the reference
    side, with elections and config entries on: "cpu" the host lane over records,
    "gpu" an Engine through gr_step, "dev" an Engine on the device-resident
    schedule (gr_step_device over loopback spaces, as devsim.DeviceLockstep runs
    it). Every pass is compared at the device prefix (state, records, messages,
    results); an escalated peer's pass is finished by the reference, as the host
    would, and the peer reloaded with its exact record. After a pass the host
    persists and applies everything, and applies a committed config change on every
    replica that reached it (gr_apply_config_change; the change re-adds a voter,
    which only clears pendingConfigChange, raft.go:822-828)."""

    def __init__(self, be, peers, G, R, lib_path=None):
        from dragonboat_amd import populations as P
        self.be, self.G, self.R, self.S, self.n = be, G, R, R, G * R
        self.topo = P.Topology(G, R)
        self.ref = np.array(peers, abi.PEER, copy=True)
        self.refcc = np.zeros(self.n, abi.CC_INDEX)
        self.all = np.arange(self.n, dtype=np.uint32)
        self.msgs = np.zeros(0, abi.MESSAGE)  # the next inbox (receiver peer, sender slot)
        self.muted = np.zeros(self.n, bool)    # peers whose messages are dropped for good
        self.esc = {}                          # reason -> count
        self.promoted_pending = 0              # promotions that set pendingConfigChange
        self.pending = {}                      # group -> (index, term, replicas applied)
        self.k = 0
        if be == "cpu":
            from oracle.pyoracle import hostlane_step
            self.state, _, _ = hostlane_step(peers, None, None, self.S)
            self.cc = np.zeros(self.n, abi.CC_INDEX)
            self.ref = self.state.copy()
            return
        from dragonboat_amd.engine import Engine
        self.eng = Engine(self.n, self.S, config_entries=True, elections=True, lib_path=lib_path)
        assert self.eng.get_config_entries() and self.eng.get_elections()
        self.eng.load(peers)
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

    # -- one pass on the engine side: (state, cc, messages as the next inbox's records, results)
    def _engine_pass(self, loc):
        if self.be == "cpu":
            st, cc, out, res = host_step(self.state, self.cc, self.msgs, loc, self.S, elect=True)
            return st, cc, self.topo.route_messages(out), res
        if self.be == "gpu":
            out, res = self.eng.step(self.msgs, loc)
            return self.eng.sync(self.n), self.eng.get_cc_indexes(self.all), self.topo.route_messages(out), res
        from dragonboat_amd.engine import decode_space
        src, dst = self.spaces[self.k % 2], self.spaces[(self.k + 1) % 2]
        if self.dirty:
            self._encode(self.msgs, src)
            self.dirty = False
        self.eng.set_locals(loc)
        self.eng.step_device(src.data_ptr(), dst.data_ptr(), 1, self.positions, 1, self.positions, self.n,
                             self.stream.cuda_stream, depth=self.depth)
        self.torch.cuda.synchronize()
        res = self.eng.collect_results(self.n)
        got = decode_space(dst.cpu().numpy(), 1, self.positions, self.depth)
        pos = got["peer"].astype(np.int64)
        got["peer"] = self.inv[0][pos].astype(np.uint32)
        got["slot"] = self.inv[1][pos].astype(np.uint8)
        return self.eng.sync(self.n), self.eng.get_cc_indexes(self.all), got, res

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

    def _load(self, idx, recs, cc):
        idx = np.asarray(idx, np.int64)
        if self.be == "cpu":
            self.state[idx], self.cc[idx] = recs, cc
        else:
            self.eng.load_peers(idx.astype(np.uint32), recs)
            self.eng.set_cc_indexes(idx.astype(np.uint32), cc)

    def step(self, loc, allowed=()):
        """One pass; `allowed`: escalation reasons the script causes this pass."""
        k = self.k
        before = self.ref
        st, cc, nxt, res = self._engine_pass(loc)
        lim = parity.limits_from(res, self.n)
        rst, rcc, rout, rres, panic = ref_step(self.ref, self.refcc, self.msgs, loc, self.S, lim)
        assert np.all(panic < 0), (k, np.nonzero(panic >= 0)[0][:4])
        bad = parity.compare_states(st, rst, self.S)
        assert not bad, f"pass {k}: state {bad[:3]}"
        a, b = norm_cc(cc, st["committed"]), norm_cc(rcc, rst["committed"])
        assert a.tobytes() == b.tobytes(), f"pass {k}: records {np.nonzero(a != b)[0][:4]}"
        bad = parity.compare_msgs(norm_marks(nxt), norm_marks(self.topo.route_messages(rout)))
        assert not bad, f"pass {k}: messages {bad[:3]}"
        bad = parity.compare_results(res, rres)
        assert not bad, f"pass {k}: results {bad[:3]}"
        esc = res[res["escalation"] != 0]
        for r in esc:
            nm = abi.ESC_NAMES[r["escalation"]]
            self.esc[nm] = self.esc.get(nm, 0) + 1
            assert nm in allowed or nm not in ("unsupported", "election", "config_change"), (k, int(r["peer"]), nm)
        if len(esc):  # the host runs their suffix and reloads them with exact records
            rst, rcc, rout, _, panic = ref_step(self.ref, self.refcc, self.msgs, loc, self.S)
            assert np.all(panic < 0), (k, "the reference panicked in an escalated suffix")
            idx = esc["peer"].astype(np.int64)
            if self.be == "cpu":
                self.state, self.cc = st, cc
            self._load(idx, rst[idx], rcc[idx])
            if self.be == "dev":
                self.dirty = True
        elif self.be == "cpu":
            self.state, self.cc = st, cc
        turned = (before["state"] != abi.LEADER) & (rst["state"] == abi.LEADER)
        self.promoted_pending += int(np.sum(turned & ((rst["flags"] & PENDING) != 0)))
        self.ref, self.refcc = rst, rcc
        out = self.topo.route_messages(rout)
        # a sender's engine slot: replica (its slot at the receiver) * G + group
        sender = out["slot"].astype(np.int64) * self.G + out["peer"].astype(np.int64) % self.G
        keep = ~self.muted[sender]
        if not keep.all() and self.be == "dev":
            self.dirty = True
        self.msgs = out[keep]
        self.k += 1
        self._host_applies()
        return res

    def _host_applies(self):
        uc = parity.update_commits(self.ref)
        new = ref_commit_all(self.ref, self.S)
        if self.be == "cpu":
            from oracle.pyoracle import hostlane_commit_update
            rc, stt = hostlane_commit_update(self.state, self.all, uc, self.S)
            assert rc == 0, (rc, stt[stt != 0][:4])
            self.state["applied"] = new["applied"]
        else:
            rc, stt = self.eng.commit_update(self.all, uc)
            assert rc == 0, (rc, stt[stt != 0][:4])
            self.eng.notify_applied(self.all, new["applied"])
        self.ref = new
        # committed config changes: every replica that reached one applies it
        for g, (index, term, done) in list(self.pending.items()):
            for r in range(self.R):
                p = r * self.G + g
                if p in done or int(self.ref[p]["committed"]) < index:
                    continue
                done.add(p)
                if _term_at(self.ref[p], index) != term:
                    continue  # another entry was committed there: the proposal was lost
                self.ref["flags"][p] &= ~np.uint8(PENDING)
                if self.be == "cpu":
                    self.state["flags"][p] &= ~np.uint8(PENDING)
                else:
                    ch = np.zeros(1, abi.CONFIG_CHANGE)
                    ch["node_id"], ch["type"] = self.ref[p]["remote_id"][0], abi.CC_ADD_NODE
                    rc, stt = self.eng.apply_config_change([p], ch)
                    assert rc == 0 and int(stt[0]) == abi.CC_APPLIED, (rc, stt)
            if len(done) == self.R:
                del self.pending[g]

    def propose_cc(self, loc, leaders):
        """Mark a config change in the proposals of `leaders` whose
        pendingConfigChange is clear; remembers (index, term) per group."""
        for p in leaders:
            p = int(p)
            if int(self.ref[p]["flags"]) & PENDING or (p % self.G) in self.pending:
                continue
            loc["propose_has_config_change"][p] = 1
            self.pending[p % self.G] = (int(self.ref[p]["last_index"]) + 1, int(self.ref[p]["term"]), set())

    def close(self):
        if self.be != "cpu":
            self.eng.close()

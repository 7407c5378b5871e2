"""TEST INFRASTRUCTURE: bindings of tests/_build/libhostlane_snap*.so and the
driver the snapshot tests share.

host_step: the engine's lane code on the CPU with snapshots compiled on
(tests/native/hostlane_snap.hip), over records plus the snapshot records and the
restored list. ref_step: the reference side, the oracle's raft object built from
the same records and driven through the pass's items (tests/native/
snapshot_ref.cpp). host_restore / ref_restore: gr_restore_remotes the same way.
Side runs one backend (the host lane, or an Engine) beside the reference and
compares everything a pass leaves: peer records, snapshot records, messages,
results and the restored list.
"""
import ctypes
import os

import numpy as np

from dragonboat_amd import abi
import parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = {False: os.path.join(ROOT, "tests", "_build", "libhostlane_snap.so"),
        True: os.path.join(ROOT, "tests", "_build", "libhostlane_snap_elect.so")}
_libs = {}

INSTALL_SNAPSHOT = 16  # gr_msg_type GR_INSTALL_SNAPSHOT
ESC = {"term_window": 1, "random": 2, "unsupported": 3, "election": 4, "panic": 5, "capacity": 6, "snapshot": 7}


def lib(elect=False):
    """The host lane with snapshots on; elect: with elections on too."""
    if elect not in _libs:
        c = ctypes
        l = c.CDLL(LIBS[elect])
        l.hl_step_snap.argtypes = [c.c_uint32, c.c_uint64, c.c_void_p, c.c_uint32, c.POINTER(abi.Inbox), c.c_void_p,
                                   c.c_size_t, c.POINTER(c.c_size_t), c.c_void_p, c.POINTER(c.c_size_t), c.c_void_p,
                                   c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t)]
        l.snr_step.argtypes = [c.c_uint32, c.c_uint64, c.c_void_p, c.c_uint32, c.POINTER(abi.Inbox), c.c_void_p,
                               c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t), c.c_void_p,
                               c.POINTER(c.c_size_t), c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t), c.c_void_p]
        l.hl_restore_remotes.argtypes = [c.c_uint32, c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p, c.c_uint32,
                                         c.c_void_p]
        l.snr_restore_remotes.argtypes = [c.c_uint32, c.c_uint64, c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p,
                                          c.c_uint32, c.c_void_p]
        l.hl_coverage_snap.argtypes = [c.c_void_p, c.c_uint32]
        l.hl_coverage_snap_names.restype = c.c_char_p
        l.hl_steady_lanes.restype = c.c_uint64
        l.hl_counters.argtypes = [c.POINTER(c.c_uint64), c.POINTER(c.c_uint64)]
        l.hl_counters.restype = None
        _libs[elect] = l
    return _libs[elect]


def _inbox(msgs, loc):
    msgs = np.zeros(0, abi.MESSAGE) if msgs is None else np.ascontiguousarray(msgs, abi.MESSAGE)
    loc = np.zeros(0, abi.LOCAL) if loc is None else np.ascontiguousarray(loc, abi.LOCAL)
    return msgs, loc, abi.inbox_of(msgs, loc)


def host_step(peers, snap, msgs, loc, S, elect=False):
    """One pass of the host lane: (peers', snap', messages, results, restored)."""
    peers = np.array(peers, abi.PEER, copy=True)
    snap = np.array(snap, abi.SNAPSHOT_REC, copy=True)
    msgs, loc, ib = _inbox(msgs, loc)
    cap = max(16, 8 * len(peers) * S)
    out, res, rest = np.zeros(cap, abi.MESSAGE), np.zeros(len(peers), abi.RESULT), np.zeros(2 * len(peers), abi.RESTORED)
    n_out, n_res, n_rest = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    rc = lib(elect).hl_step_snap(S, abi.MAX_ENTRY_SIZE, peers.ctypes.data, len(peers), ctypes.byref(ib),
                                 out.ctypes.data, cap, ctypes.byref(n_out), res.ctypes.data, ctypes.byref(n_res),
                                 snap.ctypes.data, rest.ctypes.data, len(rest), ctypes.byref(n_rest))
    assert rc == 0, rc
    return peers, snap, out[:n_out.value], res[:n_res.value], rest[:n_rest.value]


def ref_step(peers, snap, msgs, loc, S, limits=None):
    """The same pass on the reference side, each peer stopped before item
    limits[p]: (peers', snap', messages, results by peer, restored, the item at
    which the oracle panicked or -1, by peer)."""
    peers = np.array(peers, abi.PEER, copy=True)
    snap = np.array(snap, abi.SNAPSHOT_REC, copy=True)
    msgs, loc, ib = _inbox(msgs, loc)
    n = len(peers)
    cap = max(16, 8 * n * S)
    out, res, rest = np.zeros(cap, abi.MESSAGE), np.zeros(n, abi.RESULT), np.zeros(cap, abi.RESTORED)
    n_out, n_res, n_rest = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    panic = np.full(n, -1, np.int32)
    lim = None if limits is None else np.ascontiguousarray(limits, np.uint32)
    rc = lib().snr_step(S, abi.MAX_ENTRY_SIZE, peers.ctypes.data, n, ctypes.byref(ib),
                        None if lim is None else lim.ctypes.data, snap.ctypes.data, out.ctypes.data, cap,
                        ctypes.byref(n_out), res.ctypes.data, ctypes.byref(n_res), rest.ctypes.data, cap,
                        ctypes.byref(n_rest), panic.ctypes.data)
    assert rc == 0, rc
    by_peer = np.zeros(n, abi.RESULT)
    r = res[:n_res.value]
    by_peer[r["peer"]] = r
    return peers, snap, out[:n_out.value], by_peer, rest[:n_rest.value], panic


def membership(ids_kinds, rand=0):
    """One abi.MEMBERSHIP record from [(node id, kind), ...]."""
    m = np.zeros(1, abi.MEMBERSHIP)
    for k, (i, kind) in enumerate(ids_kinds):
        m[0]["node_id"][k], m[0]["kind"][k] = i, kind
    m[0]["rand"] = rand
    return m


def _rr_args(peers, idx, ms):
    assert peers.flags["C_CONTIGUOUS"] and peers.dtype == abi.PEER
    idx = np.ascontiguousarray(idx, np.uint32)
    ms = np.ascontiguousarray(ms, abi.MEMBERSHIP)
    assert len(idx) == len(ms)
    return idx, ms, np.full(len(idx), -1, np.int32)


def host_restore(peers, idx, ms, S):
    """The engine's code on records, in place: (rc, status) as gr_restore_remotes."""
    idx, ms, st = _rr_args(peers, idx, ms)
    rc = lib().hl_restore_remotes(S, peers.ctypes.data, len(peers), idx.ctypes.data, ms.ctypes.data, len(idx),
                                  st.ctypes.data)
    return rc, st


def ref_restore(peers, idx, ms, S):
    """The reference side on records, in place: (rc, status)."""
    idx, ms, st = _rr_args(peers, idx, ms)
    rc = lib().snr_restore_remotes(S, abi.MAX_ENTRY_SIZE, peers.ctypes.data, len(peers), idx.ctypes.data,
                                   ms.ctypes.data, len(idx), st.ctypes.data)
    assert rc in (0, -6), rc
    return rc, st


def _rest_key(r):
    return sorted((int(x["peer"]), int(x["index"]), int(x["term"])) for x in r)


class Side:
    """`peers` and their snapshot records on one backend (cpu: the host lane over
    records; gpu: an Engine) beside the reference side, stepped together. on =
    False: the switch off (the default host lane, a default Engine)."""

    def __init__(self, be, peers, S, snap=None, elect=False, on=True):
        self.be, self.S, self.n, self.elect, self.on = be, S, len(peers), elect, on
        self.snap = np.zeros(self.n, abi.SNAPSHOT_REC) if snap is None else np.array(snap, abi.SNAPSHOT_REC)
        self.all = np.arange(self.n, dtype=np.uint32)
        if be == "gpu":
            from dragonboat_amd.engine import Engine
            self.eng = Engine(self.n, S, snapshots=on, elections=elect)
            assert self.eng.get_snapshots() == on
            self.eng.load(peers)
            self.eng.set_snapshot_recs(self.all, self.snap)
            self.state = self.eng.sync(self.n)
        else:
            from oracle.pyoracle import hostlane_step
            self.state, _, _ = hostlane_step(peers, None, None, S)  # a load and a sync
        self.ref = self.state.copy()
        self.restored = []  # every record drained so far

    def step(self, msgs=None, loc=None, esc=None):
        """One pass on both sides, compared field for field. esc: {peer: reason}
        the pass must escalate with, exactly (None: no escalation). Returns
        (state, messages, results, restored)."""
        if self.be == "gpu":
            out, res = self.eng.step(msgs, loc)
            st = self.eng.sync(self.n)
            snap = self.eng.get_snapshot_recs(self.all)
            rest = self.eng.restored_snapshots()
        elif self.on:
            st, snap, out, res, rest = host_step(self.state, self.snap, msgs, loc, self.S, self.elect)
        else:
            from oracle.pyoracle import hostlane_step
            st, out, res = hostlane_step(self.state, msgs, loc, self.S)
            snap, rest = self.snap.copy(), np.zeros(0, abi.RESTORED)
        got = {int(r["peer"]): int(r["escalation"]) for r in res if r["escalation"]}
        want = {int(p): ESC[v] for p, v in (esc or {}).items()}
        assert got == want, (got, want, [(int(r["peer"]), int(r["esc_item"])) for r in res if r["escalation"]])
        lim = parity.limits_from(res, self.n)
        rst, rsnap, rout, rres, rrest, panic = ref_step(self.ref, self.snap, msgs, loc, self.S, lim)
        assert np.all(panic < 0), panic  # every reference panic lies at or past an escalation
        bad = parity.compare_states(st, rst, self.S)
        assert not bad, bad[:3]
        assert snap.tobytes() == rsnap.tobytes(), (snap, rsnap)
        bad = parity.compare_msgs(out, rout)
        assert not bad, bad[:3]
        bad = parity.compare_results(res, rres)
        assert not bad, bad[:3]
        assert _rest_key(rest) == _rest_key(rrest), (rest, rrest)
        self.state, self.ref, self.snap = st, rst, snap
        self.restored.extend(_rest_key(rest))
        return st, out, res, rest

    def restore_raw(self, idx, ms):
        """gr_restore_remotes on the engine side alone: (rc or the raised error's
        code, status, state after)."""
        from dragonboat_amd.engine import GpuRaftError
        if self.be == "gpu":
            try:
                rc, st = self.eng.restore_remotes(idx, ms)
            except GpuRaftError as e:
                rc, st = int(str(e).rsplit("(", 1)[1].rstrip(")")), None
            new = self.eng.sync(self.n)
        else:
            new = self.state.copy()
            rc, st = host_restore(new, idx, ms, self.S)
        return rc, st, new

    def restore(self, idx, ms):
        """One gr_restore_remotes on both sides; returns the statuses. Refused and
        unlisted peers are untouched bit for bit, the others equal the reference."""
        idx = np.asarray(idx, np.uint32)
        old = self.state.copy()
        rc, st, new = self.restore_raw(idx, ms)
        ref = self.ref.copy()
        # the reference's own export drops a removed node's ack (it maps ids through
        # member slots); the record that went in carries it, as the reference does
        for f in ("from_slot", "ack_bits"):
            ref["read_index"][f] = np.where(np.arange(abi.GR_Q)[None, :] < ref["read_index_count"][:, None],
                                            old["read_index"][f], ref["read_index"][f])
        rrc, rst = ref_restore(ref, idx, ms, self.S)
        assert st is not None and list(st) == list(rst), (st, rst)
        assert rc == rrc == (-6 if np.any(st != 0) else 0), (rc, rrc)
        touched = np.zeros(self.n, bool)
        touched[idx[st == 0]] = True
        assert new[~touched].tobytes() == old[~touched].tobytes(), "a refused or unlisted peer changed"
        bad = parity.compare_states(new, ref, self.S)
        assert not bad, bad[:3]
        self.state, self.ref = new, ref
        return st

    def close(self):
        if self.be == "gpu":
            self.eng.close()

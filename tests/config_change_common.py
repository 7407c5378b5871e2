"""TEST INFRASTRUCTURE: bindings of tests/_build/libconfig_change_host.so and the
drivers the membership-change tests share.

host_apply: gr_config_change.h (what gr_apply_config_change runs on the device)
over gr_peer records. ref_apply: the reference side, the oracle's raft object
built from the record, changed by raft::addNode / addObserver / removeNode /
clearPendingConfigChange and exported again (tests/native/config_change_ref.cpp).
"""
import ctypes
import os

import numpy as np

from dragonboat_amd import abi
from oracle.pyoracle import OraclePopulation, hostlane_step
import parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "_build", "libconfig_change_host.so")
_lib = None

# gr_layout.h: the header's remote summaries, the commit lag field, F_LSLOT in the flags byte
H_SYNC_MASK = (7 << 56) | (1 << 59) | (7 << 40)
H_CL_MASK = 7 << 21
H_RUN_MASK = (1 << 60) | (1 << 61)
H_GE_LO = 1 << 9
H_F_LSLOT = 0x38 << 10


def lib():
    global _lib
    if _lib is None:
        c = ctypes
        l = c.CDLL(LIB)
        l.cch_apply.argtypes = [c.c_uint32, c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p, c.c_uint32, c.c_void_p]
        l.ccr_apply.argtypes = [c.c_uint32, c.c_uint64, c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p, c.c_uint32,
                                c.c_void_p]
        l.cch_headers.argtypes = [c.c_uint32, c.c_void_p, c.c_void_p, c.POINTER(c.c_uint64), c.POINTER(c.c_uint64)]
        _lib = l
    return _lib


def changes(n, type_, node_id, rand=0):
    cc = np.zeros(n, abi.CONFIG_CHANGE)
    cc["type"], cc["node_id"], cc["rand"] = type_, node_id, rand
    return cc


def _args(peers, idx, cc):
    assert peers.flags["C_CONTIGUOUS"] and peers.dtype == abi.PEER
    idx = np.ascontiguousarray(idx, np.uint32)
    cc = np.ascontiguousarray(cc, abi.CONFIG_CHANGE)
    assert len(idx) == len(cc)
    return idx, cc, np.full(len(idx), -1, np.int32)


def host_apply(peers, idx, cc, S):
    """The engine's code on records, in place: (rc, status) as gr_apply_config_change."""
    idx, cc, st = _args(peers, idx, cc)
    rc = lib().cch_apply(S, peers.ctypes.data, len(peers), idx.ctypes.data, cc.ctypes.data, len(idx), st.ctypes.data)
    return rc, st


def ref_apply(peers, idx, cc, S):
    """The reference side on records, in place: (rc, status)."""
    idx, cc, st = _args(peers, idx, cc)
    rc = lib().ccr_apply(S, abi.MAX_ENTRY_SIZE, peers.ctypes.data, len(peers), idx.ctypes.data, cc.ctypes.data,
                         len(idx), st.ctypes.data)
    assert rc in (0, -6), rc
    return rc, st


def headers(peer, cc, S):
    """(status, header word as loaded, header word after the change) of one record."""
    peer = np.ascontiguousarray(peer, abi.PEER)
    cc = np.ascontiguousarray(cc, abi.CONFIG_CHANGE)
    b, a = ctypes.c_uint64(), ctypes.c_uint64()
    rc = lib().cch_headers(S, peer.ctypes.data, cc.ctypes.data, ctypes.byref(b), ctypes.byref(a))
    return rc, b.value, a.value


class Side:
    """`peers` on one backend (cpu: the host build over records; gpu: an Engine)
    and in an OraclePopulation, changed and stepped together."""

    def __init__(self, be, peers, S):
        self.be, self.S, self.n = be, S, len(peers)
        self.pop = OraclePopulation(peers, S)
        if be == "gpu":
            from dragonboat_amd.engine import Engine
            self.eng = Engine(self.n, S)
            self.eng.load(peers)
            self.state = self.eng.sync(self.n)
        else:
            self.state, _, _ = hostlane_step(peers, None, None, S)  # a load and a sync: the record as the engine keeps it

    def apply_raw(self, idx, cc):
        """The call on the engine side alone: (rc or the raised error's code, status, state after)."""
        from dragonboat_amd.engine import GpuRaftError
        if self.be == "gpu":
            try:
                rc, st = self.eng.apply_config_change(idx, cc)
            except GpuRaftError as e:
                rc, st = int(str(e).rsplit("(", 1)[1].rstrip(")")), None
            new = self.eng.sync(self.n)
        else:
            new = self.state.copy()
            rc, st = host_apply(new, idx, cc, self.S)
        return rc, st, new

    def change(self, idx, cc):
        """One gr_apply_config_change on both sides; returns the statuses. Peers
        whose status is not applied are untouched, the others equal the reference."""
        idx = np.asarray(idx, np.uint32)
        old = self.state.copy()
        rc, st, new = self.apply_raw(idx, cc)
        ref = self.pop.export()
        # the population's own export drops a removed node's ack (it maps ids through
        # member slots); the record that went in carries it, as the reference does
        for f in ("from_slot", "ack_bits"):
            ref["read_index"][f] = np.where(np.arange(abi.GR_Q)[None, :] < ref["read_index_count"][:, None],
                                            old["read_index"][f], ref["read_index"][f])
        rrc, rst = ref_apply(ref, idx, cc, self.S)
        assert st is not None and list(st) == list(rst), (st, rst)
        assert rc == rrc == (-6 if np.any(st != 0) else 0), (rc, rrc)
        touched = np.zeros(self.n, bool)
        touched[idx[st == 0]] = True
        assert new[~touched].tobytes() == old[~touched].tobytes(), "a refused or unlisted peer changed"
        bad = parity.compare_states(new, ref, self.S)
        assert not bad, bad[:3]
        ok = idx[st == 0]
        if len(ok):
            self.pop.reload(ok, ref[ok])
        self.state = new
        return st

    def step(self, msgs=None, loc=None):
        """One pass on both sides under parity (state, messages, results)."""
        msgs = np.zeros(0, abi.MESSAGE) if msgs is None else msgs
        loc = np.zeros(0, abi.LOCAL) if loc is None else loc
        if self.be == "gpu":
            out, res = self.eng.step(msgs, loc)
            st = self.eng.sync(self.n)
        else:
            st, out, res = hostlane_step(self.state, msgs, loc, self.S)
        lim = parity.limits_from(res, self.n)
        o = self.pop.step(msgs, loc, lim)
        assert not parity.compare_states(st, o["mid"], self.S)
        assert not parity.compare_msgs(out, parity.prefix_msgs(o, lim))
        assert not parity.compare_results(res, o["results"])
        self.state = st
        return st, out, res

    def close(self):
        if self.be == "gpu":
            self.eng.close()

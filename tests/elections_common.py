"""Shared pieces of the election tests (test_elections_hostlane.py on the CPU,
test_elections_gpu.py on the device): the host-lane backend built with elections
on, the cold-start population and its lockstep run."""
import ctypes
import os

import numpy as np

from dragonboat_amd import abi, populations as P
import simulate as SIM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_elib = None


def hostlane_elect_lib():
    """tests/_build/libhostlane_elect.so (build.build_hostlane_elect): the host
    lane compiled with -DGR_ELECTIONS_FORCE=1, bound as pyoracle binds the default."""
    global _elib
    if _elib is None:
        from dragonboat_amd import build
        lib = ctypes.CDLL(build.build_hostlane_elect())
        c = ctypes
        lib.hl_step.argtypes = [c.c_uint32, c.c_uint64, c.c_void_p, c.c_uint32, c.POINTER(abi.Inbox),
                                c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t), c.c_void_p, c.POINTER(c.c_size_t)]
        _elib = lib
    return _elib


class TallyLost(AssertionError):
    pass


class ElectHostlaneBackend(SIM.HostlaneBackend):
    """simulate.HostlaneBackend over the elections build of the host lane."""

    def step(self, msgs, loc):
        lib = hostlane_elect_lib()
        peers = np.array(self.state, dtype=abi.PEER, copy=True)
        msgs = np.ascontiguousarray(msgs, abi.MESSAGE)
        loc = np.ascontiguousarray(loc, abi.LOCAL)
        ib = abi.inbox_of(msgs, loc)
        cap = max(16, 8 * len(peers) * self.slots)
        out = np.zeros(cap, abi.MESSAGE)
        n_out, n_res = ctypes.c_size_t(), ctypes.c_size_t()
        res = np.zeros(len(peers), abi.RESULT)
        rc = lib.hl_step(self.slots, self.max_entry_size, peers.ctypes.data, len(peers), ctypes.byref(ib),
                         out.ctypes.data, cap, ctypes.byref(n_out), res.ctypes.data, ctypes.byref(n_res))
        assert rc == 0, f"hl_step rc={rc}"
        self.state = peers
        return out[:n_out.value], res[:n_res.value]

    def load(self, idx, recs):
        check_tally_kept(self.state[np.asarray(idx, np.int64)], np.asarray(recs, abi.PEER), idx)
        super().load(idx, recs)


def check_tally_kept(dev, recs, idx):
    """The candidate reload guard: the oracle's record cannot carry raft.votes,
    so reloading a candidate that stays in its campaign (same term) while the
    device tally holds a remote slot's response would lose that response."""
    dev = np.ascontiguousarray(dev).view(abi.PEER_VOTES)
    own = np.uint8(1) << dev["self_slot"].astype(np.uint8)
    remote = (dev["votes_granted"] & ~own) | dev["votes_rejected"]
    lost = (dev["state"] == abi.CANDIDATE) & (recs["state"] == abi.CANDIDATE) & (dev["term"] == recs["term"]) & \
           (remote != 0)
    if lost.any():
        raise TallyLost(f"reload of candidate(s) {np.asarray(idx)[lost][:5]} whose device tally holds remote votes: "
                        "the oracle's record cannot carry them; choose another seed")


def cold_peers(G, R, seed, check_quorum=False):
    return P.cold_start(G, R, seed=seed, check_quorum=check_quorum)


def leaders_per_group(state, G, R):
    return (state["state"].reshape(R, G) == abi.LEADER).sum(axis=0)


def cold_start(backend, G, R, seed, passes=60, propose_passes=12, check_quorum=False, after_pass=None):
    """Cold start through simulate.Lockstep: `passes` passes of one tick each
    (the draw of the pass in rand), then `propose_passes` with a proposal on every
    leader. after_pass(ls, k, before, res): called after each pass with the
    device state before it and the engine's results. Returns (stats, state when
    the proposals start, final state)."""
    peers = cold_peers(G, R, seed, check_quorum=check_quorum)
    topo = P.Topology(G, R)
    ls = SIM.Lockstep(backend, peers, R)
    msgs = np.zeros(0, abi.MESSAGE)
    elected = None
    try:
        for k in range(passes + propose_passes):
            st = ls.export()
            if k == passes:
                elected = st.copy()
            lead = np.nonzero(st["state"] == abi.LEADER)[0] if k >= passes else np.zeros(0, np.int64)
            loc = P.propose_locals(R * G, lead, seed=seed, pass_index=k, ticks=1)
            before = ls.eng.sync() if after_pass else None
            out, res = ls.step(msgs, loc)
            if after_pass:
                after_pass(ls, k, before, res)
            ls.apply_all()
            msgs = topo.route_messages(out)
        return ls.stats, elected, ls.export()
    finally:
        ls.close()


def assert_cold_start(stats, elected, final, G, R):
    nl = leaders_per_group(elected, G, R)
    assert np.all(nl == 1), f"groups without exactly one leader: {np.nonzero(nl != 1)[0][:8]} have {nl[nl != 1][:8]}"
    assert np.all(leaders_per_group(final, G, R) == 1)
    lead = elected["state"] == abi.LEADER
    adv = final["committed"][lead] > elected["committed"][lead]
    assert np.all(adv), f"{int((~adv).sum())} leaders' commits did not advance"
    reasons = stats["esc_reasons"]
    assert reasons.get("election", 0) == 0 and reasons.get("unsupported", 0) == 0, reasons

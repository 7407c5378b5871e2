"""Result rows the steady lanes no longer write (gr_layout.h RF_APPEND_LAST,
RF_PROP_OK): a steady follower's append_from and a steady leader's proposal
result follow from the result flags instead of their lane rows.

Every case compares every state record, message and result with the oracle
after every pass (simulate.Lockstep over the host lane with the device's wave
hints; devsim.DeviceLockstep over gr_step_device). On the device the lane rows
persist from pass to pass, so a reader that still took append_from or the
proposal result from a row the steady lanes no longer write would report an
earlier pass's value, and the result comparison would fail.
"""
import numpy as np
import pytest

from dragonboat_amd import abi, populations as P
import simulate as SIM


def _peers(G, R, seed, **kw):
    return P.make_groups(G, R, seed=seed, election=10, heartbeat=1, **kw)


class _HoldNet:
    """The network between passes. The Replicates that call `at` carries to the
    followers of replica block 2 in the odd groups are held for one pass and
    arrive ahead of the next pass's; the entry-less ones of both passes (commit
    broadcasts) are lost on the way. Those followers then get nothing for one
    pass, and two Replicates in the next, each with an entry: the lowest index
    appended is then not the last one."""

    def __init__(self, G, at):
        self.G, self.at, self.calls = G, at, 0
        self.held = np.zeros(0, abi.MESSAGE)
        self.changed = False  # the last call delivered something other than what was sent

    def targets(self):
        g = np.arange(self.G)
        return 2 * self.G + g[g % 2 == 1]

    def __call__(self, k, msgs):
        c, self.calls = self.calls, self.calls + 1
        self.changed = False
        peer = msgs["peer"].astype(np.int64)
        tgt = (msgs["type"] == abi.REPLICATE) & (peer // self.G == 2) & ((peer % self.G) % 2 == 1)
        if c == self.at:
            self.held = msgs[tgt & (msgs["n_entries"] > 0)].copy()
            self.changed = True
            return msgs[~tgt]
        if c == self.at + 1:
            rest = msgs[~(tgt & (msgs["n_entries"] == 0))]
            out = np.concatenate([self.held, rest])
            self.held = np.zeros(0, abi.MESSAGE)
            self.changed = True
            order = np.lexsort((np.arange(len(out)), out["slot"], out["peer"]))  # held ones first in their mailbox
            return out[order]
        return msgs


class _HostDriver:
    """simulate.Lockstep over the host lane, with the device's wave hints."""

    def __init__(self, peers, G, R):
        from oracle.pyoracle import hostlane_lib
        self.G, self.R, self.n = G, R, R * G
        self.topo = P.Topology(G, R)
        self.hl = hostlane_lib()
        self.hl.hl_true_hints(1)
        self.ls = SIM.Lockstep(SIM.HostlaneBackend, peers, R)
        self.msgs = np.zeros(0, abi.MESSAGE)

    def step(self, loc, net=None):
        out, res = self.ls.step(self.msgs, loc)
        self.msgs = self.topo.route_messages(out)
        if net is not None:
            self.msgs = net(0, self.msgs)
        return res

    def steady_lanes(self):
        from oracle.pyoracle import hostlane_steady_lanes
        return hostlane_steady_lanes()

    @property
    def stats(self):
        return self.ls.stats

    def close(self):
        self.hl.hl_true_hints(0)
        self.ls.close()


class _DevDriver:
    """devsim.DeviceLockstep: gr_step_device over loopback spaces."""

    def __init__(self, peers, G, R):
        import devsim
        self.G, self.R, self.n = G, R, R * G
        self.ls = devsim.DeviceLockstep(peers, G, R)

    def step(self, loc, net=None):
        res = self.ls.step(loc, drop_fn=net)
        # DeviceLockstep re-encodes the next inbox only when the count of messages
        # changed; a held batch can swap messages at the same count
        if net is not None and net.changed:
            self.ls.override_inbox(self.ls.msgs)
        return res

    def steady_lanes(self):
        return None  # not visible through the interface: the timed passes' bailed_lanes stand for it

    @property
    def stats(self):
        return self.ls.stats

    def close(self):
        self.ls.close()


def _by_peer(res, n):
    """Result records by peer (one per peer in these populations)."""
    out = np.zeros(n, abi.RESULT)
    out[res["peer"].astype(np.int64)] = res
    return out


# ---------------------------------------------------------------- scenarios
def _scenario_steady(drv, passes=8, warm=4):
    """One proposal per leader per pass: every follower appends one entry, the
    last one (RF_APPEND_LAST), every leader's proposal is appended (RF_PROP_OK)."""
    G, R, n = drv.G, drv.R, drv.n
    counts = [drv.steady_lanes()]
    for k in range(passes):
        res = _by_peer(drv.step(P.propose_locals(n, np.arange(G), pass_index=k)), n)
        counts.append(drv.steady_lanes())
        assert np.all(res["propose_result"][:G] == abi.PROP_APPENDED)
        assert np.all(res["propose_first"][:G] == res["last_index"][:G])
        if k >= 1:  # the Replicate of pass k - 1 arrives
            assert np.all(res["append_from"][G:] == res["last_index"][G:])
        assert np.all(res["append_from"][:G] == 0) and np.all(res["propose_result"][G:] == abi.PROP_NONE)
    assert drv.stats["escalations"] == 0 and drv.stats["commits"] > 0
    if counts[0] is not None:
        per_pass = np.diff(counts)[warm:]
        # R = 5: SteadyLeader is the median of three voters, a five-replica leader is FastLane's
        assert np.all(per_pass == (R if R == 3 else R - 1) * G), per_pass


def _scenario_hold(drv):
    """_HoldNet: append_from is not the last index for the held followers, so
    the steady follower stores the LR_APPEND_FROM row (and leaves RF_APPEND_LAST
    clear); the passes around it take the flag."""
    G, R, n = drv.G, drv.R, drv.n
    net = _HoldNet(G, at=4)
    tgt = net.targets()
    rest = np.setdiff1d(np.arange(G, n), tgt)
    seen = False
    for k in range(10):
        before = drv.steady_lanes()
        res = _by_peer(drv.step(P.propose_locals(n, np.arange(G), pass_index=k), net), n)
        if k == 5:  # nothing arrived
            assert np.all(res["append_from"][tgt] == 0)
        if k == 6:  # two entries at once
            assert np.all(res["append_from"][tgt] == res["last_index"][tgt] - 1), res["append_from"][tgt][:4]
            assert np.all(res["append_from"][rest] == res["last_index"][rest])
            seen = True
            if before is not None:  # every follower is still the closed form's
                assert drv.steady_lanes() - before >= (R - 1) * G, drv.steady_lanes() - before
        if k >= 7:
            assert np.all(res["append_from"][G:] == res["last_index"][G:])
    assert seen and drv.stats["escalations"] == 0


def _scenario_locals(drv):
    """Local inputs the closed forms do not take: two proposals on the even
    leaders (propose_first is then not the last index) and a ReadIndex on a
    quarter of the followers of block 1, beside untouched steady lanes whose
    result rows stay unwritten, then steady passes again."""
    G, R, n = drv.G, drv.R, drv.n
    for k in range(4):
        drv.step(P.propose_locals(n, np.arange(G), pass_index=k))
    for k in range(4, 7):
        loc = P.propose_locals(n, np.arange(G), pass_index=k)
        loc["propose_entries"][np.arange(0, G, 2)] = 2
        ri = np.zeros(n, bool)
        ri[G + 1:2 * G:4] = True
        loc["read_index"] = ri
        loc["read_ctx_low"] = np.where(ri, np.arange(n) + 1000 * k + 1, 0)
        loc["read_ctx_high"] = np.where(ri, k + 1, 0)
        before = drv.steady_lanes()
        res = _by_peer(drv.step(loc), n)
        assert np.all(res["propose_first"][0:G:2] == res["last_index"][0:G:2] - 1)
        if before is not None:  # those lanes left the closed form
            assert drv.steady_lanes() - before <= n - G // 2 - len(range(G + 1, 2 * G, 4))
    for k in range(7, 12):
        drv.step(P.propose_locals(n, np.arange(G), pass_index=k))
    assert drv.stats["commits"] > 0


def _scenario_term(drv, wide):
    """A population whose term is 2^32 - 1 (the last one the steady lanes and the
    mailboxes take) or 2^32 + 7 (every message escalates GR_ESC_WIDE_TERM, as it
    did before: the comparison with the oracle is the check)."""
    G, R, n = drv.G, drv.R, drv.n
    counts = [drv.steady_lanes()]
    for k in range(6):
        drv.step(P.propose_locals(n, np.arange(G), pass_index=k))
        counts.append(drv.steady_lanes())
    if not wide:
        assert drv.stats["escalations"] == 0 and drv.stats["commits"] > 0
        if counts[0] is not None:
            assert np.all(np.diff(counts)[4:] == n), np.diff(counts)
    else:
        assert drv.stats["escalations"] > 0
        assert set(drv.stats["esc_reasons"]) == {"wide_term"}, drv.stats["esc_reasons"]
        if counts[0] is not None:
            assert counts[-1] == counts[0], np.diff(counts)


# ---------------------------------------------------------------- CPU cases
@pytest.mark.parametrize("R", [3, 5])
def test_steady_host(built, R):
    drv = _HostDriver(_peers(64, R, 11), 64, R)
    try:
        _scenario_steady(drv)
    finally:
        drv.close()


def test_hold_host(built):
    drv = _HostDriver(_peers(64, 3, 11), 64, 3)
    try:
        _scenario_hold(drv)
    finally:
        drv.close()


def test_locals_host(built):
    drv = _HostDriver(_peers(64, 3, 13), 64, 3)
    try:
        _scenario_locals(drv)
    finally:
        drv.close()


@pytest.mark.parametrize("term,wide", [(2**32 - 1, False), (2**32 + 7, True)])
def test_term_host(built, term, wide):
    drv = _HostDriver(_peers(64, 3, 17, term_lo=term, term_hi=term), 64, 3)
    try:
        _scenario_term(drv, wide)
    finally:
        drv.close()


# ---------------------------------------------------------------- device cases
def _split(monkeypatch):
    monkeypatch.setenv("GR_SPLIT_MIN_LANES", "1")  # read at gr_create
    monkeypatch.setenv("GR_SMALL_BLOCKS", "0")     # the split schedule, not the fused small-pass kernel


def _timed_steady(drv, want_wu, steady_lanes):
    """Four warm-up passes, then two timed ones: no lane may leave the steady
    kernel (gr_timing bailed_lanes), and the results still resolve."""
    G, n = drv.G, drv.n
    eng = drv.ls.eng
    assert eng.steady_wave_uniform() == want_wu
    for k in range(4):
        drv.step(P.propose_locals(n, np.arange(G), pass_index=k))
    eng.timing_begin()
    for k in range(4, 6):
        res = _by_peer(drv.step(P.propose_locals(n, np.arange(G), pass_index=k)), n)
        assert np.all(res["append_from"][G:] == res["last_index"][G:])
        assert np.all(res["propose_result"][:G] == abi.PROP_APPENDED)
    t = eng.timing_end()
    print("timed passes:", t)
    assert t["passes"] == 2
    if steady_lanes:
        assert t["bailed_lanes"] == 0, t
    assert drv.stats["escalations"] == 0 and drv.stats["commits"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("G,R,want_wu", [(64, 3, True), (192, 3, True), (320, 3, True), (130, 3, False), (64, 5, True)])
def test_steady_device_split(gpu, monkeypatch, G, R, want_wu):
    """The wave-uniform instance at 64, 192 and 320 groups x 3, the per-lane one
    at 130 (its waves mix roles, so some lanes are the tail kernels': no count
    asserted), and the S = 5 follower (its leaders are FastLane's)."""
    _split(monkeypatch)
    drv = _DevDriver(_peers(G, R, 11), G, R)
    try:
        _timed_steady(drv, want_wu, steady_lanes=want_wu and R == 3)
        _scenario_steady(drv, passes=2)
    finally:
        drv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("G", [64, 192, 320])
def test_hold_device_split(gpu, monkeypatch, G):
    _split(monkeypatch)
    drv = _DevDriver(_peers(G, 3, 11), G, 3)
    try:
        _scenario_hold(drv)
    finally:
        drv.close()


@pytest.mark.gpu
def test_locals_device_split(gpu, monkeypatch):
    _split(monkeypatch)
    drv = _DevDriver(_peers(64, 3, 13), 64, 3)
    try:
        _scenario_locals(drv)
    finally:
        drv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("term,wide", [(2**32 - 1, False), (2**32 + 7, True)])
def test_term_device_split(gpu, monkeypatch, term, wide):
    _split(monkeypatch)
    drv = _DevDriver(_peers(64, 3, 17, term_lo=term, term_hi=term), 64, 3)
    try:
        _scenario_term(drv, wide)
    finally:
        drv.close()


@pytest.mark.gpu
def test_steady_hold_device_small_kernel(gpu):
    """64 x 3 under the default thresholds: the fused small kernel."""
    drv = _DevDriver(_peers(64, 3, 11), 64, 3)
    try:
        _scenario_hold(drv)
    finally:
        drv.close()


@pytest.mark.gpu
def test_compact_round_trip_after_steady(gpu, monkeypatch):
    """gr_step_compact on an engine whose lane rows four steady device passes
    left behind (LR_PROP_RESULT and LR_APPEND_FROM unwritten, the flags set):
    the compact results (propose_result, last_index, commit lag, save count;
    a compact result carries no append_from, save_from stands for it) equal the
    oracle's."""
    _split(monkeypatch)
    G, R = 64, 3
    n = R * G
    topo = P.Topology(G, R)
    drv = _DevDriver(_peers(G, R, 23), G, R)
    try:
        for k in range(4):
            drv.step(P.propose_locals(n, np.arange(G), pass_index=k))
        dls = drv.ls
        eng = dls.eng

        class Reuse(SIM.GpuCompactBackend):  # the Lockstep's backend over the same engine
            def __init__(self, peers, slots, max_entry_size=abi.MAX_ENTRY_SIZE):
                self.eng, self.n = eng, n

            def close(self):
                pass
        ls = SIM.Lockstep(Reuse, dls.pop.export(), R)
        msgs = dls.msgs
        for k in range(4, 7):
            out, res = ls.step(msgs, P.propose_locals(n, np.arange(G), pass_index=k))
            res = _by_peer(res, n)
            assert np.all(res["propose_result"][:G] == abi.PROP_APPENDED)
            msgs = topo.route_messages(out)
        assert ls.stats["escalations"] == 0 and ls.stats["commits"] > 0
    finally:
        drv.close()

"""lane_update_fields (gr_host.h), the classify kernel's shortcut to the fields
Peer.HasUpdate asks about, against update_fields(make_result(..)), the record
update_pack builds for a reported peer. The shortcut reads only the lane rows a
set result flag names, resolves RF_PROP_OK itself and reads SR_COMMITTED only
where the header carries no lag; a lane it gets wrong is classified from other
fields than the record it then sends (or is not reported at all).

No GPU: tests/native/hostlane.hip exports both for every lane of its last pass
(hl_update_fields), and the all-switches and elections builds of the host lane
inherit the export. The shortcut indexes lane and state rows by one number, so
the export refuses a pass in which some lane stepped another peer; every
population here gives every peer a local input in peer order. Each run also
requires the flag forms it is there for to have occurred."""
import numpy as np

from dragonboat_amd import abi, populations as P
import all_switches_common as C
import elections_common as EC
import simulate as SIM
import updates_common as UC
from test_all_switches import live_all


def _lockstep(backend, lib, peers, G, R, passes, locals_fn):
    """simulate.Lockstep under oracle parity, everything committed after each
    pass; the fields compared after every pass."""
    n = G * R
    topo = P.Topology(G, R)
    ls = SIM.Lockstep(backend, peers, R)
    chk = UC.FieldsCheck()
    msgs = np.zeros(0, abi.MESSAGE)
    try:
        for k in range(passes):
            loc = locals_fn(k, ls.export())
            assert len(loc) == n and np.array_equal(loc["peer"], np.arange(n))
            out, res = ls.step(msgs, loc)
            chk.after(lib(), n, res)
            ls.apply_all()
            msgs = topo.route_messages(out)
    finally:
        ls.close()
    return chk


def test_all_switches_population(built, monkeypatch):
    """live_all("cpu", 192): restores, promotions, config-change entries, 960 lanes."""
    chk = UC.FieldsCheck()
    step = C.host_step

    def host_step(peers, *a):
        r = step(peers, *a)
        chk.after(C.lib(), len(peers), r[4])
        return r
    monkeypatch.setattr(C, "host_step", host_step)
    live_all("cpu", 192)
    assert chk.passes == 20
    assert chk.saw(UC.RF_PROPOSE, UC.RF_APPEND, UC.RF_HARDSTATE), hex(chk.seen)
    assert chk.by_field[UC.UF_FIELDS.index("save_from")] and chk.by_field[UC.UF_FIELDS.index("propose_result")]


def test_elections_cold_start(built):
    """elections_common.cold_start on the elections build, 200 x 3, seed 21, 12
    passes: campaigns and votes move term and vote (RF_HARDSTATE)."""
    chk = UC.FieldsCheck()
    G, R = 200, 3
    EC.cold_start(EC.ElectHostlaneBackend, G, R, 21, passes=12, propose_passes=0,
                  after_pass=lambda ls, k, before, res: chk.after(EC.hostlane_elect_lib(), G * R, res))
    assert chk.passes == 12 and chk.saw(UC.RF_HARDSTATE), hex(chk.seen)


def test_steady_proposals(built):
    """Steady groups, a proposal on every leader each pass: the commit-lag header
    form (SR_COMMITTED not read), RF_PROP_OK (LR_PROP_RESULT not written) and
    RF_APPEND_LAST."""
    from oracle.pyoracle import hostlane_lib, hostlane_step
    G, R = 140, 3
    peers = P.make_groups(G, R, seed=41)
    chk = _lockstep(SIM.HostlaneBackend, hostlane_lib, peers, G, R, 12,
                    lambda k, st: P.propose_locals(G * R, np.arange(G), seed=41, pass_index=k))
    assert chk.saw(UC.HDR_LAG, UC.RF_PROP_OK, UC.RF_APPEND_LAST, UC.RF_PROPOSE, UC.RF_APPEND), hex(chk.seen)
    # the export refuses a pass whose lanes are not the peers in order
    loc = P.propose_locals(G * R, np.arange(G), seed=41)
    hostlane_step(peers, None, loc[1:], R)
    assert UC.lane_update_fields(hostlane_lib(), G * R)[0] == -6


def test_read_index_and_forwarded(built):
    """ReadIndex on the leaders and proposals on the followers of replica 1,
    which forward them: RF_READY (LR_RTR_COUNT) and RF_FORWARDED (LR_FWD_COUNT)."""
    from oracle.pyoracle import hostlane_lib
    G, R = 140, 3
    n = G * R

    def locals_fn(k, st):
        loc = P.propose_locals(n, np.arange(G, 2 * G), seed=42, pass_index=k, ticks=1 if k % 3 == 0 else 0)
        loc["read_index"][:G] = 1
        loc["read_ctx_low"][:G] = 1 + k * n + np.arange(G)
        loc["read_ctx_high"][:G] = 9
        return loc
    chk = _lockstep(SIM.HostlaneBackend, hostlane_lib, P.make_groups(G, R, seed=42), G, R, 10, locals_fn)
    assert chk.saw(UC.RF_READY, UC.RF_FORWARDED), hex(chk.seen)
    assert chk.by_field[UC.UF_FIELDS.index("n_ready")] and chk.by_field[UC.UF_FIELDS.index("n_forwarded")]

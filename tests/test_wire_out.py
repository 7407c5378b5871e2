"""Frames straight out of the step (gpuraft.h gr_step_wire_out /
gr_step_compact_wire_out): the pass's entry-free out mailboxes leave as grw_batch /
grw_message records in HBM, grouped by send queue on the device. Checked record
for record against gr_wire_out_host over a twin engine's full outbox, and in
lockstep with the oracle with frames as the only way out for that mail."""
import numpy as np
import pytest

from dragonboat_amd import abi, populations as P, wire as W
import simulate as SIM
import wireout as WO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def steady(gpu):
    """The inputs of test_wire_compact_outbox (G = 300, R = 3: a first pass's
    messages and the second pass's proposals) with a tick on every 7th peer, and
    what the parent's entry points return for them: the full outbox (gr_step) and
    the compact one (gr_step_wire_compact). Computed once."""
    import wirefeed
    from dragonboat_amd.engine import Engine
    from oracle.pyoracle import OraclePopulation
    G, R = 300, 3
    peers = P.make_groups(G, R, seed=4)
    topo = P.Topology(G, R)
    cl = (np.arange(R * G) % G) + 1
    pop = OraclePopulation(peers, R)
    o = pop.step(np.zeros(0, abi.MESSAGE), P.propose_locals(R * G, np.arange(G), pass_index=0))
    msgs = topo.route_messages(o["msgs"])
    loc = P.propose_locals(R * G, np.arange(G), pass_index=1)
    loc["ticks"][::7] = 1
    full = Engine(R * G, R)
    full.load(peers)
    out, res = full.step(msgs, loc)
    state = full.sync(R * G)
    full.close()
    feed = wirefeed.WireFeed(peers, cl)
    comp = Engine(R * G, R)
    comp.load(peers)
    comp.bind_nodes(cl, peers["node_id"])
    d_m, nm, d_e, ne, keep = feed.decode(msgs)
    cout, idx, why = comp.step_wire(d_m, nm, d_e, ne, loc, compact=True)
    assert len(idx) == 0 and np.array_equal(comp.sync(R * G), state)
    comp.close()
    feed.close()
    for a in (out, res, state) + tuple(cout):
        a.setflags(write=False)
    return dict(G=G, R=R, peers=peers, cl=cl, msgs=msgs, loc=loc, out=out, res=res, state=state, cout=cout)


def _layouts(n, R):
    tail = np.zeros((n, R), np.uint32)
    tail[768:] = 1  # the last, partial workgroup (lanes 768..899) alone holds target 1's mail
    mixed = WO.replica_targets(n, R) * 2  # targets 1 and 3 never used
    mixed[5] = abi.TARGET_HOST
    mixed[n - 1, 0] = abi.TARGET_HOST
    return {"replica": (WO.replica_targets(n, R), R), "tail": (tail, 2), "mixed": (mixed, 2 * R),
            "many": ((np.arange(n * R, dtype=np.uint32).reshape(n, R) * 7) % 256, 256)}


def _without_wire(cout, held_boxes):
    """A compact outbox with the wire mailboxes removed (ext indexes renumbered)."""
    om, ox, cr, rx = cout
    keep = np.array([(int(p), int(j)) in held_boxes for p, j in zip(om["peer"], om["slot"])], bool)
    om = om[keep].copy()
    x = (om["flags"] & abi.CM_EXT) != 0
    ox = ox[om["aux"][x].astype(np.int64)]
    om["aux"][x] = np.arange(int(x.sum()))
    return om, ox, cr, rx


def _check_against_host(S, torch, got, wo, targets, n_targets, cfg):
    from dragonboat_amd.engine import wire_out_host
    bat, wm, bt, held = wire_out_host(S["out"], S["cl"], S["peers"]["node_id"], S["peers"]["remote_id"], targets,
                                      n_targets, cfg)
    d_wm = WO.download(torch, wo.d_msgs, W.WMESSAGE, wo.n_msgs)
    d_bat = WO.download(torch, wo.d_batches, W.BATCH, wo.n_batches)
    assert wo.n_msgs == len(wm) and wo.n_batches == len(bat)
    assert np.array_equal(d_wm, wm)                 # every byte of every record, padding included
    assert np.array_equal(d_bat, bat)
    assert np.array_equal(wo.batch_target, bt)
    WO.check_batches(d_bat, wo.batch_target, wo.n_msgs, cfg, n_targets)
    held_boxes = {(int(p), int(j)) for p, j in zip(S["out"]["peer"][held], S["out"]["slot"][held])}
    want = _without_wire(S["cout"], held_boxes)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    return len(wm), int(held.sum())


@pytest.mark.parametrize("entry", ["wire", "compact"])
@pytest.mark.parametrize("layout,mbm", [("replica", 64), ("tail", 5), ("mixed", 1), ("many", 2**31)])
def test_twin_engines(steady, gpu, entry, layout, mbm):
    """Engine A steps with the new entry point; the twins stepped the same
    records with gr_step and gr_step_wire_compact (the fixture). A's device
    records equal gr_wire_out_host over the twin's full outbox element for
    element; its coutbox is the twin's without the wire mailboxes; results and
    state are equal. `tail`: 900 lanes (a multiple of neither 64 nor 256), the
    last partial workgroup alone holding one target's mail."""
    import wirefeed
    from dragonboat_amd.engine import Engine
    S = steady
    G, R = S["G"], S["R"]
    targets, n_targets = _layouts(R * G, R)[layout]
    cfg = dict(WO.CFG, max_batch_msgs=mbm)
    eng = Engine(R * G, R)
    feed = None
    try:
        eng.load(S["peers"])
        eng.bind_nodes(S["cl"], S["peers"]["node_id"])
        eng.bind_targets(targets, n_targets)
        if entry == "wire":
            feed = wirefeed.WireFeed(S["peers"], S["cl"])
            d_m, nm, d_e, ne, keep = feed.decode(S["msgs"])
            got, idx, why, wo = eng.step_wire(d_m, nm, d_e, ne, S["loc"], wire_out=cfg)
            assert len(idx) == 0
        else:
            cm, xm = eng.pack_messages(S["msgs"])
            cloc, xloc = eng.pack_locals(S["loc"])
            got, wo = eng.step_compact(cm, xm, cloc, xloc, wire_out=cfg)
        nw, nh = _check_against_host(S, gpu, got, wo, targets, n_targets, cfg)
        assert nw > 0 and nh > 0
        assert np.array_equal(eng.sync(R * G), S["state"])
    finally:
        if feed:
            feed.close()
        eng.close()


def _lockstep_backend(**kw):
    seen = {}

    class B(WO.GpuWireOutBackend):
        def close(self):
            seen.update(wire=self.wire_msgs, held=self.held_msgs, types=set(self.types))
            super().close()
    for k, v in kw.items():
        setattr(B, k, v)
    return B, seen


def test_lockstep_churn(gpu):
    """test_wire_path_churn's shape: leader changes with divergent suffixes;
    rejects, accepts and commit broadcasts leave by frame, Replicates with entries stay."""
    G, R = 400, 3
    topo = P.Topology(G, R)
    rng = np.random.default_rng(5)
    B, seen = _lockstep_backend()
    st = SIM.simulate(B, P.make_groups(G, R, seed=5), topo, 12,
                      lambda k, s: P.propose_locals(R * G, P.current_leaders(s, topo), pass_index=k),
                      inject_fn=lambda k, cur: P.inject_leader_change(cur, topo, 0.1, rng))
    assert st["commits"] > 0 and st["msgs"] > 0
    assert seen["wire"] > 0 and seen["held"] > 0, seen


def test_lockstep_ticks_read_index(gpu):
    """test_wire_path_ticks_read_index's shape (config 3, R = 5, dropped acks):
    every message of these passes is entry-free, so nothing is held."""
    G, R = 200, 5
    peers, active = P.config3(G, R)
    rng = np.random.default_rng(3)
    B, seen = _lockstep_backend()
    st = SIM.simulate(B, peers, P.Topology(G, R), 8, lambda k: P.config3_locals(G, R, active, k), slots=5,
                      drop_fn=lambda k, m: P.drop_acks(m, 0.1, rng))
    assert st["ready"] > 0
    assert seen["wire"] > 0 and seen["held"] == 0, seen


def test_lockstep_elections(gpu, monkeypatch):
    """Elections on the device: a cold start's RequestVotes and their responses
    leave by frame, and the lockstep with the oracle stays green."""
    import elections_common as EC
    monkeypatch.setenv("GR_ELECTIONS", "1")
    G, R = 70, 3
    B, seen = _lockstep_backend()
    stats, elected, final = EC.cold_start(B, G, R, 11, passes=45, propose_passes=3)
    EC.assert_cold_start(stats, elected, final, G, R)
    assert {abi.REQUEST_VOTE, abi.REQUEST_VOTE_RESP} <= seen["types"], seen["types"]
    assert seen["held"] > 0  # the proposals' Replicates


def test_all_pairs_with_host(steady, gpu):
    """Every pair bound to GR_TARGET_HOST: no batch, and the coutbox is gr_step_wire_compact's."""
    import wirefeed
    from dragonboat_amd.engine import Engine
    S = steady
    G, R = S["G"], S["R"]
    eng = Engine(R * G, R)
    feed = wirefeed.WireFeed(S["peers"], S["cl"])
    try:
        eng.load(S["peers"])
        eng.bind_nodes(S["cl"], S["peers"]["node_id"])
        eng.bind_targets(np.full((R * G, R), abi.TARGET_HOST, np.uint32), 1)
        d_m, nm, d_e, ne, keep = feed.decode(S["msgs"])
        got, idx, why, wo = eng.step_wire(d_m, nm, d_e, ne, S["loc"], wire_out=WO.CFG)
        assert wo.n_batches == 0 and wo.n_msgs == 0 and len(wo.batch_target) == 0
        for a, b in zip(got, S["cout"]):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    finally:
        feed.close()
        eng.close()


def test_no_output_and_state_errors(steady, gpu):
    from dragonboat_amd.engine import Engine, GpuRaftError
    S = steady
    G, R = S["G"], S["R"]
    eng = Engine(R * G, R)
    try:
        eng.load(S["peers"])
        quiet = np.zeros(33, abi.LOCAL)  # followers with nothing to do: lanes without output
        quiet["peer"] = G + np.arange(33)
        eng.bind_nodes(S["cl"], S["peers"]["node_id"])
        with pytest.raises(GpuRaftError) as ei:  # GR_ESTATE before gr_bind_targets
            eng.step_wire(0, 0, 0, 0, quiet, wire_out=WO.CFG)
        assert ei.value.rc == -6
        cl0, xl0 = eng.pack_locals(quiet)
        none = np.zeros(0, abi.CMSG), np.zeros(0, abi.MESSAGE)
        with pytest.raises(GpuRaftError) as ei:
            eng.step_compact(none[0], none[1], cl0, xl0, wire_out=WO.CFG)
        assert ei.value.rc == -6
        for bad in (dict(n_targets=0), dict(n_targets=abi.MAX_TARGETS + 1), dict(index=R)):
            t = WO.replica_targets(R * G, R)
            t[7, 1] = bad.get("index", 1)
            with pytest.raises(GpuRaftError) as ei:
                eng.bind_targets(t, bad.get("n_targets", R))
            assert ei.value.rc == -1
        eng.bind_targets(WO.replica_targets(R * G, R), R)
        with pytest.raises(GpuRaftError) as ei:
            eng.step_wire(0, 0, 0, 0, quiet, wire_out=dict(WO.CFG, max_batch_msgs=0))
        assert ei.value.rc == -1
        # refused while a gr_step_compact_begin waits for its _end, as gr_bind_nodes
        import ctypes
        ib = abi.cinbox_of(none[0], none[1], cl0, xl0)
        assert eng.lib.gr_step_compact_begin(eng._h, ctypes.byref(ib)) == 0
        with pytest.raises(GpuRaftError) as ei:
            eng.bind_targets(WO.replica_targets(R * G, R), R)
        assert ei.value.rc == -6
        with pytest.raises(GpuRaftError) as ei:
            eng.step_compact(none[0], none[1], cl0, xl0, wire_out=WO.CFG)
        assert ei.value.rc == -6
        ob = abi.COutbox()
        assert eng.lib.gr_step_compact_end(eng._h, ctypes.byref(ob)) == 0 and ob.n_results == 33
        assert eng.lib.gr_release_coutbox(eng._h, ctypes.byref(ob)) == 0
        # a pass with no output at all, and an empty inbox
        (om, ox, cr, rx), idx, why, wo = eng.step_wire(0, 0, 0, 0, quiet, wire_out=WO.CFG)
        assert len(om) == 0 and len(ox) == 0 and len(cr) == 33
        assert wo.n_batches == 0 and wo.n_msgs == 0
        (om, ox, cr, rx), idx, why, wo = eng.step_wire(0, 0, 0, 0, None, wire_out=WO.CFG)
        assert len(om) == 0 and len(cr) == 0 and wo.n_batches == 0 and wo.n_msgs == 0
        (om, ox, cr, rx), wo = eng.step_compact(none[0], none[1], cl0, xl0, wire_out=WO.CFG)
        assert len(om) == 0 and len(cr) == 33 and wo.n_batches == 0 and wo.n_msgs == 0
    finally:
        eng.close()


def _twins_other_slots(torch, peers, slots, msgs, loc, cl, targets, n_targets, cfg):
    """The twin check for a slot count the module fixture does not cover: gr_step
    and gr_step_compact on the same records give the full and the compact outbox,
    a third engine steps them with gr_step_compact_wire_out."""
    from dragonboat_amd.engine import Engine
    n = len(peers)
    engs = [Engine(n, slots) for _ in range(3)]
    try:
        full, comp, eng = engs
        for e in engs:
            e.load(peers)
        out, res = full.step(msgs, loc)
        state = full.sync(n)
        cm, xm = comp.pack_messages(msgs)
        cloc, xloc = comp.pack_locals(loc)
        cout = comp.step_compact(cm, xm, cloc, xloc)
        eng.bind_nodes(cl, peers["node_id"])
        eng.bind_targets(targets, n_targets)
        got, wo = eng.step_compact(cm, xm, cloc, xloc, wire_out=cfg)
        S = dict(out=out, cl=cl, peers=peers, cout=cout)
        nw, nh = _check_against_host(S, torch, got, wo, targets, n_targets, cfg)
        assert np.array_equal(eng.sync(n), state) and np.array_equal(comp.sync(n), state)
        return nw, nh
    finally:
        for e in engs:
            e.close()


def test_twin_engines_four_slots(gpu):
    """gr_config.slots = 4 runs the 8-slot instantiation: gr_bind_targets takes rows
    of 4 (the configured count), every pair with its own queue index, so a row read
    at another stride would put mail on the wrong queue."""
    from dragonboat_amd.engine import Engine
    G, R, slots = 100, 3, 4
    n = R * G
    peers = P.make_groups(G, R, seed=6, slots=slots)
    first = Engine(n, slots)
    try:
        first.load(peers)
        out0, _ = first.step(None, P.propose_locals(n, np.arange(G), pass_index=0))
        peers = first.sync(n)
    finally:
        first.close()
    msgs = P.Topology(G, R).route_messages(out0)
    loc = P.propose_locals(n, np.arange(G), pass_index=1)
    loc["ticks"][::7] = 1
    targets = ((np.arange(n * slots, dtype=np.uint32).reshape(n, slots)) % 7).astype(np.uint32)
    targets[11, 2] = abi.TARGET_HOST
    nw, nh = _twins_other_slots(gpu, peers, slots, msgs, loc, (np.arange(n) % G) + 1, targets, 7,
                                dict(WO.CFG, max_batch_msgs=9))
    assert nw > 0 and nh > 0


def test_twin_engines_one_slot(gpu):
    """gr_config.slots = 1 (the 1-slot instantiation): followers whose only slot is
    their leader answer a Heartbeat; the acks leave by frame."""
    G = 70
    peers = P.make_groups(G, 3, seed=8)[G:2 * G].copy()  # replica 1: node 2, leader (node 1) in slot 0
    peers["self_slot"] = abi.GR_SLOT_NONE
    peers["remote_id"][:, 1:] = 0
    for f in ("match", "next", "snapshot_index", "state", "active", "kind"):
        peers["remotes"][f][:, 1:] = 0
    hb = np.zeros(G, abi.MESSAGE)
    hb["peer"], hb["type"], hb["slot"] = np.arange(G), abi.HEARTBEAT, 0
    hb["term"], hb["commit"] = peers["term"], peers["committed"]
    loc = P.propose_locals(G, np.zeros(0, np.int64), pass_index=1)
    targets = (np.arange(G, dtype=np.uint32).reshape(G, 1) % 3).astype(np.uint32)
    nw, nh = _twins_other_slots(gpu, peers, 1, hb, loc, np.arange(G) + 1, targets, 3, dict(WO.CFG, max_batch_msgs=4))
    assert nw == G and nh == 0

"""gr_collect_updates on the device-resident path (gpuraft.h): which peers have
a pb.Update after a pass, as compact records. The reference for every
comparison is the dense gr_collect_results plus Engine.sync taken at the same
moment, fed through the Python restatement of Peer.HasUpdate / Peer.Commit in
tests/updates_common.py; devsim.DeviceLockstep keeps both of those under oracle
parity pass by pass."""
import numpy as np
import pytest

from dragonboat_amd import abi, populations as P
from dragonboat_amd.engine import Engine, GpuRaftError
import devsim
import parity
import updates_common as UC

pytestmark = pytest.mark.gpu
U32 = np.uint32


def _commit_both(sim, state, slots):
    """Persist and apply everything the listed peers have outstanding, on the
    engine and in the oracle (stable_log_to = last_index, applied_to = committed)."""
    slots = np.asarray(slots, np.int64)
    if len(slots) == 0:
        return
    uc = parity.update_commits(state[slots])
    rc, st = sim.eng.commit_update(slots.astype(U32), uc)
    assert rc == 0 and not st.any(), (rc, st[st != 0][:4])
    rc, st = sim.pop.commit_update(slots.astype(U32), uc)
    assert rc == 0 and not st.any()


def _persisting(dense, state, slots):
    """Peers of `slots` with entries still to save or to apply."""
    d, s = dense[slots], state[slots]
    return (d["save_from"] != 0) | (d["committed"] > np.maximum(s["log_applied"], s["first_index_m1"]))


def test_steady_small(gpu):
    """900 slots (three full tiles and a partial one, replica blocks of 300 not
    tile-aligned), proposals on the leaders, a collect after every pass; then the
    second and third collect of one pass."""
    G, R = 300, 3
    n = G * R
    sim = devsim.DeviceLockstep(P.make_groups(G, R, seed=12), G, R)
    ref = UC.RefUpdates(n)  # new nodes: the empty prevState
    try:
        for k in range(4):
            loc = P.propose_locals(n, np.arange(G), pass_index=k)
            sim.step(loc)
            cr, rx, dense, state = UC.check_collect(sim.eng, ref, n, propose_entries=loc["propose_entries"])
            assert len(cr) == n  # steady: committed moves on every peer
            # the first collect is all EXT (term and vote against the empty State), later ones compact
            assert len(rx) == n if k == 0 else len(rx) < n // 2
            if k < 3:
                _commit_both(sim, state, cr["peer"])
        # an immediate second collect: the records took the per-pass fields and
        # moved prev, so only entries to save / to apply are left to report
        cr2, rx2, dense2, state2 = UC.check_collect(sim.eng, ref, n)
        p2 = cr2["peer"].astype(np.int64)
        assert 0 < len(cr2) <= n and len(rx2) == 0
        assert _persisting(dense2, state2, p2).all()
        st = ref.prev[p2]
        assert np.array_equal(st["term"], dense2["term"][p2]) and np.array_equal(st["commit"], dense2["committed"][p2])
        assert not dense2["propose_result"].any() and not dense2["append_from"].any()
        _commit_both(sim, state2, p2)
        cr3, rx3, _, _ = UC.check_collect(sim.eng, ref, n)
        assert len(cr3) == 0 and len(rx3) == 0
        # and the next pass reports again
        loc = P.propose_locals(n, np.arange(G), pass_index=4)
        sim.step(loc)
        cr4, _, _, _ = UC.check_collect(sim.eng, ref, n, propose_entries=loc["propose_entries"])
        assert len(cr4) == n
    finally:
        sim.close()


def test_ranges_and_refusals(gpu):
    G, R = 300, 3
    n = G * R
    peers = P.make_groups(G, R, seed=13)
    # a fresh engine, loaded peers, no pass: reported from state alone (new
    # nodes: State against the empty prevState; log_applied = first_index_m1)
    eng = Engine(n, R)
    try:
        eng.load(peers)
        ref = UC.RefUpdates(n)
        cr, rx, dense, _ = UC.check_collect(eng, ref, n)
        assert len(cr) == n and not dense["propose_result"].any()
        cr, _, _, state = UC.check_collect(eng, ref, n)  # prev moved: entries to apply are left
        assert len(cr) == n
        UC.commit_all(eng, state, np.arange(n))
        cr, _, _, _ = UC.check_collect(eng, ref, n)
        assert len(cr) == 0
    finally:
        eng.close()
    sim = devsim.DeviceLockstep(peers, G, R)
    try:
        eng = sim.eng
        ref = UC.RefUpdates(n)
        eng.set_update_states(np.arange(n, dtype=U32), ref.launch(peers))
        # ranges: a pass, then the collect of a range equals that slice of the full
        # answer at the same moment, and moves no update state outside the range
        # (a reported lane's per-pass fields go with its record, so every range
        # gets a pass of its own)
        for k, (first, cnt) in enumerate(((37, 700), (256, 256), (899, 1))):
            loc = P.propose_locals(n, np.arange(G), pass_index=k)
            sim.step(loc)
            full = UC.RefUpdates(n)
            full.prev = before = ref.prev.copy()
            before = before.copy()
            cr, rx, dense, state = UC.check_collect(eng, ref, n, first=first, n=cnt,
                                                    propose_entries=loc["propose_entries"])
            rep, cls = full.collect(dense, state, 0, n, UC.MORE)
            inr = (rep >= first) & (rep < first + cnt)
            assert inr.any() and np.array_equal(cr["peer"].astype(np.int64), rep[inr])
            assert np.array_equal((cr["flags"] & abi.CR_EXT) != 0, cls[inr] == abi.UPD_EXT)
            out = np.ones(n, bool)
            out[first:first + cnt] = False
            # (check_collect held the engine's update states equal to ref.prev)
            assert ref.prev[out].tobytes() == before[out].tobytes()
            assert ref.prev[~out].tobytes() == full.prev[~out].tobytes()
        cr, rx = eng.collect_updates(0)  # n = 0
        assert len(cr) == 0 and len(rx) == 0
        cr, rx = eng.collect_updates(0, first=n)
        assert len(cr) == 0
        for first, cnt, flags in ((0, n + 1, 0), (n, 1, 0), (1, 0xFFFFFFFF, 0), (0, n, 4), (0, n, 0x80000001)):
            with pytest.raises(GpuRaftError) as ei:
                eng.collect_updates_flags(first, cnt, flags)
            assert ei.value.rc == -1, (first, cnt, flags)
        # GR_ESTATE while a gr_step_compact_begin is pending
        import ctypes
        loc = P.propose_locals(n, np.arange(G), pass_index=9)[:4]
        cl, lx = eng.pack_locals(loc)
        ib = abi.cinbox_of(np.zeros(0, abi.CMSG), np.zeros(0, abi.MESSAGE), cl, lx)
        assert eng.lib.gr_step_compact_begin(eng._h, ctypes.byref(ib)) == 0
        try:
            with pytest.raises(GpuRaftError) as ei:
                eng.collect_updates(n)
            assert ei.value.rc == -6
            for call in (lambda: eng.set_update_states([0], np.zeros(1, abi.UPDATE_STATE)),
                         lambda: eng.get_update_states([0])):
                with pytest.raises(GpuRaftError) as ei:
                    call()
                assert ei.value.rc == -6
        finally:
            ob = abi.COutbox()
            assert eng.lib.gr_step_compact_end(eng._h, ctypes.byref(ob)) == 0
            eng.lib.gr_release_coutbox(eng._h, ctypes.byref(ob))
        # ... and after that host-path pass, and after a gr_step: lanes are not slots
        with pytest.raises(GpuRaftError) as ei:
            eng.collect_updates(n)
        assert ei.value.rc == -6
        eng.step(None, P.propose_locals(n, np.arange(G), pass_index=10)[:8])
        with pytest.raises(GpuRaftError) as ei:
            eng.collect_updates(n)
        assert ei.value.rc == -6
        # a device-resident pass brings it back
        eng.bind_routes(sim.in_pos, sim.out_pos)
        eng.set_locals(P.propose_locals(n, np.arange(0), pass_index=11))
        eng.step_device(sim.spaces[0].data_ptr(), sim.spaces[1].data_ptr(), 1, sim.positions, 1, sim.positions, n,
                        sim.stream.cuda_stream, depth=sim.depth)
        gpu.cuda.synchronize()
        eng.collect_updates(n)
    finally:
        sim.close()


def test_sparse_config3(gpu):
    """BASELINE config 3 in small: 90 % of the groups quiesced. With everything
    outstanding committed, a pass leaves an update on few peers. The bound 0 <
    n_results < n / 2 holds for the reference itself: the CPU oracle stepping this
    population with these inputs, the rule applied to its results, reports 2, 4, 56
    and 58 of the 3,200 peers after passes 0..3 (at 100k x 5: 403, 868, 9,938 and
    10,413 of 500,000), from the third pass on the active leaders' ReadyToReads."""
    G, R = 640, 5
    n = G * R
    peers, active = P.config3(G, R, active_frac=0.1)
    sim = devsim.DeviceLockstep(peers, G, R)
    ref = UC.RefUpdates(n)
    try:
        sim.eng.set_update_states(np.arange(n, dtype=U32), ref.launch(peers))  # LaunchPeer, lastIndex > 0
        _commit_both(sim, sim.eng.sync(n), np.arange(n))
        cr, _, _, _ = UC.check_collect(sim.eng, ref, n)
        assert len(cr) == 0
        for k in range(4):
            sim.step(P.config3_locals(G, R, active, k))
            cr, rx, dense, state = UC.check_collect(sim.eng, ref, n)
            _commit_both(sim, state, cr["peer"])
        # the last of those passes: ReadIndex confirmations on the active leaders
        assert 0 < len(cr) < n // 2, len(cr)
        assert dense["n_ready"][cr["peer"].astype(np.int64)].any() and len(rx) > 0
    finally:
        sim.close()


def test_uncollected_term_change(gpu):
    """Leader changes (config 5's churn), two passes and no collect in between: a
    term or vote that moved in the first of them still arrives as a full record."""
    G, R = 300, 3
    n = G * R
    topo = P.Topology(G, R)
    rng = np.random.default_rng(7)
    peers = P.make_groups(G, R, seed=14)
    sim = devsim.DeviceLockstep(peers, G, R)
    ref = UC.RefUpdates(n)
    try:
        sim.eng.set_update_states(np.arange(n, dtype=U32), ref.launch(peers))
        loc = P.propose_locals(n, np.arange(G), pass_index=0)
        sim.step(loc)
        UC.check_collect(sim.eng, ref, n, propose_entries=loc["propose_entries"])
        cur = sim.export()
        ch = P.inject_leader_change(cur, topo, 0.3, rng)
        assert len(ch)
        sim.inject(ch, cur[ch])
        for k in (1, 2):  # no collect between these two
            loc = P.propose_locals(n, P.current_leaders(sim.export(), topo), pass_index=k)
            sim.step(loc)
        before = ref.prev.copy()
        cr, rx, dense, _ = UC.check_collect(sim.eng, ref, n, propose_entries=loc["propose_entries"])
        moved = np.nonzero((dense["term"] != before["term"]) | (dense["vote"] != before["vote"]))[0]
        assert len(moved) >= len(ch) // 2
        at = {int(p): k for k, p in enumerate(cr["peer"])}
        for p in moved:
            c = cr[at[int(p)]]  # reported, and in full
            assert c["flags"] & abi.CR_EXT
            x = rx[int(c["aux"])]
            assert x["peer"] == p and x["term"] == dense["term"][p] and x["vote"] == dense["vote"][p]
        # some of them changed term in the pass that was not collected: the last
        # pass alone left their State's term and vote as they were
        assert len(moved) > 0 and len(cr) >= len(moved)
    finally:
        sim.close()


def test_many_tiles(gpu):
    """180,224 x 3 = 540,672 slots: 2,112 tile counts, more than one scan tile of
    2,048. No oracle: two steady passes, then the default flags and GR_UPD_EVERY
    against the dense collect and sync."""
    G, R = 180_224, 3
    n = G * R
    topo = P.Topology(G, R)
    peers = P.make_groups(G, R, seed=15)
    eng = Engine(n, R)
    try:
        eng.load(peers)
        in_pos, out_pos = topo.loopback_routes(R)
        eng.bind_routes(in_pos, out_pos)
        nb = eng.space_bytes(1, n * R)
        spaces = [gpu.zeros(nb, dtype=gpu.uint8, device="cuda") for _ in range(2)]
        stream = gpu.cuda.current_stream()
        loc = P.propose_locals(n, np.arange(G), pass_index=0)
        eng.set_locals(loc)
        ref = UC.RefUpdates(n)
        eng.set_update_states(np.arange(n, dtype=U32), ref.launch(peers))
        for k in range(2):
            eng.step_device(spaces[k % 2].data_ptr(), spaces[(k + 1) % 2].data_ptr(), 1, n * R, 1, n * R, n,
                            stream.cuda_stream)
        gpu.cuda.synchronize()
        # a sparse answer first: only slots of a few tiles far apart have anything
        # new against prev = their current State
        dense, state = eng.collect_results(n), eng.sync(n)
        now = np.zeros(n, abi.UPDATE_STATE)
        now["term"], now["vote"], now["commit"] = dense["term"], dense["vote"], dense["committed"]
        keep = np.ones(n, bool)
        keep[[0, 255, 256, 300_000, 524_287, 524_288, 540_671]] = False
        ref.prev[keep] = now[keep]
        eng.set_update_states(np.arange(n, dtype=U32), ref.prev)
        UC.commit_all(eng, state, np.nonzero(keep)[0])
        cr, rx, _, _ = UC.check_collect(eng, ref, n, propose_entries=loc["propose_entries"])
        assert (~keep).sum() <= len(cr) < n
        cr, rx, _, _ = UC.check_collect(eng, ref, n, flags=UC.MORE | UC.EVERY)
        assert len(cr) == n
    finally:
        eng.close()


def test_set_get_update_states(gpu):
    n = 700
    eng = Engine(n, 3)
    try:
        every = np.arange(n, dtype=U32)
        assert not eng.get_update_states(every).view(np.uint64).any()  # zeroed: the empty State
        rng = np.random.default_rng(3)
        slots = rng.permutation(n)[:300].astype(U32)
        recs = np.zeros(300, abi.UPDATE_STATE)
        for f in recs.dtype.names:
            recs[f] = rng.integers(0, 2**63, 300, dtype=np.uint64)
        eng.set_update_states(slots, recs)
        assert eng.get_update_states(slots).tobytes() == recs.tobytes()
        want = np.zeros(n, abi.UPDATE_STATE)
        want[slots] = recs
        assert eng.get_update_states(every).tobytes() == want.tobytes()
        eng.load(P.make_groups(100, 3, seed=1))  # a load leaves the records alone
        assert eng.get_update_states(every).tobytes() == want.tobytes()
        for bad in ([n], [5, 5], [0, 1, n + 7]):
            for call in (lambda b: eng.set_update_states(b, np.ones(len(b), abi.UPDATE_STATE)),
                         eng.get_update_states):
                with pytest.raises(GpuRaftError) as ei:
                    call(bad)
                assert ei.value.rc == -4  # GR_ERANGE, before anything is written
        assert eng.get_update_states(every).tobytes() == want.tobytes()
        eng.set_update_states([], np.zeros(0, abi.UPDATE_STATE))
        assert len(eng.get_update_states([])) == 0
    finally:
        eng.close()

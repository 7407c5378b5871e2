"""The steady kernel's wave-uniform addressing instance on the device.

Small populations under the split schedule (tests/test_commit_lag.py's
settings: GR_SPLIT_MIN_LANES=1, GR_SMALL_BLOCKS=0), so the steady kernel, not
the fused small pass, steps them. devsim.DeviceLockstep compares every peer's
state, every mailbox, every result and the escalations with the oracle after
every pass; these cases add which instance ran (gr_steady_wave_uniform) and that
the steady lanes, not the tail kernels, finished the lanes.

The shapes: 64 groups per replica block (one wave per role; the mailbox runs of
the three blocks start at positions 64, 128, 192 of a tile), 192 (state tiles
and mailbox tiles cut the blocks at different phases, as 1M x 3 does: 3M / 256
is not whole), 320 (several tiles, an odd workgroup count), and 130, where only
the per-lane instance is valid.
"""
import numpy as np
import pytest

from dragonboat_amd import populations as P


def _split(monkeypatch):
    monkeypatch.setenv("GR_SPLIT_MIN_LANES", "1")  # read at gr_create
    monkeypatch.setenv("GR_SMALL_BLOCKS", "0")     # the split schedule, not the fused small-pass kernel


def _lockstep(G, R=3, seed=11):
    import devsim
    return devsim.DeviceLockstep(P.make_groups(G, R, seed=seed, election=10, heartbeat=1), G, R)


def _run_parity(ls, G, R, want_wu, steady_lanes):
    """Six passes with a proposal per leader, then five with one every other
    pass (unshared mailbox pairs, H_MP clears and MATCH row stores). The last two
    passes of the first phase run timed: no lane may leave the steady kernel."""
    n = R * G
    assert ls.eng.steady_wave_uniform() == want_wu
    k = 0
    for _ in range(4):  # warm-up: the pipeline fills, the waves get their hints
        ls.step(P.propose_locals(n, np.arange(G), pass_index=k))
        k += 1
    ls.eng.timing_begin()
    for _ in range(2):
        ls.step(P.propose_locals(n, np.arange(G), pass_index=k))
        k += 1
    t = ls.eng.timing_end()
    print("timed passes:", t)
    assert t["passes"] == 2
    if steady_lanes:
        assert t["bailed_lanes"] == 0, t
    for x in range(5):
        ls.step(P.propose_locals(n, np.arange(G) if x % 2 else [], pass_index=k))
        k += 1
    assert ls.eng.steady_wave_uniform() == want_wu  # the spaces of the passes allow it too
    assert ls.stats["escalations"] == 0 and ls.stats["commits"] > 0, ls.stats


@pytest.mark.gpu
@pytest.mark.parametrize("G,want_wu", [(64, True), (192, True), (320, True), (130, False)])
def test_parity_loopback(gpu, monkeypatch, G, want_wu):
    _split(monkeypatch)
    ls = _lockstep(G)
    try:
        # 130: the per-lane instance (its waves mix roles, so some are unhinted
        # and their lanes are the tail kernels': no count asserted)
        _run_parity(ls, G, 3, want_wu, steady_lanes=want_wu)
    finally:
        ls.close()


@pytest.mark.gpu
def test_parity_per_lane_instance_forced(gpu, monkeypatch):
    """GR_STEADY_WU=0: routes that allow the wave-uniform instance run the per-lane one."""
    _split(monkeypatch)
    monkeypatch.setenv("GR_STEADY_WU", "0")
    ls = _lockstep(192)
    try:
        _run_parity(ls, 192, 3, False, steady_lanes=False)
    finally:
        ls.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tail_mode", [1, 2])
def test_parity_hand_overs(gpu, monkeypatch, tail_mode):
    """192 x 3 with leader changes (p = 0.1 per pass) and ticks. Tail mode 1 runs
    the LC = true instance (role instances after it) on the new addressing, mode
    2 the LC = false one with the general kernel walking the retry lists. A lane
    that fails a precondition must have stored nothing: its later step, by
    another kernel, still equals the oracle's.

    The retry lists' counts are not visible through the interface. What is: on a
    pass without ticks, whose tick lists are therefore empty, every lane the tick
    or general lane stepped (gr_timing bailed_lanes) came through the steady
    kernel's retry lists, directly (mode 2) or by way of the role instances
    (mode 1). The case asserts such lanes on a tickless pass."""
    _split(monkeypatch)
    monkeypatch.setenv("GR_TAIL_MODE", str(tail_mode))
    G, R = 192, 3
    n = R * G
    ls = _lockstep(G, seed=31)
    topo = P.Topology(G, R)
    rng = np.random.default_rng(77)
    try:
        assert ls.eng.steady_wave_uniform()
        for k in range(4):
            ls.step(P.propose_locals(n, np.arange(G), pass_index=k))
        injected, retried = 0, 0
        for k in range(4, 12):
            cur = ls.export()
            ch = P.inject_leader_change(cur, topo, 0.1, rng)
            ls.inject(ch, cur[ch])
            injected += len(ch)
            ticks = 1 if k % 2 else 0
            ls.eng.timing_begin()
            ls.step(P.propose_locals(n, P.current_leaders(ls.export(), topo), pass_index=k, ticks=ticks))
            t = ls.eng.timing_end()
            if not ticks:
                retried += t["bailed_lanes"]
        print("injected", injected, "retry lanes on tickless passes", retried, ls.stats)
        assert injected > 0 and retried > 0
    finally:
        ls.close()


@pytest.mark.gpu
def test_parity_affine_exchange(gpu, monkeypatch):
    """RT_AFFINE through the exchange path (spread placement on one rank: block
    bases k * G, 64-aligned at G = 192): the wave-uniform instance is selected
    and devsim.run_device's per-pass parity holds. An unaligned base cannot come
    out of these helpers (every base is a multiple of G, and a G that is no
    multiple of 64 already fails on route_g), so that row of the truth table is
    tested on the CPU: tests/test_steady_wu.py::test_predicate_affine_bases."""
    import devsim
    from dragonboat_amd.engine import Engine
    from dragonboat_amd.exchange import Exchange
    _split(monkeypatch)
    G, R = 192, 3
    ex = Exchange(G, R, R, 1, 0, "spread", seed=2, exchange=True)
    base = ex.in_pos[ex.in_pos != 0xFFFFFFFF]
    assert np.all((base - np.tile(np.arange(G), len(base) // G)) % 64 == 0)
    eng = Engine(ex.n_peers, R)
    try:
        eng.load(ex.peers)
        eng.bind_routes(ex.in_pos, ex.out_pos)
        assert eng.steady_wave_uniform()
    finally:
        eng.close()
    devsim.run_device(G, R, 8, placement="spread")
    # and a population whose blocks are not 64-aligned keeps the per-lane instance
    ex = Exchange(130, R, R, 1, 0, "spread", seed=2, exchange=True)
    eng = Engine(ex.n_peers, R)
    try:
        eng.load(ex.peers)
        eng.bind_routes(ex.in_pos, ex.out_pos)
        assert not eng.steady_wave_uniform()
    finally:
        eng.close()

"""gr_wire_out_host (gpuraft.h): the outbound wire rule on the CPU. The same
GR_HD code runs in the kernels of gr_step_wire_out (tests/test_wire_out.py), so
what is pinned here is the semantics: which mailboxes go by wire, the records,
their order and the batch cuts, through the oracle's own codec and back."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from dragonboat_amd import abi, populations as P, wire as W
import parity
import wireout as WO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gpuraft.h")


def _steady_outbox():
    """The oracle's outbox after two proposal passes, G = 64, R = 3: commit
    broadcasts + proposals (held pairs) and accepts (entry-free)."""
    from oracle.pyoracle import OraclePopulation
    G, R = 64, 3
    peers = P.make_groups(G, R, seed=4)
    topo = P.Topology(G, R)
    pop = OraclePopulation(peers, R)
    o = pop.step(np.zeros(0, abi.MESSAGE), P.propose_locals(R * G, np.arange(G), pass_index=0))
    o = pop.step(topo.route_messages(o["msgs"]), P.propose_locals(R * G, np.arange(G), pass_index=1))
    return G, R, peers, WO.outbox_order(o["msgs"])


def _config3_outbox():
    """P.config3(40, 5) with ticks and ReadIndex: heartbeats with contexts, their
    acks, ReadIndex forwards; two passes' outboxes (the second answers the first)."""
    from oracle.pyoracle import OraclePopulation
    G, R = 40, 5
    peers, active = P.config3(G, R)
    topo = P.Topology(G, R)
    pop = OraclePopulation(peers, R)
    msgs = np.zeros(0, abi.MESSAGE)
    outs = []
    for k in range(3):
        o = pop.step(msgs, P.config3_locals(G, R, active, k))
        msgs = topo.route_messages(o["msgs"])
        outs.append(WO.outbox_order(o["msgs"]))
    return G, R, peers, outs


@pytest.fixture(scope="module")
def outboxes(built):
    G, R, peers, out = _steady_outbox()
    G3, R3, peers3, outs3 = _config3_outbox()
    return [(G, R, peers, out)] + [(G3, R3, peers3, o) for o in outs3]


def _through_codec(G, R, peers, out, cfg, targets, n_targets):
    """gr_wire_out_host, then the oracle's MarshalTo and Unmarshal, then back to
    outbox records. Returns (merged outbox, held flags, batches, batch_target)."""
    from dragonboat_amd.engine import wire_out_host
    from oracle import pywire
    n = R * G
    cl = (np.arange(n) % G) + 1
    bat, wm, bt, held = wire_out_host(out, cl, peers["node_id"], peers["remote_id"], targets, n_targets, cfg)
    WO.check_batches(bat, bt, len(wm), cfg, n_targets)
    assert len(wm) + int(held.sum()) == len(out)
    if len(bat):
        assert np.array_equal(wm["batch"], np.repeat(np.arange(len(bat)), bat["n_msgs"]))
        frames = pywire.encode(WO.SOURCE, bat, wm, np.zeros(0, W.WENTRY))
        table, dm, de = pywire.decode(frames, W.frames_table(bat["frame_off"], bat["frame_len"]))
        assert np.all(table["status"] == W.OK) and len(de) == 0 and len(dm) == len(wm)
        assert np.array_equal(table["n_msgs"], bat["n_msgs"])
        for f in W.MSG_VALUE_FIELDS:
            if f not in ("msg_off", "msg_len"):
                assert np.array_equal(dm[f], wm[f]), f
    else:
        dm = wm
    d = WO.Directory(cl, peers["node_id"], peers["remote_id"], R)
    return WO.merge(out[held], d.records(dm)), held, bat, bt


def test_parity_through_oracle_codec(outboxes):
    wired = heldn = 0
    for G, R, peers, out in outboxes:
        targets = WO.replica_targets(R * G, R)
        merged, held, bat, bt = _through_codec(G, R, peers, out, WO.CFG, targets, R)
        # the wire mail plus the held records are the outbox: as a set and in per-mailbox order
        assert len(merged) == len(out) and not parity.compare_msgs(merged, out)
        assert np.array_equal(merged[["peer", "slot"]], out[["peer", "slot"]])
        want, why = WO.rule(out, targets)
        assert np.array_equal(held, want)
        assert all(w is not None for w, h in zip(why, held) if h)       # every held record breaks a clause
        assert all(w is None for w, h in zip(why, held) if not h)       # no wire record breaks any
        wired += int((~held).sum())
        heldn += int(held.sum())
    assert wired > 0 and heldn > 0


@pytest.mark.parametrize("mbm", [1, 3, 2**31])
def test_batch_cuts(outboxes, mbm):
    for G, R, peers, out in outboxes[:2]:
        n = R * G
        # targets 0, 2, 4, ..: the odd ones get no mail; one pair with mail stays with the host
        targets = WO.replica_targets(n, R) * 2
        k = int(np.nonzero(out["n_entries"] == 0)[0][0])
        hp, hj = int(out["peer"][k]), int(out["slot"][k])
        targets[hp, hj] = abi.TARGET_HOST
        cfg = dict(WO.CFG, max_batch_msgs=mbm)
        merged, held, bat, bt = _through_codec(G, R, peers, out, cfg, targets, 2 * R)
        assert len(merged) == len(out) and not parity.compare_msgs(merged, out)
        assert np.all(held[(out["peer"] == hp) & (out["slot"] == hj)])
        assert np.all(bt % 2 == 0)  # a target without mail gets no batch
        per_target = {}
        want, _ = WO.rule(out, targets)
        assert np.array_equal(held, want)
        for t in targets[out["peer"][~want].astype(np.int64), out["slot"][~want].astype(np.int64)]:
            per_target[int(t)] = per_target.get(int(t), 0) + 1
        assert len(bat) == sum(-(-c // mbm) for c in per_target.values())
        for t, c in per_target.items():
            sizes = bat["n_msgs"][bt == t]
            assert np.all(sizes[:-1] == mbm) and sizes.sum() == c


def _raw_call(lib, msgs, cl, nd, rid, tg, n_peers, slots, n_targets, cfg, null=None):
    n = len(msgs)
    bat = np.full(n, 0xAB, np.uint8).repeat(W.BATCH.itemsize)
    wm = np.full(n * W.WMESSAGE.itemsize, 0xAB, np.uint8)
    bt = np.full(n, 0xABABABAB, np.uint32)
    held = np.full(n, 0xAB, np.uint8)
    nb, nw = ctypes.c_size_t(777), ctypes.c_size_t(777)
    args = dict(msgs=msgs.ctypes.data, cl=cl.ctypes.data, nd=nd.ctypes.data, rid=rid.ctypes.data, tg=tg.ctypes.data,
                bat=bat.ctypes.data, wm=wm.ctypes.data, bt=bt.ctypes.data, held=held.ctypes.data)
    if null:
        args[null] = None
    rc = lib.gr_wire_out_host(args["msgs"], n, args["cl"], args["nd"], args["rid"], n_peers, slots, args["tg"],
                              n_targets, ctypes.byref(cfg) if cfg is not None else None, args["bat"],
                              ctypes.byref(nb), args["wm"], ctypes.byref(nw), args["bt"], args["held"])
    untouched = np.all(bat == 0xAB) and np.all(wm == 0xAB) and np.all(bt == 0xABABABAB) and np.all(held == 0xAB) \
        and nb.value == 777 and nw.value == 777
    return rc, untouched


def test_refusals_write_nothing(outboxes):
    from dragonboat_amd.engine import load_library, wire_out_cfg
    lib = load_library()
    G, R, peers, out = outboxes[0]
    n = R * G
    cl = np.ascontiguousarray((np.arange(n) % G) + 1, np.uint64)
    nd = np.ascontiguousarray(peers["node_id"], np.uint64)
    rid = np.ascontiguousarray(peers["remote_id"][:, :R], np.uint64)
    tg = np.ascontiguousarray(WO.replica_targets(n, R))
    cfg = wire_out_cfg(WO.CFG)
    EINVAL, ESTATE = -1, -6
    rc, clean = _raw_call(lib, out, cl, nd, rid, tg, n, R, R, cfg)
    assert rc == 0 and not clean  # the accepted call does write
    bad = tg.copy()
    bad[n // 2, 1] = R  # a target index out of range
    cases = {
        "index": dict(tg=bad, n_targets=R), "zero targets": dict(n_targets=0),
        "too many targets": dict(n_targets=abi.MAX_TARGETS + 1),
        "zero batch": dict(cfg=wire_out_cfg(dict(WO.CFG, max_batch_msgs=0))), "no cfg": dict(cfg=None),
    }
    for name, kw in cases.items():
        rc, clean = _raw_call(lib, out, cl, nd, rid, kw.get("tg", tg), n, R, kw.get("n_targets", R),
                              kw.get("cfg", cfg))
        assert rc in (EINVAL, ESTATE) and clean, name
    for null in ("msgs", "cl", "nd", "rid", "tg", "bat", "wm", "bt", "held"):
        rc, clean = _raw_call(lib, out, cl, nd, rid, tg, n, R, R, cfg, null=null)
        assert rc in (EINVAL, ESTATE) and clean, null
    # the accepted maximum
    rc, clean = _raw_call(lib, out, cl, nd, rid, tg, n, R, abi.MAX_TARGETS, cfg)
    assert rc == 0


def test_struct_sizes_match_header(tmp_path):
    fields = {"gr_wire_out_cfg": [f for f in abi.WIRE_OUT_CFG.names if f != "pad"],
              "gr_wire_out": ["d_batches", "n_batches", "d_msgs", "n_msgs", "batch_target"]}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', "int main(void){",
             'printf("GR_TARGET_HOST x %u\\n", GR_TARGET_HOST);', 'printf("GR_MAX_TARGETS x %u\\n", GR_MAX_TARGETS);']
    for t, fs in fields.items():
        lines.append(f'printf("{t} sizeof %zu\\n", sizeof({t}));')
        lines += [f'printf("{t} {f} %zu\\n", offsetof({t}, {f}));' for f in fs]
    lines.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(c)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        t, f, v = line.split()
        got[(t, f)] = int(v)
    assert got[("gr_wire_out_cfg", "sizeof")] == abi.WIRE_OUT_CFG.itemsize == ctypes.sizeof(abi.WireOutCfg)
    assert got[("gr_wire_out", "sizeof")] == ctypes.sizeof(abi.WireOut)
    for f in fields["gr_wire_out_cfg"]:
        assert got[("gr_wire_out_cfg", f)] == abi.WIRE_OUT_CFG.fields[f][1] == getattr(abi.WireOutCfg, f).offset, f
    for f in fields["gr_wire_out"]:
        assert got[("gr_wire_out", f)] == getattr(abi.WireOut, f).offset, f
    assert got[("GR_TARGET_HOST", "x")] == abi.TARGET_HOST and got[("GR_MAX_TARGETS", "x")] == abi.MAX_TARGETS


def test_sanitizer_program():
    """tests/native/wire_out_san.hip: the host function's code under ASAN + UBSAN
    in a stand-alone program (its own main), refusal cases included."""
    from dragonboat_amd import build
    exe = build.build_wire_out_san()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "wire_out_san ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])

"""The quiesce manager off the GPU: the reference's quiesce_test.go tables, the
Python model (tests/quiesce_model.py) and the host build of gr_quiesce.h (the
code the device kernel runs) must agree, call by call and pass by pass."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from dragonboat_amd import abi
from quiesce_model import NO_LIMIT, QuiesceManager

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = os.path.join(ROOT, "tests", "golden", "quiesce_tables.json")
QH_TICK, QH_ACT, QH_TRY_ENTER, QH_QUIESCED, QH_NEW_TO_QUIESCE, QH_JUST_EXITED, QH_MESSAGE = range(7)


@pytest.fixture(scope="module")
def qh():
    from dragonboat_amd import build
    lib = ctypes.CDLL(build.build_quiesce_host())
    lib.qh_op.restype = ctypes.c_uint64
    lib.qh_op.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32]
    lib.qh_run_passes.restype = None
    lib.qh_run_passes.argtypes = [ctypes.c_uint32] + [ctypes.c_void_p] * 8
    lib.qh_roundtrip.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.qh_splitmix64.restype = ctypes.c_uint64
    lib.qh_splitmix64.argtypes = [ctypes.c_uint64]
    return lib


class HostManager:
    """One record driven through libquiesce_host.so's qh_op."""

    def __init__(self, lib, election_tick, enabled):
        self.lib = lib
        self.rec = np.zeros(1, abi.QUIESCE_STATE)
        self.rec["election_tick"] = election_tick
        self.rec["enabled"] = enabled
        self.flag = np.zeros(1, np.uint8)

    def op(self, op, arg=0):
        return self.lib.qh_op(self.rec.ctypes.data, self.flag.ctypes.data, op, arg)


def test_struct_size_matches_header(tmp_path, qh):
    hdr = os.path.join(ROOT, "include", "gpuraft.h")
    names = [f for f in abi.QUIESCE_STATE.names if f != "pad"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{hdr}"', "int main(void){",
             'printf("%zu\\n", sizeof(gr_quiesce_state));']
    lines += [f'printf("%zu\\n", offsetof(gr_quiesce_state, {f}));' for f in names]
    lines.append("return 0;}")
    c = tmp_path / "q.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "q"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(c)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == abi.QUIESCE_STATE.itemsize == 48 == qh.qh_sizeof_state()
    assert got[1:] == [abi.QUIESCE_STATE.fields[f][1] for f in names]


def test_golden_tables_model_and_host_build(qh):
    tables = json.load(open(TABLES))["tests"]
    assert len(tables) == 5
    for t in tables:
        for case in t["cases"]:
            m = QuiesceManager(t["election_tick"], t["enabled"])
            h = HostManager(qh, t["election_tick"], t["enabled"])
            for op in case:
                where = (t["name"], op)
                if op["op"] == "tick":
                    for _ in range(op["n"]):
                        assert m.increase_quiesce_tick() == h.op(QH_TICK), where
                elif op["op"] == "act":
                    m.record_activity(op["type"])
                    h.op(QH_ACT, op["type"])
                elif op["op"] == "tick_act":
                    for _ in range(op["n"]):
                        assert m.increase_quiesce_tick() == h.op(QH_TICK), where
                        m.record_activity(op["type"])
                        h.op(QH_ACT, op["type"])
                else:
                    assert op["op"] == "expect"
                    assert m.tick == op["tick"] == int(h.rec["tick"][0]), where
                    if "quiesced" in op:
                        assert m.quiesced() == op["quiesced"] == bool(h.op(QH_QUIESCED)), where
                    if "new_to_quiesce" in op:
                        assert m.new_to_quiesce() == op["new_to_quiesce"] == bool(h.op(QH_NEW_TO_QUIESCE)), where
                    if op.get("no_activity_since_is_tick"):
                        assert m.no_activity_since == m.tick, where
                        assert int(h.rec["no_activity_since"][0]) == int(h.rec["tick"][0]), where
                rec = np.zeros(1, abi.QUIESCE_STATE)
                m.to_record(rec[0])
                assert rec.tobytes() == h.rec.tobytes() and m.flag == bool(h.flag[0]), where


def test_quirks(qh):
    # a disabled manager returns tick 0 and is never quiesced, whatever its fields
    m, h = QuiesceManager(2, False, quiesced_since=5), HostManager(qh, 2, 0)
    h.rec["quiesced_since"] = 5
    assert m.increase_quiesce_tick() == 0 == h.op(QH_TICK)
    assert not m.quiesced() and not h.op(QH_QUIESCED)
    # tryEnterQuiesce at tick 0 (electionTick 0, so no just-exited window): quiescedSince
    # stays 0, the peer is not quiesced, the flag is set
    m, h = QuiesceManager(0, True), HostManager(qh, 0, 1)
    m.try_enter_quiesce()
    h.op(QH_TRY_ENTER)
    assert m.flag and h.flag[0] == 1 and not m.quiesced() and not h.op(QH_QUIESCED)
    assert m.quiesced_since == 0 == int(h.rec["quiesced_since"][0])
    # ... and inside the just-exited window of a fresh manager (tick 0 - exit 0 < threshold): nothing
    m, h = QuiesceManager(2, True), HostManager(qh, 2, 1)
    m.try_enter_quiesce()
    h.op(QH_TRY_ENTER)
    assert not m.flag and h.flag[0] == 0


def _draw_pass(rng, n, mode):
    """Inputs of one pass for n peers: (read_index, msgs per peer, raw ticks, limits)."""
    ri = (rng.random(n) < 0.02).astype(np.uint8)
    ticks = rng.choice([0, 1, 1, 1, 1, 2, 3], n).astype(np.uint32)
    active = rng.random(n) < np.where(mode == 0, 0.03, np.where(mode == 1, 0.6, 0.15))
    nm = np.where(active, rng.integers(1, 4, n), 0)
    pool = [abi.HEARTBEAT, abi.HEARTBEAT_RESP, abi.HEARTBEAT, abi.QUIESCE, abi.QUIESCE, abi.REPLICATE,
            abi.REPLICATE_RESP, abi.SNAPSHOT_STATUS, abi.UNREACHABLE, abi.PROPOSE, abi.REQUEST_VOTE, abi.READ_INDEX]
    hb_only = [abi.HEARTBEAT, abi.HEARTBEAT_RESP]
    msgs = []
    for x in range(n):
        src = hb_only if mode[x] == 1 else pool
        ms = []
        for _ in range(nm[x]):
            t = src[rng.integers(len(src))]
            hint = int(rng.random() < 0.1) * 7 if t in hb_only else int(rng.integers(0, 3))
            ms.append((t, hint))
        msgs.append(ms)
    limits = np.where(rng.random(n) < 0.05, rng.integers(0, 6, n), NO_LIMIT).astype(np.uint32)
    return ri, msgs, ticks, limits


def test_random_sequences_host_build_matches_model(qh):
    n, passes = 2000, 200
    rng = np.random.default_rng(20240611)
    recs = np.zeros(n, abi.QUIESCE_STATE)
    recs["election_tick"] = rng.choice([0, 1, 2, 2, 2, 3], n)
    recs["enabled"] = rng.random(n) >= 0.2  # disabled peers
    warm = rng.random(n) < 0.3  # random initial records, some already quiesced
    recs["tick"][warm] = rng.integers(1, 500, warm.sum())
    recs["no_activity_since"][warm] = recs["tick"][warm] - rng.integers(0, 2, warm.sum())
    recs["exit_quiesce_tick"][warm] = rng.integers(0, 2, warm.sum()) * (recs["tick"][warm] - 1)
    qd = warm & (rng.random(n) < 0.4)
    recs["quiesced_since"][qd] = recs["tick"][qd] - rng.integers(0, 4, qd.sum())
    models = [QuiesceManager.from_record(r) for r in recs]
    mode = rng.choice([0, 0, 1, 2], n)  # mostly idle / heartbeats only / chatty
    seen = dict.fromkeys(("disabled", "tick0_notice", "hb_new_window", "hb_past_window", "notice_just_exited",
                          "hint_heartbeat_exit", "send", "prefix"), 0)
    out = np.zeros(3 * n, np.uint32)
    want = np.zeros(n, abi.QUIESCE_STATE)
    for _ in range(passes):
        ri, msgs, ticks, limits = _draw_pass(rng, n, mode)
        off = np.zeros(n + 1, np.uint32)
        off[1:] = np.cumsum([len(m) for m in msgs])
        types = np.array([t for ms in msgs for t, _ in ms] + [0], np.uint8)
        hints = np.array([h > 0 for ms in msgs for _, h in ms] + [0], np.uint8)
        qh.qh_run_passes(n, recs.ctypes.data, ri.ctypes.data, off.ctypes.data, types.ctypes.data, hints.ctypes.data,
                         ticks.ctypes.data, limits.ctypes.data, out.ctypes.data)
        for x, m in enumerate(models):
            lim = int(limits[x])
            if lim == NO_LIMIT and not ri[x]:  # which of the issue's cases this pass exercises
                s = m.copy()
                for t, h in msgs[x]:
                    hb = t in (abi.HEARTBEAT, abi.HEARTBEAT_RESP)
                    seen["disabled"] += not s.enabled
                    seen["tick0_notice"] += t == abi.QUIESCE and s.tick == 0 and s.enabled
                    seen["hb_new_window"] += hb and not h and s.new_to_quiesce()
                    seen["hb_past_window"] += hb and not h and s.quiesced() and not s.new_to_quiesce()
                    seen["notice_just_exited"] += t == abi.QUIESCE and s.enabled and s.tick > 0 and \
                        s.just_exited_quiesce()
                    seen["hint_heartbeat_exit"] += hb and h > 0 and s.quiesced()
                    s.message(t, h)
            else:
                seen["prefix"] += lim != NO_LIMIT
            k, q, send = m.run_pass(bool(ri[x]), msgs[x], int(ticks[x]), lim)
            seen["send"] += send
            assert (k, q, int(send)) == tuple(int(v) for v in out[3 * x:3 * x + 3]), (x, msgs[x], ticks[x], lim)
            m.to_record(want[x])
        bad = np.nonzero(want != recs)[0]
        assert not len(bad), (bad[:5], want[bad[:5]], recs[bad[:5]])
    assert all(v > 0 for v in seen.values()), seen


def test_device_encoding_holds_what_it_accepts(qh):
    rng = np.random.default_rng(5)
    a = np.zeros(64, abi.QUIESCE_STATE)
    for f in ("tick", "quiesced_since", "no_activity_since", "exit_quiesce_tick"):
        a[f] = rng.integers(0, 1 << 32, 64, dtype=np.uint64)
    a["election_tick"] = rng.integers(0, 1 << 31, 64, dtype=np.uint64)
    a["enabled"] = rng.integers(0, 2, 64)
    b = np.zeros(1, abi.QUIESCE_STATE)
    for r in a:
        r1 = np.array([r])
        assert qh.qh_roundtrip(r1.ctypes.data, b.ctypes.data) == 1 and b.tobytes() == r1.tobytes()
    for f, v in (("tick", 1 << 32), ("quiesced_since", 1 << 40), ("no_activity_since", 1 << 32),
                 ("exit_quiesce_tick", 1 << 63), ("election_tick", 1 << 31), ("enabled", 2)):
        r1 = np.zeros(1, abi.QUIESCE_STATE)
        r1[f] = v
        assert qh.qh_roundtrip(r1.ctypes.data, b.ctypes.data) == 0, f


def test_splitmix64_mirror(qh):
    # Vigna's splitmix64 from state 0: the generator's first outputs
    assert abi.splitmix64(0) == 0xE220A8397B1DCDAF
    for x in (0, 1, 12345, (1 << 64) - 1, 0x9E3779B97F4A7C15):
        assert abi.splitmix64(x) == qh.qh_splitmix64(x)

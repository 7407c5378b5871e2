"""The quiesce manager on the device, stepped beside its model: a
devsim.DeviceLockstep whose device side gets raw LocalTick counts (gr_tick_all
or gr_set_locals) while the oracle gets the split that tests/quiesce_model.py
computes. After every pass: everything DeviceLockstep compares (state, every
mailbox, results, escalations), plus every quiesce record and every Quiesce
message, which must be the first of its mailbox."""
import numpy as np

from dragonboat_amd import abi
from dragonboat_amd.engine import decode_space
import devsim
import parity
from quiesce_model import QuiesceManager


def tick_locals(peers, ticks, seed):
    """gr_tick_all's local inputs as the oracle needs them: `ticks` for every
    loaded slot, the documented draw abi.splitmix64(seed + slot)."""
    n = len(peers)
    loc = np.zeros(n, abi.LOCAL)
    loc["peer"] = np.arange(n, dtype=np.uint32)
    loc["ticks"] = np.where(peers["election_timeout"] != 0, ticks, 0)
    loc["rand"] = [abi.splitmix64(seed + p) for p in range(n)]
    return loc


def quiesce_records(n, election_tick, enabled=True):
    recs = np.zeros(n, abi.QUIESCE_STATE)
    recs["election_tick"] = election_tick
    recs["enabled"] = enabled
    return recs


class QuiesceLockstep(devsim.DeviceLockstep):
    def __init__(self, peers, G, R, qrecs, lib_path=None, quiesce=True):
        super().__init__(peers, G, R, lib_path=lib_path)
        self.peers0 = peers
        self.on = quiesce
        if quiesce:
            self.eng.set_quiesce(True)
        self.eng.load_quiesce(qrecs)
        self.model = [QuiesceManager.from_record(r) for r in qrecs]
        self.qstats = {"quiesce_msgs": 0, "entered": 0, "exited": 0, "split": 0, "prefix_sends": 0}

    def all_quiesced(self):
        return all(m.quiesced() for m in self.model if m.enabled)

    def _inbox_of_peer(self):
        """[(type, hint)] per peer in item order (by sender slot, then arrival)."""
        per = [[] for _ in range(self.n)]
        m = self.msgs
        order = np.lexsort((np.arange(len(m)), m["slot"], m["peer"]))
        for x in order:
            per[int(m["peer"][x])].append((int(m["type"][x]), int(m["hint"][x])))
        return per

    def _quiesce_msgs(self, senders, st):
        """Outbox records of sendEnterQuiesceMessages (node.go:530-543): to every
        voter slot but the sender's own (st: the peers' records)."""
        out = []
        for p in senders:
            for j in range(self.S):
                if st["remotes"][p][j]["kind"] == abi.SLOT_VOTER and j != st["self_slot"][p]:
                    r = np.zeros(1, abi.MESSAGE)
                    r["peer"], r["slot"], r["type"] = p, j, abi.QUIESCE
                    out.append(r)
        return np.concatenate(out) if out else np.zeros(0, abi.MESSAGE)

    def step(self, loc=None, drop_fn=None, tick_all=None, collect=None):
        """tick_all=(ticks, seed): bind with gr_tick_all; else gr_set_locals(loc).
        loc carries raw LocalTick counts either way. collect(o): as
        DeviceLockstep.step, after the parity checks and before any reload."""
        import torch
        k = self.k
        if tick_all is not None:
            self.eng.tick_all(*tick_all)
            loc = tick_locals(self.peers0, *tick_all)
        else:
            loc = np.asarray(loc, abi.LOCAL)
            self.eng.set_locals(loc)
        assert len(loc) == self.n and np.array_equal(loc["peer"], np.arange(self.n))
        dev0 = self.eng.sync(self.n)
        q0 = self.eng.sync_quiesce(self.n)
        src, dst = self.spaces[k % 2], self.spaces[(k + 1) % 2]
        self.eng.step_device(src.data_ptr(), dst.data_ptr(), 1, self.positions, 1, self.positions, self.n,
                             self.stream.cuda_stream, depth=self.depth)
        torch.cuda.synchronize()
        res = self.eng.collect_results(self.n)
        lim = parity.limits_from(res, self.n)
        # ---- the model: the full pass gives the split the oracle steps with,
        # the prefix (items below esc_item) what the device must hold
        inbox = self._inbox_of_peer()
        eff = loc.copy()
        want_q = np.zeros(self.n, abi.QUIESCE_STATE)
        full_send, prefix_send = [], []
        for p, m in enumerate(self.model):
            ri, raw = bool(loc["read_index"][p]), int(loc["ticks"][p])
            if not self.on:
                m.to_record(want_q[p])
                continue
            was = m.quiesced()
            pre = m.copy()
            tk, qt, send = m.run_pass(ri, inbox[p], raw)
            eff["ticks"][p], eff["quiesced_ticks"][p] = tk, qt
            self.qstats["split"] += bool(tk and qt)
            self.qstats["entered"] += (not was) and m.quiesced()
            self.qstats["exited"] += was and not m.quiesced()
            if send:
                full_send.append(p)
            if lim[p] != 0xFFFFFFFF:
                _, _, ps = pre.run_pass(ri, inbox[p], raw, int(lim[p]))
                pre.to_record(want_q[p])
                if ps:
                    prefix_send.append(p)
                    self.qstats["prefix_sends"] += 1
            else:
                m.to_record(want_q[p])
                if send:
                    prefix_send.append(p)
        got_q = self.eng.sync_quiesce(self.n)
        bad = np.nonzero(got_q != want_q)[0]
        assert not len(bad), f"pass {k}: quiesce records {bad[:4]}: device {got_q[bad[:4]]} model {want_q[bad[:4]]} " \
                             f"before {q0[bad[:4]]} limits {lim[bad[:4]]}"
        o = self.pop.step(self.msgs, eff, lim, dev_before=dev0, threads=self.threads)
        dev = self.eng.sync(self.n)
        bad = parity.compare_states(dev, o["mid"], self.S)
        assert not bad, f"pass {k}: state {bad[:3]}"
        got = decode_space(dst.cpu().numpy(), 1, self.positions, self.depth)
        pos = got["peer"].astype(np.int64)
        got["peer"] = self.inv[0][pos].astype(np.uint32)
        got["slot"] = self.inv[1][pos].astype(np.uint8)
        # the Quiesce messages lead their mailboxes: stepNode sends them before getUpdate
        full = self.pop.export()
        want_prefix = self._route(np.concatenate([self._quiesce_msgs(prefix_send, full), parity.prefix_msgs(o, lim)]))
        bad = parity.compare_msgs(got, want_prefix)
        assert not bad, f"pass {k}: mailboxes {bad[:3]}"
        nq = int(np.sum(got["type"] == abi.QUIESCE))
        assert nq == int(np.sum(want_prefix["type"] == abi.QUIESCE))
        self.qstats["quiesce_msgs"] += nq
        bad = parity.compare_results(res, o["results"])
        assert not bad, f"pass {k}: results {bad[:3]}"
        bad = parity.check_escalations(res, o["esc_mask"])
        assert not bad, f"pass {k}: unjustified escalations {bad[:3]}"
        esc = res[res["escalation"] != 0]
        st = self.stats
        st["escalations"] += len(esc)
        for r in esc:
            nm = abi.ESC_NAMES[r["escalation"]]
            st["esc_reasons"][nm] = st["esc_reasons"].get(nm, 0) + 1
        st["commits"] += int(np.sum(dev["committed"] > dev0["committed"]))
        st["msgs"] += len(got)
        if collect is not None:
            o["limits"], o["device_results"] = lim, res  # which item each escalated peer stopped before
            collect(o)
            full = self.pop.export()  # the callback may have committed on the oracle
        nxt = self._route(np.concatenate([self._quiesce_msgs(full_send, full), o["msgs"]]))
        n_full = len(nxt)
        if drop_fn is not None:
            nxt = drop_fn(k, nxt)
        if len(esc) or len(nxt) != n_full:
            if len(esc):  # the host ran their suffix: raft state from the oracle, the manager from the model
                idx = esc["peer"].astype(np.int64)
                self.eng.load_peers(idx.astype(np.uint32), full[idx])
                if self.on:
                    hq = np.zeros(len(idx), abi.QUIESCE_STATE)
                    for x, p in enumerate(idx):
                        self.model[p].to_record(hq[x])
                    self.eng.load_quiesce(hq, slots=idx.astype(np.uint32))
            self._encode(nxt, dst)
            st["reencoded"] += 1
        self.msgs = nxt
        self.k += 1
        return res

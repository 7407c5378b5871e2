"""Updates out of a device-resident pass: gr_collect_updates against the dense
gr_collect_results, the only way out the device-resident path had before it.

Two populations on one GPU: the headline one (1M x 3, steady: one proposal per
leader per pass, so every peer has an update after every pass) and BASELINE
config 3 (100k x 5, 10 % of the groups active with a Tick per replica and a
ReadIndex on the leader, the rest quiesced). After a warm-up, with the update
states set as LaunchPeer sets them and everything outstanding committed
(gr_commit_update), every round is: one device pass, one timed collect, one
commit of what that collect reported. The three variants (dense
gr_collect_results over all slots, gr_collect_updates with GR_UPD_EVERY, and
with the default flags) alternate round by round within the run, --runs of
each. Collects are timed on the host clock around the call (each waits for the
device and returns with the records on the host); the two kernels of
gr_collect_updates by events (gr_updates_last).

Checked, not measured: the bytes a collect copies device to host are the two
totals' words plus 24 per record plus 168 per ext record, and on config 3 the
default collect reports exactly the peers the rule names from the dense records
and the synced state of the same moment.

Counted bytes per slot (kernel_bytes below): what the two kernels must move,
from the rows gr_io.h update_classify / update_pack list.

Usage: python tools/bench_updates.py [--runs N] [--warmup N] [--small] [--out profiles/updates/summary.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ("dense", "every", "default")


def kernel_bytes(n, n_results, n_ext, committed_rows=0):
    """Bytes the two kernels must move for n slots of which n_results are
    reported and n_ext need the full record. Classify, per slot: the result
    flag byte, eight state rows of 8 B (header, lastIndex, term, vote, savedTo,
    markerIndex, entryLog.applied, firstIndex - 1), the 24-B update state, the
    class byte written; plus the committed row where the header does not carry
    the lag (committed_rows slots; none in the steady state), the few lane rows a
    set flag names (ignored: a byte each) and 8 B per 256-slot tile. Pack, per
    slot: the class byte; per reported slot: the flag byte read and cleared, the
    six state rows a result record needs (header, lastIndex, term, vote, savedTo,
    markerIndex), the 24-B record and the 24-B update state written; per ext
    record 168 B more."""
    tiles = (n + 255) // 256
    classify = n * (1 + 8 * 8 + 24 + 1) + 8 * committed_rows + 8 * tiles
    pack = n * 1 + 8 * tiles + n_results * (2 + 6 * 8 + 24 + 24) + n_ext * 168
    return {"classify": classify, "pack": pack}


def ref_reported(np, abi, dense, state, prev):
    """Peer.HasUpdate(moreEntriesToApply = true) over dense records, the state and
    the update states (peer.go:218-241 without the msgs and snapshot conditions,
    plus the engine's own: gpuraft.h gr_update_class)."""
    U = np.uint64
    t, v, c = dense["term"], dense["vote"], dense["committed"]
    rep = ((t != 0) | (v != 0) | (c != 0)) & ((t != prev["term"]) | (v != prev["vote"]) | (c != prev["commit"]))
    rep |= dense["save_from"] != 0
    rep |= (c + U(1)) > np.maximum(state["log_applied"] + U(1), state["first_index_m1"] + U(1))
    rep |= (dense["n_ready"] != 0) | (dense["escalation"] != 0) | (dense["propose_result"] != 0) | \
        (dense["n_forwarded"] != 0)
    return np.nonzero(rep)[0]


def commits_of(np, abi, res):
    """gr_update_commit records for full result records: persist up to last_index
    (at the current term: these populations append at no other) and apply up to
    committed."""
    uc = np.zeros(len(res), abi.UPDATE_COMMIT)
    has = res["save_from"] != 0
    uc["stable_log_to"] = np.where(has, res["last_index"], 0)
    uc["stable_log_term"] = np.where(has, res["term"], 0)
    uc["applied_to"] = res["committed"]
    return uc


def run_population(name, peers, G, R, locals_fn, runs, warmup, check_sparse):
    import numpy as np
    import torch
    from dragonboat_amd import abi, populations as P
    from dragonboat_amd.engine import Engine, expand_updates

    n = G * R
    topo = P.Topology(G, R)
    eng = Engine(n, R)
    eng.load(peers)
    in_pos, out_pos = topo.loopback_routes(R)
    eng.bind_routes(in_pos, out_pos)
    nb = eng.space_bytes(1, n * R)
    spaces = [torch.zeros(nb, dtype=torch.uint8, device="cuda") for _ in range(2)]
    stream = torch.cuda.current_stream()
    every = np.arange(n, dtype=np.uint32)
    prev = np.zeros(n, abi.UPDATE_STATE)  # the host's copy of the update states
    prev["term"], prev["vote"], prev["commit"] = peers["term"], peers["vote"], peers["committed"]
    eng.set_update_states(every, prev)  # LaunchPeer with lastIndex > 0
    k = 0

    def one_pass():
        nonlocal k
        eng.set_locals(locals_fn(k))
        eng.step_device(spaces[k % 2].data_ptr(), spaces[(k + 1) % 2].data_ptr(), 1, n * R, 1, n * R, n,
                        stream.cuda_stream)
        torch.cuda.synchronize()
        k += 1

    def commit(res):
        """Commit what the full records `res` report, and move the host's prev."""
        nonlocal prev
        if len(res) == 0:
            return
        p = res["peer"].astype(np.int64)
        rc, st = eng.commit_update(res["peer"], commits_of(np, abi, res))
        assert rc == 0 and not st.any(), (rc, np.unique(st, return_counts=True))
        prev["term"][p], prev["vote"][p], prev["commit"][p] = res["term"], res["vote"], res["committed"]

    # everything outstanding after the load (entries to apply), then the warm-up
    cr, rx = eng.collect_updates(n, every=True)
    commit(expand_updates(cr, rx, prev["term"], prev["vote"]))
    for _ in range(warmup):
        one_pass()
        cr, rx = eng.collect_updates(n, every=True)
        commit(expand_updates(cr, rx, prev["term"], prev["vote"]))
    ms = {v: [] for v in VARIANTS}
    kern = {v: {"classify_ms": [], "pack_ms": []} for v in VARIANTS[1:]}
    counts = {}
    for _ in range(runs):
        for v in VARIANTS:
            one_pass()
            if v == "dense":
                t0 = time.perf_counter()
                res = eng.collect_results(n)
                ms[v].append((time.perf_counter() - t0) * 1e3)
                counts[v] = {"n_results": n, "n_ext_results": n, "bytes_down": n * abi.RESULT.itemsize}
                # (the update states stay with gr_collect_updates: set what its records would have)
                rep = ref_reported(np, abi, res, eng.sync(n) if check_sparse else
                                   {"log_applied": res["committed"], "first_index_m1": res["committed"]}, prev)
                res = res[rep]
                commit(res)
                if len(res):
                    eng.set_update_states(res["peer"], prev[res["peer"].astype(np.int64)])
                continue
            want = None
            if v == "default" and check_sparse:  # the reference count, from the same moment
                want = ref_reported(np, abi, eng.collect_results(n), eng.sync(n), prev)
            eng.timing_begin()
            t0 = time.perf_counter()
            cr, rx = eng.collect_updates(n, every=(v == "every"))
            ms[v].append((time.perf_counter() - t0) * 1e3)
            last = eng.updates_last()
            eng.timing_end()
            assert last["bytes_down"] == 8 + 24 * len(cr) + 168 * len(rx), last
            assert last["timed"] and (last["n_results"], last["n_ext_results"]) == (len(cr), len(rx))
            if want is not None:
                assert np.array_equal(cr["peer"].astype(np.int64), want), (len(cr), len(want))
            kern[v]["classify_ms"].append(last["classify_ms"])
            kern[v]["pack_ms"].append(last["pack_ms"])
            kb = kernel_bytes(n, len(cr), len(rx))
            counts[v] = {"n_results": len(cr), "n_ext_results": len(rx), "bytes_down": last["bytes_down"],
                         "kernel_bytes": kb, "kernel_bytes_per_slot": {a: b / n for a, b in kb.items()}}
            commit(expand_updates(cr, rx, prev["term"], prev["vote"]))
    eng.close()
    out = {"population": name, "slots": n, "runs": runs, "warmup": warmup,
           "collect_ms": {v: {"all": ms[v], "median": float(np.median(ms[v])), "min": min(ms[v]), "max": max(ms[v])}
                          for v in VARIANTS},
           "kernels_ms": {v: {a: {"all": b, "median": float(np.median(b))} for a, b in kern[v].items()}
                          for v in kern},
           "counts": counts}
    for v in kern:  # the kernels' times set against the bytes they must move
        for a in ("classify", "pack"):
            t = out["kernels_ms"][v][a + "_ms"]["median"]
            out["kernels_ms"][v][a + "_GBps_of_counted_bytes"] = \
                counts[v]["kernel_bytes"][a] / (t * 1e-3) / 1e9 if t > 0 else None
    d, s = out["collect_ms"]["dense"], out["collect_ms"]["default"]
    out["default_faster_than_dense_beyond_spread"] = bool(s["max"] < d["min"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--small", action="store_true", help="1/100 of both populations (a quick check of the tool)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from dragonboat_amd import build, populations as P

    torch.cuda.set_device(0)
    div = 100 if args.small else 1
    pops = []
    G, R = 1_000_000 // div, 3
    peers = P.make_groups(G, R, seed=2)
    pops.append(run_population(f"headline {G} x {R}, steady", peers, G, R,
                               lambda k, G=G, R=R: P.propose_locals(R * G, np.arange(G), pass_index=k),
                               args.runs, args.warmup, check_sparse=False))
    del peers
    G, R = 100_000 // div, 5
    peers, active = P.config3(G, R, active_frac=0.1)
    pops.append(run_population(f"config 3: {G} x {R}, 10 % active", peers, G, R,
                               lambda k, G=G, R=R: P.config3_locals(G, R, active, k),
                               args.runs, args.warmup, check_sparse=True))
    out = {"tool": "tools/bench_updates.py", "order": "alternated per round: " + ", ".join(VARIANTS),
           "round": "one device pass, one timed collect, gr_commit_update of what it reported",
           "populations": pops, "source_digest": build.source_digest(),
           "built": (build.build_record() or {}).get("source_digest")}
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

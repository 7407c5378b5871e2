"""Decommissioning a host: RemoveNode of one node id on every loaded peer of
100k groups x 3, through gr_apply_config_change, against the route a host had
before it: gr_sync_peers_to_host + gr_load_peers of the same slot list (the Go
work between the two left out, which favours that route).

Both legs are timed on the host clock around the calls (each returns after its
device work and copies are done), alternated in one session, --runs of each; the
groups are loaded afresh before every timed leg, so every leg does the same work.
Expected from the bytes that cross PCIe: 32 B per peer (a 4-byte slot and a
24-byte record up, a 4-byte status down) against 2 x (4 + sizeof(gr_peer)) = 1336.

Usage: python tools/bench_config_change.py [--groups N] [--runs N] [--out profiles/config_change.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from dragonboat_amd import abi, build, populations as P
    from dragonboat_amd.engine import Engine

    torch.cuda.set_device(0)
    G, R = args.groups, 3
    n = R * G
    peers = P.make_groups(G, R, seed=args.seed)
    slots = np.random.default_rng(args.seed).permutation(n).astype(np.uint32)
    cc = np.zeros(n, abi.CONFIG_CHANGE)
    cc["type"], cc["node_id"] = abi.CC_REMOVE_NODE, 3
    eng = Engine(n, R)
    # one untimed leg of each first: buffers grow and pages pin on first use
    eng.load(peers)
    eng.apply_config_change(slots, cc)
    eng.load_peers(slots, eng.sync_peers(slots))
    call_ms, trip_ms, sync_ms, load_ms = [], [], [], []
    for _ in range(args.runs):
        eng.load(peers)
        t0 = time.perf_counter()
        rc, st = eng.apply_config_change(slots, cc)
        call_ms.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0 and not st.any(), (rc, np.unique(st, return_counts=True))
        after = eng.sync(n)
        assert np.all(after["remotes"]["kind"][:, 2] == abi.SLOT_EMPTY)
        assert np.all(after["self_slot"][2 * G:] == abi.GR_SLOT_NONE)
        eng.load(peers)
        t0 = time.perf_counter()
        recs = eng.sync_peers(slots)
        t1 = time.perf_counter()
        eng.load_peers(slots, recs)
        t2 = time.perf_counter()
        trip_ms.append((t2 - t0) * 1e3)
        sync_ms.append((t1 - t0) * 1e3)
        load_ms.append((t2 - t1) * 1e3)
    eng.close()
    out = {"workload": f"RemoveNode of one node on all {n} peers of {G} x {R}, shuffled slot list",
           "runs": args.runs, "order": "alternated: call, round trip, call, ...",
           "apply_config_change_ms": call_ms, "sync_plus_load_ms": trip_ms, "sync_ms": sync_ms, "load_ms": load_ms,
           "bytes_per_peer": {"apply_config_change": 4 + abi.CONFIG_CHANGE.itemsize + 4,
                              "sync_plus_load": 2 * (4 + abi.PEER.itemsize)},
           "speedup_of_medians": float(np.median(trip_ms) / np.median(call_ms)),
           "source_digest": build.source_digest(), "built": (build.build_record() or {}).get("source_digest")}
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

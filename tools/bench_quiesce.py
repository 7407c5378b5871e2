"""Idle cluster: 100k groups x 3 with leaders and no proposals on one GPU,
device-resident (gr_step_device over loopback mailbox spaces in HBM), the
quiesce manager on the device (gr_set_quiesce) and one gr_tick_all(1) per pass:
no local record is uploaded. Every manager starts awake at tick 0, so after
10 x election ticks without activity every peer enters quiesce, tells its
voters, and from then on takes QuiescedTicks only.

Then one pass with a proposal in every group (the first burst: leaders wake on
the acks, followers on the Replicate), and a second burst a few passes later,
inside the just-exited window, where Quiesce notices are ignored.

Reported: the first pass after which every peer is quiesced, device ms per
pass (the kernels' HIP-event time, gr_timing, quiesce pass included) while
active and while quiesced, Quiesce messages sent (decoded from the out space on
the passes where peers entered quiesce), peers awake three passes after the
first burst, and escalations by the engine's counter (expected 0).

Usage: python tools/bench_quiesce.py [--groups N] [--election N] > bench_out/quiesce.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(G, R, election, seed, quiet_passes, gap):
    import numpy as np
    import torch
    from dragonboat_amd import abi, build, populations as P
    from dragonboat_amd.engine import Engine, decode_space
    from dragonboat_amd.exchange import Exchange

    ex = Exchange(G, R, R, 1, 0, "local")
    n = ex.n_peers
    eng = Engine(n, R, quiesce=True)
    peers = P.make_groups(G, R, seed=seed, election=election)
    peers["election_tick"] = 0
    eng.load(peers)
    q = np.zeros(n, abi.QUIESCE_STATE)
    q["election_tick"], q["enabled"] = election, 1
    eng.load_quiesce(q)
    eng.bind_routes(ex.in_pos, ex.out_pos)
    spaces = ex.allocate(eng, torch.device("cuda", 0))
    stream = torch.cuda.current_stream()
    pad = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")  # hides the launch latency (bench_configs.py)
    leaders = np.arange(G)
    ms, asleep = [], []
    notices = 0
    k = 0

    def one_pass(burst):
        nonlocal k, notices
        if burst:
            eng.set_locals(P.propose_locals(n, leaders, seed=seed, pass_index=k, ticks=1))
        else:
            eng.tick_all(1, seed * 1_000_003 + k)
        eng.timing_begin()
        pad.fill_(k & 0xFF)
        ex.step(eng, spaces, k, stream)
        tm = eng.timing_end()
        ms.append(tm["fast_ms"] + tm["general_ms"])
        qs = int(np.count_nonzero(eng.sync_quiesce(n)["quiesced_since"]))
        if asleep and qs > asleep[-1] or (not asleep and qs):  # someone entered: count the notices in the space written
            out = decode_space(spaces[(k + 1) % 2].cpu().numpy(), ex.n_chunks, ex.positions, ex.depth)
            notices += int(np.count_nonzero(out["type"] == abi.QUIESCE))
        asleep.append(qs)
        k += 1

    limit = 10 * election + 20
    while (not asleep or asleep[-1] < n) and k < limit:
        one_pass(False)
    all_quiesced_at = k if asleep[-1] == n else None
    active_ms = ms[:max(1, k - 1)]
    for _ in range(quiet_passes):
        one_pass(False)
    quiet_ms = ms[-quiet_passes:]
    one_pass(True)  # first burst
    for _ in range(3):
        one_pass(False)
    awake_after_burst = n - asleep[-1]
    for _ in range(max(0, gap - 3)):
        one_pass(False)
    one_pass(True)  # second burst, inside the just-exited window
    notices_before = notices
    for _ in range(10 * election + 10):
        one_pass(False)
        if asleep[-1] == n:
            break
    st = eng.stats()
    out = {"workload": f"idle {G} x {R}, gr_tick_all(1) per pass, election {election}", "passes": k,
           "all_quiesced_by_pass": all_quiesced_at,
           "device_ms_per_pass_active": sum(active_ms) / len(active_ms),
           "device_ms_per_pass_quiesced": sum(quiet_ms) / len(quiet_ms),
           "quiesce_messages": notices, "quiesce_messages_after_bursts": notices - notices_before,
           "peers": n, "awake_3_passes_after_first_burst": awake_after_burst,
           "asleep_at_end": asleep[-1], "escalations": st["escalations"],
           "bytes_uploaded_per_tick": 0, "bytes_per_tick_with_local_records": n * abi.LOCAL.itemsize,
           "source_digest": build.source_digest(), "built": (build.build_record() or {}).get("source_digest")}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=100_000)
    ap.add_argument("--election", type=int, default=10, help="election timeout = the managers' electionTick")
    ap.add_argument("--quiet-passes", type=int, default=20, help="timed passes with every peer quiesced")
    ap.add_argument("--gap", type=int, default=6, help="passes between the two bursts")
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    print(json.dumps(run(args.groups, 3, args.election, args.seed, args.quiet_passes, args.gap)), flush=True)


if __name__ == "__main__":
    main()

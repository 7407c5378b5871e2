"""Election storm: a cold start of 100k groups x 3 on one GPU, device-resident
(gr_step_device over loopback mailbox spaces in HBM), one Tick per replica per
pass with the pass's random draw. Every group has lost its leader
(populations.cold_start), so every group times out, campaigns, votes and
promotes a leader.

Run with elections on the device and, beside it, off (the default engine, where
every campaign and vote escalates): the escalations of the second run are the
host round trips the first avoids. With elections off nothing replays the
escalated items (this tool has no host side), so no leader appears and the run
stops after --passes.

Reported per run: device ms per pass (the kernels' HIP-event time, gr_timing),
lanes per pass stepped by the general kernel, escalations by the engine's
counter, promotions drained (gr_promotions), and the first pass, checked every
--check passes, after which every group has exactly one leader.

Usage: python tools/bench_election.py [--groups N] [--passes N] > bench_out/election.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(G, R, passes, check, elections, seed):
    import numpy as np
    import torch
    from dragonboat_amd import abi, build, populations as P
    from dragonboat_amd.engine import Engine
    from dragonboat_amd.exchange import Exchange

    ex = Exchange(G, R, R, 1, 0, "local")
    eng = Engine(ex.n_peers, R, elections=elections)
    eng.load(P.cold_start(G, R, seed=seed))
    eng.bind_routes(ex.in_pos, ex.out_pos)
    spaces = ex.allocate(eng, torch.device("cuda", 0))
    stream = torch.cuda.current_stream()
    pad = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")  # hides the launch latency (bench_configs.py)
    ms = []
    general = promoted = 0
    led_at = None
    for k in range(passes):
        eng.set_locals(P.propose_locals(ex.n_peers, np.zeros(0, np.int64), seed=seed, pass_index=k, ticks=1))
        eng.timing_begin()
        pad.fill_(k & 0xFF)
        ex.step(eng, spaces, k, stream)
        tm = eng.timing_end()
        ms.append(tm["fast_ms"] + tm["general_ms"])
        general += tm["bailed_lanes"]
        if elections:
            promoted += len(eng.promotions())
            if (k + 1) % check == 0:
                st = eng.sync(ex.n_peers)
                if np.all((st["state"].reshape(R, G) == abi.LEADER).sum(axis=0) == 1):
                    led_at = k + 1
                    break
    n = len(ms)
    st = eng.stats()
    res = eng.collect_results(ex.n_peers)
    esc = res["escalation"][res["escalation"] != 0]
    out = {"workload": f"cold start {G} x {R}, one tick per pass", "elections": bool(elections), "passes": n,
           "device_ms_per_pass": sum(ms) / n, "device_ms_max_pass": max(ms),
           "general_lanes_per_pass": general / n, "escalations": st["escalations"],
           "last_pass_escalations": {abi.ESC_NAMES[int(e)]: int(c) for e, c in zip(*np.unique(esc, return_counts=True))},
           "promotions": promoted, "all_groups_led_by_pass": led_at,
           "source_digest": build.source_digest(), "built": (build.build_record() or {}).get("source_digest")}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=100_000)
    ap.add_argument("--passes", type=int, default=120)
    ap.add_argument("--check", type=int, default=5, help="look for a leader in every group every this many passes")
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    for on in (True, False):
        print(json.dumps(run(args.groups, 3, args.passes if on else min(args.passes, 40), args.check, on, args.seed)),
              flush=True)


if __name__ == "__main__":
    main()

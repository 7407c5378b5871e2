"""What the quiesce manager on the device costs and saves, device-resident on one
GPU (gr_step_device over loopback spaces, HIP-event time per pass, gr_timing):

  steady: the headline's shape (G x 3, a proposal on every leader each pass) with
          the switch off and on (every manager enabled and awake, kept awake by
          the traffic): the difference is the quiesce pass's own time.
  config3: config 3's shape (G x 5, 90% of the groups quiesced, 10% ticking) with
          today's host-chosen quiesced_ticks (gr_set_locals per tick: one 48-byte
          record per peer uploaded) beside gr_tick_all(1) per tick with the
          managers on the device (no upload).

Usage: python tools/bench_quiesce_ab.py [--steady-groups N] [--config3-groups N] > profiles/quiesce_ab.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(eng, ex, spaces, stream, pad, passes, warmup, before_pass):
    ms = []
    for k in range(warmup + passes):
        before_pass(k)
        eng.timing_begin()
        pad.fill_(k & 0xFF)
        ex.step(eng, spaces, k, stream)
        tm = eng.timing_end()
        if k >= warmup:
            ms.append(tm["fast_ms"] + tm["general_ms"])
    ms.sort()
    return {"device_ms_per_pass_median": ms[len(ms) // 2], "device_ms_per_pass_min": ms[0],
            "device_ms_per_pass_max": ms[-1], "passes": passes}


def setup(G, R, peers, quiesce, qrecs=None):
    import torch
    from dragonboat_amd.engine import Engine
    from dragonboat_amd.exchange import Exchange
    ex = Exchange(G, R, R, 1, 0, "local")
    eng = Engine(ex.n_peers, R, quiesce=quiesce)
    eng.load(peers)
    if qrecs is not None:
        eng.load_quiesce(qrecs)
    eng.bind_routes(ex.in_pos, ex.out_pos)
    return eng, ex, ex.allocate(eng, torch.device("cuda", 0)), torch.cuda.current_stream()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steady-groups", type=int, default=1_000_000)
    ap.add_argument("--config3-groups", type=int, default=100_000)
    ap.add_argument("--passes", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    args = ap.parse_args()
    import numpy as np
    import torch
    from dragonboat_amd import abi, build, populations as P
    torch.cuda.set_device(0)
    pad = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")  # hides the launch latency (bench_configs.py)
    out = {"source_digest": build.source_digest(), "built": (build.build_record() or {}).get("source_digest")}

    # ---- steady state, switch off / on
    G, R = args.steady_groups, 3
    peers = P.make_groups(G, R, seed=2)
    loc = P.propose_locals(R * G, np.arange(G))
    for on in (False, True, False, True):
        q = np.zeros(R * G, abi.QUIESCE_STATE)
        q["election_tick"], q["enabled"] = 10, 1
        eng, ex, spaces, stream = setup(G, R, peers, on, q)
        eng.set_locals(loc)
        r = timed(eng, ex, spaces, stream, pad, args.passes, args.warmup, lambda k: None)
        r["escalations"] = eng.stats()["escalations"]
        if on:
            r["awake"] = int(np.count_nonzero(eng.sync_quiesce(R * G)["quiesced_since"] == 0))
        out.setdefault(f"steady_{G}x{R}_quiesce_{'on' if on else 'off'}", []).append(r)
        eng.close()
        del spaces

    # ---- config 3's shape: host-chosen split per tick beside gr_tick_all
    G, R = args.config3_groups, 5
    peers, active = P.config3(G, R)
    n = R * G
    act = np.tile(active, R)

    def host_locals(k):
        loc = P.config3_locals(G, R, active, k)
        loc["read_index"], loc["read_ctx_low"], loc["read_ctx_high"] = 0, 0, 0  # gr_tick_all carries no ReadIndex
        return loc
    eng, ex, spaces, stream = setup(G, R, peers, False)
    r = timed(eng, ex, spaces, stream, pad, args.passes, args.warmup, lambda k: eng.set_locals(host_locals(k)))
    r.update(escalations=eng.stats()["escalations"], bytes_uploaded_per_tick=n * abi.LOCAL.itemsize)
    out[f"config3_{G}x{R}_host_quiesced_ticks"] = r
    eng.close()
    del spaces
    q = np.zeros(n, abi.QUIESCE_STATE)
    q["election_tick"], q["enabled"], q["tick"] = 10, 1, 1000
    q["quiesced_since"] = np.where(act, 0, 900)  # 90% asleep long ago, 10% awake
    q["no_activity_since"] = np.where(act, 1000, 900)
    eng, ex, spaces, stream = setup(G, R, peers, True, q)
    r = timed(eng, ex, spaces, stream, pad, args.passes, args.warmup, lambda k: eng.tick_all(1, 7919 * k))
    qs = eng.sync_quiesce(n)
    r.update(escalations=eng.stats()["escalations"], bytes_uploaded_per_tick=0,
             asleep=int(np.count_nonzero(qs["quiesced_since"])), peers=n)
    out[f"config3_{G}x{R}_gr_tick_all"] = r
    eng.close()
    print(json.dumps(out, indent=1), flush=True)


if __name__ == "__main__":
    main()

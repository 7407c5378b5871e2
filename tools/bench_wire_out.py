"""Frames straight out of the step, measured: the same inbox (decoded wire records
in HBM) and the same starting state go through

  compact   gr_step_wire_compact: every outbox message comes down as a compact
            record (the comparison: the path the host then builds pb.Messages from);
  wire_out  gr_step_wire_out + grw_encode_device + the download of the frames and
            of the batch table's 64 B per frame (frame_off / frame_len).

Repetitions alternate between the two paths in one process; before each one the
groups are reloaded (untimed), so every repetition steps the same pass. Wall clock
around the C calls; bytes down PCIe are counted from the records returned.

  (a) --workload steady  G x 3, every leader proposes: 4 of a group-round's 8
      messages are entry-free (the accepts), the leaders' commit broadcasts share
      their mailbox with the proposal and stay compact records;
  (b) --workload ticks   G x 5, BASELINE config 3's tick pass: all mail is entry-free.

What the wire_out path removes is the host's per-message work on the entry-free
mail (pb.Message build, queueing, MarshalTo), which this repository cannot time
without the Go host; what it adds is measured here.

  --stats-csv FILE   a rocprofv3 --kernel-trace --stats kernel_stats.csv of a
                     separate run (--profile-run: the wire_out path only, untimed);
                     the wire_out_* kernels' rows are added to the JSON line.

    python tools/bench_wire_out.py --workload steady --groups 1000000 --reps 5
"""
import argparse
import csv
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SOURCE = b"10.0.0.1:63001"


class DeviceBytes:
    """Engine-owned device memory as an object torch.as_tensor can view."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def kernel_rows(path):
    rows = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            name = r.get("Name") or r.get("KernelName") or ""
            if "wire_out_" in name or "out_counts_c" in name or "pack_outbox_c" in name:
                rows.append({"kernel": name.split("(")[0][-60:], "calls": int(r["Calls"]),
                             "avg_us": float(r["AverageNs"]) / 1e3, "total_ms": float(r["TotalDurationNs"]) / 1e6})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["steady", "ticks"], default="steady")
    ap.add_argument("--groups", type=int, default=None, help="default: 1M (steady), 100k (ticks)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-batch-msgs", type=int, default=1024)
    ap.add_argument("--targets", type=int, default=None, help="send queues (default: one per replica block)")
    ap.add_argument("--profile-run", action="store_true", help="the wire_out path only, for a profiler")
    ap.add_argument("--stats-csv", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from dragonboat_amd import abi, populations as P, wire as W
    from dragonboat_amd.engine import Engine, wire_out_cfg
    import wirefeed
    torch.cuda.set_device(0)
    if a.workload == "steady":
        G, R = a.groups or 1_000_000, 3
        peers = P.make_groups(G, R, seed=2)

        def locals_of(k):
            return P.propose_locals(R * G, np.arange(G), pass_index=k)
    else:
        G, R = a.groups or 100_000, 5
        peers, active = P.config3(G, R)

        def locals_of(k):
            return P.config3_locals(G, R, active, k)
    n = R * G
    topo = P.Topology(G, R)
    cl = (np.arange(n) % G) + 1
    eng = Engine(n, R)
    eng.load(peers)
    eng.bind_nodes(cl, peers["node_id"])
    T = a.targets or R
    eng.bind_targets((np.tile(np.arange(R, dtype=np.uint32), (n, 1)) % T).astype(np.uint32), T)
    # two passes with host records reach the pass to measure; its inbox becomes frames in HBM
    msgs = np.zeros(0, abi.MESSAGE)
    for k in range(2):
        out, _ = eng.step(msgs, locals_of(k))
        msgs = topo.route_messages(out)
    state = eng.sync(n)
    loc = np.ascontiguousarray(locals_of(2), abi.LOCAL)
    codec = W.WireCodec(0)
    batches, wm, we, payload = wirefeed.to_wire(msgs, peers["node_id"], peers["remote_id"], cl, per_frame=256)
    frames = codec.marshal(payload, batches, wm, we)
    table = W.frames_table(batches["frame_off"], batches["frame_len"])
    d_buf = torch.from_numpy(frames).cuda()
    d_bat = torch.from_numpy(table.view(np.uint8)).cuda()
    d_msgs = torch.empty(len(wm) * W.WMESSAGE.itemsize, dtype=torch.uint8, device="cuda")
    d_ents = torch.empty(max(1, len(we)) * W.WENTRY.itemsize, dtype=torch.uint8, device="cuda")
    nm, ne = codec.unmarshal_device(d_buf.data_ptr(), len(frames), d_bat.data_ptr(), len(table), d_msgs.data_ptr(),
                                    len(wm), d_ents.data_ptr(), max(1, len(we)))
    cfg = wire_out_cfg(dict(deployment_id=7, bin_ver=210, max_batch_msgs=a.max_batch_msgs, source_off=0,
                            source_len=len(SOURCE)))
    d_payload = torch.from_numpy(np.frombuffer(SOURCE, np.uint8).copy()).cuda()
    # one untimed probe pass sizes the frame buffers: an entry-free message encodes to < 128 B, a
    # batch header with this SourceAddress to < 64 B
    ob, un, wo = abi.COutbox(), abi.WireUnrouted(), abi.WireOut()
    rc = eng.lib.gr_step_wire_out(eng._h, d_msgs.data_ptr(), nm, d_ents.data_ptr(), ne, loc.ctypes.data, len(loc),
                                  ctypes.byref(ob), ctypes.byref(un), ctypes.byref(cfg), ctypes.byref(wo))
    assert rc == 0 and un.n == 0, (rc, un.n)
    eng.lib.gr_release_coutbox(eng._h, ctypes.byref(ob))
    out_cap = 128 * wo.n_msgs + 64 * wo.n_batches + 4096
    d_out = torch.empty(out_cap, dtype=torch.uint8, device="cuda")
    h_out = torch.empty(out_cap, dtype=torch.uint8).pin_memory()
    h_bat = torch.empty(64 * wo.n_batches + 64, dtype=torch.uint8).pin_memory()
    hip = torch.cuda.current_stream()

    def down_bytes(ob):
        return ob.n_msgs * 24 + ob.n_ext_msgs * 80 + ob.n_results * 24 + ob.n_ext_results * 168

    def run(path):
        eng.load(state)  # untimed: every repetition steps the same pass
        torch.cuda.synchronize()
        ob, un = abi.COutbox(), abi.WireUnrouted()
        r = {"path": path}
        t0 = time.perf_counter()
        if path == "compact":
            rc = eng.lib.gr_step_wire_compact(eng._h, d_msgs.data_ptr(), nm, d_ents.data_ptr(), ne, loc.ctypes.data,
                                              len(loc), ctypes.byref(ob), ctypes.byref(un))
            t1 = t2 = t3 = time.perf_counter()
            assert rc == 0 and un.n == 0, (rc, un.n)
            r.update(msgs_compact=ob.n_msgs, bytes_down=down_bytes(ob))
        else:
            wo = abi.WireOut()
            rc = eng.lib.gr_step_wire_out(eng._h, d_msgs.data_ptr(), nm, d_ents.data_ptr(), ne, loc.ctypes.data,
                                          len(loc), ctypes.byref(ob), ctypes.byref(un), ctypes.byref(cfg),
                                          ctypes.byref(wo))
            t1 = time.perf_counter()
            assert rc == 0 and un.n == 0, (rc, un.n)
            need = 0
            if wo.n_batches:
                need = codec.marshal_device(d_payload.data_ptr(), len(SOURCE), wo.d_batches, wo.n_batches, wo.d_msgs,
                                            wo.n_msgs, 0, 0, d_out.data_ptr(), out_cap)
            t2 = time.perf_counter()
            if wo.n_batches:
                h_out[:need].copy_(d_out[:need], non_blocking=True)
                nb = 64 * wo.n_batches
                h_bat[:nb].copy_(torch.as_tensor(DeviceBytes(wo.d_batches, nb), device="cuda"), non_blocking=True)
                hip.synchronize()
            t3 = time.perf_counter()
            r.update(msgs_compact=ob.n_msgs, msgs_wire=wo.n_msgs, frames=wo.n_batches, frame_bytes=need,
                     bytes_down=down_bytes(ob) + need + 68 * wo.n_batches)
        eng.lib.gr_release_coutbox(eng._h, ctypes.byref(ob))
        r.update(step_ms=(t1 - t0) * 1e3, encode_ms=(t2 - t1) * 1e3, frame_download_ms=(t3 - t2) * 1e3,
                 total_ms=(t3 - t0) * 1e3)
        return r

    if a.profile_run:
        for _ in range(a.reps):
            run("wire_out")
        codec.close()
        eng.close()
        return
    recs = {"compact": [], "wire_out": []}
    for k in range(a.warmup + a.reps):
        for path in (("compact", "wire_out") if k % 2 == 0 else ("wire_out", "compact")):  # alternated
            r = run(path)
            if k >= a.warmup:
                recs[path].append(r)
    line = {"tool": "bench_wire_out", "workload": a.workload, "groups": G, "replicas": R, "targets": T,
            "max_batch_msgs": a.max_batch_msgs, "reps": a.reps, "inbox_msgs": int(nm),
            "note": "wire_out removes the host's per-message pb.Message build and MarshalTo of the entry-free mail, "
                    "which is not timed here (no Go host in this repository)"}
    for path, rs in recs.items():
        tot = sorted(x["total_ms"] for x in rs)
        d = {k: rs[0][k] for k in rs[0] if k not in ("path", "step_ms", "encode_ms", "frame_download_ms", "total_ms")}
        for k in ("step_ms", "encode_ms", "frame_download_ms", "total_ms"):
            d[k + "_median"] = sorted(x[k] for x in rs)[len(rs) // 2]
        d["total_ms_min"], d["total_ms_max"] = tot[0], tot[-1]
        line[path] = d
    if a.stats_csv:
        line["kernels"] = kernel_rows(a.stats_csv)
    print(json.dumps(line), flush=True)
    codec.close()
    eng.close()


if __name__ == "__main__":
    main()

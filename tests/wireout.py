"""Test infrastructure for the outbound wire path (gr_step_wire_out): the rule
restated in plain Python, the way back from decoded frames to outbox records,
and a Lockstep backend whose entry-free mail leaves only as frames.

The backend steps with gr_step_wire_out, encodes the engine's grw_batch /
grw_message records with grw_encode_device into a device buffer, downloads the
frames, decodes them with the CPU oracle codec (oracle.pywire.decode) and merges
the decoded messages with the held compact records into outbox order, so the
Lockstep compares them with the oracle's outbox like any other backend's.
"""
import numpy as np

from dragonboat_amd import abi, wire as W
import simulate as SIM

SOURCE = np.frombuffer(b"10.0.0.1:63001", np.uint8).copy()  # SourceAddress, payload offset 0
CFG = dict(deployment_id=7, bin_ver=210, max_batch_msgs=64, source_off=0, source_len=len(SOURCE))
VALUE_FIELDS = ("term", "log_term", "log_index", "commit", "hint", "hint_high")


def replica_targets(n, slots):
    """One send queue per replica block: slot j of every peer sends to block j's host."""
    return np.tile(np.arange(slots, dtype=np.uint32), (n, 1))


class _DeviceBytes:
    """Engine-owned device memory as an object torch.as_tensor can view."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def download(torch, ptr, dtype, n):
    """n records of `dtype` at device pointer `ptr`, copied to the host."""
    if n == 0:
        return np.zeros(0, dtype)
    t = torch.as_tensor(_DeviceBytes(ptr, n * dtype.itemsize), device="cuda")
    return t.cpu().numpy().view(dtype).copy()


def outbox_order(msgs):
    """Records in outbox order: sender, remote slot, then as given (stable)."""
    msgs = np.asarray(msgs, abi.MESSAGE)
    return msgs[np.lexsort((np.arange(len(msgs)), msgs["slot"], msgs["peer"]))]


def rule(msgs, target_of):
    """held[k] by the rule of gpuraft.h, mailbox by mailbox, and for every held
    record the clause its mailbox breaks ("host", "entries" or "snapshot")."""
    msgs = np.asarray(msgs, abi.MESSAGE)
    held = np.zeros(len(msgs), bool)
    why = [None] * len(msgs)
    a = 0
    while a < len(msgs):
        b = a
        while b < len(msgs) and msgs["peer"][b] == msgs["peer"][a] and msgs["slot"][b] == msgs["slot"][a]:
            b += 1
        box = msgs[a:b]
        clause = None
        if target_of[int(box["peer"][0]), int(box["slot"][0])] == abi.TARGET_HOST:
            clause = "host"
        elif np.any(box["n_entries"] != 0):
            clause = "entries"
        elif np.any(box["type"] == abi.INSTALL_SNAPSHOT):
            clause = "snapshot"
        if clause:
            held[a:b] = True
            why[a:b] = [clause] * (b - a)
        a = b
    return held, why


class Directory:
    """(cluster, node id) -> engine slot and (engine slot, node id) -> remote slot."""

    def __init__(self, cluster_of, node_id, remote_id, slots):
        self.slot_of = {(int(c), int(n)): p for p, (c, n) in enumerate(zip(cluster_of, node_id))}
        self.remote_id = np.asarray(remote_id, np.uint64)[:, :slots]

    def records(self, wm):
        """Decoded wire messages -> outbox records (peer = sender, slot = target)."""
        out = np.zeros(len(wm), abi.MESSAGE)
        for k, m in enumerate(wm):
            p = self.slot_of[(int(m["cluster_id"]), int(m["from"]))]
            j = np.nonzero(self.remote_id[p] == m["to"])[0]
            assert len(j) >= 1, (p, int(m["to"]))
            out["peer"][k], out["slot"][k] = p, j[0]
        out["type"] = wm["type"]
        out["reject"] = wm["reject"]
        for f in VALUE_FIELDS:
            out[f] = wm[f]
        assert np.all(wm["n_entries"] == 0) and np.all(wm["snapshot_host"] == 0)
        return out


def check_batches(bat, bt, n_msgs, cfg, n_targets):
    """The batch table's invariants: contiguous first_msg, ascending targets,
    every batch of a target but its last full, cfg's fields, zero elsewhere."""
    mbm = int(cfg["max_batch_msgs"])
    assert len(bat) == len(bt)
    at = 0
    for b in range(len(bat)):
        assert bat["first_msg"][b] == at and 1 <= bat["n_msgs"][b] <= mbm
        at += int(bat["n_msgs"][b])
        if b + 1 < len(bat):
            assert bt[b] <= bt[b + 1]
            if bt[b] == bt[b + 1]:
                assert bat["n_msgs"][b] == mbm
    assert at == n_msgs and (len(bt) == 0 or bt.max() < n_targets)
    for f in ("deployment_id", "bin_ver", "source_off", "source_len"):
        assert np.all(bat[f] == cfg[f])
    for f in ("frame_off", "frame_len", "status", "err_msg", "err_field", "err_level"):
        assert np.all(bat[f] == 0), f
    assert np.all(bat["pad"] == 0)


def merge(held_msgs, wire_msgs):
    """Held records and records rebuilt from frames, in outbox order: a mailbox is
    wholly one or the other, so a stable sort by (sender, slot) restores it."""
    return outbox_order(np.concatenate([np.asarray(held_msgs, abi.MESSAGE), np.asarray(wire_msgs, abi.MESSAGE)]))


class GpuWireOutBackend(SIM.GpuWireBackend):
    """Frames in (GpuWireBackend), and frames as the only way out for entry-free
    mail (gr_step_wire_out + grw_encode_device + the CPU oracle's decode)."""
    result_fields = SIM.GpuCompactBackend.result_fields
    expand = SIM.GpuCompactBackend.expand
    targets = None  # [n, slots] send queues; default: one per replica block
    n_targets = None
    cfg = CFG

    def __init__(self, peers, slots, max_entry_size=abi.MAX_ENTRY_SIZE):
        super().__init__(peers, slots, max_entry_size=max_entry_size)
        import torch
        self.torch = torch
        n = len(peers)
        t = self.targets
        if t is None:
            t = replica_targets(n, slots)
        self.eng.bind_targets(t, self.n_targets or slots)
        self.dir = Directory(self.feed.cluster_of, peers["node_id"], peers["remote_id"], slots)
        self.d_payload = torch.from_numpy(SOURCE).cuda()
        self.wire_msgs = self.held_msgs = 0
        self.types = set()

    def load(self, idx, recs):
        super().load(idx, recs)
        recs = np.asarray(recs, abi.PEER)
        self.dir.remote_id[np.asarray(idx, np.int64)] = recs["remote_id"][:, :self.dir.remote_id.shape[1]]

    def frames_to_records(self, wo):
        """Encode on the device, download the frames, decode them on the CPU."""
        from oracle import pywire
        if wo.n_batches == 0:
            assert wo.n_msgs == 0
            return np.zeros(0, abi.MESSAGE)
        torch = self.torch
        cap = 64 * wo.n_batches + 160 * wo.n_msgs  # header + SourceAddress per batch; an entry-free message is < 160 B
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        need = self.feed.codec.marshal_device(self.d_payload.data_ptr(), len(SOURCE), wo.d_batches, wo.n_batches,
                                              wo.d_msgs, wo.n_msgs, 0, 0, d_out.data_ptr(), cap)
        frames = d_out[:need].cpu().numpy()
        bat = download(torch, wo.d_batches, W.BATCH, wo.n_batches)  # frame_off / frame_len, filled by the encoder
        assert np.all(bat["status"] == 0) and int(bat["frame_len"].astype(np.int64).sum()) == need
        table = W.frames_table(bat["frame_off"], bat["frame_len"])
        table, wm, we = pywire.decode(frames, table)
        assert np.all(table["status"] == W.OK) and len(we) == 0 and len(wm) == wo.n_msgs
        assert np.all(table["deployment_id"] == self.cfg["deployment_id"]) and \
            np.all(table["bin_ver"] == self.cfg["bin_ver"])
        assert np.array_equal(table["n_msgs"], bat["n_msgs"])
        self.types.update(int(t) for t in np.unique(wm["type"]))
        return self.dir.records(wm)

    def step(self, msgs, loc):
        dm, nm, de, ne, keep = self.feed.decode(msgs)
        (om, ox, cr, rx), idx, why, wo = self.eng.step_wire(dm, nm, de, ne, loc, wire_out=self.cfg)
        assert len(idx) == 0, [abi.WIRE_REASONS[w] for w in why[:4]]
        wire = self.frames_to_records(wo)
        held, res = self.expand(om, ox, cr, rx, loc)
        self.wire_msgs += len(wire)
        self.held_msgs += len(held)
        return merge(held, wire), res

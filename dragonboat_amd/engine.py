"""Python binding of libgpuraft.so (the product C-ABI, include/gpuraft.h).

This is the host-side mirror a Go ``internal/gpuraft`` package would be
(INTEGRATION.md): load groups, step them with messages and local inputs, read
back messages, results and state. The library is loaded from the in-tree
build (``dragonboat_amd/_build``); there is no fallback: if the HIP library
is missing or no GPU is usable, construction raises.
"""
import ctypes
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GPURAFT_LIB") or os.path.join(_HERE, "_build", "libgpuraft.so")  # env: A/B builds
_lib = None
_libs = {}  # other builds by path (e.g. the coverage build), loaded beside the default
MAILBOX_DEPTH = abi.GR_C  # full-depth spaces; exchange.py uses 2 for spaces that cross GPUs


class GpuRaftError(RuntimeError):
    pass


def load_library(path=LIB_PATH):
    """Load the HIP engine library (import torch first so one HIP runtime is shared)."""
    global _lib
    if path == LIB_PATH and _lib is not None:
        return _lib
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise GpuRaftError(f"libgpuraft.so not built at {path}; run __graft_entry__.build()")
    lib = ctypes.CDLL(path)
    c = ctypes
    lib.gr_create.argtypes = [c.POINTER(abi.Config), c.POINTER(c.c_void_p)]
    lib.gr_destroy.argtypes = [c.c_void_p]
    lib.gr_destroy.restype = None
    lib.gr_strerror.restype = c.c_char_p
    lib.gr_strerror.argtypes = [c.c_int]
    lib.gr_escalation_name.restype = c.c_char_p
    lib.gr_escalation_name.argtypes = [c.c_int]
    lib.gr_load_groups.argtypes = [c.c_void_p, c.c_uint32, c.c_void_p, c.c_size_t]
    lib.gr_sync_groups_to_host.argtypes = [c.c_void_p, c.c_uint32, c.c_void_p, c.c_size_t]
    lib.gr_load_peers.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t]
    lib.gr_sync_peers_to_host.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t]
    lib.gr_notify_applied.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t]
    lib.gr_compact_log.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    lib.gr_step_compact.argtypes = [c.c_void_p, c.POINTER(abi.CInbox), c.POINTER(abi.COutbox)]
    lib.gr_step_compact_begin.argtypes = [c.c_void_p, c.POINTER(abi.CInbox)]
    lib.gr_step_compact_end.argtypes = [c.c_void_p, c.POINTER(abi.COutbox)]
    lib.gr_cinbox_reserve.argtypes = [c.c_void_p, c.c_size_t, c.c_size_t, c.c_size_t, c.c_size_t,
                                      c.POINTER(abi.CInbox)]
    lib.gr_release_coutbox.argtypes = [c.c_void_p, c.POINTER(abi.COutbox)]
    lib.gr_pack_messages.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.POINTER(c.c_size_t)]
    lib.gr_unpack_messages.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p]
    lib.gr_cmsg_count.argtypes = [c.c_void_p, c.c_size_t]
    lib.gr_cmsg_count.restype = c.c_size_t
    lib.gr_pair_messages.argtypes = [c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t)]
    lib.gr_pack_locals.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.POINTER(c.c_size_t)]
    lib.gr_commit_update.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    lib.gr_apply_config_change.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    lib.gr_step.argtypes = [c.c_void_p, c.POINTER(abi.Inbox), c.POINTER(abi.Outbox)]
    lib.gr_release_outbox.argtypes = [c.c_void_p, c.POINTER(abi.Outbox)]
    lib.gr_inbox_reserve.argtypes = [c.c_void_p, c.c_size_t, c.c_size_t, c.POINTER(abi.Inbox)]
    lib.gr_stats_get.argtypes = [c.c_void_p, c.POINTER(abi.Stats)]
    lib.gr_stats_reset.argtypes = [c.c_void_p]
    lib.gr_space_bytes.restype = c.c_uint64
    lib.gr_space_bytes.argtypes = [c.c_uint32, c.c_uint32, c.c_uint32]
    lib.gr_space_chunk_bytes.restype = c.c_uint64
    lib.gr_space_chunk_bytes.argtypes = [c.c_uint32, c.c_uint32]
    lib.gr_space_hot_chunk_bytes.restype = c.c_uint64
    lib.gr_space_hot_chunk_bytes.argtypes = [c.c_uint32, c.c_uint32]
    lib.gr_space_hot_tile_bytes.restype = c.c_uint64
    lib.gr_space_hot_tile_bytes.argtypes = [c.c_uint32]
    lib.gr_space_tile_positions.restype = c.c_uint32
    lib.gr_space_tile_positions.argtypes = []
    lib.gr_space_cold_used.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_uint32, c.c_void_p,
                                       c.POINTER(c.c_uint32)]
    lib.gr_space_side_bytes.restype = c.c_uint64
    lib.gr_space_side_bytes.argtypes = [c.c_uint32, c.c_uint32, c.c_uint32]
    for f in ("gr_space_side_pack", "gr_space_side_unpack"):
        getattr(lib, f).argtypes = [c.c_void_p, c.c_uint32, c.c_uint32, c.c_uint32, c.c_void_p, c.c_uint32,
                                    c.c_void_p]
    for f in ("gr_space_side_pack_host", "gr_space_side_unpack_host"):
        getattr(lib, f).argtypes = [c.c_void_p, c.c_uint32, c.c_uint32, c.c_uint32, c.c_void_p, c.c_uint32]
    lib.gr_space_cx_bytes.restype = c.c_uint64
    lib.gr_space_cx_bytes.argtypes = [c.c_uint32, c.c_uint32, c.c_uint32, c.c_void_p, c.c_uint32]
    for f in ("gr_space_cx_pack", "gr_space_cx_unpack"):
        getattr(lib, f).argtypes = [c.c_void_p, c.c_uint32, c.c_uint32, c.c_uint32, c.c_void_p, c.c_void_p,
                                    c.c_uint32, c.c_void_p]
    for f in ("gr_space_cx_pack_host", "gr_space_cx_unpack_host"):
        getattr(lib, f).argtypes = [c.c_void_p, c.c_uint32, c.c_uint32, c.c_uint32, c.c_void_p, c.c_void_p,
                                    c.c_uint32]
    lib.gr_bind_routes.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint32]
    lib.gr_bind_nodes.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint32]
    lib.gr_step_wire.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p,
                                 c.c_size_t, c.POINTER(abi.Outbox), c.POINTER(abi.WireUnrouted)]
    lib.gr_step_wire_compact.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p,
                                         c.c_size_t, c.POINTER(abi.COutbox), c.POINTER(abi.WireUnrouted)]
    lib.gr_set_locals.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t]
    lib.gr_step_device.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32,
                                   c.c_uint32, c.c_uint32, c.c_uint32, c.c_uint32, c.c_void_p]
    lib.gr_collect_results.argtypes = [c.c_void_p, c.c_uint32, c.c_void_p, c.c_size_t]
    if hasattr(lib, "gr_graph_capture"):  # (older builds loaded for A/B runs lack graph mode)
        lib.gr_graph_capture.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_uint32,
                                         c.c_uint32, c.c_uint32, c.POINTER(c.c_void_p)]
        lib.gr_graph_replay.argtypes = [c.c_void_p, c.c_void_p]
        lib.gr_graph_destroy.argtypes = [c.c_void_p]
        lib.gr_graph_destroy.restype = None
    lib.gr_space_decode.argtypes = [c.c_void_p, c.c_uint32, c.c_uint32, c.c_uint32, c.c_void_p, c.c_size_t,
                                    c.POINTER(c.c_size_t)]
    lib.gr_space_encode.argtypes = [c.c_void_p, c.c_uint32, c.c_uint32, c.c_uint32, c.c_void_p, c.c_size_t,
                                    c.c_void_p]
    lib.gr_timing_begin.argtypes = [c.c_void_p]
    lib.gr_timing_end.argtypes = [c.c_void_p, c.POINTER(abi.Timing)]
    if hasattr(lib, "gr_coverage_read"):  # coverage build only (GR_COVERAGE)
        lib.gr_coverage_read.argtypes = [c.c_void_p, c.c_uint32]
        lib.gr_coverage_names.restype = c.c_char_p
        lib.gr_coverage_elect_read.argtypes = [c.c_void_p, c.c_uint32]
        lib.gr_coverage_elect_names.restype = c.c_char_p
    if hasattr(lib, "gr_coverage_quiesce_read"):
        lib.gr_coverage_quiesce_read.argtypes = [c.c_void_p, c.c_uint32]
        lib.gr_coverage_quiesce_names.restype = c.c_char_p
    if hasattr(lib, "gr_set_elections"):  # (older builds loaded for A/B runs lack elections)
        lib.gr_set_elections.argtypes = [c.c_void_p, c.c_int]
        lib.gr_get_elections.argtypes = [c.c_void_p]
        lib.gr_promotions.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t)]
    if hasattr(lib, "gr_coverage_snap_read"):
        lib.gr_coverage_snap_read.argtypes = [c.c_void_p, c.c_uint32]
        lib.gr_coverage_snap_names.restype = c.c_char_p
    if hasattr(lib, "gr_set_snapshots"):  # (older builds loaded for A/B runs lack snapshots)
        lib.gr_set_snapshots.argtypes = [c.c_void_p, c.c_int]
        lib.gr_get_snapshots.argtypes = [c.c_void_p]
        lib.gr_set_snapshot_recs.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t]
        lib.gr_get_snapshot_recs.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t]
        lib.gr_restored_snapshots.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t)]
        lib.gr_restore_remotes.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    if hasattr(lib, "gr_coverage_cc_read"):
        lib.gr_coverage_cc_read.argtypes = [c.c_void_p, c.c_uint32]
        lib.gr_coverage_cc_names.restype = c.c_char_p
    if hasattr(lib, "gr_set_config_entries"):  # (older builds loaded for A/B runs lack config entries)
        lib.gr_set_config_entries.argtypes = [c.c_void_p, c.c_int]
        lib.gr_get_config_entries.argtypes = [c.c_void_p]
        lib.gr_set_cc_indexes.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t]
        lib.gr_get_cc_indexes.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t]
    if hasattr(lib, "gr_set_quiesce"):  # (older builds loaded for A/B runs lack the quiesce manager)
        lib.gr_set_quiesce.argtypes = [c.c_void_p, c.c_int]
        lib.gr_get_quiesce.argtypes = [c.c_void_p]
        lib.gr_load_quiesce.argtypes = [c.c_void_p, c.c_uint32, c.c_void_p, c.c_size_t]
        lib.gr_sync_quiesce.argtypes = [c.c_void_p, c.c_uint32, c.c_void_p, c.c_size_t]
        lib.gr_load_quiesce_peers.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t]
        lib.gr_sync_quiesce_peers.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t]
        lib.gr_tick_all.argtypes = [c.c_void_p, c.c_uint32, c.c_uint64]
        lib.gr_splitmix64.argtypes = [c.c_uint64]
        lib.gr_splitmix64.restype = c.c_uint64
    if hasattr(lib, "gr_steady_wave_uniform"):  # (older builds loaded for A/B runs lack it)
        lib.gr_steady_wave_uniform.argtypes = [c.c_void_p]
    if hasattr(lib, "gr_bind_targets"):  # (older builds loaded for A/B runs lack the outbound wire path)
        lib.gr_bind_targets.argtypes = [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32]
        lib.gr_step_wire_out.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p, c.c_size_t, c.c_void_p,
                                         c.c_size_t, c.POINTER(abi.COutbox), c.POINTER(abi.WireUnrouted),
                                         c.POINTER(abi.WireOutCfg), c.POINTER(abi.WireOut)]
        lib.gr_step_compact_wire_out.argtypes = [c.c_void_p, c.POINTER(abi.CInbox), c.POINTER(abi.COutbox),
                                                 c.POINTER(abi.WireOutCfg), c.POINTER(abi.WireOut)]
        lib.gr_wire_out_host.argtypes = [c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint32,
                                         c.c_uint32, c.c_void_p, c.c_uint32, c.POINTER(abi.WireOutCfg), c.c_void_p,
                                         c.POINTER(c.c_size_t), c.c_void_p, c.POINTER(c.c_size_t), c.c_void_p,
                                         c.c_void_p]
    if hasattr(lib, "gr_collect_updates"):  # (older builds loaded for A/B runs lack the updates path)
        lib.gr_set_update_states.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t]
        lib.gr_get_update_states.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t]
        lib.gr_collect_updates.argtypes = [c.c_void_p, c.c_uint32, c.c_uint32, c.c_uint32, c.POINTER(abi.Updates)]
        lib.gr_update_class.argtypes = [c.c_void_p, c.c_uint64, c.c_uint64, c.c_void_p, c.c_uint32]
        lib.gr_updates_last.argtypes = [c.c_void_p, c.POINTER(abi.UpdatesInfo)]
    if path == LIB_PATH:
        _lib = lib
    _libs[path] = lib
    return lib


def _check(rc, what):
    if rc != 0:
        err = GpuRaftError(f"{what}: {load_library().gr_strerror(rc).decode()} ({rc})")
        err.rc = rc
        raise err


def wire_out_cfg(cfg):
    """An abi.WireOutCfg from one, or from a mapping of its fields (gpuraft.h gr_wire_out_cfg)."""
    if isinstance(cfg, abi.WireOutCfg):
        return cfg
    return abi.WireOutCfg(**{k: int(v) for k, v in dict(cfg).items()})


class WireOut:
    """What gr_step_wire_out left for grw_encode_device: device pointers of the
    grw_batch / grw_message records (engine-owned, valid until the engine's next
    stepping call) and a host copy of batch_target."""

    def __init__(self, wo):
        self.d_batches, self.n_batches = wo.d_batches or 0, wo.n_batches
        self.d_msgs, self.n_msgs = wo.d_msgs or 0, wo.n_msgs
        self.batch_target = np.zeros(wo.n_batches, np.uint32)
        if wo.n_batches:
            ctypes.memmove(self.batch_target.ctypes.data, wo.batch_target, wo.n_batches * 4)


def wire_out_host(msgs, cluster_ids, node_ids, remote_ids, target_of, n_targets, cfg, slots=None, lib=None):
    """gr_wire_out_host: the outbound wire rule on the CPU (no engine, no GPU).
    msgs: full outbox records in outbox order; cluster_ids / node_ids [n_peers],
    remote_ids / target_of [n_peers, slots]. Returns (batches, wire messages,
    batch_target, held flags); raises GpuRaftError on a refusal."""
    from . import wire as W
    lib = lib or load_library()
    msgs = np.ascontiguousarray(msgs, abi.MESSAGE)
    cl = np.ascontiguousarray(cluster_ids, np.uint64)
    nd = np.ascontiguousarray(node_ids, np.uint64)
    target_of = np.asarray(target_of, np.uint32)
    slots = target_of.shape[1] if slots is None else slots
    rid = np.ascontiguousarray(np.asarray(remote_ids, np.uint64)[:, :slots])
    tg = np.ascontiguousarray(target_of)
    n = len(msgs)
    bat = np.zeros(n, W.BATCH)
    wm = np.zeros(n, W.WMESSAGE)
    bt = np.zeros(n, np.uint32)
    held = np.zeros(n, np.uint8)
    nb, nw = ctypes.c_size_t(), ctypes.c_size_t()
    c = wire_out_cfg(cfg)

    def ptr(a):
        return a.ctypes.data if a.size else None
    _check(lib.gr_wire_out_host(ptr(msgs), n, ptr(cl), ptr(nd), ptr(rid), len(cl), slots, ptr(tg), n_targets,
                                ctypes.byref(c), ptr(bat), ctypes.byref(nb), ptr(wm), ctypes.byref(nw), ptr(bt),
                                ptr(held)), "gr_wire_out_host")
    return bat[:nb.value].copy(), wm[:nw.value].copy(), bt[:nb.value].copy(), held.astype(bool)


def update_class(results, log_applied, first_index_m1, prev, more_to_apply=True, every=False, lib=None):
    """gr_update_class (the host form of the rule gr_collect_updates runs on the
    device; no engine, no GPU) for arrays of abi.RESULT records, their peers'
    log_applied and first_index_m1, and their abi.UPDATE_STATE records. Returns
    abi.UPD_NONE / UPD_COMPACT / UPD_EXT per record."""
    lib = lib or load_library()
    res = np.ascontiguousarray(np.atleast_1d(results), abi.RESULT)
    prev = np.ascontiguousarray(np.atleast_1d(prev), abi.UPDATE_STATE)
    la = np.broadcast_to(np.asarray(log_applied, np.uint64), res.shape)
    lo = np.broadcast_to(np.asarray(first_index_m1, np.uint64), res.shape)
    assert len(prev) == len(res)
    flags = (abi.UPD_MORE_TO_APPLY if more_to_apply else 0) | (abi.UPD_EVERY if every else 0)
    out = np.zeros(len(res), np.int32)
    rs, ps = abi.RESULT.itemsize, abi.UPDATE_STATE.itemsize
    for k in range(len(res)):
        out[k] = lib.gr_update_class(res.ctypes.data + k * rs, int(la[k]), int(lo[k]), prev.ctypes.data + k * ps,
                                     flags)
    if np.any(out < 0):
        _check(int(out.min()), "gr_update_class")
    return out


def expand_updates(cresults, ext, term, vote, propose_entries=None):
    """What gr_collect_updates returned as abi.RESULT records, by gpuraft.h's
    gr_cresult rules. term / vote: per engine slot, the host's update states
    before the collect (a compact record says they did not change; a changed
    term or vote arrives as an ext record). propose_entries: per engine slot,
    the bound ProposeEntries counts, which propose_first of a GR_PROP_APPENDED
    record follows from (omitted: propose_first stays 0). A compact record has no
    ReadyToRead and no forwarded batches, and does not carry append_from."""
    cr = np.asarray(cresults, abi.CRESULT)
    res = np.zeros(len(cr), abi.RESULT)
    for f in ("peer", "escalation", "propose_result", "last_index"):
        res[f] = cr[f]
    res["esc_item"] = cr["aux"]
    res["committed"] = cr["last_index"] - cr["commit_lag"]
    sc = cr["save_count"].astype(np.uint64)
    res["save_from"] = np.where(sc > 0, cr["last_index"] - sc + np.uint64(1), 0)
    p = cr["peer"].astype(np.int64)
    res["term"], res["vote"] = np.asarray(term, np.uint64)[p], np.asarray(vote, np.uint64)[p]
    if propose_entries is not None:
        app = cr["propose_result"] == abi.PROP_APPENDED
        res["propose_first"] = np.where(app, cr["last_index"] - np.asarray(propose_entries, np.uint64)[p] +
                                        np.uint64(1), 0)
    x = (cr["flags"] & abi.CR_EXT) != 0
    if x.any():
        res[x] = np.asarray(ext, abi.RESULT)[cr["aux"][x].astype(np.int64)]
    return res


class Engine:
    """One engine = one device's slab of group slots (engine slots 0..max_peers-1)."""

    def __init__(self, max_peers, slots=3, device=0, max_entry_size=abi.MAX_ENTRY_SIZE, lib_path=None,
                 elections=False, quiesce=False, snapshots=False, config_entries=False):
        """config_entries: config-change proposals, their Replicate marks and promotions
        over uncommitted entries on the device (gr_set_config_entries); False leaves
        the default, which GR_CONFIG_ENTRIES=1 turns on.
        snapshots: send and restore snapshots on the device (gr_set_snapshots);
        False leaves the default, which GR_SNAPSHOTS=1 turns on.
        elections: run elections on the device (gr_set_elections); False leaves
        the engine's default, which GR_ELECTIONS=1 in the environment turns on.
        quiesce: run the quiesce manager on the device (gr_set_quiesce); False
        leaves the default, which GR_QUIESCE_ON_DEVICE=1 turns on."""
        lib = load_library(lib_path or LIB_PATH)
        cfg = abi.Config(max_peers=max_peers, slots=slots, window_runs=abi.GR_K,
                         read_index_depth=abi.GR_Q, mailbox_depth=abi.GR_C, device=device,
                         max_entry_size=max_entry_size)
        h = ctypes.c_void_p()
        _check(lib.gr_create(ctypes.byref(cfg), ctypes.byref(h)), "gr_create")
        self._h = h
        self.max_peers = max_peers
        self.slots = slots
        self.lib = lib
        if elections:
            self.set_elections(True)
        if quiesce:
            self.set_quiesce(True)
        if snapshots:
            self.set_snapshots(True)
        if config_entries:
            self.set_config_entries(True)

    def set_config_entries(self, on):
        """Config-change entries on the device (gpuraft.h gr_set_config_entries)."""
        _check(self.lib.gr_set_config_entries(self._h, 1 if on else 0), "gr_set_config_entries")

    def get_config_entries(self):
        return bool(self.lib.gr_get_config_entries(self._h))

    def set_cc_indexes(self, slots, recs):
        """The groups' config-change index records (abi.CC_INDEX: the two highest
        ConfigChangeEntry indexes above committed) for a list of engine slots
        (gr_set_cc_indexes): call it with every load of a group while the switch is on."""
        slots = np.ascontiguousarray(slots, np.uint32)
        recs = np.ascontiguousarray(recs, abi.CC_INDEX)
        assert len(slots) == len(recs)
        _check(self.lib.gr_set_cc_indexes(self._h, slots.ctypes.data if len(slots) else None,
                                          recs.ctypes.data if len(recs) else None, len(slots)),
               "gr_set_cc_indexes")

    def get_cc_indexes(self, slots):
        slots = np.ascontiguousarray(slots, np.uint32)
        out = np.zeros(len(slots), abi.CC_INDEX)
        _check(self.lib.gr_get_cc_indexes(self._h, slots.ctypes.data if len(slots) else None,
                                          out.ctypes.data if len(out) else None, len(slots)),
               "gr_get_cc_indexes")
        return out

    def set_snapshots(self, on):
        """InstallSnapshot sends and restores on the device (gpuraft.h gr_set_snapshots)."""
        _check(self.lib.gr_set_snapshots(self._h, 1 if on else 0), "gr_set_snapshots")

    def get_snapshots(self):
        return bool(self.lib.gr_get_snapshots(self._h))

    def set_snapshot_recs(self, slots, recs):
        """The groups' latest snapshots (abi.SNAPSHOT_REC) for a list of engine
        slots (gr_set_snapshot_recs): call it after LogReader.CreateSnapshot."""
        slots = np.ascontiguousarray(slots, np.uint32)
        recs = np.ascontiguousarray(recs, abi.SNAPSHOT_REC)
        assert len(slots) == len(recs)
        _check(self.lib.gr_set_snapshot_recs(self._h, slots.ctypes.data if len(slots) else None,
                                             recs.ctypes.data if len(recs) else None, len(slots)),
               "gr_set_snapshot_recs")

    def get_snapshot_recs(self, slots):
        slots = np.ascontiguousarray(slots, np.uint32)
        out = np.zeros(len(slots), abi.SNAPSHOT_REC)
        _check(self.lib.gr_get_snapshot_recs(self._h, slots.ctypes.data if len(slots) else None,
                                             out.ctypes.data if len(out) else None, len(slots)),
               "gr_get_snapshot_recs")
        return out

    def restored_snapshots(self):
        """Drain the restored list: abi.RESTORED records (peer, index, term) of
        every snapshot restored on the device since the last call."""
        out = np.zeros(2 * self.max_peers, abi.RESTORED)  # a peer restores at most twice per pass
        n = ctypes.c_size_t()
        _check(self.lib.gr_restored_snapshots(self._h, out.ctypes.data, len(out), ctypes.byref(n)),
               "gr_restored_snapshots")
        return out[:n.value].copy()

    def restore_remotes(self, slots, ms):
        """Peer.RestoreRemotes on the device (gr_restore_remotes): ms is an
        abi.MEMBERSHIP array, one record per listed engine slot. Returns (rc,
        per-slot status) as apply_config_change does, and raises as it does."""
        slots = np.ascontiguousarray(slots, np.uint32)
        ms = np.ascontiguousarray(ms, abi.MEMBERSHIP)
        assert len(slots) == len(ms)
        st = np.full(len(slots), -1, np.int32)  # no gr_cc_status: still there after a refused call
        rc = self.lib.gr_restore_remotes(self._h, slots.ctypes.data if len(slots) else None,
                                         ms.ctypes.data if len(ms) else None, len(slots),
                                         st.ctypes.data if len(st) else None)
        if rc not in (0, -6) or (rc == -6 and st[0] < 0):
            _check(rc, "gr_restore_remotes")
        return rc, st

    def set_elections(self, on):
        """Campaigns, votes and promotions on the device (gpuraft.h gr_set_elections)."""
        _check(self.lib.gr_set_elections(self._h, 1 if on else 0), "gr_set_elections")

    def get_elections(self):
        return bool(self.lib.gr_get_elections(self._h))

    def set_quiesce(self, on):
        """The quiesce manager on the device (gpuraft.h gr_set_quiesce): local
        inputs then carry LocalTick counts and the device splits them. Drops
        bound local inputs."""
        _check(self.lib.gr_set_quiesce(self._h, 1 if on else 0), "gr_set_quiesce")

    def get_quiesce(self):
        return bool(self.lib.gr_get_quiesce(self._h))

    def load_quiesce(self, recs, first=0, slots=None):
        """abi.QUIESCE_STATE records into slots [first, first+n), or into a slot
        list (gr_load_quiesce / gr_load_quiesce_peers)."""
        recs = np.ascontiguousarray(recs, abi.QUIESCE_STATE)
        ptr = recs.ctypes.data if len(recs) else None
        if slots is None:
            _check(self.lib.gr_load_quiesce(self._h, first, ptr, len(recs)), "gr_load_quiesce")
            return
        slots = np.ascontiguousarray(slots, np.uint32)
        assert len(slots) == len(recs)
        _check(self.lib.gr_load_quiesce_peers(self._h, slots.ctypes.data if len(slots) else None, ptr, len(recs)),
               "gr_load_quiesce_peers")

    def sync_quiesce(self, n=None, first=0, slots=None):
        """The managers' records (gr_sync_quiesce / gr_sync_quiesce_peers)."""
        if slots is None:
            n = self.max_peers - first if n is None else n
            out = np.zeros(n, abi.QUIESCE_STATE)
            _check(self.lib.gr_sync_quiesce(self._h, first, out.ctypes.data if n else None, n), "gr_sync_quiesce")
            return out
        slots = np.ascontiguousarray(slots, np.uint32)
        out = np.zeros(len(slots), abi.QUIESCE_STATE)
        _check(self.lib.gr_sync_quiesce_peers(self._h, slots.ctypes.data if len(slots) else None,
                                              out.ctypes.data if len(out) else None, len(slots)),
               "gr_sync_quiesce_peers")
        return out

    def tick_all(self, ticks=1, rand_seed=0):
        """gr_tick_all: bind `ticks` LocalTicks for every loaded slot of the
        device-resident path, built on the device; slot p's draw is
        abi.splitmix64(rand_seed + p)."""
        _check(self.lib.gr_tick_all(self._h, ticks, rand_seed & ((1 << 64) - 1)), "gr_tick_all")

    def promotions(self):
        """Drain the promotion list: abi.PROMOTION records (peer, term, noop_index)
        of every peer that became leader on the device since the last call."""
        out = np.zeros(self.max_peers, abi.PROMOTION)
        n = ctypes.c_size_t()
        _check(self.lib.gr_promotions(self._h, out.ctypes.data, len(out), ctypes.byref(n)), "gr_promotions")
        return out[:n.value].copy()

    def close(self):
        if self._h:
            self.lib.gr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load(self, peers, first=0):
        peers = np.ascontiguousarray(peers, dtype=abi.PEER)
        _check(self.lib.gr_load_groups(self._h, first, peers.ctypes.data, len(peers)), "gr_load_groups")

    def sync(self, n=None, first=0):
        n = self.max_peers - first if n is None else n
        out = np.zeros(n, dtype=abi.PEER)
        _check(self.lib.gr_sync_groups_to_host(self._h, first, out.ctypes.data, n), "gr_sync")
        return out

    def load_peers(self, slots, peers):
        """Load records into a list of engine slots (gr_load_peers)."""
        slots = np.ascontiguousarray(slots, np.uint32)
        peers = np.ascontiguousarray(peers, dtype=abi.PEER)
        assert len(slots) == len(peers)
        _check(self.lib.gr_load_peers(self._h, slots.ctypes.data if len(slots) else None,
                                      peers.ctypes.data if len(peers) else None, len(peers)), "gr_load_peers")

    def sync_peers(self, slots):
        """Records of a list of engine slots (gr_sync_peers_to_host)."""
        slots = np.ascontiguousarray(slots, np.uint32)
        out = np.zeros(len(slots), dtype=abi.PEER)
        _check(self.lib.gr_sync_peers_to_host(self._h, slots.ctypes.data if len(slots) else None,
                                              out.ctypes.data if len(out) else None, len(slots)),
               "gr_sync_peers_to_host")
        return out

    def notify_applied(self, slots, applied):
        """Peer.NotifyRaftLastApplied for a list of engine slots (gr_notify_applied)."""
        slots = np.ascontiguousarray(slots, np.uint32)
        applied = np.ascontiguousarray(applied, np.uint64)
        assert len(slots) == len(applied)
        _check(self.lib.gr_notify_applied(self._h, slots.ctypes.data if len(slots) else None,
                                          applied.ctypes.data if len(applied) else None, len(slots)),
               "gr_notify_applied")

    def compact_log(self, slots, index):
        """LogReader.Compact mirrored on the device (gr_compact_log); returns
        (rc, per-slot status: 0 ok, 1 ErrCompacted, 2 ErrUnavailable)."""
        slots = np.ascontiguousarray(slots, np.uint32)
        index = np.ascontiguousarray(index, np.uint64)
        assert len(slots) == len(index)
        st = np.zeros(len(slots), np.int32)
        rc = self.lib.gr_compact_log(self._h, slots.ctypes.data if len(slots) else None,
                                     index.ctypes.data if len(index) else None, len(slots),
                                     st.ctypes.data if len(st) else None)
        if rc not in (0, -6):
            _check(rc, "gr_compact_log")
        return rc, st

    def commit_update(self, slots, uc):
        """entryLog.commitUpdate on the device (gr_commit_update): uc is an
        abi.UPDATE_COMMIT array. Returns (rc, per-slot status: 0 ok, 1 the
        reference panics, 2 term below the device window)."""
        slots = np.ascontiguousarray(slots, np.uint32)
        uc = np.ascontiguousarray(uc, abi.UPDATE_COMMIT)
        assert len(slots) == len(uc)
        st = np.zeros(len(slots), np.int32)
        rc = self.lib.gr_commit_update(self._h, slots.ctypes.data if len(slots) else None,
                                       uc.ctypes.data if len(uc) else None, len(slots),
                                       st.ctypes.data if len(st) else None)
        if rc not in (0, -6):
            _check(rc, "gr_commit_update")
        return rc, st

    def apply_config_change(self, slots, cc):
        """Peer.ApplyConfigChange / RejectConfigChange on the device
        (gr_apply_config_change): cc is an abi.CONFIG_CHANGE array, one record per
        listed engine slot. Returns (rc, per-slot status: abi.CC_APPLIED, or
        CC_HOST / CC_NO_SLOT for a peer left untouched, which the host syncs,
        changes and reloads); rc is -6 (GR_ESTATE) when some status is not
        CC_APPLIED. A slot out of range or listed twice, or an unknown type,
        raises before anything is written, and so does a call refused while a
        step_compact_begin is pending (GR_ESTATE with no status written)."""
        slots = np.ascontiguousarray(slots, np.uint32)
        cc = np.ascontiguousarray(cc, abi.CONFIG_CHANGE)
        assert len(slots) == len(cc)
        st = np.full(len(slots), -1, np.int32)  # no gr_cc_status: still there after a refused call
        rc = self.lib.gr_apply_config_change(self._h, slots.ctypes.data if len(slots) else None,
                                             cc.ctypes.data if len(cc) else None, len(slots),
                                             st.ctypes.data if len(st) else None)
        if rc not in (0, -6) or (rc == -6 and st[0] < 0):
            _check(rc, "gr_apply_config_change")
        return rc, st

    def step(self, msgs=None, locals_=None):
        """One synchronous pass (gr_step). Returns (messages, results) record arrays."""
        msgs = np.zeros(0, abi.MESSAGE) if msgs is None else np.ascontiguousarray(msgs, abi.MESSAGE)
        locals_ = np.zeros(0, abi.LOCAL) if locals_ is None else np.ascontiguousarray(locals_, abi.LOCAL)
        ib = abi.inbox_of(msgs, locals_)
        ob = abi.Outbox()
        _check(self.lib.gr_step(self._h, ctypes.byref(ib), ctypes.byref(ob)), "gr_step")
        out = np.zeros(ob.n_msgs, abi.MESSAGE)
        res = np.zeros(ob.n_results, abi.RESULT)
        if ob.n_msgs:
            ctypes.memmove(out.ctypes.data, ob.msgs, ob.n_msgs * abi.MESSAGE.itemsize)
        if ob.n_results:
            ctypes.memmove(res.ctypes.data, ob.results, ob.n_results * abi.RESULT.itemsize)
        _check(self.lib.gr_release_outbox(self._h, ctypes.byref(ob)), "gr_release_outbox")
        return out, res

    def bind_nodes(self, cluster_ids, node_ids):
        """gr_bind_nodes: engine slot p is node node_ids[p] of cluster cluster_ids[p]."""
        cl = np.ascontiguousarray(cluster_ids, np.uint64)
        nd = np.ascontiguousarray(node_ids, np.uint64)
        assert len(cl) == len(nd)
        _check(self.lib.gr_bind_nodes(self._h, cl.ctypes.data if len(cl) else None,
                                      nd.ctypes.data if len(nd) else None, len(cl)), "gr_bind_nodes")

    def bind_targets(self, target_of, n_targets):
        """gr_bind_targets: target_of[p, j] is the send queue of engine slot p's
        remote slot j (abi.TARGET_HOST: that pair's mail stays with the host)."""
        t = np.ascontiguousarray(target_of, np.uint32)
        assert t.ndim == 2 and t.shape[1] == self.slots
        _check(self.lib.gr_bind_targets(self._h, t.ctypes.data if t.size else None, t.shape[0], n_targets),
               "gr_bind_targets")

    wire_out_host = staticmethod(wire_out_host)

    def step_wire(self, d_msgs, n_msgs, d_ents, n_ents, locals_=None, compact=False, wire_out=None):
        """gr_step_wire over decoded wire records already in HBM (device pointers, as
        grw_decode_device leaves them). Returns (messages, results, unrouted
        indices, unrouted reasons); with compact=True gr_step_wire_compact, whose
        outbox is returned as step_compact returns it: ((cmsgs, ext msgs, cresults,
        ext results), unrouted indices, unrouted reasons). wire_out=cfg (an
        abi.WireOutCfg or a mapping of its fields): gr_step_wire_out, the compact
        return with a WireOut appended; the entry-free mailboxes are in it and not
        in the compact outbox."""
        locals_ = np.zeros(0, abi.LOCAL) if locals_ is None else np.ascontiguousarray(locals_, abi.LOCAL)
        if wire_out is not None:
            ob, un, wo, cfg = abi.COutbox(), abi.WireUnrouted(), abi.WireOut(), wire_out_cfg(wire_out)
            _check(self.lib.gr_step_wire_out(self._h, d_msgs, n_msgs, d_ents, n_ents,
                                             locals_.ctypes.data if len(locals_) else None, len(locals_),
                                             ctypes.byref(ob), ctypes.byref(un), ctypes.byref(cfg), ctypes.byref(wo)),
                   "gr_step_wire_out")
            idx = np.zeros(un.n, np.uint32)
            why = np.zeros(un.n, np.uint8)
            if un.n:
                ctypes.memmove(idx.ctypes.data, un.index, un.n * 4)
                ctypes.memmove(why.ctypes.data, un.reason, un.n)
            w = WireOut(wo)
            return self._take_coutbox(ob), idx, why, w
        ob = abi.COutbox() if compact else abi.Outbox()
        un = abi.WireUnrouted()
        fn = self.lib.gr_step_wire_compact if compact else self.lib.gr_step_wire
        _check(fn(self._h, d_msgs, n_msgs, d_ents, n_ents, locals_.ctypes.data if len(locals_) else None,
                  len(locals_), ctypes.byref(ob), ctypes.byref(un)), fn.__name__)
        idx = np.zeros(un.n, np.uint32)
        why = np.zeros(un.n, np.uint8)
        if un.n:
            ctypes.memmove(idx.ctypes.data, un.index, un.n * 4)
            ctypes.memmove(why.ctypes.data, un.reason, un.n)
        if compact:
            return self._take_coutbox(ob), idx, why
        out = np.zeros(ob.n_msgs, abi.MESSAGE)
        res = np.zeros(ob.n_results, abi.RESULT)
        if ob.n_msgs:
            ctypes.memmove(out.ctypes.data, ob.msgs, ob.n_msgs * abi.MESSAGE.itemsize)
        if ob.n_results:
            ctypes.memmove(res.ctypes.data, ob.results, ob.n_results * abi.RESULT.itemsize)
        _check(self.lib.gr_release_outbox(self._h, ctypes.byref(ob)), "gr_release_outbox")
        return out, res, idx, why

    def pack_messages(self, msgs):
        """gr_pack_messages: full records -> (compact records, ext records)."""
        msgs = np.ascontiguousarray(msgs, abi.MESSAGE)
        c = np.zeros(len(msgs), abi.CMSG)
        ext = np.zeros(len(msgs), abi.MESSAGE)
        nx = ctypes.c_size_t()
        _check(self.lib.gr_pack_messages(msgs.ctypes.data if len(msgs) else None, len(msgs),
                                         c.ctypes.data if len(c) else None, ext.ctypes.data if len(ext) else None,
                                         ctypes.byref(nx)), "gr_pack_messages")
        return c, ext[:nx.value].copy()

    def pair_messages(self, c):
        """gr_pair_messages: compact records with every pair GR_CM_PAIR carries merged."""
        c = np.array(c, abi.CMSG)
        n = ctypes.c_size_t()
        _check(self.lib.gr_pair_messages(c.ctypes.data if len(c) else None, len(c), ctypes.byref(n)),
               "gr_pair_messages")
        return c[:n.value].copy()

    def unpack_messages(self, c, ext):
        """gr_unpack_messages: compact (and ext) records -> full records (a pair record -> two)."""
        c = np.ascontiguousarray(c, abi.CMSG)
        ext = np.ascontiguousarray(ext, abi.MESSAGE)
        out = np.zeros(int(self.lib.gr_cmsg_count(c.ctypes.data if len(c) else None, len(c))), abi.MESSAGE)
        _check(self.lib.gr_unpack_messages(c.ctypes.data if len(c) else None, len(c),
                                           ext.ctypes.data if len(ext) else None, len(ext),
                                           out.ctypes.data if len(out) else None), "gr_unpack_messages")
        return out

    def pack_locals(self, loc):
        loc = np.ascontiguousarray(loc, abi.LOCAL)
        c = np.zeros(len(loc), abi.CLOCAL)
        ext = np.zeros(len(loc), abi.LOCAL)
        nx = ctypes.c_size_t()
        _check(self.lib.gr_pack_locals(loc.ctypes.data if len(loc) else None, len(loc),
                                       c.ctypes.data if len(c) else None, ext.ctypes.data if len(ext) else None,
                                       ctypes.byref(nx)), "gr_pack_locals")
        return c, ext[:nx.value].copy()

    def step_compact(self, cmsgs, ext_msgs, clocals, ext_locals, halves=False, wire_out=None):
        """One synchronous pass with compact records (gr_step_compact, or with
        halves=True its two halves gr_step_compact_begin + _end). Returns
        (cmsgs, ext msgs, cresults, ext results) copied out of the engine's outbox.
        wire_out=cfg: gr_step_compact_wire_out; returns (that tuple, WireOut)."""
        ib = abi.cinbox_of(cmsgs, ext_msgs, clocals, ext_locals)
        ob = abi.COutbox()
        if wire_out is not None:
            wo, cfg = abi.WireOut(), wire_out_cfg(wire_out)
            _check(self.lib.gr_step_compact_wire_out(self._h, ctypes.byref(ib), ctypes.byref(ob), ctypes.byref(cfg),
                                                     ctypes.byref(wo)), "gr_step_compact_wire_out")
            w = WireOut(wo)
            return self._take_coutbox(ob), w
        if halves:
            _check(self.lib.gr_step_compact_begin(self._h, ctypes.byref(ib)), "gr_step_compact_begin")
            _check(self.lib.gr_step_compact_end(self._h, ctypes.byref(ob)), "gr_step_compact_end")
        else:
            _check(self.lib.gr_step_compact(self._h, ctypes.byref(ib), ctypes.byref(ob)), "gr_step_compact")
        return self._take_coutbox(ob)

    def _take_coutbox(self, ob):
        """(cmsgs, ext msgs, cresults, ext results) copied out of a gr_coutbox, released."""
        out = []
        for ptr, n, dt in ((ob.msgs, ob.n_msgs, abi.CMSG), (ob.ext_msgs, ob.n_ext_msgs, abi.MESSAGE),
                           (ob.results, ob.n_results, abi.CRESULT), (ob.ext_results, ob.n_ext_results, abi.RESULT)):
            a = np.zeros(n, dt)
            if n:
                ctypes.memmove(a.ctypes.data, ptr, n * dt.itemsize)
            out.append(a)
        _check(self.lib.gr_release_coutbox(self._h, ctypes.byref(ob)), "gr_release_coutbox")
        return tuple(out)

    def reserve_inbox(self, n_msgs, n_locals):
        """gr_inbox_reserve: (Inbox, msgs view, locals view) over engine-owned pinned
        memory; fill the views, then step_inbox(Inbox)."""
        ib = abi.Inbox()
        _check(self.lib.gr_inbox_reserve(self._h, n_msgs, n_locals, ctypes.byref(ib)), "gr_inbox_reserve")
        msgs = np.ctypeslib.as_array(ctypes.cast(ib.msgs, ctypes.POINTER(ctypes.c_uint8)),
                                     (max(n_msgs, 1) * abi.MESSAGE.itemsize,)).view(abi.MESSAGE)[:n_msgs]
        loc = np.ctypeslib.as_array(ctypes.cast(ib.locals, ctypes.POINTER(ctypes.c_uint8)),
                                    (max(n_locals, 1) * abi.LOCAL.itemsize,)).view(abi.LOCAL)[:n_locals]
        return ib, msgs, loc

    def stats(self):
        s = abi.Stats()
        _check(self.lib.gr_stats_get(self._h, ctypes.byref(s)), "gr_stats_get")
        return {k: getattr(s, k) for k, _ in abi.Stats._fields_}

    def reset_stats(self):
        _check(self.lib.gr_stats_reset(self._h), "gr_stats_reset")

    def timing_begin(self):
        """Record HIP events around each pass's two kernels until timing_end()."""
        _check(self.lib.gr_timing_begin(self._h), "gr_timing_begin")

    def timing_end(self):
        t = abi.Timing()
        _check(self.lib.gr_timing_end(self._h, ctypes.byref(t)), "gr_timing_end")
        return {k: getattr(t, k) for k, _ in abi.Timing._fields_}

    # ---- device-resident path -------------------------------------------------
    def space_bytes(self, n_chunks, positions, depth=MAILBOX_DEPTH):
        return int(self.lib.gr_space_bytes(n_chunks, positions, depth))

    def chunk_bytes(self, positions, depth=MAILBOX_DEPTH):
        return int(self.lib.gr_space_chunk_bytes(positions, depth))

    def hot_chunk_bytes(self, positions, depth=MAILBOX_DEPTH):
        return int(self.lib.gr_space_hot_chunk_bytes(positions, depth))

    def hot_tile_bytes(self, depth=MAILBOX_DEPTH):
        """Bytes per 64-position tile of a hot chunk (its first 64 are the count bytes)."""
        return int(self.lib.gr_space_hot_tile_bytes(depth))

    def cold_used(self, space_ptr, n_chunks, positions, depth=MAILBOX_DEPTH, stream=0):
        """True when some mailbox of the device space needs its cold fields (waits for `stream`)."""
        v = ctypes.c_uint32()
        _check(self.lib.gr_space_cold_used(self._h, space_ptr, n_chunks, positions, depth, stream,
                                           ctypes.byref(v)), "gr_space_cold_used")
        return bool(v.value)

    def side_bytes(self, n_chunks, depth, capacity):
        """Bytes of the side buffers of n_chunks chunks (gr_space_side_bytes)."""
        return int(self.lib.gr_space_side_bytes(n_chunks, depth, capacity))

    def side_pack(self, space_ptr, n_chunks, positions, depth, side_ptr, capacity, stream=0):
        """Compact the device space's cold fields into the side buffers, on `stream` (no wait)."""
        _check(self.lib.gr_space_side_pack(space_ptr, n_chunks, positions, depth, side_ptr, capacity, stream),
               "gr_space_side_pack")

    def side_unpack(self, space_ptr, n_chunks, positions, depth, side_ptr, capacity, stream=0):
        """Write received side-buffer entries into the device space's cold chunks, on `stream`."""
        _check(self.lib.gr_space_side_unpack(space_ptr, n_chunks, positions, depth, side_ptr, capacity, stream),
               "gr_space_side_unpack")

    def cx_bytes(self, n_chunks, positions, depth, capacities, side_capacity):
        """Bytes of the compact-exchange buffers of n_chunks chunks (gr_space_cx_bytes);
        capacities: the record capacity of each chunk."""
        caps = cx_caps_array(capacities, n_chunks)
        return int(self.lib.gr_space_cx_bytes(n_chunks, positions, depth, caps.ctypes.data, side_capacity))

    def cx_pack(self, space_ptr, n_chunks, positions, depth, cx_ptr, capacities, side_capacity, stream=0):
        """Pack the device out space's mailboxes into the compact buffers, on `stream` (no wait)."""
        caps = cx_caps_array(capacities, n_chunks)
        _check(self.lib.gr_space_cx_pack(space_ptr, n_chunks, positions, depth, cx_ptr, caps.ctypes.data,
                                         side_capacity, stream), "gr_space_cx_pack")

    def cx_unpack(self, space_ptr, n_chunks, positions, depth, cx_ptr, capacities, side_capacity, stream=0):
        """Write received compact buffers into the device in space, on `stream`."""
        caps = cx_caps_array(capacities, n_chunks)
        _check(self.lib.gr_space_cx_unpack(space_ptr, n_chunks, positions, depth, cx_ptr, caps.ctypes.data,
                                           side_capacity, stream), "gr_space_cx_unpack")

    def bind_routes(self, in_pos, out_pos):
        """in_pos/out_pos: uint32 arrays [slots][n_peers] (mailbox positions, 0xFFFFFFFF = none)."""
        in_pos = np.ascontiguousarray(in_pos, np.uint32)
        out_pos = np.ascontiguousarray(out_pos, np.uint32)
        n = in_pos.shape[1]
        _check(self.lib.gr_bind_routes(self._h, in_pos.ctypes.data, out_pos.ctypes.data, n), "gr_bind_routes")

    def steady_wave_uniform(self):
        """Whether the bound routes (and the last device pass's spaces) select the
        steady kernel's wave-uniform addressing instance (gpuraft.h gr_steady_wave_uniform)."""
        rc = self.lib.gr_steady_wave_uniform(self._h)
        if rc < 0:
            _check(rc, "gr_steady_wave_uniform")
        return bool(rc)

    def set_locals(self, locals_):
        locals_ = np.ascontiguousarray(locals_, abi.LOCAL)
        _check(self.lib.gr_set_locals(self._h, locals_.ctypes.data if len(locals_) else None,
                                      len(locals_)), "gr_set_locals")

    def step_device(self, in_ptr, out_ptr, in_chunks, in_positions, out_chunks, out_positions,
                    n_peers, stream=0, depth=MAILBOX_DEPTH):
        _check(self.lib.gr_step_device(self._h, in_ptr, out_ptr, in_chunks, in_positions, out_chunks,
                                       out_positions, depth, n_peers, stream), "gr_step_device")

    def graph_capture(self, space_a, space_b, n_chunks, positions, n_peers, n_passes=2, depth=MAILBOX_DEPTH):
        """gr_graph_capture: n_passes (even) device passes over the ping-pong spaces
        (device pointers) recorded into a HIP graph; returns the graph handle."""
        g = ctypes.c_void_p()
        _check(self.lib.gr_graph_capture(self._h, space_a, space_b, n_chunks, positions, depth, n_peers, n_passes,
                                         ctypes.byref(g)), "gr_graph_capture")
        return g

    def graph_replay(self, g, stream=0):
        _check(self.lib.gr_graph_replay(g, stream), "gr_graph_replay")

    def graph_destroy(self, g):
        self.lib.gr_graph_destroy(g)

    def collect_results(self, n=None, first=0):
        n = self.max_peers - first if n is None else n
        out = np.zeros(n, abi.RESULT)
        _check(self.lib.gr_collect_results(self._h, first, out.ctypes.data, n), "gr_collect_results")
        return out

    def collect_updates(self, n=None, first=0, more_to_apply=True, every=False):
        """gr_collect_updates: the peers of slots [first, first+n) that have a
        pb.Update after the last device-resident pass (Peer.HasUpdate), as
        (abi.CRESULT records by ascending slot, abi.RESULT ext records), copied out
        of the engine's memory. Every reported peer's update state moves to its
        State (the prevState half of Peer.Commit)."""
        n = self.max_peers - first if n is None else n
        flags = (abi.UPD_MORE_TO_APPLY if more_to_apply else 0) | (abi.UPD_EVERY if every else 0)
        return self.collect_updates_flags(first, n, flags)

    def collect_updates_flags(self, first, n, flags):
        """collect_updates with the raw GR_UPD_* flag word."""
        u = abi.Updates()
        _check(self.lib.gr_collect_updates(self._h, first, n, flags, ctypes.byref(u)), "gr_collect_updates")
        cr = np.zeros(u.n_results, abi.CRESULT)
        rx = np.zeros(u.n_ext_results, abi.RESULT)
        if u.n_results:
            ctypes.memmove(cr.ctypes.data, u.results, u.n_results * abi.CRESULT.itemsize)
        if u.n_ext_results:
            ctypes.memmove(rx.ctypes.data, u.ext_results, u.n_ext_results * abi.RESULT.itemsize)
        return cr, rx

    def updates_last(self):
        """gr_updates_last: the last collect_updates' record counts, the bytes it
        copied device to host and, when per-pass timing was on, its two kernels'
        event times (classify_ms, pack_ms, timed), as a dict."""
        u = abi.UpdatesInfo()
        _check(self.lib.gr_updates_last(self._h, ctypes.byref(u)), "gr_updates_last")
        return {k: getattr(u, k) for k, _ in abi.UpdatesInfo._fields_ if k != "pad"}

    def set_update_states(self, slots, recs):
        """The peers' update states (abi.UPDATE_STATE, Peer.prevState) for a list of
        engine slots (gr_set_update_states): a host that loads a group with
        lastIndex > 0 sets it to the loaded {term, vote, committed}, as LaunchPeer does."""
        slots = np.ascontiguousarray(slots, np.uint32)
        recs = np.ascontiguousarray(recs, abi.UPDATE_STATE)
        assert len(slots) == len(recs)
        _check(self.lib.gr_set_update_states(self._h, slots.ctypes.data if len(slots) else None,
                                             recs.ctypes.data if len(recs) else None, len(slots)),
               "gr_set_update_states")

    def get_update_states(self, slots):
        slots = np.ascontiguousarray(slots, np.uint32)
        out = np.zeros(len(slots), abi.UPDATE_STATE)
        _check(self.lib.gr_get_update_states(self._h, slots.ctypes.data if len(slots) else None,
                                             out.ctypes.data if len(out) else None, len(slots)),
               "gr_get_update_states")
        return out


def cx_caps_array(capacities, n_chunks):
    """Per-chunk record capacities as the uint32 array the C-ABI takes (an int
    means the same capacity for every chunk)."""
    if np.isscalar(capacities):
        capacities = [capacities] * n_chunks
    caps = np.ascontiguousarray(capacities, np.uint32)
    assert len(caps) == n_chunks
    return caps


def decode_space(buf, n_chunks, positions, depth=MAILBOX_DEPTH, lost_ok=False):
    """Decode a host copy of a message space (bytes/uint8 array) into records.

    peer = mailbox position, slot = index within the mailbox. A mailbox whose
    cold fields were lost in the exchange decodes to records with reject 0xFF:
    an error unless lost_ok."""
    lib = load_library()
    buf = np.ascontiguousarray(buf, np.uint8)
    n = ctypes.c_size_t()
    _check(lib.gr_space_decode(buf.ctypes.data, n_chunks, positions, depth, None, 0, ctypes.byref(n)),
           "decode")
    out = np.zeros(n.value, abi.MESSAGE)
    if n.value:
        _check(lib.gr_space_decode(buf.ctypes.data, n_chunks, positions, depth, out.ctypes.data, n.value,
                                   ctypes.byref(n)), "decode")
    if not lost_ok and np.any(out["reject"] == 0xFF):
        raise RuntimeError("space holds mailboxes whose cold fields were lost in the exchange")
    return out

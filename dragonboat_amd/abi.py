"""numpy / ctypes mirrors of include/gpuraft.h (the C-ABI of libgpuraft.so).

The record layouts here must match the C structs byte for byte; the
``-m "not gpu"`` tests check every size against the library's expectations.
"""
import ctypes

import numpy as np

GR_K = 4
GR_Q = 4
GR_C = 6
GR_SMAX = 8
GR_SLOT_NONE = 0xFF

# raftpb/raft.pb.go:26-50
LOCAL_TICK, ELECTION, LEADER_HEARTBEAT, CONFIG_CHANGE_EVENT, NOOP, PING, PONG, PROPOSE = range(8)
SNAPSHOT_STATUS, UNREACHABLE, CHECK_QUORUM, BATCHED_READ_INDEX, REPLICATE, REPLICATE_RESP = range(8, 14)
REQUEST_VOTE, REQUEST_VOTE_RESP, INSTALL_SNAPSHOT, HEARTBEAT, HEARTBEAT_RESP = range(14, 19)
READ_INDEX, READ_INDEX_RESP, QUIESCE, SNAPSHOT_RECEIVED, LEADER_TRANSFER, TIMEOUT_NOW = range(19, 25)

MSG_NAMES = {
    0: "LocalTick", 1: "Election", 2: "LeaderHeartbeat", 3: "ConfigChangeEvent", 4: "NoOP",
    5: "Ping", 6: "Pong", 7: "Propose", 8: "SnapshotStatus", 9: "Unreachable", 10: "CheckQuorum",
    11: "BatchedReadIndex", 12: "Replicate", 13: "ReplicateResp", 14: "RequestVote",
    15: "RequestVoteResp", 16: "InstallSnapshot", 17: "Heartbeat", 18: "HeartbeatResp",
    19: "ReadIndex", 20: "ReadIndexResp", 21: "Quiesce", 22: "SnapshotReceived",
    23: "LeaderTransfer", 24: "TimeoutNow",
}

FOLLOWER, CANDIDATE, LEADER, OBSERVER = 0, 1, 2, 3
RETRY, WAIT, REPLICATE_ST, SNAPSHOT_ST = 0, 1, 2, 3
SLOT_EMPTY, SLOT_VOTER, SLOT_OBSERVER = 0, 1, 2
F_CHECK_QUORUM, F_IS_LEADER_TRANSFER_TARGET, F_PENDING_CONFIG_CHANGE = 1, 2, 4
PROP_NONE, PROP_APPENDED, PROP_DROPPED, PROP_FORWARDED = 0, 1, 2, 3

ESC_NAMES = ["none", "term_window", "random", "unsupported", "election", "panic", "capacity",
             "snapshot", "entry_size", "msg_runs", "nonmember", "config_change", "wide_term"]

u8, u32, u64 = np.uint8, np.uint32, np.uint64

REMOTE = np.dtype([("match", u64), ("next", u64), ("snapshot_index", u64), ("state", u8),
                   ("active", u8), ("kind", u8), ("pad", u8, (5,))])
READ_STATUS = np.dtype([("index", u64), ("ctx_low", u64), ("ctx_high", u64), ("from_slot", u8),
                        ("ack_bits", u8), ("pad", u8, (6,))])
PEER = np.dtype([
    ("term", u64), ("vote", u64), ("committed", u64), ("applied", u64), ("last_index", u64),
    ("first_index_m1", u64), ("leader_id", u64), ("leader_transfer_target", u64), ("node_id", u64),
    ("election_tick", u64), ("heartbeat_tick", u64), ("randomized_election_timeout", u64),
    ("election_timeout", u64), ("heartbeat_timeout", u64), ("entry_size_ub", u64),
    ("saved_to", u64), ("marker_index", u64), ("log_applied", u64),
    ("run_start", u64, (GR_K,)), ("run_term", u64, (GR_K,)), ("remote_id", u64, (GR_SMAX,)),
    ("remotes", REMOTE, (GR_SMAX,)), ("read_index", READ_STATUS, (GR_Q,)),
    ("state", u8), ("n_runs", u8), ("self_slot", u8), ("flags", u8), ("read_index_count", u8),
    ("pad", u8, (3,)),
])
# gr_peer with its vote tally bytes named (gpuraft.h votes_granted / votes_rejected:
# a candidate's tally over remote slots, 0 unless state == CANDIDATE): the same
# 664 bytes, so recs.view(PEER_VOTES) reads and writes them in place. PEER keeps
# them inside "pad": bench.py --dump-outputs writes one column per named field of
# PEER, and those columns are compared from one build to the next.
PEER_VOTES = np.dtype([(n, PEER.fields[n][0]) for n in PEER.names if n != "pad"] +
                      [("votes_granted", u8), ("votes_rejected", u8), ("pad", u8, (1,))])
assert PEER_VOTES.itemsize == PEER.itemsize and \
    PEER_VOTES.fields["votes_granted"][1] == PEER.fields["pad"][1]
MESSAGE = np.dtype([
    ("peer", u32), ("type", u8), ("slot", u8), ("reject", u8), ("n_runs", u8),
    ("n_entries", u32), ("run2_offset", u32),
    ("term", u64), ("log_index", u64), ("log_term", u64), ("commit", u64), ("hint", u64),
    ("hint_high", u64), ("run_term", u64, (2,)),
])
LOCAL = np.dtype([
    ("peer", u32), ("ticks", u32), ("quiesced_ticks", u32), ("propose_entries", u32),
    ("read_index", u8), ("propose_has_config_change", u8), ("pad", u8, (6,)),
    ("read_ctx_low", u64), ("read_ctx_high", u64), ("rand", u64),
])
READY = np.dtype([("index", u64), ("ctx_low", u64), ("ctx_high", u64)])
RESULT = np.dtype([
    ("peer", u32), ("escalation", u8), ("propose_result", u8), ("n_ready", u8), ("n_forwarded", u8),
    ("esc_item", u32), ("forwarded_entries", u32), ("append_from", u64), ("propose_first", u64),
    ("committed", u64), ("last_index", u64), ("save_from", u64), ("term", u64), ("vote", u64),
    ("ready", READY, (GR_Q,)),
])
# Compact boundary records (gr_step_compact)
CM_REJECT, CM_ENTRY, CM_LOG_TERM, CM_COMMIT, CM_HINT, CM_EXT = 0x01, 0x02, 0x04, 0x08, 0x10, 0x80
CM_ENTRY2, CM_PAIR = 0x20, 0x40  # a record standing for two messages (gpuraft.h GR_CM_PAIR)
CL_CONFIG_CHANGE, CL_EXT = 0x01, 0x80
CR_EXT = 0x80
CMSG = np.dtype([("peer", u32), ("type", u8), ("slot", u8), ("flags", u8), ("pad", u8), ("term", u32),
                 ("aux", u32), ("log_index", u64)])
CLOCAL = np.dtype([("peer", u32), ("propose_entries", u32), ("ticks", np.uint16), ("quiesced_ticks", u8),
                   ("flags", u8), ("ext", u32), ("rand", u64)])
CRESULT = np.dtype([("peer", u32), ("escalation", u8), ("propose_result", u8), ("flags", u8), ("save_count", u8),
                    ("aux", u32), ("commit_lag", u32), ("last_index", u64)])
assert CMSG.itemsize == 24 and CLOCAL.itemsize == 24 and CRESULT.itemsize == 24
PROMOTION = np.dtype([("peer", u32), ("pad", u32), ("term", u64), ("noop_index", u64)])
assert PROMOTION.itemsize == 24
# gr_quiesce_state: one peer's quiesceManager (quiesce.go:24-34). QUIESCE is
# the message type above, so the record's dtype carries the struct's name.
QUIESCE_STATE = np.dtype([("tick", u64), ("election_tick", u64), ("quiesced_since", u64),
                          ("no_activity_since", u64),
                          ("exit_quiesce_tick", u64), ("enabled", u8), ("pad", u8, (7,))])
assert QUIESCE_STATE.itemsize == 48
UPDATE_COMMIT = np.dtype([("stable_log_to", u64), ("stable_log_term", u64), ("applied_to", u64)])
# gr_config_change (gr_apply_config_change): type numbered as raftpb.ConfigChangeType
# (raftpb/raft.pb.go:167-169), status as gr_cc_status
CC_ADD_NODE, CC_REMOVE_NODE, CC_ADD_OBSERVER = 0, 1, 2
CC_APPLIED, CC_HOST, CC_NO_SLOT = 0, 1, 2
CONFIG_CHANGE = np.dtype([("node_id", u64), ("rand", u64), ("type", u8), ("pad", u8, (7,))])
assert CONFIG_CHANGE.itemsize == 24
# gr_snapshot_rec / gr_restored / gr_membership (gpuraft.h, snapshots on the device)
SNAPSHOT_REC = np.dtype([("index", u64), ("term", u64)])
assert SNAPSHOT_REC.itemsize == 16
RESTORED = np.dtype([("peer", u32), ("pad", u32), ("index", u64), ("term", u64)])
assert RESTORED.itemsize == 24
MEMBERSHIP = np.dtype([("node_id", u64, (GR_SMAX,)), ("kind", u8, (GR_SMAX,)), ("rand", u64)])
assert MEMBERSHIP.itemsize == 80
# gr_cc_index (gpuraft.h, config-change entries on the device)
CC_INDEX = np.dtype([("last", u64), ("prev", u64)])
assert CC_INDEX.itemsize == 16
# gr_update_state / gr_updates (gpuraft.h, updates out of the device-resident path)
UPD_MORE_TO_APPLY, UPD_EVERY = 0x1, 0x2
UPD_NONE, UPD_COMPACT, UPD_EXT = 0, 1, 2
UPDATE_STATE = np.dtype([("term", u64), ("vote", u64), ("commit", u64)])
assert UPDATE_STATE.itemsize == 24
SIZES = {"gr_peer": 664, "gr_message": 80, "gr_local_input": 48, "gr_peer_result": 168,
         "gr_remote": 32, "gr_read_status": 32}
assert PEER.itemsize == SIZES["gr_peer"], PEER.itemsize
assert MESSAGE.itemsize == SIZES["gr_message"], MESSAGE.itemsize
assert LOCAL.itemsize == SIZES["gr_local_input"], LOCAL.itemsize
assert RESULT.itemsize == SIZES["gr_peer_result"], RESULT.itemsize


class Config(ctypes.Structure):
    _fields_ = [("max_peers", ctypes.c_uint32), ("slots", ctypes.c_uint32),
                ("window_runs", ctypes.c_uint32), ("read_index_depth", ctypes.c_uint32),
                ("mailbox_depth", ctypes.c_uint32), ("device", ctypes.c_uint32),
                ("max_entry_size", ctypes.c_uint64)]


class Inbox(ctypes.Structure):
    _fields_ = [("msgs", ctypes.c_void_p), ("n_msgs", ctypes.c_size_t),
                ("locals", ctypes.c_void_p), ("n_locals", ctypes.c_size_t)]


class Outbox(ctypes.Structure):
    _fields_ = [("msgs", ctypes.c_void_p), ("n_msgs", ctypes.c_size_t),
                ("results", ctypes.c_void_p), ("n_results", ctypes.c_size_t)]


class WireUnrouted(ctypes.Structure):
    _fields_ = [("n", ctypes.c_size_t), ("index", ctypes.c_void_p), ("reason", ctypes.c_void_p)]


WIRE_REASONS = ["routed", "no_peer", "nonmember", "snapshot", "type", "runs", "index"]

# Entry-free outbox mail by wire (gpuraft.h gr_step_wire_out)
TARGET_HOST = 0xFFFFFFFF
MAX_TARGETS = 256
WIRE_OUT_CFG = np.dtype([("deployment_id", u64), ("source_off", u64), ("source_len", u32), ("bin_ver", u32),
                         ("max_batch_msgs", u32), ("pad", u32)])
assert WIRE_OUT_CFG.itemsize == 32


class WireOutCfg(ctypes.Structure):
    _fields_ = [("deployment_id", ctypes.c_uint64), ("source_off", ctypes.c_uint64),
                ("source_len", ctypes.c_uint32), ("bin_ver", ctypes.c_uint32),
                ("max_batch_msgs", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class WireOut(ctypes.Structure):
    _fields_ = [("d_batches", ctypes.c_void_p), ("n_batches", ctypes.c_size_t),
                ("d_msgs", ctypes.c_void_p), ("n_msgs", ctypes.c_size_t),
                ("batch_target", ctypes.c_void_p)]


class Updates(ctypes.Structure):
    _fields_ = [("results", ctypes.c_void_p), ("n_results", ctypes.c_size_t),
                ("ext_results", ctypes.c_void_p), ("n_ext_results", ctypes.c_size_t)]


class UpdatesInfo(ctypes.Structure):
    _fields_ = [("n_results", ctypes.c_uint64), ("n_ext_results", ctypes.c_uint64), ("bytes_down", ctypes.c_uint64),
                ("classify_ms", ctypes.c_double), ("pack_ms", ctypes.c_double), ("timed", ctypes.c_uint32),
                ("pad", ctypes.c_uint32)]


class CInbox(ctypes.Structure):
    _fields_ = [("msgs", ctypes.c_void_p), ("n_msgs", ctypes.c_size_t),
                ("ext_msgs", ctypes.c_void_p), ("n_ext_msgs", ctypes.c_size_t),
                ("locals", ctypes.c_void_p), ("n_locals", ctypes.c_size_t),
                ("ext_locals", ctypes.c_void_p), ("n_ext_locals", ctypes.c_size_t)]


class COutbox(ctypes.Structure):
    _fields_ = [("msgs", ctypes.c_void_p), ("n_msgs", ctypes.c_size_t),
                ("ext_msgs", ctypes.c_void_p), ("n_ext_msgs", ctypes.c_size_t),
                ("results", ctypes.c_void_p), ("n_results", ctypes.c_size_t),
                ("ext_results", ctypes.c_void_p), ("n_ext_results", ctypes.c_size_t)]


def cinbox_of(msgs, ext, locals_, lext):
    """A CInbox over numpy record arrays (kept alive by the caller)."""
    ib = CInbox()
    for name, a in (("msgs", msgs), ("ext_msgs", ext), ("locals", locals_), ("ext_locals", lext)):
        setattr(ib, name, a.ctypes.data if len(a) else None)
        setattr(ib, "n_" + name, len(a))
    return ib


class Stats(ctypes.Structure):
    _fields_ = [("passes", ctypes.c_uint64), ("leader_commits", ctypes.c_uint64),
                ("follower_commits", ctypes.c_uint64), ("escalations", ctypes.c_uint64),
                ("msgs_in", ctypes.c_uint64), ("msgs_out", ctypes.c_uint64),
                ("leader_msgs_in", ctypes.c_uint64), ("leader_msgs_out", ctypes.c_uint64),
                ("replicate_entries", ctypes.c_uint64)]


class Timing(ctypes.Structure):
    _fields_ = [("passes", ctypes.c_uint64), ("fast_ms", ctypes.c_double), ("general_ms", ctypes.c_double),
                ("bailed_lanes", ctypes.c_uint64)]


# settings.Soft.MaxEntrySize (internal/settings/soft.go:236)
MAX_ENTRY_SIZE = 2 * 32 * 1024 * 1024

# Every symbol include/gpuraft.h declares.
EXPORTS = [
    "gr_create", "gr_destroy", "gr_strerror", "gr_escalation_name", "gr_load_groups",
    "gr_sync_groups_to_host", "gr_step", "gr_inbox_reserve", "gr_release_outbox", "gr_stats_get", "gr_stats_reset",
    "gr_load_peers", "gr_sync_peers_to_host", "gr_notify_applied", "gr_compact_log", "gr_commit_update", "gr_apply_config_change", "gr_space_bytes", "gr_space_chunk_bytes",
    "gr_space_hot_chunk_bytes", "gr_space_hot_tile_bytes", "gr_space_tile_positions", "gr_space_cold_used",
    "gr_space_side_bytes", "gr_space_side_pack", "gr_space_side_unpack", "gr_space_side_pack_host",
    "gr_space_side_unpack_host", "gr_space_cx_bytes", "gr_space_cx_pack", "gr_space_cx_unpack",
    "gr_space_cx_pack_host", "gr_space_cx_unpack_host", "gr_bind_routes", "gr_steady_wave_uniform",
    "gr_set_locals", "gr_step_device", "gr_step_compact", "gr_step_compact_begin", "gr_step_compact_end", "gr_cinbox_reserve", "gr_release_coutbox",
    "gr_pack_messages", "gr_unpack_messages", "gr_cmsg_count", "gr_pair_messages", "gr_pack_locals",
    "gr_collect_results", "gr_space_decode", "gr_space_encode", "gr_timing_begin", "gr_timing_end",
    "gr_bind_nodes", "gr_step_wire", "gr_step_wire_compact",
    "gr_bind_targets", "gr_step_wire_out", "gr_step_compact_wire_out", "gr_wire_out_host",
    "gr_graph_capture", "gr_graph_replay", "gr_graph_destroy",
    "gr_set_elections", "gr_get_elections", "gr_promotions",
    "gr_set_snapshots", "gr_get_snapshots", "gr_set_snapshot_recs", "gr_get_snapshot_recs", "gr_restored_snapshots",
    "gr_restore_remotes",
    "gr_set_config_entries", "gr_get_config_entries", "gr_set_cc_indexes", "gr_get_cc_indexes",
    "gr_set_quiesce", "gr_get_quiesce", "gr_load_quiesce", "gr_sync_quiesce", "gr_load_quiesce_peers",
    "gr_sync_quiesce_peers", "gr_tick_all", "gr_splitmix64",
    "gr_set_update_states", "gr_get_update_states", "gr_collect_updates", "gr_update_class", "gr_updates_last",
]


def splitmix64(x):
    """gr_splitmix64 (gpuraft.h): gr_tick_all gives engine slot p the draw
    splitmix64(rand_seed + p)."""
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def inbox_of(msgs, locals_):
    """Build an Inbox over numpy record arrays (kept alive by the caller)."""
    ib = Inbox()
    ib.msgs = msgs.ctypes.data if len(msgs) else None
    ib.n_msgs = len(msgs)
    ib.locals = locals_.ctypes.data if len(locals_) else None
    ib.n_locals = len(locals_)
    return ib

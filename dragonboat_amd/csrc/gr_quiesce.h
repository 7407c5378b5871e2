// gr_quiesce.h — the quiesce manager (quiesce.go:24-125) and the node.go hooks
// that drive it, as code shared by the device (gr_quiesce_kernel, the general
// lane's prefix re-run) and the host (tests/native/quiesce_host.cpp). Nothing
// here touches raft state: the manager only decides which of a pass's
// LocalTicks are Peer.Tick() and which Peer.QuiescedTick() (node.go:877-890),
// and whether the peer announces that it went idle (node.go:530-543, 643-645).
#pragma once
#include <stdint.h>

#include "gpuraft.h"

#if defined(__HIPCC__)
#define GQ_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GQ_HD inline
#endif

namespace gr {

// quiesceManager (quiesce.go:24-34) without the ids it only logs; flag is
// newQuiesceStateFlag, consumed once per pass (node.go:643).
struct QuiesceMgr {
  uint64_t tick, election_tick, quiesced_since, no_activity_since, exit_quiesce_tick;
  bool enabled, flag;
};

GQ_HD QuiesceMgr q_from_state(const gr_quiesce_state& s) {
  QuiesceMgr q;
  q.tick = s.tick;
  q.election_tick = s.election_tick;
  q.quiesced_since = s.quiesced_since;
  q.no_activity_since = s.no_activity_since;
  q.exit_quiesce_tick = s.exit_quiesce_tick;
  q.enabled = s.enabled != 0;
  q.flag = false;
  return q;
}
GQ_HD gr_quiesce_state q_to_state(const QuiesceMgr& q) {
  gr_quiesce_state s;
  s.tick = q.tick;
  s.election_tick = q.election_tick;
  s.quiesced_since = q.quiesced_since;
  s.no_activity_since = q.no_activity_since;
  s.exit_quiesce_tick = q.exit_quiesce_tick;
  s.enabled = q.enabled ? 1 : 0;
  for (int k = 0; k < 7; ++k) s.pad[k] = 0;
  return s;
}

// quiesceThreshold (quiesce.go:88-90)
GQ_HD uint64_t q_threshold(const QuiesceMgr& q) { return q.election_tick * 10; }
// quiesced (quiesce.go:58-63): a disabled manager is never quiesced
GQ_HD bool q_quiesced(const QuiesceMgr& q) { return q.enabled && q.quiesced_since > 0; }
// enterQuiesce (quiesce.go:115-120). At tick 0 this leaves quiescedSince = 0:
// the peer is not quiesced, but the new-state flag is set.
GQ_HD void q_enter_quiesce(QuiesceMgr& q) {
  q.quiesced_since = q.tick;
  q.no_activity_since = q.tick;
  q.flag = true;
}
// exitQuiesce (quiesce.go:122-125)
GQ_HD void q_exit_quiesce(QuiesceMgr& q) {
  q.quiesced_since = 0;
  q.exit_quiesce_tick = q.tick;
}
// newToQuiesce (quiesce.go:92-97)
GQ_HD bool q_new_to_quiesce(const QuiesceMgr& q) {
  if (!q_quiesced(q)) return false;
  return q.tick - q.quiesced_since < q.election_tick;
}
// justExitedQuiesce (quiesce.go:99-104); unsigned arithmetic as in Go
GQ_HD bool q_just_exited_quiesce(const QuiesceMgr& q) {
  if (q_quiesced(q)) return false;
  return q.tick - q.exit_quiesce_tick < q_threshold(q);
}
// increaseQuiesceTick (quiesce.go:44-56): a disabled manager returns tick 0
GQ_HD uint64_t q_increase_quiesce_tick(QuiesceMgr& q) {
  if (!q.enabled) return 0;
  const uint64_t threshold = q_threshold(q);
  q.tick++;
  if (!q_quiesced(q)) {
    if (q.tick - q.no_activity_since > threshold) q_enter_quiesce(q);
  }
  return q.tick;
}
// recordActivity (quiesce.go:65-86): a Heartbeat or HeartbeatResp is no
// activity unless the peer is quiesced and past its first electionTick ticks
GQ_HD void q_record_activity(QuiesceMgr& q, uint32_t type) {
  if (!q.enabled) return;
  if (type == GR_HEARTBEAT || type == GR_HEARTBEAT_RESP) {
    if (!q_quiesced(q)) return;
    if (q_new_to_quiesce(q)) return;
  }
  q.no_activity_since = q.tick;
  if (q_quiesced(q)) q_exit_quiesce(q);
}
// tryEnterQuiesce (quiesce.go:106-113). Not guarded by `enabled` in the
// reference either: a disabled manager's quiescedSince may move, quiesced()
// stays false.
GQ_HD void q_try_enter_quiesce(QuiesceMgr& q) {
  if (q_just_exited_quiesce(q)) return;
  if (!q_quiesced(q)) q_enter_quiesce(q);
}

// One inbound message (node.go:752-769): handleMessage takes Quiesce
// (tryEnterQuiesce, :784-785), SnapshotStatus and Unreachable (:788-797, no
// activity); every other type goes through tryRecordNodeActivity (:736-743),
// where a Heartbeat or HeartbeatResp with Hint > 0 counts as a ReadIndex.
GQ_HD void q_message(QuiesceMgr& q, uint32_t type, bool hint_nonzero) {
  if (type == GR_QUIESCE) {
    q_try_enter_quiesce(q);
  } else if (type == GR_SNAPSHOT_STATUS || type == GR_UNREACHABLE) {
  } else if ((type == GR_HEARTBEAT || type == GR_HEARTBEAT_RESP) && hint_nonzero) {
    q_record_activity(q, GR_READ_INDEX);
  } else {
    q_record_activity(q, type);
  }
}

// One node.tick (node.go:885-890): true = Peer.QuiescedTick, false = Peer.Tick
GQ_HD bool q_tick(QuiesceMgr& q) {
  q_increase_quiesce_tick(q);
  return q_quiesced(q);
}

// What a pass leaves besides the record: the LocalTick split the step kernels
// read, and whether the peer sends Quiesce to its voters (newQuiesceState,
// node.go:643-645).
struct QuiescePass {
  uint32_t ticks, quiesced_ticks;
  bool send;
};

// The pass over a peer's items below `limit`, in the engine's item order
// (gr_peer_result.esc_item): one item per message, one for a local ReadIndex,
// one per Tick, one for all QuiescedTicks, one for a proposal. The ReadIndex
// item is counted after the messages, where the raft lane runs it, but its
// recordActivity runs before them (handleReadIndexRequests is first in
// handleEvents, node.go:655, 687-693), so it is part of the prefix only when
// limit is past it. No tick rouses a peer, so n LocalTicks are k Ticks then
// n - k QuiescedTicks; a prefix that ends inside the Ticks ran that many
// LocalTicks, one that includes the QuiescedTick item ran all n.
// each(nm, sink) calls sink(type, hint_nonzero) for the first nm <= n_msgs
// messages in item order (by slot, then arrival).
template <class EachFn>
GQ_HD QuiescePass q_run_pass(QuiesceMgr& q, bool read_index, uint32_t n_msgs, uint32_t raw_ticks, uint32_t limit,
                             EachFn each) {
  QuiescePass r;
  r.ticks = 0;
  r.quiesced_ticks = 0;
  q.flag = false;
  const uint32_t nm = n_msgs < limit ? n_msgs : limit;
  uint32_t left = limit - nm;  // items past the messages
  if (read_index && nm == n_msgs && left > 0) {
    q_record_activity(q, GR_READ_INDEX);
    left--;
  } else if (read_index) {
    left = 0;
  }
  each(nm, [&](uint32_t type, bool hint_nonzero) { q_message(q, type, hint_nonzero); });
  if (nm == n_msgs) {
    for (uint32_t t = 0; t < raw_ticks; ++t) {
      // the QuiescedTicks are one item: once it is in the prefix, all of them are
      if (!r.quiesced_ticks && left == 0) break;
      const bool qt = q_tick(q);
      if (!(qt && r.quiesced_ticks)) left--;  // a Tick, or the one item of the QuiescedTicks
      if (qt) r.quiesced_ticks++;
      else r.ticks++;
    }
  }
  r.send = q.flag;
  q.flag = false;
  return r;
}

// The device record: 16 bytes a peer, ticks in 32 bits, plus a word that no
// pass writes (electionTick | enabled << 31). gr_load_quiesce refuses
// (GR_EINVAL) a record with a tick field of 2^32 or more, an election_tick of
// 2^31 or more, or enabled above 1.
struct alignas(16) QuiesceRec {
  uint32_t tick, quiesced_since, no_activity_since, exit_quiesce_tick;
};
constexpr uint32_t QC_ENABLED = 0x80000000u;
GQ_HD bool q_encodable(const gr_quiesce_state& s) {
  return !((s.tick | s.quiesced_since | s.no_activity_since | s.exit_quiesce_tick) >> 32) &&
         s.election_tick < 0x80000000ull && s.enabled <= 1;
}
GQ_HD QuiesceMgr q_decode(const QuiesceRec& r, uint32_t cfg) {
  QuiesceMgr q;
  q.tick = r.tick;
  q.quiesced_since = r.quiesced_since;
  q.no_activity_since = r.no_activity_since;
  q.exit_quiesce_tick = r.exit_quiesce_tick;
  q.election_tick = cfg & ~QC_ENABLED;
  q.enabled = (cfg & QC_ENABLED) != 0;
  q.flag = false;
  return q;
}
GQ_HD QuiesceRec q_encode(const QuiesceMgr& q) {
  QuiesceRec r;
  r.tick = (uint32_t)q.tick;
  r.quiesced_since = (uint32_t)q.quiesced_since;
  r.no_activity_since = (uint32_t)q.no_activity_since;
  r.exit_quiesce_tick = (uint32_t)q.exit_quiesce_tick;
  return r;
}
GQ_HD uint32_t q_cfg(const gr_quiesce_state& s) { return (uint32_t)s.election_tick | (s.enabled ? QC_ENABLED : 0u); }

// gr_tick_all's draw for engine slot `peer` (gpuraft.h): splitmix64 of
// rand_seed + peer.
GQ_HD uint64_t q_splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

}  // namespace gr

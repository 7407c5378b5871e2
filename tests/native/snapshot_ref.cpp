// snapshot_ref.cpp — TEST INFRASTRUCTURE: the reference side of snapshots on
// the device (gpuraft.h gr_set_snapshots, gr_restore_remotes). A gr_peer record
// and the group's snapshot record become an oracle raft object through the
// oracle's own build_peer (RunLogDB::snap is what LogReader.Snapshot() returns);
// the pass's items run through the oracle's Handle / tick / propose in the
// engine's item order, as ob_step2 runs them (ref_pass.h, shared with the other
// reference sides); export_peer and to_record give
// the records back. This translation unit includes oracle/batch.cpp to reach
// those functions; the oracle itself is unchanged. What this file adds is
// gpuraft.h's message convention: an InstallSnapshot record carries
// Snapshot.Index / Snapshot.Term in log_index / log_term, and an inbound one
// with reject set names the receiver in Snapshot.Membership.Observers.
// Linked with hostlane_snap.hip into tests/_build/libhostlane_snap*.so.
#include "batch.cpp"
#include "ref_pass.h"

namespace {

// gr_message -> raftpb.Message, an InstallSnapshot by the convention
Message expand(const OPeer& op, const gr_message& g) {
  Message m = from_record(op, g);
  if (m.Type == InstallSnapshot) refpass::expand_install(op, g, &m);
  return m;
}

// raftpb.Message -> gr_message, an InstallSnapshot by the convention
bool contract(const OPeer& op, uint32_t peer, const Message& m, gr_message* o) {
  const bool ok = to_record(op, peer, m, o);
  if (m.Type == InstallSnapshot) refpass::contract_install(m, o);
  return ok;
}

using refpass::PassOut;

// node id -> slot, members first, then an empty slot that still carries the id
uint32_t slot_any(const OPeer& op, u64 id) {
  const uint32_t s = op.slotOf(id);
  if (s != GR_SLOT_NONE) return s;
  for (size_t j = 0; j < op.ids.size(); ++j)
    if (op.kinds[j] == GR_SLOT_EMPTY && op.ids[j] == id) return (uint32_t)j;
  return GR_SLOT_NONE;
}

// gpuraft.h's free-slot rule (gr_apply_config_change): the lowest empty slot
// that no live readStatus (its requester, its confirmed ids) maps to
uint32_t free_slot(const OPeer& op) {
  std::vector<bool> named(op.ids.size(), false);
  for (auto& ctx : op.r->readIdx.queue) {
    auto s = op.r->readIdx.pending.at(ctx);
    std::vector<u64> who;
    if (s->from) who.push_back(s->from);
    for (auto& kv : s->confirmed) who.push_back(kv.first);
    for (u64 w : who) {
      const uint32_t j = slot_any(op, w);
      if (j != GR_SLOT_NONE) named[j] = true;
    }
  }
  for (size_t j = 0; j < op.ids.size(); ++j)
    if (op.kinds[j] == GR_SLOT_EMPTY && !named[j]) return (uint32_t)j;
  return GR_SLOT_NONE;
}

// export_peer maps a readStatus's ids through member slots only; the record
// carries a removed node's confirmation as the ack bit of the slot that keeps its id
void export_with_removed_acks(const OPeer& op, uint32_t S, gr_peer* g) {
  export_peer(op, S, g);
  int q = 0;
  for (auto& ctx : op.r->readIdx.queue) {
    if (q >= GR_Q) break;
    auto s = op.r->readIdx.pending.at(ctx);
    gr_read_status& rs = g->read_index[q++];
    rs.from_slot = s->from == 0 ? GR_SLOT_NONE : (uint8_t)slot_any(op, s->from);
    uint8_t ack = 0;
    for (auto& kv : s->confirmed) {
      const uint32_t j = slot_any(op, kv.first);
      if (j != GR_SLOT_NONE) ack |= (uint8_t)(1u << j);
    }
    rs.ack_bits = ack;
  }
}

// Peer.RestoreRemotes on one record: the oracle's restoreRemotes, then the slot
// table by gpuraft.h's rule.
int32_t restore_one(gr_peer& g, uint32_t S, u64 maxEntrySize, const gr_membership& m) {
  if (g.state == GR_CANDIDATE) return GR_CC_HOST;
  OPeer op;
  build_peer(g, S, maxEntrySize, &op);
  raft& r = *op.r;
  Snapshot ss;
  std::vector<std::pair<u64, uint8_t>> list;
  for (uint32_t k = 0; k < GR_SMAX && m.kind[k] != GR_SLOT_EMPTY; ++k) {
    for (auto& kv : list)
      if (kv.first == m.node_id[k]) return GR_CC_HOST;
    list.push_back({m.node_id[k], m.kind[k]});
    if (m.kind[k] == GR_SLOT_VOTER) ss.membership.Addresses[m.node_id[k]] = "";
    else ss.membership.Observers[m.node_id[k]] = "";
  }
  uint32_t promoted = 0;
  for (auto& kv : ss.membership.Addresses) promoted += r.observers.count(kv.first) ? 1 : 0;
  if (promoted > 1) return GR_CC_HOST;  // one draw per becomeFollower
  if (promoted && r.electionTimeout == 0) return GR_CC_HOST;
  op.rand.assign(1, m.rand);
  op.randNext = 0;
  r.restoreRemotes(ss);
  if (!r.msgs.empty()) return GR_CC_HOST;
  for (uint32_t j = 0; j < S; ++j) {
    bool keep = false;
    for (auto& kv : list) keep = keep || kv.first == op.ids[j];
    if (!keep) op.kinds[j] = GR_SLOT_EMPTY;
  }
  std::vector<bool> done(list.size(), false);
  for (size_t k = 0; k < list.size(); ++k) {
    const uint32_t j = slot_any(op, list[k].first);
    if (j == GR_SLOT_NONE) continue;
    op.kinds[j] = list[k].second;
    done[k] = true;
  }
  for (size_t k = 0; k < list.size(); ++k) {
    if (done[k]) continue;
    const uint32_t f = free_slot(op);
    if (f == GR_SLOT_NONE) return GR_CC_NO_SLOT;
    op.ids[f] = list[k].first;
    op.kinds[f] = list[k].second;
  }
  export_with_removed_acks(op, S, &g);
  return GR_CC_APPLIED;
}

}  // namespace

// One pass over records. peers[p] / snap[p] are read and, for every peer with
// input, written back as the state after the items below limits[p] (NULL: all
// items). Results come one per peer with input, in peer order; messages in
// peer, then item order; `restored` as gr_restored_snapshots lists them.
// panic_item[p] (may be NULL) is the item at which the oracle panicked, or -1.
extern "C" int snr_step(uint32_t slots, uint64_t max_entry_size, gr_peer* peers, uint32_t n_peers,
                        const gr_inbox* in, const uint32_t* limits, gr_snapshot_rec* snap, gr_message* out,
                        size_t out_cap, size_t* n_out, gr_peer_result* results, size_t* n_results,
                        gr_restored* restored, size_t restored_cap, size_t* n_restored, int32_t* panic_item) {
  if (!in || !n_out || !n_results || !n_restored || !snap) return GR_EINVAL;
  const uint32_t S = slots;
  refpass::Sorted so;
  if (refpass::sort_inbox(in, S, n_peers, &so)) return GR_EINVAL;
  size_t no = 0, nr = 0, ns = 0;
  int rc = GR_OK;
  for (uint32_t pi = 0; pi < n_peers; ++pi) {
    if (panic_item) panic_item[pi] = -1;
    if (!so.has[pi]) continue;
    OPeer op;
    PassOut po;
    try {
      build_peer(peers[pi], S, max_entry_size, &op);
    } catch (const std::exception&) {
      return GR_ESTATE;
    }
    op.db->snap.Index = snap[pi].index;
    op.db->snap.Term = snap[pi].term;
    refpass::run_peer(op, pi, so.of(pi), so.loc[pi], limits ? limits[pi] : 0xFFFFFFFFu, &po, expand, contract);
    if (po.panic_item >= 0) {
      if (panic_item) panic_item[pi] = po.panic_item;
      else rc = GR_ESTATE;
    }
    export_peer(op, S, &peers[pi]);
    const Snapshot ss = op.r->log->snapshot();
    snap[pi].index = ss.Index;
    snap[pi].term = ss.Term;
    for (auto& m : po.msgs) {
      if (out && no < out_cap) out[no] = m;
      no++;
    }
    for (auto& x : po.restored) {
      if (restored && ns < restored_cap) restored[ns] = x;
      ns++;
    }
    if (results) results[nr] = po.res;
    nr++;
  }
  *n_out = no;
  *n_results = nr;
  *n_restored = ns;
  if (no > out_cap || ns > restored_cap) return GR_ECAPACITY;
  return rc;
}

// gr_restore_remotes on records through the oracle's restoreRemotes.
extern "C" int snr_restore_remotes(uint32_t slots, uint64_t max_entry_size, gr_peer* peers, uint32_t n_peers,
                                   const uint32_t* list, const gr_membership* ms, uint32_t n, int32_t* status) {
  int rc = GR_OK;
  try {
    for (uint32_t x = 0; x < n; ++x) {
      if (list[x] >= n_peers) return GR_ERANGE;
      const int32_t s = restore_one(peers[list[x]], slots, max_entry_size, ms[x]);
      if (status) status[x] = s;
      if (s) rc = GR_ESTATE;
    }
  } catch (const std::exception&) {
    return -100;  // the oracle panicked
  }
  return rc;
}

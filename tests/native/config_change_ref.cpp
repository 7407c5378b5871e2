// config_change_ref.cpp — TEST INFRASTRUCTURE: the reference side of
// gr_apply_config_change. A gr_peer record becomes an oracle raft object through
// the oracle's own build_peer, the oracle's restatement of raft.addNode /
// addObserver / removeNode / clearPendingConfigChange (raft_oracle.hpp, raft.go:
// 813-901) runs, and the oracle's own export_peer gives the record back. This
// translation unit includes oracle/batch.cpp to reach those two functions; the
// oracle itself is unchanged. Linked with config_change_host.hip into
// tests/_build/libconfig_change_host.so.
//
// The reference keeps members in maps by node id, the record in slots. What
// this file adds is the slot table's side of a change, by the rule of gpuraft.h:
// a removed member's slot becomes empty and keeps its id; a new member takes
// the empty slot that already has its id, else the lowest empty slot that no
// live readStatus (its requester, its confirmed ids) maps to. Statuses:
// GR_CC_HOST exactly when the oracle sent something (r.msgs) or moved committed,
// or where the record cannot say what the reference now holds (a candidate,
// whose tally is by slot; an id in both maps); GR_CC_NO_SLOT from the rule.
#include "batch.cpp"

namespace {

// node id -> slot, members first, then an empty slot that still carries the id
uint32_t slot_any(const OPeer& op, u64 id) {
  const uint32_t s = op.slotOf(id);
  if (s != GR_SLOT_NONE) return s;
  for (size_t j = 0; j < op.ids.size(); ++j)
    if (op.kinds[j] == GR_SLOT_EMPTY && op.ids[j] == id) return (uint32_t)j;
  return GR_SLOT_NONE;
}

uint32_t free_slot(const OPeer& op, u64 id) {
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
    if (op.kinds[j] == GR_SLOT_EMPTY && op.ids[j] == id) return (uint32_t)j;
  for (size_t j = 0; j < op.ids.size(); ++j)
    if (op.kinds[j] == GR_SLOT_EMPTY && !named[j]) return (uint32_t)j;
  return GR_SLOT_NONE;
}

// export_peer maps a readStatus's ids through member slots only; a removed
// node's confirmation still counts in the reference (readindex.go:77-116), and
// the record carries it as the ack bit of the empty slot that keeps its id.
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

int32_t one(gr_peer& g, uint32_t S, u64 maxEntrySize, const gr_config_change& c) {
  if (g.state == GR_CANDIDATE) return GR_CC_HOST;
  OPeer op;
  build_peer(g, S, maxEntrySize, &op);
  raft& r = *op.r;
  const u64 committed0 = r.log->committed, id = c.node_id;
  if (id == 0) {  // peer.go:155-158, RejectConfigChange
    r.clearPendingConfigChange();
  } else if (c.type == GR_CC_REMOVE_NODE) {
    const uint32_t j = op.slotOf(id);
    r.removeNode(id);
    if (j != GR_SLOT_NONE) op.kinds[j] = GR_SLOT_EMPTY;
  } else if (c.type == GR_CC_ADD_NODE) {
    if (r.remotes.count(id)) {
      r.addNode(id);
    } else if (r.observers.count(id)) {
      if (id == r.nodeID && r.electionTimeout == 0) return GR_CC_HOST;  // reset() divides by it
      op.rand.assign(1, c.rand);
      op.randNext = 0;
      r.addNode(id);
      op.kinds[op.slotOf(id)] = GR_SLOT_VOTER;
    } else {
      const uint32_t f = free_slot(op, id);
      if (f == GR_SLOT_NONE) return GR_CC_NO_SLOT;
      r.addNode(id);
      op.ids[f] = id;
      op.kinds[f] = GR_SLOT_VOTER;
    }
  } else {
    if (r.observers.count(id)) {
      r.addObserver(id);
    } else if (r.remotes.count(id)) {
      return GR_CC_HOST;
    } else {
      const uint32_t f = free_slot(op, id);
      if (f == GR_SLOT_NONE) return GR_CC_NO_SLOT;
      r.addObserver(id);
      op.ids[f] = id;
      op.kinds[f] = GR_SLOT_OBSERVER;
    }
  }
  if (!r.msgs.empty() || r.log->committed != committed0) return GR_CC_HOST;
  export_with_removed_acks(op, S, &g);
  return GR_CC_APPLIED;
}

}  // namespace

extern "C" int ccr_apply(uint32_t slots, uint64_t max_entry_size, gr_peer* peers, uint32_t n_peers,
                         const uint32_t* list, const gr_config_change* cc, uint32_t n, int32_t* status) {
  int rc = GR_OK;
  try {
    for (uint32_t x = 0; x < n; ++x) {
      if (list[x] >= n_peers) return GR_ERANGE;
      if (cc[x].type > GR_CC_ADD_OBSERVER) return GR_EINVAL;
      const int32_t s = one(peers[list[x]], slots, max_entry_size, cc[x]);
      if (status) status[x] = s;
      if (s) rc = GR_ESTATE;
    }
  } catch (const std::exception&) {
    return -100;  // the oracle panicked
  }
  return rc;
}

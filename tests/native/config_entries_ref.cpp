// config_entries_ref.cpp — TEST INFRASTRUCTURE: the reference side of
// config-change entries on the device (gpuraft.h gr_set_config_entries). The
// batch oracle strips entry types; here a gr_peer record and the group's
// gr_cc_index record become an oracle raft object (the oracle's own build_peer)
// whose in-memory entries at the recorded indexes are typed ConfigChangeEntry, a
// marked Replicate record expands into typed entries, and the pass's items run
// through the oracle's Handle / tick / propose in the engine's item order, as
// ob_step2 runs them. Outgoing marks and the record after the pass are derived
// from the oracle's typed log: the two highest ConfigChangeEntry indexes above
// committed. Peers must keep every uncommitted entry in memory (marker_index set,
// at or below committed + 1), or their types would be lost in the typeless
// LogDB stand-in. This translation unit includes oracle/batch.cpp to reach its
// functions; the oracle itself is unchanged. Linked with hostlane_cc.hip into
// tests/_build/libhostlane_cc*.so.
#include "batch.cpp"

namespace {

void type_entry(raft& r, u64 index) {
  inMemory& im = r.log->inmem;
  if (index < im.markerIndex || index >= im.markerIndex + im.entries.size())
    throw std::runtime_error("a config-change index outside the in-memory log");
  im.entries[index - im.markerIndex].Type = ConfigChangeEntry;
}

// gr_message -> raftpb.Message, a marked Replicate by the convention
Message expand(const OPeer& op, const gr_message& g) {
  Message m = from_record(op, g);
  if (m.Type != Replicate || !g.reject) return m;
  m.Reject = false;
  m.Hint = 0;
  m.HintHigh = 0;
  for (u64 idx : {g.hint, g.hint_high}) {
    if (idx == 0) continue;
    if (idx <= g.log_index || idx > g.log_index + g.n_entries) throw std::runtime_error("a mark outside the message");
    m.Entries[idx - g.log_index - 1].Type = ConfigChangeEntry;
  }
  return m;
}

// raftpb.Message -> gr_message, a Replicate's marks from its entries' types
// (those at or below its Commit are left out, as a leader leaves them out)
bool contract(const OPeer& op, uint32_t peer, const Message& m, gr_message* o) {
  bool ok = to_record(op, peer, m, o);
  if (m.Type != Replicate) return ok;
  u64 a = 0, b = 0;
  for (const Entry& e : m.Entries) {
    if (e.Type != ConfigChangeEntry || e.Index <= m.Commit) continue;
    if (b) ok = false;  // a third one: two marks cannot say
    b = a;
    a = e.Index;
  }
  if (a) {
    o->reject = 1;
    o->hint = a;
    o->hint_high = b;
  }
  return ok;
}

struct PassOut {
  std::vector<gr_message> msgs;
  gr_peer_result res;
  int panic_item = -1;
  std::string what;
};

// One peer's pass: items below `limit` in the engine's order.
void run_peer(OPeer& op, uint32_t pi, const std::vector<const gr_message*>& ms, const gr_local_input* L,
              uint32_t limit, PassOut* po) {
  raft& r = *op.r;
  r.msgs.clear();
  r.readyToRead.clear();
  op.appendFrom = 0;
  op.rand.assign(1, L ? L->rand : 0);
  op.randNext = 0;
  memset(&po->res, 0, sizeof(po->res));
  po->res.peer = pi;
  uint32_t item = 0;
  auto flush = [&]() {
    for (auto& m : r.msgs) {
      gr_message rec;
      if (!contract(op, pi, m, &rec)) throw std::runtime_error("message not representable as a gr_message record");
      po->msgs.push_back(rec);
    }
    r.msgs.clear();
  };
  try {
    for (const gr_message* gm : ms) {
      if (item == limit) break;
      Message m = expand(op, *gm);
      const u64 before = r.log->lastIndex();
      const bool member = op.kinds[gm->slot] != GR_SLOT_EMPTY;
      if (member || !isResponseMessageType(m.Type)) r.Handle(m);  // Peer.Handle (peer.go:199-209)
      if (m.Type == Propose && r.log->lastIndex() > before) {
        if (!po->res.propose_first) po->res.propose_first = before + 1;
        po->res.n_forwarded++;
        po->res.forwarded_entries += (uint32_t)m.Entries.size();
      }
      flush();
      item++;
    }
    if (L && item != limit) {
      if (L->read_index) {
        Message m;
        m.Type = ReadIndex;
        m.Hint = L->read_ctx_low;
        m.HintHigh = L->read_ctx_high;
        r.Handle(m);
        flush();
        item++;
      }
      for (uint32_t k = 0; k < L->ticks && item != limit; ++k) {
        r.tick();
        flush();
        item++;
      }
      if (L->quiesced_ticks && item != limit) {
        for (uint32_t k = 0; k < L->quiesced_ticks; ++k) r.quiescedTick();
        item++;
      }
      if (L->propose_entries && item != limit) {
        const u64 before = r.log->lastIndex();
        std::vector<Entry> es(L->propose_entries);
        const size_t payload = op.entryUB >= 128 ? (size_t)(op.entryUB - 128) : 0;
        for (auto& e : es) e.Cmd.assign(payload, 0);
        if (L->propose_has_config_change) es[0].Type = ConfigChangeEntry;
        Message m;
        m.Type = Propose;
        m.From = r.nodeID;
        m.Entries = es;
        r.Handle(m);
        bool fwd = false;
        for (auto& x : r.msgs) fwd = fwd || x.Type == Propose;
        flush();
        if (r.log->lastIndex() > before) {
          po->res.propose_result = GR_PROP_APPENDED;
          if (!po->res.propose_first) po->res.propose_first = before + 1;
        } else {
          po->res.propose_result = fwd ? GR_PROP_FORWARDED : GR_PROP_DROPPED;
        }
        item++;
      }
    }
  } catch (const std::exception& ex) {
    po->panic_item = (int)item;
    po->what = ex.what();
    r.msgs.clear();
  }
  gr_peer_result& res = po->res;
  res.n_ready = (uint8_t)std::min<size_t>(r.readyToRead.size(), 255);
  for (size_t q = 0; q < r.readyToRead.size() && q < GR_Q; ++q) {
    res.ready[q].index = r.readyToRead[q].Index;
    res.ready[q].ctx_low = r.readyToRead[q].ctx.Low;
    res.ready[q].ctx_high = r.readyToRead[q].ctx.High;
  }
  res.append_from = op.appendFrom;
  res.committed = r.log->committed;
  res.last_index = r.log->lastIndex();
  auto es = r.log->entriesToSave();
  res.save_from = es.empty() ? 0 : es.front().Index;
  res.term = r.term;
  res.vote = r.vote;
}

}  // namespace

// One pass over records. peers[p] / cc[p] are read and, for every peer with
// input, written back as the state after the items below limits[p] (NULL: all
// items); cc[p] then holds the two highest ConfigChangeEntry indexes above
// committed in the oracle's log. Results come one per peer with input, in peer
// order; messages in peer, then item order. panic_item[p] (may be NULL) is the
// item at which the oracle panicked, or -1.
extern "C" int ccr_step(uint32_t slots, uint64_t max_entry_size, gr_peer* peers, uint32_t n_peers, const gr_inbox* in,
                        const uint32_t* limits, gr_cc_index* cc, gr_message* out, size_t out_cap, size_t* n_out,
                        gr_peer_result* results, size_t* n_results, int32_t* panic_item) {
  if (!in || !n_out || !n_results || !cc) return GR_EINVAL;
  const uint32_t S = slots;
  std::vector<std::vector<const gr_message*>> by((size_t)n_peers * S);
  std::vector<uint8_t> has(n_peers, 0);
  std::vector<const gr_local_input*> loc(n_peers, nullptr);
  for (size_t k = 0; k < in->n_msgs; ++k) {
    const gr_message& m = in->msgs[k];
    if (m.peer >= n_peers || m.slot >= S) return GR_EINVAL;
    by[(size_t)m.peer * S + m.slot].push_back(&m);
    has[m.peer] = 1;
  }
  for (size_t k = 0; k < in->n_locals; ++k) {
    if (in->locals[k].peer >= n_peers) return GR_EINVAL;
    loc[in->locals[k].peer] = &in->locals[k];
    has[in->locals[k].peer] = 1;
  }
  size_t no = 0, nr = 0;
  int rc = GR_OK;
  for (uint32_t pi = 0; pi < n_peers; ++pi) {
    if (panic_item) panic_item[pi] = -1;
    if (!has[pi]) continue;
    OPeer op;
    PassOut po;
    try {
      const gr_peer& g = peers[pi];
      // every uncommitted entry must be in memory, where it keeps its type
      if (g.committed < g.last_index && (g.marker_index == 0 || g.marker_index > g.committed + 1)) return GR_ESTATE;
      build_peer(g, S, max_entry_size, &op);
      for (u64 idx : {cc[pi].last, cc[pi].prev})
        if (idx > g.committed) type_entry(*op.r, idx);
      // build_peer leaves raft.votes empty: a candidate's tally from the record,
      // its own vote included as a load includes it (gpuraft.h gr_peer.votes_granted)
      if (g.state == GR_CANDIDATE) {
        op.r->votes[g.node_id] = true;
        for (uint32_t j = 0; j < S; ++j) {
          if (g.votes_granted & (1u << j)) op.r->votes[g.remote_id[j]] = true;
          if (g.votes_rejected & (1u << j)) op.r->votes[g.remote_id[j]] = false;
        }
      }
    } catch (const std::exception&) {
      return GR_ESTATE;
    }
    std::vector<const gr_message*> ms;
    for (uint32_t j = 0; j < S; ++j)
      for (const gr_message* m : by[(size_t)pi * S + j]) ms.push_back(m);
    run_peer(op, pi, ms, loc[pi], limits ? limits[pi] : 0xFFFFFFFFu, &po);
    if (po.panic_item >= 0) {
      if (panic_item) panic_item[pi] = po.panic_item;
      else rc = GR_ESTATE;
    }
    export_peer(op, S, &peers[pi]);
    gr_cc_index rec = {0, 0};
    for (const Entry& e : op.r->log->inmem.entries) {
      if (e.Type != ConfigChangeEntry || e.Index <= op.r->log->committed) continue;
      rec.prev = rec.last;
      rec.last = e.Index;
    }
    cc[pi] = rec;
    for (auto& m : po.msgs) {
      if (out && no < out_cap) out[no] = m;
      no++;
    }
    if (results) results[nr] = po.res;
    nr++;
  }
  *n_out = no;
  *n_results = nr;
  if (no > out_cap) return GR_ECAPACITY;
  return rc;
}

// The host persists and applies everything a pass left (the oracle's
// commit_peer: entriesToSave -> LogDB, StableLogTo, AppliedTo = committed,
// NotifyRaftLastApplied) on every record; the in-memory marker then stands at
// the applied index, so the uncommitted entries stay in memory.
extern "C" int ccr_commit_all(uint32_t slots, uint64_t max_entry_size, gr_peer* peers, uint32_t n_peers) {
  try {
    for (uint32_t pi = 0; pi < n_peers; ++pi) {
      OPeer op;
      build_peer(peers[pi], slots, max_entry_size, &op);
      commit_peer(op);
      export_peer(op, slots, &peers[pi]);
    }
  } catch (const std::exception&) {
    return GR_ESTATE;
  }
  return GR_OK;
}

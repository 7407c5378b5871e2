// ref_pass.h — TEST INFRASTRUCTURE: what the reference sides of the device
// switches share (snapshot_ref.cpp, config_entries_ref.cpp,
// all_switches_ref.cpp). Included after oracle/batch.cpp, whose build_peer /
// export_peer / from_record / to_record it drives. One peer's pass runs through
// the oracle's Handle / tick / propose in the engine's item order, as ob_step2
// runs them, with the propose bookkeeping of a gr_peer_result and the oracle's
// panic captured with the item it struck. The message conventions differ per
// switch, so the caller passes its own expand (gr_message -> raftpb.Message) and
// contract (raftpb.Message -> gr_message).
#pragma once

namespace refpass {

struct PassOut {
  std::vector<gr_message> msgs;
  std::vector<gr_restored> restored;  // one per InstallSnapshot that restored, in item order
  gr_peer_result res;
  int panic_item = -1;  // the item at which the oracle panicked, or -1
  std::string what;
};

// Items below `limit`: the messages in `ms` (already in slot, then arrival
// order), then ReadIndex, the ticks, the quiesced ticks as one item, the proposal.
template <class Expand, class Contract>
void run_peer(OPeer& op, uint32_t pi, const std::vector<const gr_message*>& ms, const gr_local_input* L,
              uint32_t limit, PassOut* po, Expand expand, Contract contract) {
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
      const u64 snap0 = r.log->inmem.snapshot ? r.log->inmem.snapshot->Index : 0;
      const bool member = op.kinds[gm->slot] != GR_SLOT_EMPTY;
      if (member || !isResponseMessageType(m.Type)) r.Handle(m);  // Peer.Handle (peer.go:199-209)
      if (m.Type == InstallSnapshot && r.log->inmem.snapshot && r.log->inmem.snapshot->Index != snap0) {
        gr_restored rr;
        memset(&rr, 0, sizeof(rr));
        rr.peer = pi;
        rr.index = r.log->inmem.snapshot->Index;
        rr.term = r.log->inmem.snapshot->Term;
        po->restored.push_back(rr);
      }
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

// The inbox sorted as the engine reads it: per peer, the messages by sender
// slot, then arrival order; the peer's local input; whether it has any input.
struct Sorted {
  std::vector<std::vector<const gr_message*>> by;  // [peer * S + slot]
  std::vector<uint8_t> has;
  std::vector<const gr_local_input*> loc;
  uint32_t S = 0;
  std::vector<const gr_message*> of(uint32_t pi) const {
    std::vector<const gr_message*> ms;
    for (uint32_t j = 0; j < S; ++j)
      for (const gr_message* m : by[(size_t)pi * S + j]) ms.push_back(m);
    return ms;
  }
};

inline int sort_inbox(const gr_inbox* in, uint32_t S, uint32_t n_peers, Sorted* so) {
  so->S = S;
  so->by.assign((size_t)n_peers * S, {});
  so->has.assign(n_peers, 0);
  so->loc.assign(n_peers, nullptr);
  for (size_t k = 0; k < in->n_msgs; ++k) {
    const gr_message& m = in->msgs[k];
    if (m.peer >= n_peers || m.slot >= S) return GR_EINVAL;
    so->by[(size_t)m.peer * S + m.slot].push_back(&m);
    so->has[m.peer] = 1;
  }
  for (size_t k = 0; k < in->n_locals; ++k) {
    if (in->locals[k].peer >= n_peers) return GR_EINVAL;
    so->loc[in->locals[k].peer] = &in->locals[k];
    so->has[in->locals[k].peer] = 1;
  }
  return GR_OK;
}

// gpuraft.h's InstallSnapshot convention: Snapshot.Index / Snapshot.Term travel
// in log_index / log_term, and an inbound one with reject set names the receiver
// in Snapshot.Membership.Observers.
inline void expand_install(const OPeer& op, const gr_message& g, Message* m) {
  m->snapshot.Index = g.log_index;
  m->snapshot.Term = g.log_term;
  if (g.reject) m->snapshot.membership.Observers[op.r->nodeID] = "";
  m->LogIndex = 0;
  m->LogTerm = 0;
  m->Commit = 0;
  m->Reject = false;
}
inline void contract_install(const Message& m, gr_message* o) {
  o->log_index = m.snapshot.Index;
  o->log_term = m.snapshot.Term;
}

// gpuraft.h's marked-Replicate convention: reject = 1, the two highest
// config-change indexes among the entries in hint / hint_high.
inline void expand_marks(const gr_message& g, Message* m) {
  m->Reject = false;
  m->Hint = 0;
  m->HintHigh = 0;
  for (u64 idx : {g.hint, g.hint_high}) {
    if (idx == 0) continue;
    if (idx <= g.log_index || idx > g.log_index + g.n_entries) throw std::runtime_error("a mark outside the message");
    m->Entries[idx - g.log_index - 1].Type = ConfigChangeEntry;
  }
}
// A Replicate's marks from its entries' types (those at or below its Commit are
// left out, as a leader leaves them out); false when two marks cannot say.
inline bool contract_marks(const Message& m, gr_message* o) {
  bool ok = true;
  u64 a = 0, b = 0;
  for (const Entry& e : m.Entries) {
    if (e.Type != ConfigChangeEntry || e.Index <= m.Commit) continue;
    if (b) ok = false;  // a third one
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

// The typed in-memory log: the entry at `index` becomes a ConfigChangeEntry.
inline void type_entry(raft& r, u64 index) {
  inMemory& im = r.log->inmem;
  if (index < im.markerIndex || index >= im.markerIndex + im.entries.size())
    throw std::runtime_error("a config-change index outside the in-memory log");
  im.entries[index - im.markerIndex].Type = ConfigChangeEntry;
}
// The gr_cc_index record of the typed log: the two highest ConfigChangeEntry
// indexes above committed.
inline gr_cc_index cc_record(const raft& r) {
  gr_cc_index rec = {0, 0};
  for (const Entry& e : r.log->inmem.entries) {
    if (e.Type != ConfigChangeEntry || e.Index <= r.log->committed) continue;
    rec.prev = rec.last;
    rec.last = e.Index;
  }
  return rec;
}
// build_peer leaves raft.votes empty: a candidate's tally from the record, its
// own vote included as a load includes it (gpuraft.h gr_peer.votes_granted).
inline void candidate_votes(const gr_peer& g, uint32_t S, raft& r) {
  if (g.state != GR_CANDIDATE) return;
  r.votes[g.node_id] = true;
  for (uint32_t j = 0; j < S; ++j) {
    if (g.votes_granted & (1u << j)) r.votes[g.remote_id[j]] = true;
    if (g.votes_rejected & (1u << j)) r.votes[g.remote_id[j]] = false;
  }
}

}  // namespace refpass

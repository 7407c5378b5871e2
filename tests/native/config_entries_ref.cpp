// config_entries_ref.cpp — TEST INFRASTRUCTURE: the reference side of
// config-change entries on the device (gpuraft.h gr_set_config_entries). The
// batch oracle strips entry types; here a gr_peer record and the group's
// gr_cc_index record become an oracle raft object (the oracle's own build_peer)
// whose in-memory entries at the recorded indexes are typed ConfigChangeEntry, a
// marked Replicate record expands into typed entries, and the pass's items run
// through the oracle's Handle / tick / propose in the engine's item order, as
// ob_step2 runs them (ref_pass.h, shared with the other reference sides). Outgoing marks and the record after the pass are derived
// from the oracle's typed log: the two highest ConfigChangeEntry indexes above
// committed. Peers must keep every uncommitted entry in memory (marker_index set,
// at or below committed + 1), or their types would be lost in the typeless
// LogDB stand-in. This translation unit includes oracle/batch.cpp to reach its
// functions; the oracle itself is unchanged. Linked with hostlane_cc.hip into
// tests/_build/libhostlane_cc*.so.
#include "batch.cpp"
#include "ref_pass.h"

namespace {

// gr_message -> raftpb.Message, a marked Replicate by the convention
Message expand(const OPeer& op, const gr_message& g) {
  Message m = from_record(op, g);
  if (m.Type == Replicate && g.reject) refpass::expand_marks(g, &m);
  return m;
}

// raftpb.Message -> gr_message, a Replicate's marks from its entries' types
bool contract(const OPeer& op, uint32_t peer, const Message& m, gr_message* o) {
  const bool ok = to_record(op, peer, m, o);
  if (m.Type != Replicate) return ok;
  return refpass::contract_marks(m, o) && ok;
}

using refpass::PassOut;

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
  refpass::Sorted so;
  if (refpass::sort_inbox(in, S, n_peers, &so)) return GR_EINVAL;
  size_t no = 0, nr = 0;
  int rc = GR_OK;
  for (uint32_t pi = 0; pi < n_peers; ++pi) {
    if (panic_item) panic_item[pi] = -1;
    if (!so.has[pi]) continue;
    OPeer op;
    PassOut po;
    try {
      const gr_peer& g = peers[pi];
      // every uncommitted entry must be in memory, where it keeps its type
      if (g.committed < g.last_index && (g.marker_index == 0 || g.marker_index > g.committed + 1)) return GR_ESTATE;
      build_peer(g, S, max_entry_size, &op);
      for (u64 idx : {cc[pi].last, cc[pi].prev})
        if (idx > g.committed) refpass::type_entry(*op.r, idx);
      refpass::candidate_votes(g, S, *op.r);
    } catch (const std::exception&) {
      return GR_ESTATE;
    }
    refpass::run_peer(op, pi, so.of(pi), so.loc[pi], limits ? limits[pi] : 0xFFFFFFFFu, &po, expand, contract);
    if (po.panic_item >= 0) {
      if (panic_item) panic_item[pi] = po.panic_item;
      else rc = GR_ESTATE;
    }
    export_peer(op, S, &peers[pi]);
    cc[pi] = refpass::cc_record(*op.r);
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

// all_switches_ref.cpp — TEST INFRASTRUCTURE: the reference side of a pass with
// every device switch on at once (elections, snapshots, config-change entries).
// A gr_peer record, the group's snapshot record and its gr_cc_index record
// become an oracle raft object through the oracle's own build_peer:
// RunLogDB::snap is what LogReader.Snapshot() returns, and the in-memory entries
// at the recorded indexes are typed ConfigChangeEntry. The pass's items run
// through the oracle's Handle / tick / propose in the engine's item order
// (ref_pass.h), and both message conventions of gpuraft.h hold at once: an
// InstallSnapshot record carries Snapshot.Index / Snapshot.Term in log_index /
// log_term with reject naming the receiver as an observer, and a Replicate with
// reject = 1 carries its marks in hint / hint_high. After the pass the snapshot
// record, the restored list, the outgoing marks and the gr_cc_index record are
// exported from the oracle's own state; the record is derived from the typed
// log, the two highest config-change indexes above committed, so a restore that
// discards typed entries shows in it. Peers must keep every uncommitted entry in
// memory (marker_index set, at or below committed + 1), or their types would be
// lost in the typeless LogDB stand-in; a restore keeps that (it leaves
// marker_index = index + 1). This translation unit includes oracle/batch.cpp to
// reach its functions; the oracle itself is unchanged. Linked with
// hostlane_all.hip into tests/_build/libhostlane_all.so.
#include "batch.cpp"
#include "ref_pass.h"

namespace {

Message expand(const OPeer& op, const gr_message& g) {
  Message m = from_record(op, g);
  if (m.Type == InstallSnapshot) refpass::expand_install(op, g, &m);
  else if (m.Type == Replicate && g.reject) refpass::expand_marks(g, &m);
  return m;
}

bool contract(const OPeer& op, uint32_t peer, const Message& m, gr_message* o) {
  const bool ok = to_record(op, peer, m, o);
  if (m.Type == InstallSnapshot) refpass::contract_install(m, o);
  if (m.Type == Replicate) return refpass::contract_marks(m, o) && ok;
  return ok;
}

}  // namespace

// One pass over records. peers[p] / snap[p] / cc[p] are read and, for every peer
// with input, written back as the state after the items below limits[p] (NULL:
// all items). Results come one per peer with input, in peer order; messages in
// peer, then item order; `restored` as gr_restored_snapshots lists them.
// panic_item[p] (may be NULL) is the item at which the oracle panicked, or -1.
extern "C" int asr_step(uint32_t slots, uint64_t max_entry_size, gr_peer* peers, uint32_t n_peers, const gr_inbox* in,
                        const uint32_t* limits, gr_snapshot_rec* snap, gr_cc_index* cc, gr_message* out,
                        size_t out_cap, size_t* n_out, gr_peer_result* results, size_t* n_results,
                        gr_restored* restored, size_t restored_cap, size_t* n_restored, int32_t* panic_item) {
  if (!in || !n_out || !n_results || !n_restored || !snap || !cc) return GR_EINVAL;
  const uint32_t S = slots;
  refpass::Sorted so;
  if (refpass::sort_inbox(in, S, n_peers, &so)) return GR_EINVAL;
  size_t no = 0, nr = 0, ns = 0;
  int rc = GR_OK;
  for (uint32_t pi = 0; pi < n_peers; ++pi) {
    if (panic_item) panic_item[pi] = -1;
    if (!so.has[pi]) continue;
    OPeer op;
    refpass::PassOut po;
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
    cc[pi] = refpass::cc_record(*op.r);
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

// hostlane_all.hip — TEST ONLY. The host lane (hostlane.hip, included unchanged
// through hostlane_snap.hip, which also brings hl_restore_remotes and the
// snapshot coverage table) built with -DGR_ELECTIONS_FORCE=1
// -DGR_SNAPSHOTS_FORCE=1 -DGR_CONFIG_ENTRIES_FORCE=1: every device switch on at
// once, as a deployment runs them. Its entry point passes what such a pass needs
// beside the records: the groups' snapshot records and the restored list
// (gr_layout.h snap_host_hook) and the groups' gr_cc_index records
// (cc_host_hook); hl_step zeroes its StepParams, so the side arrays reach the
// lane through the hooks. Linked with all_switches_ref.cpp (the reference side)
// into tests/_build/libhostlane_all.so.
#include "hostlane_snap.hip"

// hl_step with every side array: snap[p] and cc[p] are peer p's records, read
// and written by the lanes of the run that stands; `restored` receives the
// pass's gr_restored records, *n_restored of them (GR_ECAPACITY when more than
// restored_cap were appended). cc_stage (may be NULL), n_peers records: the cc
// staging records as the pass left them, for tests that look at them.
extern "C" int hl_step_all(uint32_t slots, uint64_t max_entry_size, gr_peer* peers, uint32_t n_peers,
                           const gr_inbox* in, gr_message* out_msgs, size_t out_cap, size_t* n_out,
                           gr_peer_result* results, size_t* n_results, gr_snapshot_rec* snap, gr_restored* restored,
                           size_t restored_cap, size_t* n_restored, gr_cc_index* cc, gr_cc_index* cc_stage) {
  if (!cc) return GR_EINVAL;
  std::vector<gr_cc_index> stage((size_t)std::max<uint32_t>(n_peers, 1));
  // a pattern no index can equal: a lane that read its staging record before
  // copying the group's record into it would show
  for (auto& s : stage) s.last = s.prev = 0xDEADDEADDEADDEADull;
  cc_host_hook.cc_rec = cc;
  cc_host_hook.cc_stage = stage.data();
  const int r = hl_step_snap(slots, max_entry_size, peers, n_peers, in, out_msgs, out_cap, n_out, results, n_results,
                             snap, restored, restored_cap, n_restored);
  cc_host_hook = CcHostHook{nullptr, nullptr};
  if (cc_stage) memcpy(cc_stage, stage.data(), (size_t)n_peers * sizeof(gr_cc_index));
  return r;
}

// per-branch hit counts of the config-change-entry handlers (gr_cover.h GR_COVER_CC_IDS)
extern "C" int hl_coverage_cc(uint64_t* out, uint32_t n) {
  if (!out || n < CC_N) return -1;
  for (uint32_t k = 0; k < CC_N; ++k) out[k] = gr_cover_cc_host[k];
  return (int)CC_N;
}
extern "C" const char* hl_coverage_cc_names() {
#define GR_COVER_NAME(x) #x ","
  return GR_COVER_CC_IDS(GR_COVER_NAME);
#undef GR_COVER_NAME
}

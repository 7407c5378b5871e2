// hostlane_cc.hip — TEST ONLY. The host lane (hostlane.hip, included unchanged)
// built with -DGR_CONFIG_ENTRIES_FORCE=1, plus an entry point that passes what a
// pass with config-change entries needs beside the records: the groups'
// gr_cc_index records (gr_layout.h cc_host_hook; hl_step zeroes its StepParams,
// so the side arrays reach the lane through the hook). A second build adds
// -DGR_ELECTIONS_FORCE=1 for promotions. Linked with config_entries_ref.cpp (the
// reference side) into tests/_build/libhostlane_cc*.so.
#include "hostlane.hip"

// hl_step with the config-change index records: cc[p] is peer p's record, read
// and written by the lanes of the run that stands.
extern "C" int hl_step_cc(uint32_t slots, uint64_t max_entry_size, gr_peer* peers, uint32_t n_peers,
                          const gr_inbox* in, gr_message* out_msgs, size_t out_cap, size_t* n_out,
                          gr_peer_result* results, size_t* n_results, gr_cc_index* cc) {
  if (!cc) return GR_EINVAL;
  std::vector<gr_cc_index> stage((size_t)std::max<uint32_t>(n_peers, 1));
  // a pattern no index can equal: a lane that read its staging record before
  // copying the group's record into it would show
  for (auto& s : stage) s.last = s.prev = 0xDEADDEADDEADDEADull;
  cc_host_hook.cc_rec = cc;
  cc_host_hook.cc_stage = stage.data();
  const int r = hl_step(slots, max_entry_size, peers, n_peers, in, out_msgs, out_cap, n_out, results, n_results);
  cc_host_hook = CcHostHook{nullptr, nullptr};
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

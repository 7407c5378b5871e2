// hostlane_snap.hip — TEST ONLY. The host lane (hostlane.hip, included
// unchanged) built with -DGR_SNAPSHOTS_FORCE=1, plus an entry point that passes
// what a snapshot pass needs beside the records: the groups' snapshot records
// and the restored list (gr_layout.h snap_host_hook; hl_step zeroes its
// StepParams, so the side arrays reach the lane through the hook). A second
// build adds -DGR_ELECTIONS_FORCE=1 for the candidate's handler. Also here:
// gr_restore_remotes on records (gr_config_change.h restore_rows over one tile
// of state rows, as config_change_host.hip runs apply_rows). Linked with
// snapshot_ref.cpp (the reference side) into tests/_build/libhostlane_snap*.so.
#include "hostlane.hip"

#include "gr_config_change.h"

// hl_step with the snapshot side arrays: snap[p] is peer p's snapshot record
// (read by a leader's send, written by a restore); `restored` receives the
// pass's gr_restored records, *n_restored of them (GR_ECAPACITY when more than
// restored_cap were appended: the list's overflow flag).
extern "C" int hl_step_snap(uint32_t slots, uint64_t max_entry_size, gr_peer* peers, uint32_t n_peers,
                            const gr_inbox* in, gr_message* out_msgs, size_t out_cap, size_t* n_out,
                            gr_peer_result* results, size_t* n_results, gr_snapshot_rec* snap, gr_restored* restored,
                            size_t restored_cap, size_t* n_restored) {
  if (!snap || !n_restored || (restored_cap && !restored)) return GR_EINVAL;
  uint32_t hdr[2] = {0, 0};
  std::vector<gr_snapshot_rec> stage((size_t)n_peers * kRestStage);
  snap_host_hook.snap_rec = snap;
  snap_host_hook.rest_stage = stage.data();
  snap_host_hook.rest_hdr = hdr;
  snap_host_hook.rest = restored;
  snap_host_hook.rest_cap = (uint32_t)restored_cap;
  const int r = hl_step(slots, max_entry_size, peers, n_peers, in, out_msgs, out_cap, n_out, results, n_results);
  snap_host_hook = SnapHostHook{nullptr, nullptr, nullptr, nullptr, 0};
  *n_restored = std::min<size_t>(hdr[0], restored_cap);
  if (r) return r;
  return hdr[1] ? GR_ECAPACITY : GR_OK;
}

// per-branch hit counts of the snapshot handlers (gr_cover.h GR_COVER_SNAP_IDS)
extern "C" int hl_coverage_snap(uint64_t* out, uint32_t n) {
  if (!out || n < CS_N) return -1;
  for (uint32_t k = 0; k < CS_N; ++k) out[k] = gr_cover_snap_host[k];
  return (int)CS_N;
}
extern "C" const char* hl_coverage_snap_names() {
#define GR_COVER_NAME(x) #x ","
  return GR_COVER_SNAP_IDS(GR_COVER_NAME);
#undef GR_COVER_NAME
}

namespace {

template <int S>
int32_t restore_one(gr_peer& g, const gr_membership& m) {
  StateBase st;
  st.cap = pad_cap(1);  // one tile, written as a load writes it
  st.S = S;
  std::vector<uint64_t> buf((state_bytes(S, st.cap) + 7) / 8, 0);
  st.base = (uint8_t*)buf.data();
  for (uint32_t r = 0; r < rows_u64(S); ++r) st.u64(r)[0] = get_u64_row(g, r, S);
  for (uint32_t r = 0; r < rows_u8(S); ++r) st.u8(r)[0] = get_u8_row(g, r, S);
  const std::vector<uint64_t> before = buf;
  const int32_t rc = conf::restore_rows<S>(st, 0, m);
  if (rc != GR_CC_APPLIED) return buf == before ? rc : -100;  // a refused peer had a row written
  gr_peer o;
  memset(&o, 0, sizeof(o));
  for (uint32_t r = 0; r < rows_u64(S); ++r) set_u64_row(o, r, S, st.u64(r)[0]);
  resolve_sync(o, S, st.u64(SR_HDR)[0]);
  for (uint32_t r = 0; r < rows_u8(S); ++r) set_u8_row(o, r, S, st.u8(r)[0]);
  g = o;
  return rc;
}

}  // namespace

// gr_restore_remotes on records: the same refusals, statuses and return codes.
extern "C" int hl_restore_remotes(uint32_t slots, gr_peer* peers, uint32_t n_peers, const uint32_t* list,
                                  const gr_membership* ms, uint32_t n, int32_t* status) {
  if (slots != 1 && slots != 3 && slots != 5 && slots != 8) return GR_EINVAL;
  std::vector<uint8_t> seen(n_peers, 0);
  for (uint32_t x = 0; x < n; ++x) {
    if (list[x] >= n_peers || seen[list[x]]) return GR_ERANGE;
    seen[list[x]] = 1;
  }
  for (uint32_t x = 0; x < n; ++x)
    if (!conf::known_kinds(ms[x])) return GR_EINVAL;
  int rc = GR_OK;
  for (uint32_t x = 0; x < n; ++x) {
    gr_peer& g = peers[list[x]];
    const int32_t s = slots == 1 ? restore_one<1>(g, ms[x]) : slots == 3 ? restore_one<3>(g, ms[x])
                    : slots == 5 ? restore_one<5>(g, ms[x]) : restore_one<8>(g, ms[x]);
    if (status) status[x] = s;
    if (s) rc = GR_ESTATE;
  }
  return rc;
}

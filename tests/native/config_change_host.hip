// config_change_host.hip — TEST INFRASTRUCTURE: gr_config_change.h (what
// gr_apply_config_change runs on the device) compiled for the host over gr_peer
// records, as hostlane.hip's hl_commit_update does for commit updates. Each
// record is laid out as one tile of state rows (the load path, so a leader's
// header carries its sync bits), changed by conf::apply_rows, and read back as
// gr_sync_peers_to_host reads it. Linked with config_change_ref.cpp (the
// reference side) into tests/_build/libconfig_change_host.so.
#include <cstring>
#include <vector>

#include "gr_config_change.h"

using namespace gr;

namespace {

// One record as one tile of state rows, written as a load writes them.
struct Tile {
  StateBase st;
  std::vector<uint64_t> buf;
  Tile(const gr_peer& g, int S) {
    st.cap = pad_cap(1);
    st.S = S;
    buf.assign((state_bytes(S, st.cap) + 7) / 8, 0);
    st.base = (uint8_t*)buf.data();
    for (uint32_t r = 0; r < rows_u64(S); ++r) st.u64(r)[0] = host::get_u64_row(g, r, S);
    for (uint32_t r = 0; r < rows_u8(S); ++r) st.u8(r)[0] = host::get_u8_row(g, r, S);
  }
};

template <int S>
int32_t one(gr_peer& g, const gr_config_change& c) {
  Tile t(g, S);
  StateBase& st = t.st;
  const std::vector<uint64_t> before = t.buf;
  const int32_t rc = conf::apply_rows<S>(st, 0, c);
  if (rc != GR_CC_APPLIED) return t.buf == before ? rc : -100;  // a refused change wrote a row
  gr_peer o;
  memset(&o, 0, sizeof(o));
  for (uint32_t r = 0; r < rows_u64(S); ++r) host::set_u64_row(o, r, S, st.u64(r)[0]);
  host::resolve_sync(o, S, st.u64(SR_HDR)[0]);
  for (uint32_t r = 0; r < rows_u8(S); ++r) host::set_u8_row(o, r, S, st.u8(r)[0]);
  g = o;
  return rc;
}

}  // namespace

// gr_apply_config_change on records: the same refusals, statuses and return codes.
extern "C" int cch_apply(uint32_t slots, gr_peer* peers, uint32_t n_peers, const uint32_t* list,
                         const gr_config_change* cc, uint32_t n, int32_t* status) {
  if (slots != 1 && slots != 3 && slots != 5 && slots != 8) return GR_EINVAL;
  std::vector<uint8_t> seen(n_peers, 0);
  for (uint32_t x = 0; x < n; ++x) {
    if (list[x] >= n_peers || seen[list[x]]) return GR_ERANGE;
    seen[list[x]] = 1;
  }
  for (uint32_t x = 0; x < n; ++x)
    if (!conf::known_type(cc[x].type)) return GR_EINVAL;
  int rc = GR_OK;
  for (uint32_t x = 0; x < n; ++x) {
    gr_peer& g = peers[list[x]];
    const int32_t s = slots == 1 ? one<1>(g, cc[x]) : slots == 3 ? one<3>(g, cc[x])
                    : slots == 5 ? one<5>(g, cc[x]) : one<8>(g, cc[x]);
    if (status) status[x] = s;
    if (s) rc = GR_ESTATE;
  }
  return rc;
}

// The header word a change leaves (device bits included), for tests of the
// summaries: *before as a load writes it, *after as apply_rows leaves it.
extern "C" int cch_headers(uint32_t slots, const gr_peer* peer, const gr_config_change* cc, uint64_t* before,
                           uint64_t* after) {
  if (slots != 3 && slots != 5) return GR_EINVAL;
  Tile t(*peer, (int)slots);
  StateBase& st = t.st;
  *before = st.u64(SR_HDR)[0];
  const int32_t rc = slots == 3 ? conf::apply_rows<3>(st, 0, *cc) : conf::apply_rows<5>(st, 0, *cc);
  *after = st.u64(SR_HDR)[0];
  return rc;
}

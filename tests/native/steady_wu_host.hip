// steady_wu_host.hip — TEST ONLY. The host build of the steady kernel's
// wave-uniform addressing (gr_steady.h WaveAddr) and of the predicate that
// selects it (gr_layout.h steady_wu_routes / steady_wu_space), behind a C
// interface for tests/test_steady_wu.py. It computes addresses over made-up
// base pointers and never dereferences one; it never touches the HIP runtime.
#include <hip/hip_runtime.h>

#include <cstring>

#include "gr_steady.h"

using namespace gr;

namespace {

struct Regions {
  uint8_t *st, *ln, *in, *out;
  uint64_t st_bytes, ln_bytes, in_hot, out_hot;
};

// One access: both policies' addresses must agree and lie inside the region.
struct Tally {
  uint64_t checked = 0, bad = 0;
  void same(const void* a, const void* b, const uint8_t* lo, uint64_t bytes, uint32_t size) {
    checked++;
    const uint8_t* x = (const uint8_t*)b;
    if (a != b || x < lo || x + size > lo + bytes) bad++;
  }
};

template <int S, int RM>
uint64_t compare(const StepParams& kp, const Regions& rg, uint64_t* checked) {
  Tally t;
  for (uint32_t i = 0; i < kp.n_lanes; ++i) {
    const LaneAddr<S, RM> l(kp, i, i);
    const WaveAddr<S, RM> w(kp, i, i);
    for (uint32_t row = 0; row < rows_u64(S); ++row) t.same(&l.s64(row), &w.s64(row), rg.st, rg.st_bytes, 8);
    t.same(&l.lword(), &w.lword(), rg.ln, rg.ln_bytes, 4);
    t.same(&l.rflags(), &w.rflags(), rg.ln, rg.ln_bytes, 1);
    t.same(&l.prop_result(), &w.prop_result(), rg.ln, rg.ln_bytes, 1);
    t.same(&l.append_from(), &w.append_from(), rg.ln, rg.ln_bytes, 8);
    for (int j = 0; j < S; ++j) {
      if (l.has_in(j) != w.has_in(j) || l.has_out(j) != w.has_out(j)) t.bad++;
      bool hl = false, hw = false;
      const Mailbox sl = l.in_of((uint32_t)j, &hl);
      const WaveBox sw = w.in_of((uint32_t)j, &hw);
      if (hl != hw || hl != l.has_in(j) || l.has_out_of((uint32_t)j) != w.has_out_of((uint32_t)j)) t.bad++;
      if (hl) t.same(&sl.cnt(), &sw.cnt(), rg.in, rg.in_hot, 1);
      for (int d = 0; d < 2; ++d) {
        if (!(d ? l.has_out(j) : l.has_in(j))) continue;
        const Mailbox a = d ? l.mout(j) : l.min(j);
        const WaveBox b = d ? w.mout(j) : w.min(j);
        const uint8_t* lo = d ? rg.out : rg.in;
        const uint64_t n = d ? rg.out_hot : rg.in_hot;
        t.same(&a.cnt(), &b.cnt(), lo, n, 1);
        t.same(&a.mterm(), &b.mterm(), lo, n, 4);
        for (uint32_t k = 0; k < (d ? kp.out.depth : kp.in.depth); ++k) {
          t.same(&a.t32(k, MT_CDELTA), &b.t32(k, MT_CDELTA), lo, n, 4);
          t.same(&a.u64(k, MF_LOG_INDEX), &b.u64(k, MF_LOG_INDEX), lo, n, 8);
        }
      }
    }
  }
  *checked = t.checked;
  return t.bad;
}

SpaceView view_of(uint8_t* base, uint32_t n_chunks, uint32_t pc, uint32_t depth) {
  SpaceView v;
  v.base = base;
  v.n_chunks = n_chunks;
  v.pc = pc;
  v.hot_bytes = space_hot_chunk_bytes_pc(pc, depth);
  v.cold_bytes = space_cold_chunk_bytes_pc(pc, depth);
  v.depth = depth;
  return v;
}

}  // namespace

extern "C" {

int wu_routes(uint32_t mode, uint32_t S, uint32_t route_g, uint32_t route_r, const uint32_t* base) {
  return steady_wu_routes(mode, S, route_g, route_r, base) ? 1 : 0;
}

int wu_space(uint32_t n_chunks, uint64_t hot_bytes) {
  SpaceView v{};
  v.n_chunks = n_chunks;
  v.hot_bytes = hot_bytes;
  return steady_wu_space(v) ? 1 : 0;
}

// replica_chain<NR> against the division it replaces
uint32_t wu_replica_chain(uint32_t nr, uint32_t i, uint32_t route_g) {
  switch (nr) {
    case 1: return replica_chain<1>(i, route_g);
    case 3: return replica_chain<3>(i, route_g);
    case 5: return replica_chain<5>(i, route_g);
    case 8: return replica_chain<8>(i, route_g);
  }
  return 0xFFFFFFFFu;
}

// Every address WaveAddr forms for lanes [0, route_r * route_g) against
// LaneAddr's, over spaces of n_chunks chunks of pc positions (the in space;
// the out space alike; no memory behind them, so a hot region may reach 4 GiB).
// mode: RT_LOOPBACK (3; one chunk) or RT_AFFINE (2; base = the
// [2][GR_SMAX][GR_SMAX] block bases).
// Returns the number of disagreements or out-of-region addresses, -1 for
// arguments the predicate refuses; *checked = the accesses compared.
int64_t wu_addr_mismatches(uint32_t S, uint32_t mode, uint32_t route_g, uint32_t route_r, uint32_t n_chunks,
                           uint32_t pc, uint32_t depth, const uint32_t* base, uint64_t* checked) {
  StepParams kp;
  memset(&kp, 0, sizeof(kp));
  const uint32_t n = route_r * route_g, cap = pad_cap(n);
  Regions rg;
  rg.st = (uint8_t*)0x100000000000ull;
  rg.ln = (uint8_t*)0x200000000000ull;
  rg.in = (uint8_t*)0x300000000000ull;
  rg.out = (uint8_t*)0x400000000000ull;
  kp.st = StateBase{rg.st, cap, S};
  kp.ln = LaneBase{rg.ln, cap, S};
  kp.in = view_of(rg.in, n_chunks, pc, depth);
  kp.out = view_of(rg.out, n_chunks, pc, depth);
  rg.st_bytes = 8ull * cap * rows_u64(S);  // the u64 rows
  rg.ln_bytes = lane_bytes(S, cap);
  rg.in_hot = rg.out_hot = (uint64_t)n_chunks * kp.in.hot_bytes;
  kp.n_lanes = n;
  kp.route_g = route_g;
  kp.route_r = route_r;
  kp.route_base = base;
  kp.route_mode = (uint8_t)mode;
  kp.route_wu = 1;
  kp.has_locals = 1;
  if (!steady_wu_routes(mode, S, route_g, route_r, base) || !steady_wu_space(kp.in)) return -1;
  uint64_t c = 0, bad = 0;
#define WU_CASE(SS)                                                                   \
  case SS:                                                                            \
    bad = mode == RT_LOOPBACK ? compare<SS, RT_LOOPBACK>(kp, rg, &c) : compare<SS, RT_AFFINE>(kp, rg, &c); \
    break;
  switch (S) {
    WU_CASE(1)
    WU_CASE(3)
    WU_CASE(5)
    WU_CASE(8)
    default: return -1;
  }
#undef WU_CASE
  if (checked) *checked = c;
  return (int64_t)bad;
}

}  // extern "C"

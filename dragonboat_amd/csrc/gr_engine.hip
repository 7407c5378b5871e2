// gr_engine.hip — libgpuraft.so: the C-ABI declared in include/gpuraft.h, the
// boundary passes (gr_io.h) and the pass launcher; the step kernels themselves
// are in gr_kernels.h, one translation unit per slot count (gr_kernels_s*.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "gr_host.h"
#include "gr_io.h"
#include "gr_kernels.h"
#include "gpuraft_wire.h"

namespace gr {

#ifdef GR_COVERAGE
#define GR_EXTERN_COVER(SS) extern template hipError_t cover_read<SS>(uint32_t, uint64_t*);
#else
#define GR_EXTERN_COVER(SS)
#endif
#define GR_EXTERN_SLOTS(SS)                                                                                  \
  extern template hipError_t launch<SS>(const StepParams&, uint32_t*, uint32_t*, uint32_t, uint32_t, hipStream_t, \
                                        const PassTiming*, bool);                                            \
  GR_EXTERN_COVER(SS)
GR_EXTERN_SLOTS(1)
GR_EXTERN_SLOTS(3)
GR_EXTERN_SLOTS(5)
GR_EXTERN_SLOTS(8)

// with_slots(S, f): f(std::integral_constant<int, N>{}) for the instantiated
// slot count N == S (instantiated_slots), so a kernel template is named once;
// any other S is GR_EINVAL, or hipErrorInvalidValue where f returns hipError_t.
static_assert(GR_SMAX == 8, "with_slots and instantiated_slots list the instantiated slot counts");
static inline gr_error no_such_slots(gr_error) { return GR_EINVAL; }
static inline hipError_t no_such_slots(hipError_t) { return hipErrorInvalidValue; }
template <class F>
static auto with_slots(uint32_t S, F&& f) -> decltype(f(std::integral_constant<int, 1>{})) {
  switch (S) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 8: return f(std::integral_constant<int, 8>{});
  }
  return no_such_slots(decltype(f(std::integral_constant<int, 1>{})){});
}

// tick_lanes: launch the tick kernel (some lane may carry ticks or a ReadIndex).
static hipError_t launch_slots(uint32_t S, const StepParams& kp, uint32_t* bail_list, uint32_t* counters,
                               uint32_t list_cap, uint32_t parity, hipStream_t s, const PassTiming* t,
                               bool tick_lanes = true) {
  return with_slots(S, [&](auto ss) {
    return launch<decltype(ss)::value>(kp, bail_list, counters, list_cap, parity, s, t, tick_lanes);
  });
}

static uint32_t instantiated_slots(uint32_t want) {
  if (want <= 1) return 1;
  if (want <= 3) return 3;
  if (want <= 5) return 5;
  if (want <= GR_SMAX) return GR_SMAX;  // wide groups (e.g. 5 voters + 2 observers): leaders take the general lane
  return 0;
}

}  // namespace gr

using namespace gr;
using namespace gr::host;

#ifndef GR_INBOX_WC
#define GR_INBOX_WC 1
#endif
// Pinned memory the host reads (outboxes) is plain; the inboxes the host only
// writes and the device reads once are write-combined (no snooping of dirty
// host cache lines during the upload).
static const unsigned kInboxPinned =
    GR_INBOX_WC ? (hipHostMallocDefault | hipHostMallocWriteCombined) : hipHostMallocDefault;

// A device buffer (Buf) or a pinned host one (Pinned), grown on demand, reused,
// and freed with its engine; the contents do not survive a grow.
template <bool kPinned>
struct GrowBuf {
  uint8_t* p = nullptr;
  size_t n = 0;
  const unsigned flags = hipHostMallocDefault;  // of a pinned buffer
  GrowBuf() = default;
  explicit GrowBuf(unsigned f) : flags(f) {}
  GrowBuf(const GrowBuf&) = delete;
  GrowBuf& operator=(const GrowBuf&) = delete;
  ~GrowBuf() { release(); }
  void release() {
    if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    n = 0;
  }
  int grow(size_t want) {
    if (n >= want) return GR_OK;
    release();
    if ((kPinned ? hipHostMalloc((void**)&p, want, flags) : hipMalloc((void**)&p, want)) != hipSuccess) {
      p = nullptr;
      return GR_EDEVICE;
    }
    n = want;
    return GR_OK;
  }
  template <class T>
  T* as() const {
    return (T*)p;
  }
};

struct gr_engine {
  gr_config cfg{};
  uint32_t S = 0;
  uint32_t cap = 0;  // padded slot capacity (row stride)
  hipStream_t stream = nullptr;

  StateBase st{};
  LaneBase ln{};
  uint64_t* stats = nullptr;
  uint32_t stats_rows = 0;
  uint32_t* bail = nullptr;      // kBailLists lists of cap lanes each, then the tick lists (bail_words)
  uint64_t* tick_stage = nullptr;  // a TickStage record per tick-list entry (gr_layout.h)
  uint32_t* counters = nullptr;  // [2 (pass parity)][kCounters][kCounterStride]
  // gr_step_device passes of at least this many lanes run the role instances
  // (StepParams::split); GR_SPLIT_MIN_LANES at gr_create overrides it (tests)
  uint32_t split_min = kSplitMinLanes;
  // passes of at most this many workgroups run fused (gr_small_kernel);
  // GR_SMALL_BLOCKS at gr_create overrides it (0: never; tests and A/B runs)
  uint32_t small_blocks = kSmallBlocks;
  uint8_t* hints = nullptr;      // 2 x [hint_stride(cap)] wave hints of the device-resident path (gr_layout.h WH_*):
                                 // one set read by a pass, the other written for the next
  uint64_t hint_flip = 0;
  uint64_t launches = 0;         // never reset: selects the live counter set
  uint64_t timing_bailed0 = 0;   // ST_BAILED when timing began
  bool timing = false;
  std::vector<PassTiming> timings;  // one per pass while timing
  bool routes_bound = false;
  uint8_t route_mode = RT_TABLE;  // of the bound routes (RT_TABLE, RT_AFFINE or RT_LOOPBACK)
  uint32_t route_g = 0, route_r = 0;
  uint32_t* route_base = nullptr;  // device [2][GR_SMAX][GR_SMAX]
  // the steady kernel's wave-uniform addressing (gr_layout.h steady_wu_routes):
  // whether the bound routes allow it, whether the spaces of the last
  // gr_step_device pass did (steady_wu_space; true before the first), and
  // GR_STEADY_WU=0 at gr_create (tests: the per-lane instance)
  bool wu_routes = false, wu_spaces = true, wu_enabled = true;
  bool locals_set = false;
  bool locals_other = false;  // some bound local input has ticks / a ReadIndex / oversized counts (LW_OTHER)
  uint64_t passes = 0;
  // GR_WAVE_CLOCK=<path> at gr_create (profiling): the general kernel records
  // each wave's span; gr_destroy writes the last pass's records to <path>
  uint64_t* wclock = nullptr;
  uint32_t* tail_hint = nullptr;  // StepParams::tail_hint: pinned, host-visible
  uint8_t tail_mode = 0;          // StepParams::tail_mode (GR_TAIL_MODE at gr_create: tests, A/B runs)
  uint8_t elections = 0;          // StepParams::elections (gr_set_elections; GR_ELECTIONS=1 at gr_create)
  // the promotion list (gr_promotions): a 16-byte header (count, overflow flag)
  // and max_peers gr_promotion records, one device allocation
  uint8_t* promo = nullptr;
  uint8_t snapshots = 0;          // StepParams::snapshots (gr_set_snapshots; GR_SNAPSHOTS=1 at gr_create)
  // the groups' snapshot records (gr_set_snapshot_recs): max_peers records,
  // zeroed; and the restored list (gr_restored_snapshots), laid out as promo
  // with kRestStage records per engine slot
  gr_snapshot_rec* snap_rec = nullptr;  // max_peers records, then the lanes' staging records (kRestStage each)
  uint8_t* rest = nullptr;
  uint8_t config_entries = 0;  // StepParams::config_entries (gr_set_config_entries; GR_CONFIG_ENTRIES=1 at gr_create)
  // the groups' config-change index records (gr_set_cc_indexes): max_peers
  // records, zeroed, then as many staging records (one per engine slot)
  gr_cc_index* cc_rec = nullptr;
  // the quiesce manager (gr_set_quiesce; GR_QUIESCE_ON_DEVICE=1 at gr_create):
  // one allocation, made by the first gr_load_quiesce or when the switch first
  // goes on, of cap records (qrec), as many pre-pass records (qprev), the words
  // no pass writes (qcfg) and the bound raw LocalTick counts (qraw)
  uint8_t quiesce = 0;
  uint8_t* qmem = nullptr;
  QuiesceRec* qrec = nullptr;
  QuiesceRec* qprev = nullptr;
  uint32_t* qcfg = nullptr;
  uint32_t* qraw = nullptr;
  // the update states (gr_set_update_states, gr_collect_updates): Peer.prevState,
  // cap records, allocated zeroed by the first call that uses them
  gr_update_state* upd_state = nullptr;
  // the lane rows are in the device-resident form (lane l steps peer l), so
  // gr_collect_updates may read them: true while they are all zero (gr_create),
  // set by gr_step_device and gr_graph_replay, cleared by every staged host pass
  bool lanes_by_slot = true;
  // gr_updates_last: what the last gr_collect_updates copied down, and, with
  // per-pass timing on, events around its two kernels (made on first use)
  hipEvent_t upd_ev[4] = {nullptr, nullptr, nullptr, nullptr};
  gr_updates_info upd_last{};
  std::string wclock_path;

  // gr_step buffers (gr_io.h)
  using Buf = GrowBuf<false>;
  using Pinned = GrowBuf<true>;
  Buf d_in, d_out;          // mailbox spaces
  Buf d_msgs, d_locals;     // caller records, as given
  Buf d_mark, d_lop;        // [max_peers] input flags, lane of peer
  Buf d_keys, d_idx, d_skeys, d_sidx;  // mailbox sort
  Buf d_win, d_oc, d_off;   // [lanes]
  Buf d_tmp;                // scan tile sums (io_scan)
  Buf d_kcnt, d_kbase;      // sort_keys: records per mailbox and their exclusive scan
  Buf d_scal;               // lane count, error, outbox total
  Buf d_outmsgs, d_results; // packed outbox
  Buf d_peers, d_slots;     // gr_peer records of a load/sync, slot list
  Buf d_ext, d_lext;        // gr_step_compact: ext message / local records
  Buf d_oc64, d_off64, d_rx, d_roff;  // compact outbox counts and offsets
  Buf d_outext, d_resext;   // compact outbox ext records
  Buf d_ucls, d_ucnt, d_uoff;  // gr_collect_updates: class bytes, tile counts and their exclusive scan
  Pinned h_upd, h_updext;      // its records, the caller's until the next gr_collect_updates
  Buf d_nodes;              // gr_bind_nodes: (cluster, node) -> slot table
  Buf d_wrec, d_why, d_unr; // gr_step_wire: routed records, per-message reason, unrouted indices
  uint32_t nodes_cap = 0;
  // gr_step_wire_out: per-slot cluster ids (gr_bind_nodes), send queues per
  // (slot, remote slot) (gr_bind_targets), and the pass's grouping scratch and
  // records (gr_io.h wire_out_*)
  Buf d_cluster, d_target;
  uint32_t n_targets = 0;
  Buf d_wf, d_wrank, d_wcnt, d_wbase, d_wplan, d_wtot, d_wmsgs, d_wbat, d_wbt;
  Pinned h_wbt;   // batch_target
  Pinned h_wtot;  // message and batch totals
  Pinned h_unr;   // unrouted indices + reasons
  Pinned h_inmsgs{kInboxPinned}, h_inlocals{kInboxPinned};  // inbox the caller may fill in place (gr_inbox_reserve)
  Pinned h_outmsgs, h_results;  // returned to the caller until gr_release_outbox
  Pinned h_scal;
  // gr_cinbox_reserve's ext arrays (the compact ones reuse h_inmsgs / h_inlocals)
  Pinned h_inext{kInboxPinned}, h_inlext{kInboxPinned};
  Pinned h_outext, h_resext;  // gr_step_compact's ext outputs (the compact ones reuse h_outmsgs / h_results)
  std::mutex mu;  // one host-path pass at a time per engine
  // gr_step_compact_begin -> _end: the uploaded pass waiting for its second half
  struct CPending {
    bool on = false;
    uint32_t nm = 0, nlc = 0, nx = 0, nlx = 0, nl = 0;
  } cpend;
  // cpend.on, readable without the mutex: between _begin and _end the pending
  // pass owns the shared scratch (d_mark, d_lop, d_msgs, d_locals, d_ext,
  // d_lext, d_scal) and the lane rows, so every other entry point that uses
  // them or steps the engine refuses with GR_ESTATE until _end has run.
  std::atomic<bool> pending{false};
};

// GR_ESTATE while a gr_step_compact_begin waits for its _end (gpuraft.h).
#define GR_REFUSE_PENDING(e)                          \
  do {                                                \
    if ((e)->pending.load(std::memory_order_acquire)) \
      return GR_ESTATE;                               \
  } while (0)

// A fresh timing record for the next pass (nullptr when timing is off or a
// HIP call fails: the pass then runs untimed and gr_timing_end reports it).
static PassTiming* next_timing(gr_engine* e) {
  if (!e->timing) return nullptr;
  PassTiming t{};
  for (int k = 0; k < 3; ++k)
    if (hipEventCreate(&t.ev[k]) != hipSuccess) return nullptr;
  e->timings.push_back(t);
  return &e->timings.back();
}

static void free_timings(gr_engine* e) {
  for (auto& t : e->timings) {
    for (int k = 0; k < 3; ++k) (void)hipEventDestroy(t.ev[k]);
  }
  e->timings.clear();
}

namespace {

// GR_PHASES=1: host-side phase times of a boundary pass on stderr (profiling aid).
struct PhaseClock {
  bool on = getenv("GR_PHASES") != nullptr;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  char buf[256];
  int len = 0;
  void mark(const char* what) {
    if (!on) return;
    const auto n = std::chrono::steady_clock::now();
    len += snprintf(buf + len, sizeof(buf) - len, "%s %.3f ms; ", what,
                    std::chrono::duration<double, std::milli>(n - t).count());
    t = n;
  }
  void report() {
    if (on) fprintf(stderr, "gr_phases: %s\n", buf);
  }
};

#define HIPCHK(x)                              \
  do {                                         \
    hipError_t _e = (x);                       \
    if (_e != hipSuccess) return GR_EDEVICE;   \
  } while (0)

constexpr size_t kPromoHeader = 16;

StepParams base_params(gr_engine* e) {
  StepParams kp;
  memset(&kp, 0, sizeof(kp));
  kp.st = e->st;
  kp.ln = e->ln;
  kp.stats = e->stats;
  kp.max_entry_size = e->cfg.max_entry_size;
  kp.small_blocks = e->small_blocks;
  kp.wclock = e->wclock;
  kp.tail_hint = e->tail_hint;
  kp.tail_mode = e->tail_mode;
  kp.tick_stage = e->tick_stage;
  kp.elections = e->elections;
  kp.promo_hdr = (uint32_t*)e->promo;
  kp.promo = (gr_promotion*)(e->promo + kPromoHeader);
  kp.promo_cap = e->cfg.max_peers;
  kp.snapshots = e->snapshots;
  kp.snap_rec = e->snap_rec;
  kp.rest_stage = e->snap_rec + e->cfg.max_peers;
  kp.rest_hdr = (uint32_t*)e->rest;
  kp.rest = (gr_restored*)(e->rest + kPromoHeader);
  kp.rest_cap = kRestStage * e->cfg.max_peers;
  kp.config_entries = e->config_entries;
  kp.cc_rec = e->cc_rec;
  kp.cc_stage = e->cc_rec + e->cfg.max_peers;
  kp.quiesce = e->quiesce;
  kp.qrec = e->qrec;
  kp.qprev = e->qprev;
  kp.qcfg = e->qcfg;
  kp.qraw = e->qraw;
  return kp;
}

// The quiesce records' allocation (zeroed: every manager disabled).
int ensure_quiesce(gr_engine* e) {
  if (e->qmem) return GR_OK;
  const size_t cap = e->cap, bytes = cap * (2 * sizeof(QuiesceRec) + 8);
  if (hipMalloc((void**)&e->qmem, bytes) != hipSuccess) {
    e->qmem = nullptr;
    return GR_ENOMEM;
  }
  if (hipMemsetAsync(e->qmem, 0, bytes, e->stream) != hipSuccess ||  // (as ensure_update_state)
      hipStreamSynchronize(e->stream) != hipSuccess) {
    (void)hipFree(e->qmem);
    e->qmem = nullptr;
    return GR_EDEVICE;
  }
  e->qrec = (QuiesceRec*)e->qmem;
  e->qprev = e->qrec + cap;
  e->qcfg = (uint32_t*)(e->qprev + cap);
  e->qraw = e->qcfg + cap;
  return GR_OK;
}

// The update states' allocation (zeroed: the empty State, peer.go:96-100).
int ensure_update_state(gr_engine* e) {
  if (e->upd_state) return GR_OK;
  const size_t bytes = (size_t)e->cap * sizeof(gr_update_state);
  if (hipMalloc((void**)&e->upd_state, bytes) != hipSuccess) {
    e->upd_state = nullptr;
    return GR_ENOMEM;
  }
  // on the engine's stream, and waited for: that stream is non-blocking, so a fill
  // on the null stream is not ordered before the kernels that use the records next
  if (hipMemsetAsync(e->upd_state, 0, bytes, e->stream) != hipSuccess ||
      hipStreamSynchronize(e->stream) != hipSuccess) {
    (void)hipFree(e->upd_state);
    e->upd_state = nullptr;
    return GR_EDEVICE;
  }
  return GR_OK;
}

// d_scal / h_scal: the four words a pass's counts, totals and error flags come down in.
int ensure_scal(gr_engine* e) {
  const int r = e->d_scal.grow(16);
  return r ? r : e->h_scal.grow(16);
}

// Grid of a boundary pass (grid-stride loops): enough workgroups to fill the chip.
uint32_t io_grid(size_t n) {
  const size_t b = (n + io::kIoBlock - 1) / io::kIoBlock;
  return (uint32_t)std::max<size_t>(1, std::min<size_t>(b, 4096));
}

// A slot list into e->d_slots, on e->stream.
int upload_slots(gr_engine* e, const uint32_t* slots, size_t n, const uint32_t** d_slots) {
  const int r = e->d_slots.grow(n * 4);
  if (r) return r;
  HIPCHK(hipMemcpyAsync(e->d_slots.p, slots, n * 4, hipMemcpyHostToDevice, e->stream));
  *d_slots = e->d_slots.as<const uint32_t>();
  return GR_OK;
}

// The operations over a slot list and one record per listed slot (gpuraft.h):
// their checks and refusals, in the one order all of them document, around the
// kernel `launch` enqueues.
//  1. a null engine, or null slots / records with n != 0: GR_EINVAL
//  2. n == 0: GR_OK
//  3. n >= 2^31: GR_EINVAL
//  4. a slot out of range or listed twice: GR_ERANGE (nothing written)
//  5. the engine's lock
//  6. a pending gr_step_compact_begin: GR_ESTATE
//  7. a record `known` does not take: GR_EINVAL
//  8. hipDeviceSynchronize (passes in flight on other streams own the rows and side arrays)
//  9. the slots, and with SL_UP the records, into d_slots / d_peers
// With SL_STATUS a status per record follows the records in d_peers and comes
// down into `status` (when given), the kernel raises `refused` for any status
// but 0, and the call is then GR_ESTATE. With SL_DOWN the records come down.
enum : unsigned { SL_UP = 1, SL_DOWN = 2, SL_STATUS = 4 };
template <class Rec>
struct SlotArgs {
  dim3 grid, blk;
  hipStream_t s;
  const uint32_t* slots;  // device
  Rec* recs;              // device
  uint32_t n;
  int32_t* status;    // device (SL_STATUS)
  uint32_t* refused;  // device (SL_STATUS)
};
template <class Rec, class Launch>
int slot_list_op(gr_engine* e, const uint32_t* slots, Rec* recs, size_t n, unsigned mode, int32_t* status,
                 Launch launch, bool (*known)(const Rec&) = nullptr) {
  if (!e || (n && (!slots || !recs))) return GR_EINVAL;
  if (n == 0) return GR_OK;
  if (n >= 0x80000000ull) return GR_EINVAL;
  const uint32_t cap = e->cfg.max_peers;
  std::vector<uint64_t> seen((cap + 63) / 64, 0);
  for (size_t x = 0; x < n; ++x) {
    const uint32_t p = slots[x];
    if (p >= cap || (seen[p >> 6] >> (p & 63)) & 1) return GR_ERANGE;  // nothing written
    seen[p >> 6] |= 1ull << (p & 63);
  }
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  for (size_t x = 0; known && x < n; ++x)
    if (!known(recs[x])) return GR_EINVAL;
  HIPCHK(hipDeviceSynchronize());
  const bool st = mode & SL_STATUS;
  const size_t bytes = n * sizeof(Rec);
  SlotArgs<Rec> a{dim3(io_grid(n)), dim3(io::kIoBlock), e->stream, nullptr, nullptr, (uint32_t)n, nullptr, nullptr};
  int r;
  if ((r = upload_slots(e, slots, n, &a.slots))) return r;
  if ((r = e->d_peers.grow(st ? bytes + n * 4 + 16 : bytes))) return r;
  a.recs = e->d_peers.as<Rec>();
  if (mode & SL_UP) HIPCHK(hipMemcpyAsync((void*)a.recs, recs, bytes, hipMemcpyHostToDevice, a.s));
  if (st) {
    if ((r = ensure_scal(e))) return r;
    a.status = (int32_t*)(a.recs + n);
    a.refused = e->d_scal.as<uint32_t>();
    HIPCHK(hipMemsetAsync(a.refused, 0, 16, a.s));
  }
  if ((r = launch(a))) return r;
  HIPCHK(hipGetLastError());
  if (mode & SL_DOWN) HIPCHK(hipMemcpyAsync((void*)recs, a.recs, bytes, hipMemcpyDeviceToHost, a.s));
  if (st && status) HIPCHK(hipMemcpyAsync(status, a.status, n * 4, hipMemcpyDeviceToHost, a.s));
  if (st) HIPCHK(hipMemcpyAsync(e->h_scal.p, a.refused, 4, hipMemcpyDeviceToHost, a.s));
  HIPCHK(hipStreamSynchronize(a.s));
  return st && *e->h_scal.as<uint32_t>() ? GR_ESTATE : GR_OK;
}

// gr_peer records <-> state rows for slots [first, first+n) or a slot list
// (gr_io.h): the records cross PCIe once, the transpose runs on the device.
int transfer(gr_engine* e, const uint32_t* slots, uint32_t first, size_t n, gr_peer* host, bool to_device) {
  if (!e || (n && !host)) return GR_EINVAL;
  const uint32_t cap = e->cfg.max_peers;
  if (!slots && (uint64_t)first + n > cap) return GR_ERANGE;
  if (n == 0) return GR_OK;
  if (n >= 0x80000000ull) return GR_EINVAL;
  if (slots && !to_device)
    for (size_t x = 0; x < n; ++x)
      if (slots[x] >= cap) return GR_ERANGE;
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  HIPCHK(hipDeviceSynchronize());  // passes in flight on other streams own the rows
  const hipStream_t s = e->stream;
  const size_t bytes = n * sizeof(gr_peer);
  int r;
  if ((r = e->d_peers.grow(bytes))) return r;
  const uint32_t* dslots = nullptr;
  if (slots && (r = upload_slots(e, slots, n, &dslots))) return r;
  gr_peer* dp = (gr_peer*)e->d_peers.p;
  const dim3 grid(io_grid(n)), blk(io::kIoBlock);
  if (to_device) {
    if ((r = e->d_mark.grow((size_t)cap * 4))) return r;
    if ((r = ensure_scal(e))) return r;
    HIPCHK(hipMemcpyAsync(dp, host, bytes, hipMemcpyHostToDevice, s));
    if (slots) HIPCHK(hipMemsetAsync(e->d_mark.p, 0, (size_t)cap * 4, s));
    HIPCHK(hipMemsetAsync(e->d_scal.p, 0, 16, s));
    hipLaunchKernelGGL(io::check_peers, grid, blk, 0, s, (const gr_peer*)dp, dslots, (uint32_t)n, e->S, cap,
                       (uint32_t*)e->d_mark.p, (uint32_t*)e->d_scal.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(e->h_scal.p, e->d_scal.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const uint32_t err = *(uint32_t*)e->h_scal.p;
    if (err & io::ERR_SLOT) return GR_ERANGE;  // no row was written
    if (err & io::ERR_PEER) return GR_EINVAL;
    hipLaunchKernelGGL(io::peers_to_rows, grid, blk, 0, s, (const gr_peer*)dp, dslots, first, (uint32_t)n, e->st,
                       e->S);
    HIPCHK(hipGetLastError());
  } else {
    HIPCHK(hipMemsetAsync(dp, 0, bytes, s));
    hipLaunchKernelGGL(io::rows_to_peers, grid, blk, 0, s, e->st, dslots, first, (uint32_t)n, e->S, dp);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(host, dp, bytes, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  return GR_OK;
}

// Exclusive sum of n values on `s` (gr_scan.h), the tile sums in e->d_tmp.
template <class T>
int io_scan_t(gr_engine* e, const T* in, T* out, uint32_t n, hipStream_t s) {
  if (n == 0) return GR_OK;
  const int r = e->d_tmp.grow((size_t)scan::scan_tiles_of(n) * sizeof(T));
  if (r) return r;
  HIPCHK(scan::exclusive_scan<T>(in, out, n, (T*)e->d_tmp.p, s));
  return GR_OK;
}
int io_scan(gr_engine* e, const uint32_t* in, uint32_t* out, uint32_t n, hipStream_t s) {
  return io_scan_t<uint32_t>(e, in, out, n, s);
}
int io_scan64(gr_engine* e, const uint64_t* in, uint64_t* out, uint32_t n, hipStream_t s) {
  return io_scan_t<uint64_t>(e, in, out, n, s);
}

// Stable sort of the inbox's mailbox keys (slot-major j*nl + lane, each below
// `positions`), so arrival order inside a mailbox survives: a counting sort
// (gr_io.h key_count, key_scatter, key_order); sorted keys/indexes in
// d_skeys/d_sidx. d_idx holds each record's slot in its mailbox meanwhile.
int sort_keys(gr_engine* e, uint32_t nm, uint32_t positions, hipStream_t s) {
  int r;
  if ((r = e->d_kcnt.grow((size_t)positions * 4 + 4))) return r;
  if ((r = e->d_kbase.grow((size_t)positions * 4 + 4))) return r;
  uint32_t* cnt = (uint32_t*)e->d_kcnt.p;
  uint32_t* base = (uint32_t*)e->d_kbase.p;
  HIPCHK(hipMemsetAsync(cnt, 0, (size_t)positions * 4, s));
  const dim3 blk(io::kIoBlock);
  hipLaunchKernelGGL(io::key_count, dim3(io_grid(nm)), blk, 0, s, (const uint32_t*)e->d_keys.p, nm, cnt,
                     (uint32_t*)e->d_idx.p);
  HIPCHK(hipGetLastError());
  if ((r = io_scan(e, cnt, base, positions, s))) return r;
  hipLaunchKernelGGL(io::key_scatter, dim3(io_grid(nm)), blk, 0, s, (const uint32_t*)e->d_keys.p,
                     (const uint32_t*)e->d_idx.p, nm, (const uint32_t*)base, (uint32_t*)e->d_skeys.p,
                     (uint32_t*)e->d_sidx.p);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(io::key_order, dim3(io_grid(positions)), blk, 0, s, (const uint32_t*)cnt,
                     (const uint32_t*)base, positions, (uint32_t*)e->d_sidx.p);
  HIPCHK(hipGetLastError());
  return GR_OK;
}

// ---------------------------------------------------------------- the staged host pass
// gr_step, the wire path and gr_step_compact run one sequence of boundary
// passes (gr_io.h) around the step kernels: inbox records -> lanes
// (stage_lanes), then mailboxes, lane rows and the pass itself
// (run_staged_pass), then the outbox. The inbox, already in HBM, is full
// records (FullInbox) or compact ones (CompactInbox): each names the kernels
// that read its record type; nothing else differs.
struct FullInbox {
  const gr_message* msgs;
  uint32_t n_msgs;
  const gr_local_input* loc;
  uint32_t n_loc;
  uint32_t n_tick_recs() const { return n_loc; }
  void check_raw_ticks(dim3 g, hipStream_t s, uint32_t* err) const {
    hipLaunchKernelGGL(io::check_raw_ticks, g, dim3(io::kIoBlock), 0, s, loc, n_loc, err);
  }
  void mark(dim3 g, hipStream_t s, uint32_t S, uint32_t cap, uint32_t* mark, uint32_t* err, uint32_t ce) const {
    hipLaunchKernelGGL(io::mark_inputs, g, dim3(io::kIoBlock), 0, s, msgs, n_msgs, loc, n_loc, S, cap, mark, err, ce);
  }
  void keys(dim3 g, hipStream_t s, const uint32_t* lop, uint32_t nl, uint32_t* keys, uint32_t* idx) const {
    hipLaunchKernelGGL(io::msg_keys, g, dim3(io::kIoBlock), 0, s, msgs, n_msgs, lop, nl, keys, idx);
  }
  void encode(dim3 g, hipStream_t s, const uint32_t* skeys, const uint32_t* sidx, const SpaceView& vin,
              uint32_t ce) const {
    hipLaunchKernelGGL(io::encode_sorted, g, dim3(io::kIoBlock), 0, s, msgs, skeys, sidx, n_msgs, vin, ce);
  }
  void winner(dim3 g, hipStream_t s, const uint32_t* lop, uint32_t* win) const {
    hipLaunchKernelGGL(io::local_winner, g, dim3(io::kIoBlock), 0, s, loc, n_loc, lop, win);
  }
  void fill(dim3 g, hipStream_t s, const uint32_t* win, uint32_t nl, const LaneBase& ln) const {
    hipLaunchKernelGGL(io::fill_locals, g, dim3(io::kIoBlock), 0, s, loc, win, nl, ln);
  }
};

struct CompactInbox {
  io::CInbox ci;
  uint32_t n_msgs, n_loc;  // ci.n_msgs, ci.n_loc
  // the engine's compact inbox buffers, holding these many records
  CompactInbox(gr_engine* e, uint32_t nm, uint32_t nlc, uint32_t nx, uint32_t nlx) : n_msgs(nm), n_loc(nlc) {
    ci.msgs = e->d_msgs.as<const gr_cmsg>();
    ci.ext = e->d_ext.as<const gr_message>();
    ci.loc = e->d_locals.as<const gr_clocal>();
    ci.lext = e->d_lext.as<const gr_local_input>();
    ci.n_msgs = nm;
    ci.n_ext = nx;
    ci.n_loc = nlc;
    ci.n_lext = nlx;
  }
  uint32_t n_tick_recs() const { return ci.n_loc + ci.n_lext; }
  void check_raw_ticks(dim3 g, hipStream_t s, uint32_t* err) const {
    hipLaunchKernelGGL(io::check_raw_ticks_c, g, dim3(io::kIoBlock), 0, s, ci.loc, ci.n_loc, ci.lext, ci.n_lext, err);
  }
  void mark(dim3 g, hipStream_t s, uint32_t S, uint32_t cap, uint32_t* mark, uint32_t* err, uint32_t ce) const {
    hipLaunchKernelGGL(io::mark_inputs_c, g, dim3(io::kIoBlock), 0, s, ci, S, cap, mark, err, ce);
  }
  void keys(dim3 g, hipStream_t s, const uint32_t* lop, uint32_t nl, uint32_t* keys, uint32_t* idx) const {
    hipLaunchKernelGGL(io::msg_keys_c, g, dim3(io::kIoBlock), 0, s, ci.msgs, ci.n_msgs, lop, nl, keys, idx);
  }
  void encode(dim3 g, hipStream_t s, const uint32_t* skeys, const uint32_t* sidx, const SpaceView& vin,
              uint32_t ce) const {
    hipLaunchKernelGGL(io::encode_sorted_c, g, dim3(io::kIoBlock), 0, s, ci, skeys, sidx, vin, ce);
  }
  void winner(dim3 g, hipStream_t s, const uint32_t* lop, uint32_t* win) const {
    hipLaunchKernelGGL(io::local_winner_c, g, dim3(io::kIoBlock), 0, s, ci.loc, ci.n_loc, lop, win);
  }
  void fill(dim3 g, hipStream_t s, const uint32_t* win, uint32_t nl, const LaneBase& ln) const {
    hipLaunchKernelGGL(io::fill_locals_c, g, dim3(io::kIoBlock), 0, s, ci, win, nl, ln);
  }
};

// Inbox records -> lanes: every slot with input marked (d_mark) and numbered
// (d_lop); waits for the lane count. *err: some record is refused (a slot out of
// range, a QuiescedTick count with the quiesce manager on the device): nothing
// of the pass may run. Caller holds e->mu.
template <class In>
int stage_lanes(gr_engine* e, const In& in, uint32_t* nl, uint32_t* err) {
  const uint32_t S = e->S, cap = e->cfg.max_peers;
  const hipStream_t s = e->stream;
  int r;
  if ((r = e->d_mark.grow((size_t)cap * 4))) return r;
  if ((r = e->d_lop.grow((size_t)cap * 4))) return r;
  if ((r = ensure_scal(e))) return r;
  uint32_t* mark = e->d_mark.as<uint32_t>();
  uint32_t* lop = e->d_lop.as<uint32_t>();
  uint32_t* scal = e->d_scal.as<uint32_t>();
  HIPCHK(hipMemsetAsync(mark, 0, (size_t)cap * 4, s));
  HIPCHK(hipMemsetAsync(scal, 0, 16, s));
  if (e->quiesce && in.n_tick_recs()) {  // ticks are LocalTicks: a QuiescedTick count is refused (scal[1])
    in.check_raw_ticks(dim3(io_grid(in.n_tick_recs())), s, scal + 1);
    HIPCHK(hipGetLastError());
  }
  in.mark(dim3(io_grid(in.n_msgs + in.n_loc)), s, S, cap, mark, scal + 1, (uint32_t)e->config_entries);
  HIPCHK(hipGetLastError());
  if ((r = io_scan(e, mark, lop, cap, s))) return r;
  hipLaunchKernelGGL(io::finish_lanes, dim3(1), dim3(64), 0, s, (const uint32_t*)mark, (const uint32_t*)lop, cap,
                     (const uint32_t*)(scal + 1), scal);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(e->h_scal.p, scal, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *nl = e->h_scal.as<uint32_t>()[0];
  *err = e->h_scal.as<uint32_t>()[1];
  return GR_OK;
}

// The nl > 0 lanes stage_lanes numbered: their mailboxes (slot-major j*nl +
// lane, arrival order kept by a stable sort), their lane rows, and the pass,
// enqueued on e->stream; *vout is the space it writes. Caller holds e->mu.
template <class In>
int run_staged_pass(gr_engine* e, const In& in, uint32_t nl, SpaceView* vout) {
  const uint32_t S = e->S, cap = e->cfg.max_peers, nm = in.n_msgs, nlc = in.n_loc;
  const hipStream_t s = e->stream;
  const dim3 blk(io::kIoBlock);
  int r;
  const uint32_t* mark = e->d_mark.as<const uint32_t>();
  const uint32_t* lop = e->d_lop.as<const uint32_t>();
  hipLaunchKernelGGL(io::lane_peers, dim3(io_grid(cap)), blk, 0, s, mark, lop, cap, e->ln.u32(LR_LANE_PEER));
  HIPCHK(hipGetLastError());
  // ---- mailboxes
  const uint32_t positions = nl * S;
  const size_t space = gr_space_bytes(1, positions, GR_C);
  if ((r = e->d_in.grow(space))) return r;
  if ((r = e->d_out.grow(space))) return r;
  const SpaceView vin = make_view(e->d_in.p, 1, positions);
  *vout = make_view(e->d_out.p, 1, positions);
  hipLaunchKernelGGL(io::clear_counts, dim3(io_grid(vin.pc)), blk, 0, s, vin, vin.pc);  // the count bytes
  HIPCHK(hipGetLastError());
  if (nm) {
    for (gr_engine::Buf* b : {&e->d_keys, &e->d_idx, &e->d_skeys, &e->d_sidx})
      if ((r = b->grow((size_t)nm * 4))) return r;
    in.keys(dim3(io_grid(nm)), s, lop, nl, e->d_keys.as<uint32_t>(), e->d_idx.as<uint32_t>());
    HIPCHK(hipGetLastError());
    if ((r = sort_keys(e, nm, positions, s))) return r;
    in.encode(dim3(io_grid(nm)), s, e->d_skeys.as<const uint32_t>(), e->d_sidx.as<const uint32_t>(), vin,
              (uint32_t)e->config_entries);
    HIPCHK(hipGetLastError());
  }
  // ---- locals -> lane rows
  if ((r = e->d_win.grow((size_t)nl * 4))) return r;
  HIPCHK(hipMemsetAsync(e->d_win.p, 0, (size_t)nl * 4, s));
  if (nlc) {
    in.winner(dim3(io_grid(nlc)), s, lop, e->d_win.as<uint32_t>());
    HIPCHK(hipGetLastError());
  }
  in.fill(dim3(io_grid(nl)), s, e->d_win.as<const uint32_t>(), nl, e->ln);
  HIPCHK(hipGetLastError());
  // ---- the pass
  StepParams kp = base_params(e);
  kp.has_locals = 1;
  kp.has_lane_peer = 1;
  kp.route_mode = RT_IDENTITY;
  kp.in = vin;
  kp.out = *vout;
  kp.n_lanes = nl;
  kp.qraw = e->ln.u32(LR_TICKS);  // this pass's rows are the raw input: the quiesce pass rewrites them in place
  HIPCHK(launch_slots(S, kp, e->bail, e->counters, e->cap, (uint32_t)e->launches++, s, next_timing(e)));
  e->passes++;
  e->lanes_by_slot = false;  // lanes are numbered by input now: gr_collect_updates waits for a device pass
  e->locals_set = false;    // the lane rows now hold this pass's compact locals
  e->routes_bound = false;  // and RT_IDENTITY replaced the bound routes
  return GR_OK;
}

}  // namespace

extern "C" {

const char* gr_strerror(int err) {
  switch (err) {
    case GR_OK: return "ok";
    case GR_EINVAL: return "invalid argument";
    case GR_ENOMEM: return "out of memory";
    case GR_EDEVICE: return "HIP device error";
    case GR_ERANGE: return "slot range out of bounds";
    case GR_ECAPACITY: return "mailbox capacity exceeded";
    case GR_ESTATE: return "engine state error";
  }
  return "unknown error";
}

const char* gr_escalation_name(int esc) {
  static const char* names[] = {"none", "term_window", "random", "unsupported", "election", "panic",
                                "capacity", "snapshot", "entry_size", "msg_runs", "nonmember",
                                "config_change", "wide_term"};
  if (esc < 0 || esc > GR_ESC_WIDE_TERM) return "unknown";
  return names[esc];
}

int gr_create(const gr_config* cfg, gr_engine** out) {
  if (!cfg || !out) return GR_EINVAL;
  *out = nullptr;
  if (cfg->window_runs != GR_K || cfg->read_index_depth != GR_Q || cfg->mailbox_depth != GR_C)
    return GR_EINVAL;
  if (cfg->max_peers == 0 || cfg->slots == 0 || cfg->slots > GR_SMAX) return GR_EINVAL;
  const uint32_t S = instantiated_slots(cfg->slots);
  if (!S) return GR_EINVAL;
  if (hipSetDevice((int)cfg->device) != hipSuccess) return GR_EDEVICE;
  gr_engine* e = new (std::nothrow) gr_engine();
  if (!e) return GR_ENOMEM;
  e->cfg = *cfg;
  e->S = S;
  e->cap = pad_cap(cfg->max_peers);
  e->st.cap = e->cap;
  e->st.S = S;
  e->ln.lcap = e->cap;
  e->ln.S = S;
  const size_t sb = state_bytes(S, e->cap), lb = lane_bytes(S, e->cap);
  e->stats_rows = (e->cap + kBlock - 1) / kBlock;
  if (const char* sm = getenv("GR_SPLIT_MIN_LANES")) {
    const long v = strtol(sm, nullptr, 10);
    if (v > 0) e->split_min = (uint32_t)v;
  }
  if (const char* sb = getenv("GR_SMALL_BLOCKS")) e->small_blocks = (uint32_t)strtoul(sb, nullptr, 10);
  if (const char* tm = getenv("GR_TAIL_MODE")) {
    const unsigned long v = strtoul(tm, nullptr, 10);
    if (v <= 2) e->tail_mode = (uint8_t)v;
  }
  if (const char* wu = getenv("GR_STEADY_WU")) e->wu_enabled = !(wu[0] == '0' && wu[1] == 0);
  if (const char* el = getenv("GR_ELECTIONS")) e->elections = el[0] == '1';
  if (const char* sn = getenv("GR_SNAPSHOTS")) e->snapshots = sn[0] == '1';
  if (const char* ce = getenv("GR_CONFIG_ENTRIES")) e->config_entries = ce[0] == '1';
  const char* qd = getenv("GR_QUIESCE_ON_DEVICE");
  if (const char* wc = getenv("GR_WAVE_CLOCK")) {
    // two regions: the general kernel's waves, then the tick kernel's (gr_kernels.h)
    if (hipMalloc((void**)&e->wclock, 2 * (size_t)kGeneralWaveSlots * kWaveClockWords * 8) == hipSuccess &&
        hipMemset(e->wclock, 0, 2 * (size_t)kGeneralWaveSlots * kWaveClockWords * 8) == hipSuccess)
      e->wclock_path = wc;
  }
  void *ds = nullptr, *dl = nullptr;
  if (hipMalloc(&ds, sb) != hipSuccess || hipMalloc(&dl, lb) != hipSuccess ||
      hipMalloc((void**)&e->stats, (size_t)e->stats_rows * NSTAT * 8) != hipSuccess ||
      hipMalloc((void**)&e->bail, bail_words(e->cap) * 4) != hipSuccess ||
      hipMalloc((void**)&e->tick_stage, (size_t)kTickLists * tick_cap(e->cap) * kTickStageWords * 8) != hipSuccess ||
      hipMalloc((void**)&e->counters, 2 * kCounters * kCounterStride * 4) != hipSuccess ||
      hipMalloc((void**)&e->route_base, 2 * GR_SMAX * GR_SMAX * 4) != hipSuccess ||
      hipMalloc((void**)&e->promo, kPromoHeader + (size_t)cfg->max_peers * sizeof(gr_promotion)) != hipSuccess ||
      hipMalloc((void**)&e->snap_rec, (size_t)cfg->max_peers * (1 + kRestStage) * sizeof(gr_snapshot_rec)) != hipSuccess ||
      hipMalloc((void**)&e->rest, kPromoHeader + (size_t)kRestStage * cfg->max_peers * sizeof(gr_restored)) != hipSuccess ||
      hipMalloc((void**)&e->cc_rec, (size_t)cfg->max_peers * 2 * sizeof(gr_cc_index)) != hipSuccess ||
      hipMalloc((void**)&e->hints, 2 * hint_stride(e->cap)) != hipSuccess) {
    if (ds) (void)hipFree(ds);
    if (dl) (void)hipFree(dl);
    e->st.base = nullptr;
    e->ln.base = nullptr;
    gr_destroy(e);
    return GR_ENOMEM;
  }
  e->st.base = (uint8_t*)ds;
  e->ln.base = (uint8_t*)dl;
  if (hipMemset(ds, 0, sb) != hipSuccess || hipMemset(dl, 0, lb) != hipSuccess ||
      hipMemset(e->stats, 0, (size_t)e->stats_rows * NSTAT * 8) != hipSuccess ||
      hipMemset(e->counters, 0, 2 * kCounters * kCounterStride * 4) != hipSuccess ||
      hipMemset(e->hints, 0, 2 * hint_stride(e->cap)) != hipSuccess ||
      hipMemset(e->promo, 0, kPromoHeader) != hipSuccess ||
      hipMemset(e->snap_rec, 0, (size_t)cfg->max_peers * (1 + kRestStage) * sizeof(gr_snapshot_rec)) != hipSuccess ||
      hipMemset(e->rest, 0, kPromoHeader) != hipSuccess ||
      hipMemset(e->cc_rec, 0, (size_t)cfg->max_peers * 2 * sizeof(gr_cc_index)) != hipSuccess ||
      hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) {
    gr_destroy(e);
    return GR_EDEVICE;
  }
  // a failed allocation only leaves every launch on
  if (hipHostMalloc((void**)&e->tail_hint, 64, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess)
    e->tail_hint = nullptr;
  else
    *(volatile uint32_t*)e->tail_hint = kTailAll;
  if (qd && qd[0] == '1') {
    const int r = ensure_quiesce(e);
    if (r) {
      gr_destroy(e);
      return r;
    }
    e->quiesce = 1;
  }
  *out = e;
  return GR_OK;
}

void gr_destroy(gr_engine* e) {
  if (!e) return;
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  if (e->st.base) (void)hipFree(e->st.base);
  if (e->ln.base) (void)hipFree(e->ln.base);
  if (e->stats) (void)hipFree(e->stats);
  if (e->bail) (void)hipFree(e->bail);
  if (e->tick_stage) (void)hipFree(e->tick_stage);
  if (e->counters) (void)hipFree(e->counters);
  if (e->route_base) (void)hipFree(e->route_base);
  if (e->hints) (void)hipFree(e->hints);
  if (e->promo) (void)hipFree(e->promo);
  if (e->snap_rec) (void)hipFree(e->snap_rec);
  if (e->rest) (void)hipFree(e->rest);
  if (e->cc_rec) (void)hipFree(e->cc_rec);
  if (e->qmem) (void)hipFree(e->qmem);
  if (e->upd_state) (void)hipFree(e->upd_state);
  for (hipEvent_t ev : e->upd_ev)
    if (ev) (void)hipEventDestroy(ev);
  if (e->tail_hint) (void)hipHostFree(e->tail_hint);
  if (e->wclock) {
    std::vector<uint64_t> h(2 * (size_t)kGeneralWaveSlots * kWaveClockWords);
    if (!e->wclock_path.empty() && hipStreamSynchronize(e->stream) == hipSuccess &&
        hipMemcpy(h.data(), e->wclock, h.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
      if (FILE* f = fopen(e->wclock_path.c_str(), "wb")) {
        fwrite(h.data(), 8, h.size(), f);
        fclose(f);
      }
    }
    (void)hipFree(e->wclock);
  }
  free_timings(e);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;  // and its Buf and Pinned members
}

int gr_load_groups(gr_engine* e, uint32_t first, const gr_peer* peers, size_t n) {
  return transfer(e, nullptr, first, n, const_cast<gr_peer*>(peers), true);
}

int gr_sync_groups_to_host(gr_engine* e, uint32_t first, gr_peer* out, size_t n) {
  return transfer(e, nullptr, first, n, out, false);
}

int gr_load_peers(gr_engine* e, const uint32_t* slots, const gr_peer* peers, size_t n) {
  if (n && !slots) return GR_EINVAL;
  return transfer(e, slots, 0, n, const_cast<gr_peer*>(peers), true);
}

int gr_sync_peers_to_host(gr_engine* e, const uint32_t* slots, gr_peer* out, size_t n) {
  if (n && !slots) return GR_EINVAL;
  return transfer(e, slots, 0, n, out, false);
}

// LogReader.Compact(index) (logreader.go:251-269) for a slot list, mirrored
// into the device's firstIndex-1 (entryLog.firstIndex, logentry.go:97-104):
// after compaction term() answers 0 below it and Replicate sends below it take
// the snapshot path, as in the reference.
int gr_compact_log(gr_engine* e, const uint32_t* slots, const uint64_t* index, size_t n, int32_t* status) {
  return slot_list_op(e, slots, index, n, SL_UP | SL_STATUS, status, [e](const SlotArgs<const uint64_t>& a) {
    return with_slots(e->S, [&](auto ss) {
      hipLaunchKernelGGL(io::compact_rows<decltype(ss)::value>, a.grid, a.blk, 0, a.s, e->st, a.slots, a.recs, a.n,
                         a.status, a.refused);
      return GR_OK;
    });
  });
}

// entryLog.commitUpdate (logentry.go:325-335) for a slot list: the host's
// persistence/apply acknowledgement moves inMemory.savedTo / markerIndex and
// entryLog.applied on the device (gr_io.h commit_rows).
int gr_commit_update(gr_engine* e, const uint32_t* slots, const gr_update_commit* uc, size_t n, int32_t* status) {
  return slot_list_op(e, slots, uc, n, SL_UP | SL_STATUS, status, [e](const SlotArgs<const gr_update_commit>& a) {
    hipLaunchKernelGGL(io::commit_rows, a.grid, a.blk, 0, a.s, e->st, a.slots, a.recs, a.n, a.status, a.refused);
    return GR_OK;
  });
}

// Peer.ApplyConfigChange / RejectConfigChange (peer.go:153-174) for a slot list
// (gr_config_change.h, gr_io.h config_rows): 24 bytes up and 4 down per record,
// the membership itself never leaves the device.
int gr_apply_config_change(gr_engine* e, const uint32_t* slots, const gr_config_change* cc, size_t n,
                           int32_t* status) {
  return slot_list_op<const gr_config_change>(
      e, slots, cc, n, SL_UP | SL_STATUS, status,
      [e](const SlotArgs<const gr_config_change>& a) {
        return with_slots(e->S, [&](auto ss) {
          hipLaunchKernelGGL(io::config_rows<decltype(ss)::value>, a.grid, a.blk, 0, a.s, e->st, a.slots, a.recs, a.n,
                             a.status, a.refused);
          return GR_OK;
        });
      },
      // "unexpected config change type", peer.go:166-167
      [](const gr_config_change& c) { return conf::known_type(c.type); });
}

// Peer.RestoreRemotes (peer.go:177-180) for a slot list (gr_config_change.h
// restore_rows, gr_io.h restore_remote_rows): the 80-byte membership and the
// slot go up, a status comes down.
int gr_restore_remotes(gr_engine* e, const uint32_t* slots, const gr_membership* ms, size_t n, int32_t* status) {
  return slot_list_op<const gr_membership>(
      e, slots, ms, n, SL_UP | SL_STATUS, status,
      [e](const SlotArgs<const gr_membership>& a) {
        return with_slots(e->S, [&](auto ss) {
          hipLaunchKernelGGL(io::restore_remote_rows<decltype(ss)::value>, a.grid, a.blk, 0, a.s, e->st, a.slots,
                             a.recs, a.n, a.status, a.refused);
          return GR_OK;
        });
      },
      [](const gr_membership& m) { return conf::known_kinds(m); });
}

// The snapshot records of a slot list (gpuraft.h): a side array, no state row.
int gr_set_snapshot_recs(gr_engine* e, const uint32_t* slots, const gr_snapshot_rec* recs, size_t n) {
  return slot_list_op(e, slots, recs, n, SL_UP, nullptr, [e](const SlotArgs<const gr_snapshot_rec>& a) {
    hipLaunchKernelGGL(io::set_snapshot_recs, a.grid, a.blk, 0, a.s, e->snap_rec, a.slots, a.recs, a.n);
    return GR_OK;
  });
}
int gr_get_snapshot_recs(gr_engine* e, const uint32_t* slots, gr_snapshot_rec* out, size_t n) {
  return slot_list_op(e, slots, out, n, SL_DOWN, nullptr, [e](const SlotArgs<gr_snapshot_rec>& a) {
    hipLaunchKernelGGL(io::get_snapshot_recs, a.grid, a.blk, 0, a.s, (const gr_snapshot_rec*)e->snap_rec, a.slots,
                       a.recs, a.n);
    return GR_OK;
  });
}

// The config-change index records of a slot list (gpuraft.h): a side array, as
// the snapshot records.
int gr_set_cc_indexes(gr_engine* e, const uint32_t* slots, const gr_cc_index* recs, size_t n) {
  return slot_list_op(e, slots, recs, n, SL_UP, nullptr, [e](const SlotArgs<const gr_cc_index>& a) {
    hipLaunchKernelGGL(io::set_cc_indexes, a.grid, a.blk, 0, a.s, e->cc_rec, a.slots, a.recs, a.n);
    return GR_OK;
  });
}
int gr_get_cc_indexes(gr_engine* e, const uint32_t* slots, gr_cc_index* out, size_t n) {
  return slot_list_op(e, slots, out, n, SL_DOWN, nullptr, [e](const SlotArgs<gr_cc_index>& a) {
    hipLaunchKernelGGL(io::get_cc_indexes, a.grid, a.blk, 0, a.s, (const gr_cc_index*)e->cc_rec, a.slots, a.recs,
                       a.n);
    return GR_OK;
  });
}

// The update states of a slot list (gpuraft.h): a side array, as the snapshot
// records, allocated by the first call.
int gr_set_update_states(gr_engine* e, const uint32_t* slots, const gr_update_state* recs, size_t n) {
  return slot_list_op(e, slots, recs, n, SL_UP, nullptr, [e](const SlotArgs<const gr_update_state>& a) -> int {
    const int r = ensure_update_state(e);
    if (r) return r;
    hipLaunchKernelGGL(io::set_update_states, a.grid, a.blk, 0, a.s, e->upd_state, a.slots, a.recs, a.n);
    return GR_OK;
  });
}
int gr_get_update_states(gr_engine* e, const uint32_t* slots, gr_update_state* out, size_t n) {
  return slot_list_op(e, slots, out, n, SL_DOWN, nullptr, [e](const SlotArgs<gr_update_state>& a) -> int {
    const int r = ensure_update_state(e);
    if (r) return r;
    hipLaunchKernelGGL(io::get_update_states, a.grid, a.blk, 0, a.s, (const gr_update_state*)e->upd_state, a.slots,
                       a.recs, a.n);
    return GR_OK;
  });
}

// Peer.NotifyRaftLastApplied (peer.go:282-284) for a slot list: raft.applied =
// the RSM's batched last applied index, as node.handleEvents does first in
// every step (node.go:632-635,653). No other field changes.
int gr_notify_applied(gr_engine* e, const uint32_t* slots, const uint64_t* applied, size_t n) {
  return slot_list_op(e, slots, applied, n, SL_UP, nullptr, [e](const SlotArgs<const uint64_t>& a) {
    hipLaunchKernelGGL(io::set_row_u64, a.grid, a.blk, 0, a.s, e->st, (uint32_t)SR_APPLIED, a.slots, a.recs, a.n);
    return GR_OK;
  });
}

uint64_t gr_space_chunk_bytes(uint32_t positions, uint32_t depth) {
  if (depth == 0 || depth > GR_C) return 0;
  return space_chunk_bytes_pc(space_pad_positions(positions), depth);
}
uint64_t gr_space_bytes(uint32_t n_chunks, uint32_t positions, uint32_t depth) {
  return (uint64_t)n_chunks * gr_space_chunk_bytes(positions, depth);
}
uint64_t gr_space_hot_chunk_bytes(uint32_t positions, uint32_t depth) {
  if (depth == 0 || depth > GR_C) return 0;
  return space_hot_chunk_bytes_pc(space_pad_positions(positions), depth);
}
uint32_t gr_space_tile_positions(void) { return kTileW; }
uint64_t gr_space_hot_tile_bytes(uint32_t depth) {
  if (depth == 0 || depth > GR_C) return 0;
  return tile_hot_bytes(depth);
}

int gr_space_cold_used(gr_engine* e, const void* space, uint32_t n_chunks, uint32_t positions, uint32_t depth,
                       void* stream, uint32_t* out) {
  if (!e || !space || !out || depth == 0 || depth > GR_C) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  int r;
  if ((r = ensure_scal(e))) return r;
  const hipStream_t s = (hipStream_t)stream;
  const SpaceView v = make_view(space, n_chunks, positions, depth);
  uint32_t* flag = (uint32_t*)e->d_scal.p + 3;
  HIPCHK(hipMemsetAsync(flag, 0, 4, s));
  hipLaunchKernelGGL(io::cold_used, dim3(io_grid((size_t)n_chunks * v.pc)), dim3(io::kIoBlock), 0, s, v, flag);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(e->h_scal.p + 12, flag, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *out = *(uint32_t*)(e->h_scal.p + 12);
  return GR_OK;
}

uint64_t gr_space_side_bytes(uint32_t n_chunks, uint32_t depth, uint32_t capacity) {
  if (depth == 0 || depth > GR_C) return 0;
  return (uint64_t)n_chunks * io::side_chunk_bytes(depth, capacity);
}

int gr_space_side_pack(void* space, uint32_t n_chunks, uint32_t positions, uint32_t depth, void* side,
                       uint32_t capacity, void* stream) {
  if (!space || !side || depth == 0 || depth > GR_C || n_chunks == 0) return GR_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  const SpaceView v = make_view(space, n_chunks, positions, depth);
  for (uint32_t c = 0; c < n_chunks; ++c)
    HIPCHK(hipMemsetAsync((uint8_t*)side + (uint64_t)c * io::side_chunk_bytes(depth, capacity), 0, io::kSideHdr, s));
  hipLaunchKernelGGL(io::side_pack, dim3(io_grid((size_t)n_chunks * v.pc)), dim3(io::kIoBlock), 0, s, v,
                     (uint8_t*)side, capacity);
  HIPCHK(hipGetLastError());
  return GR_OK;
}

int gr_space_side_unpack(void* space, uint32_t n_chunks, uint32_t positions, uint32_t depth, const void* side,
                         uint32_t capacity, void* stream) {
  if (!space || !side || depth == 0 || depth > GR_C || n_chunks == 0) return GR_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  const SpaceView v = make_view(space, n_chunks, positions, depth);
  if (capacity) {
    hipLaunchKernelGGL(io::side_unpack, dim3(io_grid((size_t)n_chunks * capacity)), dim3(io::kIoBlock), 0, s, v,
                       (const uint8_t*)side, capacity);
    HIPCHK(hipGetLastError());
  }
  return GR_OK;
}

int gr_space_side_pack_host(void* space_host, uint32_t n_chunks, uint32_t positions, uint32_t depth,
                            void* side_host, uint32_t capacity) {
  if (!space_host || !side_host || depth == 0 || depth > GR_C || n_chunks == 0) return GR_EINVAL;
  const SpaceView v = make_view(space_host, n_chunks, positions, depth);
  uint8_t* side = (uint8_t*)side_host;
  for (uint32_t c = 0; c < n_chunks; ++c) {
    uint32_t* cnt = (uint32_t*)(side + (uint64_t)c * io::side_chunk_bytes(depth, capacity));
    *cnt = 0;
    for (uint32_t l = 0; l < v.pc; ++l) {
      const uint32_t g = c * v.pc + l;
      if (io::needs_cold(v.at(g).cnt())) io::side_put(v, g, side, capacity, (*cnt)++);
    }
  }
  return GR_OK;
}

int gr_space_side_unpack_host(void* space_host, uint32_t n_chunks, uint32_t positions, uint32_t depth,
                              const void* side_host, uint32_t capacity) {
  if (!space_host || !side_host || depth == 0 || depth > GR_C || n_chunks == 0) return GR_EINVAL;
  const SpaceView v = make_view(space_host, n_chunks, positions, depth);
  const uint8_t* side = (const uint8_t*)side_host;
  for (uint32_t c = 0; c < n_chunks; ++c) {
    const uint8_t* h = side + (uint64_t)c * io::side_chunk_bytes(depth, capacity);
    const uint32_t n = *(const uint32_t*)h;
    for (uint32_t x = 0; x < n && x < capacity; ++x) {
      const uint8_t* e = h + io::kSideHdr + (uint64_t)x * io::side_entry_bytes(depth);
      io::cold_scatter(v.at(c * v.pc + ((const uint32_t*)e)[0]), mb_n(((const uint32_t*)e)[1]), e);
    }
  }
  return GR_OK;
}

uint64_t gr_space_cx_bytes(uint32_t n_chunks, uint32_t positions, uint32_t depth, const uint32_t* capacities,
                           uint32_t side_capacity) {
  if (depth == 0 || depth > GR_C || !capacities || n_chunks > io::kCxMaxChunks) return 0;
  return io::cx_caps(space_pad_positions(positions), depth, n_chunks, capacities, side_capacity).off[n_chunks];
}

#define GR_CX_ARGS_OK(space, cx, depth, n_chunks, capacities)                                                  \
  ((space) && (cx) && (capacities) && (depth) > 0 && (depth) <= GR_C && (n_chunks) > 0 &&                     \
   (n_chunks) <= io::kCxMaxChunks)

int gr_space_cx_pack(void* space, uint32_t n_chunks, uint32_t positions, uint32_t depth, void* cx,
                     const uint32_t* capacities, uint32_t side_capacity, void* stream) {
  if (!GR_CX_ARGS_OK(space, cx, depth, n_chunks, capacities)) return GR_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  const SpaceView v = make_view(space, n_chunks, positions, depth);
  const io::CxCaps C = io::cx_caps(v.pc, depth, n_chunks, capacities, side_capacity);
  for (uint32_t c = 0; c < n_chunks; ++c) HIPCHK(hipMemsetAsync((uint8_t*)cx + C.off[c], 0, io::kCxHdr, s));
  const uint32_t nwv = v.pc / 64;
  hipLaunchKernelGGL(io::cx_pack, dim3((nwv + io::kCxPackGroups - 1) / io::kCxPackGroups, n_chunks),
                     dim3(io::kIoBlock), 0, s, v, (uint8_t*)cx, C);
  HIPCHK(hipGetLastError());
  return GR_OK;
}

int gr_space_cx_unpack(void* space, uint32_t n_chunks, uint32_t positions, uint32_t depth, const void* cx,
                       const uint32_t* capacities, uint32_t side_capacity, void* stream) {
  if (!GR_CX_ARGS_OK(space, cx, depth, n_chunks, capacities)) return GR_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  const SpaceView v = make_view(space, n_chunks, positions, depth);
  const io::CxCaps C = io::cx_caps(v.pc, depth, n_chunks, capacities, side_capacity);
  const uint32_t nwv = v.pc / 64;
  hipLaunchKernelGGL(io::cx_unpack_waves, dim3((nwv + io::kCxUnpackGroups - 1) / io::kCxUnpackGroups, n_chunks),
                     dim3(io::kIoBlock), 0, s, v, (const uint8_t*)cx, C);
  HIPCHK(hipGetLastError());
  if (side_capacity) {
    hipLaunchKernelGGL(io::cx_unpack_side, dim3(io_grid((size_t)n_chunks * side_capacity)), dim3(io::kIoBlock), 0, s,
                       v, (const uint8_t*)cx, C);
    HIPCHK(hipGetLastError());
  }
  return GR_OK;
}

// The same codec over host memory (tests): records in the device's regions
// (wave group wl belongs to pack workgroup wl / kCxPackGroups, whose region is
// that workgroup's index modulo cx_regions), each region and the side entries
// filled in position order (the device packer's order within a region may
// differ; what unpacks does not).
int gr_space_cx_pack_host(void* space_host, uint32_t n_chunks, uint32_t positions, uint32_t depth, void* cx_host,
                          const uint32_t* capacities, uint32_t side_capacity) {
  if (!GR_CX_ARGS_OK(space_host, cx_host, depth, n_chunks, capacities)) return GR_EINVAL;
  const SpaceView v = make_view(space_host, n_chunks, positions, depth);
  const io::CxCaps C = io::cx_caps(v.pc, depth, n_chunks, capacities, side_capacity);
  for (uint32_t c = 0; c < n_chunks; ++c) {
    const uint32_t capacity = C.cap[c];
    const io::CxLayout L = io::cx_layout(v.pc, depth, capacity, side_capacity);
    uint8_t* buf = (uint8_t*)cx_host + C.off[c];
    memset(buf, 0, io::kCxHdr);
    uint32_t* ctr = (uint32_t*)buf;
    uint32_t* nside = ctr + io::kCxSub * io::kCxCtr;
    const uint32_t nreg = io::cx_regions(L.nwv);
    for (uint32_t wl = 0; wl < L.nwv; ++wl) {
      const uint32_t reg = (wl / io::kCxPackGroups) % nreg;
      uint32_t roff, rcap;
      io::cx_region(L.nwv, capacity, reg, &roff, &rcap);
      uint32_t* nrec = ctr + reg * io::kCxCtr;
      uint32_t hi = 0;
      bool have = false;
      for (uint32_t lane = 0; lane < 64 && !have; ++lane) {
        const Mailbox mb = v.at(c * v.pc + wl * 64 + lane);
        const uint32_t cb = mb.cnt();
        uint32_t w3;
        uint64_t li;
        bool anch;
        if (mb_n(cb) && io::cx_classify(mb, cb, depth, &w3, &li, &anch) && anch) {
          hi = (uint32_t)(li >> 32);
          have = true;
        }
      }
      uint64_t mask = 0, lost = 0;
      const uint32_t base = roff + *nrec;
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t pos = wl * 64 + lane;
        const Mailbox mb = v.at(c * v.pc + pos);
        const uint32_t cb = mb.cnt();
        uint32_t w3 = 0;
        uint64_t li = 0;
        bool anch = false;
        const bool rec = mb_n(cb) && io::cx_classify(mb, cb, depth, &w3, &li, &anch) &&
                         (!anch || (uint32_t)(li >> 32) == hi);
        if (rec && *nrec < rcap) {
          io::cx_put_record(io::cx_term_of(mb, cb), li, w3, buf, L, roff + (*nrec)++);
          mask |= 1ull << lane;
          continue;
        }
        if (rec) ++*nrec;  // counted, as the device's atomic counts it
        if (!mb_n(cb)) continue;
        if (*nside < side_capacity) io::cx_put_side(mb, cb, pos, buf, L, depth, *nside);
        else lost |= 1ull << lane;
        ++*nside;
      }
      uint8_t* h = buf + L.waves + (uint64_t)wl * io::kCxWave;
      ((uint64_t*)h)[0] = mask;
      ((uint64_t*)h)[1] = lost;
      ((uint32_t*)h)[4] = base;
      ((uint32_t*)h)[5] = hi;
    }
  }
  return GR_OK;
}

int gr_space_cx_unpack_host(void* space_host, uint32_t n_chunks, uint32_t positions, uint32_t depth,
                            const void* cx_host, const uint32_t* capacities, uint32_t side_capacity) {
  if (!GR_CX_ARGS_OK(space_host, cx_host, depth, n_chunks, capacities)) return GR_EINVAL;
  const SpaceView v = make_view(space_host, n_chunks, positions, depth);
  const io::CxCaps C = io::cx_caps(v.pc, depth, n_chunks, capacities, side_capacity);
  for (uint32_t c = 0; c < n_chunks; ++c) {
    const io::CxLayout L = io::cx_layout(v.pc, depth, C.cap[c], side_capacity);
    const uint8_t* buf = (const uint8_t*)cx_host + C.off[c];
    for (uint32_t wl = 0; wl < L.nwv; ++wl) {
      const uint8_t* h = buf + L.waves + (uint64_t)wl * io::kCxWave;
      for (uint32_t lane = 0; lane < 64; ++lane)
        io::cx_get_lane(v.at(c * v.pc + wl * 64 + lane), buf, L, ((const uint64_t*)h)[0], ((const uint64_t*)h)[1],
                        ((const uint32_t*)h)[4], ((const uint32_t*)h)[5], lane);
    }
    const uint32_t ns = ((const uint32_t*)buf)[io::kCxSub * io::kCxCtr];
    for (uint32_t x = 0; x < ns && x < side_capacity; ++x) {
      const uint8_t* e = buf + L.side + (uint64_t)x * io::cx_side_entry_bytes(depth);
      io::cx_get_side(v.at(c * v.pc + ((const uint32_t*)e)[0]), e, depth);
    }
  }
  return GR_OK;
}

int gr_space_encode(void* space_host, uint32_t n_chunks, uint32_t positions, uint32_t depth,
                    const gr_message* msgs, size_t n, const uint32_t* pos_of_msg) {
  if (!space_host || (n && (!msgs || !pos_of_msg)) || depth == 0 || depth > GR_C) return GR_EINVAL;
  const SpaceView v = make_view(space_host, n_chunks, positions, depth);
  for (size_t k = 0; k < n; ++k) {
    const uint32_t g = pos_of_msg[k];
    if (g / v.pc >= n_chunks || g % v.pc >= positions) return GR_ERANGE;
    const Mailbox mb = v.at(g);
    const uint8_t c = (uint8_t)mb_n(mb.cnt());
    if (c >= depth) return GR_ECAPACITY;
    encode_msg(mb, c, msgs[k]);
    mb.cnt() = (uint8_t)(c + 1);
  }
  return GR_OK;
}

int gr_space_decode(const void* space_host, uint32_t n_chunks, uint32_t positions, uint32_t depth,
                    gr_message* out, size_t cap, size_t* n_out) {
  if (!space_host || !n_out || depth == 0 || depth > GR_C) return GR_EINVAL;
  const SpaceView v = make_view(space_host, n_chunks, positions, depth);
  size_t n = 0;
  for (uint32_t c = 0; c < n_chunks; ++c) {
    for (uint32_t l = 0; l < positions; ++l) {
      const uint32_t g = c * v.pc + l;
      const Mailbox mb = v.at(g);
      const uint32_t cb = mb.cnt(), cnt = std::min<uint32_t>(mb_n(cb), depth);
      const bool lost = !(cb & MB_UNIFORM) && (cb & MB_COLD_LOST);  // cold fields not delivered
      for (uint32_t k = 0; k < cnt; ++k) {
        if (out && n < cap) {
          if (lost) {
            memset(&out[n], 0, sizeof(gr_message));
            out[n].reject = 0xFF;  // a record whose fields were lost in the exchange
          } else {
            out[n] = decode_msg(mb, k);
          }
          out[n].peer = g;
          out[n].slot = (uint8_t)k;
        }
        n++;
      }
    }
  }
  *n_out = n;
  return n <= cap || !out ? GR_OK : GR_ECAPACITY;
}

// The outbox mailboxes and lane results of the pass just launched, as compact
// records (+ ext records where they do not fit), downloaded into engine-owned
// pinned memory: gr_step_compact_end and gr_step_wire_compact.
static int pack_out_compact(gr_engine* e, uint32_t nl, const SpaceView& vout, gr_coutbox* out, PhaseClock* cl,
                            const gr_wire_out_cfg* wcfg, gr_wire_out* wout) {
  PhaseClock& clk = *cl;
  const uint32_t S = e->S;
  const hipStream_t s = e->stream;
  const dim3 blk(io::kIoBlock);
  int r;
  uint32_t* scal = (uint32_t*)e->d_scal.p;
  uint32_t* peer_of_lane = e->ln.u32(LR_LANE_PEER);
  // ---- outbox mailboxes + lane results -> compact records (+ ext)
  if ((r = e->d_oc64.grow((size_t)nl * 8))) return r;
  if ((r = e->d_off64.grow((size_t)nl * 8))) return r;
  if ((r = e->d_rx.grow((size_t)nl * 4))) return r;
  if ((r = e->d_roff.grow((size_t)nl * 4))) return r;
  if ((r = e->d_results.grow((size_t)nl * sizeof(gr_cresult)))) return r;
  uint64_t* oc = (uint64_t*)e->d_oc64.p;
  uint64_t* off = (uint64_t*)e->d_off64.p;
  uint32_t* rx = (uint32_t*)e->d_rx.p;
  uint32_t* roff = (uint32_t*)e->d_roff.p;
  // ---- gr_step_wire_out: the entry-free mailboxes leave as MessageBatch records
  // (gr_io.h wire_out_*): classified and ranked first, so the compact pack skips them
  const uint8_t* wf = nullptr;
  const uint32_t T = e->n_targets, nblk = (nl + io::kIoBlock - 1) / io::kIoBlock;
  if (wout) {
    const size_t pairs = (size_t)nl * S, cells = (size_t)T * nblk;
    if ((r = e->d_wf.grow(pairs))) return r;
    if ((r = e->d_wrank.grow(pairs * 4))) return r;
    if ((r = e->d_wcnt.grow(cells * 4))) return r;
    if ((r = e->d_wbase.grow(cells * 4))) return r;
    if ((r = e->d_wplan.grow((2 * (size_t)GR_MAX_TARGETS + 2) * 4))) return r;
    if ((r = e->d_wtot.grow(8))) return r;
    if ((r = e->h_wtot.grow(8))) return r;
    const uint32_t* tgt = (const uint32_t*)e->d_target.p;
    uint32_t* wrank = (uint32_t*)e->d_wrank.p;
    uint32_t* wcnt = (uint32_t*)e->d_wcnt.p;
    if ((r = with_slots(S, [&](auto ss) {
          hipLaunchKernelGGL(io::wire_out_group<decltype(ss)::value>, dim3(nblk), blk, 0, s, vout, nl,
                             (const uint32_t*)peer_of_lane, tgt, T, e->d_wf.as<uint8_t>(), wrank, wcnt);
          return GR_OK;
        })))
      return r;
    HIPCHK(hipGetLastError());
    if ((r = io_scan(e, wcnt, (uint32_t*)e->d_wbase.p, (uint32_t)cells, s))) return r;
    hipLaunchKernelGGL(io::wire_out_plan, dim3(1), blk, 0, s, (const uint32_t*)wcnt, (const uint32_t*)e->d_wbase.p, T,
                       nblk, wcfg->max_batch_msgs, (uint32_t*)e->d_wplan.p, (uint32_t*)e->d_wtot.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(e->h_wtot.p, e->d_wtot.p, 8, hipMemcpyDeviceToHost, s));
    wf = (const uint8_t*)e->d_wf.p;
  }
  hipLaunchKernelGGL(io::out_counts_c, dim3(io_grid(nl)), blk, 0, s, vout, e->ln, e->st, nl, S, oc, rx, wf);
  HIPCHK(hipGetLastError());
  if ((r = io_scan64(e, oc, off, nl, s))) return r;
  if ((r = io_scan(e, rx, roff, nl, s))) return r;
  hipLaunchKernelGGL(io::finish_total_c, dim3(1), dim3(64), 0, s, (const uint64_t*)oc, (const uint64_t*)off,
                     (const uint32_t*)rx, (const uint32_t*)roff, nl, scal + 1);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(e->h_scal.p + 4, scal + 1, 12, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  clk.mark("mailboxes+pass+counts");
  const uint32_t total = ((uint32_t*)e->h_scal.p)[1], text = ((uint32_t*)e->h_scal.p)[2], rext = ((uint32_t*)e->h_scal.p)[3];
  const size_t mbytes = (size_t)total * sizeof(gr_cmsg), xbytes = (size_t)text * sizeof(gr_message);
  const size_t rbytes = (size_t)nl * sizeof(gr_cresult), rxbytes = (size_t)rext * sizeof(gr_peer_result);
  if ((r = e->d_outmsgs.grow(mbytes + 1))) return r;
  if ((r = e->d_outext.grow(xbytes + 1))) return r;
  if ((r = e->d_resext.grow(rxbytes + 1))) return r;
  if ((r = e->h_outmsgs.grow(mbytes + 1))) return r;
  if ((r = e->h_outext.grow(xbytes + 1))) return r;
  if ((r = e->h_results.grow(rbytes))) return r;
  if ((r = e->h_resext.grow(rxbytes + 1))) return r;
  hipLaunchKernelGGL(io::pack_results_c, dim3(io_grid(nl)), blk, 0, s, e->ln, e->st, (const uint32_t*)peer_of_lane,
                     nl, (const uint32_t*)roff, (gr_cresult*)e->d_results.p, (gr_peer_result*)e->d_resext.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(e->h_results.p, e->d_results.p, rbytes, hipMemcpyDeviceToHost, s));
  if (rext) HIPCHK(hipMemcpyAsync(e->h_resext.p, e->d_resext.p, rxbytes, hipMemcpyDeviceToHost, s));
  if (total) {
    hipLaunchKernelGGL(io::pack_outbox_c, dim3(io_grid(nl)), blk, 0, s, vout, nl, S, (const uint64_t*)off,
                       (const uint32_t*)peer_of_lane, (gr_cmsg*)e->d_outmsgs.p, (gr_message*)e->d_outext.p, wf);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(e->h_outmsgs.p, e->d_outmsgs.p, mbytes, hipMemcpyDeviceToHost, s));
    if (text) HIPCHK(hipMemcpyAsync(e->h_outext.p, e->d_outext.p, xbytes, hipMemcpyDeviceToHost, s));
  }
  uint32_t wn = 0, wnb = 0;
  if (wout) {  // the totals came down with the counts above
    wn = ((uint32_t*)e->h_wtot.p)[0];
    wnb = ((uint32_t*)e->h_wtot.p)[1];
    if ((r = e->d_wmsgs.grow((size_t)wn * sizeof(grw_message) + 1))) return r;
    if ((r = e->d_wbat.grow((size_t)wnb * sizeof(grw_batch) + 1))) return r;
    if ((r = e->d_wbt.grow((size_t)wnb * 4 + 4))) return r;
    if ((r = e->h_wbt.grow((size_t)wnb * 4 + 4))) return r;
    if (wn) {
      const uint32_t* tgt = (const uint32_t*)e->d_target.p;
      const uint64_t* clu = (const uint64_t*)e->d_cluster.p;
      const uint32_t* wrank = (const uint32_t*)e->d_wrank.p;
      const uint32_t* wbase = (const uint32_t*)e->d_wbase.p;
      const uint32_t* plan = (const uint32_t*)e->d_wplan.p;
      const uint32_t mbm = wcfg->max_batch_msgs;
      grw_message* wm = (grw_message*)e->d_wmsgs.p;
      if ((r = with_slots(S, [&](auto ss) {
            hipLaunchKernelGGL(io::wire_out_scatter<decltype(ss)::value>, dim3(nblk), blk, 0, s, vout, nl,
                               (const uint32_t*)peer_of_lane, tgt, e->st, clu, wf, wrank, wbase, plan, T, mbm, wm);
            return GR_OK;
          })))
        return r;
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(io::wire_out_batches, dim3(io_grid(wnb)), blk, 0, s, plan, T, *wcfg, wnb,
                         (grw_batch*)e->d_wbat.p, (uint32_t*)e->d_wbt.p);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(e->h_wbt.p, e->d_wbt.p, (size_t)wnb * 4, hipMemcpyDeviceToHost, s));
    }
  }
  HIPCHK(hipStreamSynchronize(s));
  clk.mark("pack+download");
  clk.report();
  out->msgs = total ? (gr_cmsg*)e->h_outmsgs.p : nullptr;
  out->n_msgs = total;
  out->ext_msgs = text ? (gr_message*)e->h_outext.p : nullptr;
  out->n_ext_msgs = text;
  out->results = (gr_cresult*)e->h_results.p;
  out->n_results = nl;
  out->ext_results = rext ? (gr_peer_result*)e->h_resext.p : nullptr;
  out->n_ext_results = rext;
  if (wout) {
    wout->d_batches = wnb ? (grw_batch*)e->d_wbat.p : nullptr;
    wout->n_batches = wnb;
    wout->d_msgs = wn ? (const grw_message*)e->d_wmsgs.p : nullptr;
    wout->n_msgs = wn;
    wout->batch_target = wnb ? (const uint32_t*)e->h_wbt.p : nullptr;
  }
  return GR_OK;
}

// The device pass of gr_step over nm gr_message records already in e->d_msgs
// (copied from the host by gr_step, or routed from decoded wire records by
// gr_step_wire) and nlc host local inputs; the outbox as full records (out) or,
// with cout, as compact records (gr_step_wire_compact). Caller holds e->mu.
static int step_staged(gr_engine* e, uint32_t nm, const gr_local_input* locals, uint32_t nlc, gr_outbox* out,
                       gr_coutbox* cout = nullptr, const gr_wire_out_cfg* wcfg = nullptr,
                       gr_wire_out* wout = nullptr) {
  if (out) {
    out->msgs = nullptr;
    out->n_msgs = 0;
    out->results = nullptr;
    out->n_results = 0;
  }
  if (cout) memset(cout, 0, sizeof(*cout));
  if (nm + nlc == 0) return GR_OK;
  const uint32_t S = e->S;
  const hipStream_t s = e->stream;
  const dim3 blk(io::kIoBlock);
  int r;
  if ((r = e->d_locals.grow((size_t)nlc * sizeof(gr_local_input) + 1))) return r;
  if (nlc)
    HIPCHK(hipMemcpyAsync(e->d_locals.p, locals, (size_t)nlc * sizeof(gr_local_input), hipMemcpyHostToDevice, s));
  const FullInbox in{e->d_msgs.as<const gr_message>(), nm, e->d_locals.as<const gr_local_input>(), nlc};
  uint32_t nl, err;
  if ((r = stage_lanes(e, in, &nl, &err))) return r;
  if (err) return GR_EINVAL;  // nothing of the pass ran
  if (nl == 0) return GR_OK;
  SpaceView vout;
  if ((r = run_staged_pass(e, in, nl, &vout))) return r;
  if (cout) {
    PhaseClock clk;
    return pack_out_compact(e, nl, vout, cout, &clk, wcfg, wout);
  }
  uint32_t* scal = e->d_scal.as<uint32_t>();
  uint32_t* peer_of_lane = e->ln.u32(LR_LANE_PEER);
  // ---- outbox mailboxes + lane results -> records
  if ((r = e->d_oc.grow((size_t)nl * 4))) return r;
  if ((r = e->d_off.grow((size_t)nl * 4))) return r;
  if ((r = e->d_results.grow((size_t)nl * sizeof(gr_peer_result)))) return r;
  uint32_t* oc = (uint32_t*)e->d_oc.p;
  uint32_t* off = (uint32_t*)e->d_off.p;
  hipLaunchKernelGGL(io::out_counts, dim3(io_grid(nl)), blk, 0, s, vout, nl, S, oc);
  HIPCHK(hipGetLastError());
  if ((r = io_scan(e, oc, off, nl, s))) return r;
  hipLaunchKernelGGL(io::finish_total, dim3(1), dim3(64), 0, s, (const uint32_t*)oc, (const uint32_t*)off, nl,
                     scal + 2);
  hipLaunchKernelGGL(io::pack_results, dim3(io_grid(nl)), blk, 0, s, e->ln, e->st, (const uint32_t*)peer_of_lane,
                     0u, nl, (gr_peer_result*)e->d_results.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(e->h_scal.p + 8, scal + 2, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const uint32_t total = ((uint32_t*)e->h_scal.p)[2];
  const size_t mbytes = (size_t)total * sizeof(gr_message), rbytes = (size_t)nl * sizeof(gr_peer_result);
  if ((r = e->d_outmsgs.grow(mbytes + 1))) return r;
  if ((r = e->h_outmsgs.grow(mbytes + 1))) return r;
  if ((r = e->h_results.grow(rbytes))) return r;
  if (total) {
    hipLaunchKernelGGL(io::pack_outbox, dim3(io_grid(nl)), blk, 0, s, vout, nl, S, (const uint32_t*)off,
                       (const uint32_t*)peer_of_lane, (gr_message*)e->d_outmsgs.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(e->h_outmsgs.p, e->d_outmsgs.p, mbytes, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipMemcpyAsync(e->h_results.p, e->d_results.p, rbytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  out->msgs = total ? (gr_message*)e->h_outmsgs.p : nullptr;
  out->n_msgs = total;
  out->results = (gr_peer_result*)e->h_results.p;
  out->n_results = nl;
  return GR_OK;
}

int gr_step(gr_engine* e, const gr_inbox* in, gr_outbox* out) {
  if (!e || !in || !out) return GR_EINVAL;
  if ((in->n_msgs && !in->msgs) || (in->n_locals && !in->locals)) return GR_EINVAL;
  if (in->n_msgs + in->n_locals >= 0x80000000ull) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  const uint32_t nm = (uint32_t)in->n_msgs;
  int r;
  if ((r = e->d_msgs.grow((size_t)nm * sizeof(gr_message) + 1))) return r;
  if (nm)
    HIPCHK(hipMemcpyAsync(e->d_msgs.p, in->msgs, (size_t)nm * sizeof(gr_message), hipMemcpyHostToDevice, e->stream));
  return step_staged(e, nm, in->locals, (uint32_t)in->n_locals, out);
}

// ---------------------------------------------------------------- wire path
// gr_bind_nodes: the (cluster id, node id) -> engine slot table the wire path
// routes decoded messages with (open addressing, twice the slots, power of two).
int gr_bind_nodes(gr_engine* e, const uint64_t* cluster_ids, const uint64_t* node_ids, uint32_t n) {
  if (!e || (n && (!cluster_ids || !node_ids)) || n > e->cfg.max_peers) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  uint32_t tcap = 64;
  while (tcap < 2 * n) tcap <<= 1;
  std::vector<io::NodeKey> t(tcap);
  for (uint32_t p = 0; p < n; ++p) {
    uint32_t h = io::node_hash(cluster_ids[p], node_ids[p]) & (tcap - 1);
    while (t[h].peer != NOPOS) {
      if (t[h].cluster == cluster_ids[p] && t[h].node == node_ids[p]) return GR_EINVAL;  // listed twice
      h = (h + 1) & (tcap - 1);
    }
    t[h].cluster = cluster_ids[p];
    t[h].node = node_ids[p];
    t[h].peer = p;
  }
  int r;
  if ((r = e->d_nodes.grow((size_t)tcap * sizeof(io::NodeKey)))) return r;
  HIPCHK(hipMemcpy(e->d_nodes.p, t.data(), (size_t)tcap * sizeof(io::NodeKey), hipMemcpyHostToDevice));
  // the cluster id of every slot (0 above n): the outbound records' ClusterID
  const size_t cap = e->cfg.max_peers;
  if ((r = e->d_cluster.grow(cap * 8 + 8))) return r;
  HIPCHK(hipMemset(e->d_cluster.p, 0, cap * 8));
  if (n) HIPCHK(hipMemcpy(e->d_cluster.p, cluster_ids, (size_t)n * 8, hipMemcpyHostToDevice));
  e->nodes_cap = tcap;
  return GR_OK;
}

// gr_bind_targets: the send queue of every (engine slot, remote slot) pair. The
// caller's rows hold gr_config.slots values; the device copy has the instantiated
// slot count's (e->S) columns per row, as the kernels index it, the columns the
// configuration does not have filled with GR_TARGET_HOST.
int gr_bind_targets(gr_engine* e, const uint32_t* target_of, uint32_t n_peers, uint32_t n_targets) {
  if (!e || n_peers > e->cfg.max_peers) return GR_EINVAL;
  const uint32_t slots = e->cfg.slots, S = e->S;
  if (!host::wire_out_args_ok(target_of, (size_t)n_peers * slots, n_targets, nullptr)) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  const size_t all = (size_t)e->cfg.max_peers * S;
  std::vector<uint32_t> t(all, GR_TARGET_HOST);
  for (uint32_t p = 0; p < n_peers; ++p)
    std::copy(target_of + (size_t)p * slots, target_of + (size_t)(p + 1) * slots, t.begin() + (size_t)p * S);
  int r;
  if ((r = e->d_target.grow(all * 4 + 4))) return r;
  HIPCHK(hipMemcpy(e->d_target.p, t.data(), all * 4, hipMemcpyHostToDevice));
  e->n_targets = n_targets;
  return GR_OK;
}

// The wire path's routing half (gr_step_wire, gr_step_wire_compact): decoded
// records -> routed gr_message records in e->d_msgs (*nm of them), the rest
// listed in *unrouted. Called with e->mu held.
static int wire_route(gr_engine* e, const struct grw_message* d_msgs, size_t n_msgs, const struct grw_entry* d_ents,
                      size_t n_ents, gr_wire_unrouted* unrouted, uint32_t* nm_out) {
  *nm_out = 0;
  unrouted->n = 0;
  unrouted->index = nullptr;
  unrouted->reason = nullptr;
  if (n_msgs && !e->nodes_cap) return GR_ESTATE;  // gr_bind_nodes first
  const uint32_t nw = (uint32_t)n_msgs;
  const hipStream_t s = e->stream;
  const dim3 blk(io::kIoBlock);
  int r;
  if ((r = e->d_msgs.grow((size_t)nw * sizeof(gr_message) + 1))) return r;
  uint32_t nm = 0;
  if (nw) {
    // route every decoded message to (slot, sender slot) in a gr_message record,
    // then keep the routed ones in wire order (their arrival order)
    if ((r = e->d_wrec.grow((size_t)nw * sizeof(gr_message)))) return r;
    if ((r = e->d_keys.grow((size_t)nw * 4 + 4))) return r;
    if ((r = e->d_idx.grow((size_t)nw * 4 + 4))) return r;
    if ((r = e->d_why.grow((size_t)nw + 1))) return r;
    if ((r = e->d_unr.grow((size_t)nw * 4 + 4))) return r;
    if ((r = ensure_scal(e))) return r;
    uint32_t* flag = (uint32_t*)e->d_keys.p;
    uint32_t* pos = (uint32_t*)e->d_idx.p;
    uint32_t* scal = (uint32_t*)e->d_scal.p;
    if ((r = with_slots(e->S, [&](auto ss) {
          hipLaunchKernelGGL(io::route_wire<decltype(ss)::value>, dim3(io_grid(nw)), blk, 0, s, d_msgs, nw, d_ents,
                             (uint64_t)n_ents, e->d_nodes.as<const io::NodeKey>(), e->nodes_cap, e->st,
                             e->d_wrec.as<gr_message>(), flag, e->d_why.as<uint8_t>(), (uint32_t)e->config_entries);
          return GR_OK;
        })))
      return r;
    HIPCHK(hipGetLastError());
    if ((r = io_scan(e, flag, pos, nw, s))) return r;
    hipLaunchKernelGGL(io::keep_routed, dim3(io_grid(nw)), blk, 0, s, (const gr_message*)e->d_wrec.p,
                       (const uint32_t*)flag, (const uint32_t*)pos, nw, (gr_message*)e->d_msgs.p,
                       (uint32_t*)e->d_unr.p, scal);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(e->h_scal.p, scal, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    nm = ((uint32_t*)e->h_scal.p)[0];
    const uint32_t nu = nw - nm;
    if (nu) {  // the messages the host steps with the Go code, in wire order, and why
      if ((r = e->h_unr.grow((size_t)nu * 5))) return r;
      uint32_t* hidx = (uint32_t*)e->h_unr.p;
      uint8_t* hwhy = e->h_unr.p + (size_t)nu * 4;
      HIPCHK(hipMemcpyAsync(hidx, e->d_unr.p, (size_t)nu * 4, hipMemcpyDeviceToHost, s));
      std::vector<uint8_t> allwhy(nw);
      HIPCHK(hipMemcpyAsync(allwhy.data(), e->d_why.p, nw, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      for (uint32_t k = 0; k < nu; ++k) hwhy[k] = allwhy[hidx[k]];
      unrouted->n = nu;
      unrouted->index = hidx;
      unrouted->reason = hwhy;
    }
  }
  *nm_out = nm;
  return GR_OK;
}

int gr_step_wire(gr_engine* e, const struct grw_message* d_msgs, size_t n_msgs, const struct grw_entry* d_ents,
                 size_t n_ents, const gr_local_input* locals, size_t n_locals, gr_outbox* out,
                 gr_wire_unrouted* unrouted) {
  if (!e || !out || !unrouted || (n_msgs && !d_msgs) || (n_locals && !locals)) return GR_EINVAL;
  if (n_msgs + n_locals >= 0x80000000ull) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  uint32_t nm;
  int r;
  if ((r = wire_route(e, d_msgs, n_msgs, d_ents, n_ents, unrouted, &nm))) return r;
  return step_staged(e, nm, locals, (uint32_t)n_locals, out);
}

int gr_step_wire_compact(gr_engine* e, const struct grw_message* d_msgs, size_t n_msgs,
                         const struct grw_entry* d_ents, size_t n_ents, const gr_local_input* locals,
                         size_t n_locals, gr_coutbox* out, gr_wire_unrouted* unrouted) {
  if (!e || !out || !unrouted || (n_msgs && !d_msgs) || (n_locals && !locals)) return GR_EINVAL;
  if (n_msgs + n_locals >= 0x80000000ull) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  uint32_t nm;
  int r;
  if ((r = wire_route(e, d_msgs, n_msgs, d_ents, n_ents, unrouted, &nm))) return r;
  return step_staged(e, nm, locals, (uint32_t)n_locals, nullptr, out);
}

int gr_step_wire_out(gr_engine* e, const struct grw_message* d_msgs, size_t n_msgs, const struct grw_entry* d_ents,
                     size_t n_ents, const gr_local_input* locals, size_t n_locals, gr_coutbox* out,
                     gr_wire_unrouted* unrouted, const gr_wire_out_cfg* cfg, gr_wire_out* wout) {
  if (!e || !out || !unrouted || !cfg || !wout || (n_msgs && !d_msgs) || (n_locals && !locals)) return GR_EINVAL;
  if (n_msgs + n_locals >= 0x80000000ull || cfg->max_batch_msgs == 0) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  if (!e->nodes_cap || !e->n_targets) return GR_ESTATE;  // gr_bind_nodes and gr_bind_targets first
  memset(wout, 0, sizeof(*wout));
  uint32_t nm;
  int r;
  if ((r = wire_route(e, d_msgs, n_msgs, d_ents, n_ents, unrouted, &nm))) return r;
  return step_staged(e, nm, locals, (uint32_t)n_locals, nullptr, out, cfg, wout);
}

// gr_step with compact records (gpuraft.h gr_cmsg / gr_clocal / gr_cresult):
// the same device passes; records expand in registers on the way in and are
// packed (with ext records for what does not fit) on the way out.
static int compact_begin_locked(gr_engine* e, const gr_cinbox* in);
int gr_step_compact_begin(gr_engine* e, const gr_cinbox* in) {
  if (!e || !in) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  return compact_begin_locked(e, in);
}

// gr_step_compact_begin with e->mu held
static int compact_begin_locked(gr_engine* e, const gr_cinbox* in) {
  if ((in->n_msgs && !in->msgs) || (in->n_locals && !in->locals) || (in->n_ext_msgs && !in->ext_msgs) ||
      (in->n_ext_locals && !in->ext_locals))
    return GR_EINVAL;
  if (in->n_msgs + in->n_locals >= 0x80000000ull || in->n_ext_msgs >= 0x80000000ull ||
      in->n_ext_locals >= 0x80000000ull)
    return GR_EINVAL;
  if (e->cpend.on) return GR_EINVAL;  // the previous begin was not ended
  GR_REFUSE_PENDING(e);
  PhaseClock clk;  // GR_PHASES=1: per-phase host times on stderr
  const uint32_t nm = (uint32_t)in->n_msgs, nlc = (uint32_t)in->n_locals;
  const uint32_t nx = (uint32_t)in->n_ext_msgs, nlx = (uint32_t)in->n_ext_locals;
  e->cpend = gr_engine::CPending{};
  if (nm + nlc == 0) {
    e->cpend.on = true;  // an empty pass: _end returns an empty outbox
    e->pending.store(true, std::memory_order_release);
    return GR_OK;
  }
  const hipStream_t s = e->stream;
  int r;
  if ((r = e->d_msgs.grow((size_t)nm * sizeof(gr_cmsg) + 1))) return r;
  if ((r = e->d_locals.grow((size_t)nlc * sizeof(gr_clocal) + 1))) return r;
  if ((r = e->d_ext.grow((size_t)nx * sizeof(gr_message) + 1))) return r;
  if ((r = e->d_lext.grow((size_t)nlx * sizeof(gr_local_input) + 1))) return r;
  if (nm) HIPCHK(hipMemcpyAsync(e->d_msgs.p, in->msgs, (size_t)nm * sizeof(gr_cmsg), hipMemcpyHostToDevice, s));
  if (nlc) HIPCHK(hipMemcpyAsync(e->d_locals.p, in->locals, (size_t)nlc * sizeof(gr_clocal), hipMemcpyHostToDevice, s));
  if (nx) HIPCHK(hipMemcpyAsync(e->d_ext.p, in->ext_msgs, (size_t)nx * sizeof(gr_message), hipMemcpyHostToDevice, s));
  if (nlx)
    HIPCHK(hipMemcpyAsync(e->d_lext.p, in->ext_locals, (size_t)nlx * sizeof(gr_local_input), hipMemcpyHostToDevice, s));
  uint32_t nl, err;
  if ((r = stage_lanes(e, CompactInbox(e, nm, nlc, nx, nlx), &nl, &err))) return r;
  clk.mark("upload+lanes");
  if (err) return GR_EINVAL;  // nothing of the pass ran
  e->cpend.on = true;
  e->pending.store(true, std::memory_order_release);
  e->cpend.nm = nm;
  e->cpend.nlc = nlc;
  e->cpend.nx = nx;
  e->cpend.nlx = nlx;
  e->cpend.nl = nl;
  return GR_OK;
}

static int compact_end_locked(gr_engine* e, gr_coutbox* out, const gr_wire_out_cfg* wcfg, gr_wire_out* wout);
int gr_step_compact_end(gr_engine* e, gr_coutbox* out) {
  if (!e || !out) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  return compact_end_locked(e, out, nullptr, nullptr);
}

// gr_step_compact_end with e->mu held; with wout, gr_step_compact_wire_out's second half
static int compact_end_locked(gr_engine* e, gr_coutbox* out, const gr_wire_out_cfg* wcfg, gr_wire_out* wout) {
  if (!e->cpend.on) return GR_EINVAL;  // no pass was begun
  const gr_engine::CPending pend = e->cpend;
  e->cpend.on = false;
  // `pending` stays set until this call returns (every path): the pass below
  // still uses the lane rows, bail lists and scratch the flag protects
  struct ClearPending {
    std::atomic<bool>& f;
    ~ClearPending() { f.store(false, std::memory_order_release); }
  } clear_pending{e->pending};
  memset(out, 0, sizeof(*out));
  PhaseClock clk;
  if (pend.nl == 0) return GR_OK;
  SpaceView vout;
  int r;
  if ((r = run_staged_pass(e, CompactInbox(e, pend.nm, pend.nlc, pend.nx, pend.nlx), pend.nl, &vout))) return r;
  return pack_out_compact(e, pend.nl, vout, out, &clk, wcfg, wout);
}

int gr_step_compact(gr_engine* e, const gr_cinbox* in, gr_coutbox* out) {
  if (!e || !in || !out) return GR_EINVAL;
  memset(out, 0, sizeof(*out));
  const int r = gr_step_compact_begin(e, in);
  return r ? r : gr_step_compact_end(e, out);
}

int gr_step_compact_wire_out(gr_engine* e, const gr_cinbox* in, gr_coutbox* out, const gr_wire_out_cfg* cfg,
                             gr_wire_out* wout) {
  if (!e || !in || !out || !cfg || !wout || cfg->max_batch_msgs == 0) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);  // held over the check and both halves, as gr_step_wire_out
  GR_REFUSE_PENDING(e);
  if (!e->nodes_cap || !e->n_targets) return GR_ESTATE;  // gr_bind_nodes and gr_bind_targets first
  memset(out, 0, sizeof(*out));
  memset(wout, 0, sizeof(*wout));
  const int r = compact_begin_locked(e, in);
  return r ? r : compact_end_locked(e, out, cfg, wout);
}

int gr_wire_out_host(const gr_message* msgs, size_t n, const uint64_t* cluster_ids, const uint64_t* node_ids,
                     const uint64_t* remote_ids, uint32_t n_peers, uint32_t slots, const uint32_t* target_of,
                     uint32_t n_targets, const gr_wire_out_cfg* cfg, struct grw_batch* batches, size_t* n_batches,
                     struct grw_message* wmsgs, size_t* n_wmsgs, uint32_t* batch_target, uint8_t* held) {
  return host::wire_out_host(msgs, n, cluster_ids, node_ids, remote_ids, n_peers, slots, target_of, n_targets, cfg,
                             batches, n_batches, wmsgs, n_wmsgs, batch_target, held);
}

int gr_cinbox_reserve(gr_engine* e, size_t n_msgs, size_t n_ext_msgs, size_t n_locals, size_t n_ext_locals,
                      gr_cinbox* in) {
  if (!e || !in || n_msgs + n_locals >= 0x80000000ull || n_ext_msgs >= 0x80000000ull ||
      n_ext_locals >= 0x80000000ull)
    return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  int r;
  if ((r = e->h_inmsgs.grow(n_msgs * sizeof(gr_cmsg) + 1))) return r;
  if ((r = e->h_inlocals.grow(n_locals * sizeof(gr_clocal) + 1))) return r;
  if ((r = e->h_inext.grow(n_ext_msgs * sizeof(gr_message) + 1))) return r;
  if ((r = e->h_inlext.grow(n_ext_locals * sizeof(gr_local_input) + 1))) return r;
  in->msgs = (const gr_cmsg*)e->h_inmsgs.p;
  in->n_msgs = n_msgs;
  in->ext_msgs = (const gr_message*)e->h_inext.p;
  in->n_ext_msgs = n_ext_msgs;
  in->locals = (const gr_clocal*)e->h_inlocals.p;
  in->n_locals = n_locals;
  in->ext_locals = (const gr_local_input*)e->h_inlext.p;
  in->n_ext_locals = n_ext_locals;
  return GR_OK;
}

int gr_release_coutbox(gr_engine* e, gr_coutbox* out) {
  if (!e || !out) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);  // the pinned buffers stay for the next pass
  memset(out, 0, sizeof(*out));
  return GR_OK;
}

int gr_pack_messages(const gr_message* in, size_t n, gr_cmsg* out, gr_message* ext, size_t* n_ext) {
  if ((n && (!in || !out || !ext)) || !n_ext) return GR_EINVAL;
  size_t x = 0;
  for (size_t k = 0; k < n; ++k) {
    if (!host::cmsg_of(in[k], &out[k])) {
      out[k].flags = GR_CM_EXT;
      out[k].aux = (uint32_t)x;
      ext[x++] = in[k];
    }
  }
  *n_ext = x;
  return GR_OK;
}

int gr_unpack_messages(const gr_cmsg* in, size_t n, const gr_message* ext, size_t n_ext, gr_message* out) {
  if (n && (!in || !out)) return GR_EINVAL;
  size_t o = 0;
  for (size_t k = 0; k < n; ++k) {
    if ((in[k].flags & GR_CM_EXT) && (!ext || in[k].aux >= n_ext)) return GR_EINVAL;
    for (uint32_t q = 0; q < host::cmsg_n(in[k]); ++q) out[o++] = host::expand_cmsg(in[k], ext, q);
  }
  return GR_OK;
}

size_t gr_cmsg_count(const gr_cmsg* in, size_t n) {
  size_t t = 0;
  for (size_t k = 0; in && k < n; ++k) t += host::cmsg_n(in[k]);
  return t;
}

int gr_pair_messages(gr_cmsg* c, size_t n, size_t* n_out) {
  if ((n && !c) || !n_out) return GR_EINVAL;
  size_t o = 0;
  for (size_t k = 0; k < n;) {
    gr_cmsg pr;
    if (k + 1 < n && host::pair_of(c[k], c[k + 1], &pr)) {
      c[o++] = pr;
      k += 2;
    } else {
      c[o++] = c[k++];
    }
  }
  *n_out = o;
  return GR_OK;
}

int gr_pack_locals(const gr_local_input* in, size_t n, gr_clocal* out, gr_local_input* ext, size_t* n_ext) {
  if ((n && (!in || !out || !ext)) || !n_ext) return GR_EINVAL;
  size_t x = 0;
  for (size_t k = 0; k < n; ++k) {
    if (!host::clocal_of(in[k], &out[k])) {
      out[k].flags = GR_CL_EXT;
      out[k].ext = (uint32_t)x;
      ext[x++] = in[k];
    }
  }
  *n_ext = x;
  return GR_OK;
}

int gr_inbox_reserve(gr_engine* e, size_t n_msgs, size_t n_locals, gr_inbox* in) {
  if (!e || !in || n_msgs + n_locals >= 0x80000000ull) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  int r;
  if ((r = e->h_inmsgs.grow(n_msgs * sizeof(gr_message) + 1))) return r;
  if ((r = e->h_inlocals.grow(n_locals * sizeof(gr_local_input) + 1))) return r;
  in->msgs = (const gr_message*)e->h_inmsgs.p;
  in->n_msgs = n_msgs;
  in->locals = (const gr_local_input*)e->h_inlocals.p;
  in->n_locals = n_locals;
  return GR_OK;
}

int gr_release_outbox(gr_engine* e, gr_outbox* out) {
  if (!e || !out) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);  // the pinned outbox buffers stay for the next pass
  out->msgs = nullptr;
  out->n_msgs = 0;
  out->results = nullptr;
  out->n_results = 0;
  return GR_OK;
}

static int stat_total(gr_engine* e, uint32_t field, uint64_t* out) {
  std::vector<uint64_t> rows((size_t)e->stats_rows * NSTAT);
  HIPCHK(hipMemcpy(rows.data(), e->stats, rows.size() * 8, hipMemcpyDeviceToHost));
  uint64_t v = 0;
  for (uint32_t b = 0; b < e->stats_rows; ++b) v += rows[(size_t)b * NSTAT + field];
  *out = v;
  return GR_OK;
}

int gr_stats_get(gr_engine* e, gr_stats* out) {
  if (!e || !out) return GR_EINVAL;
  HIPCHK(hipDeviceSynchronize());
  std::vector<uint64_t> rows((size_t)e->stats_rows * NSTAT);
  HIPCHK(hipMemcpy(rows.data(), e->stats, rows.size() * 8, hipMemcpyDeviceToHost));
  memset(out, 0, sizeof(*out));
  out->passes = e->passes;
  for (uint32_t b = 0; b < e->stats_rows; ++b) {
    const uint64_t* row = rows.data() + (size_t)b * NSTAT;
    out->leader_commits += row[ST_LEADER_COMMITS];
    out->follower_commits += row[ST_FOLLOWER_COMMITS];
    out->escalations += row[ST_ESCALATIONS];
    out->msgs_in += row[ST_MSGS_IN];
    out->msgs_out += row[ST_MSGS_OUT];
    out->leader_msgs_in += row[ST_LEADER_MSGS_IN];
    out->leader_msgs_out += row[ST_LEADER_MSGS_OUT];
    out->replicate_entries += row[ST_REPLICATE_ENTRIES];
  }
  return GR_OK;
}

int gr_timing_begin(gr_engine* e) {
  if (!e) return GR_EINVAL;
  HIPCHK(hipDeviceSynchronize());
  free_timings(e);
  e->timings.reserve(1 << 16);  // records are referenced by pointer until the pass is enqueued
  int r = stat_total(e, ST_BAILED, &e->timing_bailed0);
  if (r) return r;
  e->timing = true;
  return GR_OK;
}

int gr_timing_end(gr_engine* e, gr_timing* out) {
  if (!e || !out) return GR_EINVAL;
  HIPCHK(hipDeviceSynchronize());
  memset(out, 0, sizeof(*out));
  for (auto& t : e->timings) {
    float a = 0, b = 0;
    HIPCHK(hipEventElapsedTime(&a, t.ev[0], t.ev[1]));
    HIPCHK(hipEventElapsedTime(&b, t.ev[1], t.ev[2]));
    out->fast_ms += a;
    out->general_ms += b;
    out->passes++;
  }
  uint64_t bailed = 0;
  const int r = stat_total(e, ST_BAILED, &bailed);
  if (r) return r;
  out->bailed_lanes = bailed - e->timing_bailed0;  // lanes that left the lean kernels while timing
  free_timings(e);
  e->timing = false;
  return GR_OK;
}

int gr_stats_reset(gr_engine* e) {
  if (!e) return GR_EINVAL;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemset(e->stats, 0, (size_t)e->stats_rows * NSTAT * 8));
  e->passes = 0;
  return GR_OK;
}

int gr_steady_wave_uniform(gr_engine* e) {
  if (!e) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  return e->routes_bound && e->wu_routes && e->wu_spaces && e->wu_enabled ? 1 : 0;
}

int gr_bind_routes(gr_engine* e, const uint32_t* in_pos, const uint32_t* out_pos, uint32_t n_peers) {
  if (!e || !in_pos || !out_pos || n_peers > e->cfg.max_peers) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);  // against a concurrent compact _begin/_end
  GR_REFUSE_PENDING(e);
  HIPCHK(hipDeviceSynchronize());
  std::vector<uint32_t> base(2 * GR_SMAX * GR_SMAX, NOPOS);
  uint32_t g = 0, rr = 0;
  if (detect_affine_routes(in_pos, out_pos, n_peers, e->S, base.data(), &g, &rr)) {
    HIPCHK(hipMemcpy(e->route_base, base.data(), base.size() * 4, hipMemcpyHostToDevice));
    e->route_mode = is_loopback(base.data(), g, rr, e->S) ? RT_LOOPBACK : RT_AFFINE;
    e->route_g = g;
    e->route_r = rr;
    e->wu_routes = steady_wu_routes(e->route_mode, e->S, g, rr, base.data());
  } else {
    e->route_mode = RT_TABLE;
    e->route_g = 0;
    e->wu_routes = false;
  }
  for (uint32_t j = 0; j < e->S; ++j) {
    HIPCHK(hipMemcpy(e->ln.in_pos() + (size_t)j * e->cap, in_pos + (size_t)j * n_peers, (size_t)n_peers * 4,
                     hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->ln.out_pos() + (size_t)j * e->cap, out_pos + (size_t)j * n_peers,
                     (size_t)n_peers * 4, hipMemcpyHostToDevice));
  }
  e->routes_bound = true;
  return GR_OK;
}

int gr_set_locals(gr_engine* e, const gr_local_input* locals, size_t n) {
  if (!e || (n && !locals) || n >= 0x80000000ull) return GR_EINVAL;
  const uint32_t cap = e->cfg.max_peers;
  for (size_t k = 0; k < n; ++k)
    if (locals[k].peer >= cap) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  if (e->quiesce)  // ticks are LocalTicks: the device decides the split (nothing is written)
    for (size_t k = 0; k < n; ++k)
      if (locals[k].quiesced_ticks) return GR_EINVAL;
  HIPCHK(hipDeviceSynchronize());  // a pass in flight on another stream may read the rows
  const hipStream_t s = e->stream;
  int r;
  if ((r = e->d_locals.grow(n * sizeof(gr_local_input) + 1))) return r;
  if ((r = e->d_win.grow((size_t)cap * 4))) return r;
  if (n) HIPCHK(hipMemcpyAsync(e->d_locals.p, locals, n * sizeof(gr_local_input), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(e->d_win.p, 0, (size_t)cap * 4, s));
  const gr_local_input* dloc = (const gr_local_input*)e->d_locals.p;
  if (n) {
    hipLaunchKernelGGL(io::local_winner, dim3(io_grid(n)), dim3(io::kIoBlock), 0, s, dloc, (uint32_t)n,
                       (const uint32_t*)nullptr, (uint32_t*)e->d_win.p);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(io::fill_locals, dim3(io_grid(cap)), dim3(io::kIoBlock), 0, s, dloc,
                     (const uint32_t*)e->d_win.p, cap, e->ln);
  HIPCHK(hipGetLastError());
  if (e->quiesce)  // the raw LocalTick counts, apart from the rows the quiesce pass rewrites
    HIPCHK(hipMemcpyAsync(e->qraw, e->ln.u32(LR_TICKS), (size_t)cap * 4, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  e->locals_set = n > 0;
  bool other = false;
  for (size_t k = 0; k < n && !other; ++k) {
    const gr_local_input& x = locals[k];
    other = local_word(x.ticks, x.quiesced_ticks, x.propose_entries,
                       (x.read_index ? LF_READ_INDEX : 0) | (x.propose_has_config_change ? LF_PROPOSE_CC : 0)) &
            LW_OTHER;
  }
  e->locals_other = other;
  return GR_OK;
}

// One device-resident pass, enqueued on `stream` (e->mu held by the caller).
static int step_device_locked(gr_engine* e, const void* in_space, void* out_space, uint32_t in_chunks,
                              uint32_t in_positions, uint32_t out_chunks, uint32_t out_positions, uint32_t depth,
                              uint32_t n_peers, void* stream) {
  StepParams kp = base_params(e);
  kp.has_locals = e->locals_set || e->quiesce ? 1 : 0;  // the quiesce pass writes every lane's effective rows
  kp.q_nolocals = e->locals_set ? 0 : 1;
  kp.has_lane_peer = 0;
  kp.route_mode = e->routes_bound ? e->route_mode : RT_IDENTITY;
  kp.route_g = e->route_g;
  kp.route_r = e->route_r;
  kp.route_base = e->route_base;
  kp.route_wu = (kp.route_mode == RT_LOOPBACK || kp.route_mode == RT_AFFINE) && e->route_g % 64 == 0 ? 1 : 0;
  kp.in = make_view(in_space, in_chunks, in_positions, depth);
  kp.out = make_view(out_space, out_chunks, out_positions, depth);
  kp.n_lanes = n_peers;
  e->wu_spaces = steady_wu_space(kp.in) && steady_wu_space(kp.out);
  kp.steady_wu = e->routes_bound && e->wu_routes && e->wu_spaces && e->wu_enabled ? 1 : 0;
  // lane = peer here, so a wave's hint carries over between passes
  const size_t hs = hint_stride(e->cap), hf = e->hint_flip++ & 1;
  kp.hints = e->hints + hf * hs;
  kp.hints_out = e->hints + (1 - hf) * hs;
  // the follower instance of its own pays off only when the pass is large (a
  // 10k x 3 pass is launch-bound: one instance there, 24 vs 41 us per pass)
  kp.split = n_peers >= e->split_min ? 1 : 0;
  HIPCHK(launch_slots(e->S, kp, e->bail, e->counters, e->cap, (uint32_t)e->launches++, (hipStream_t)stream,
                      next_timing(e), kp.has_locals && e->locals_other));
  e->passes++;
  return GR_OK;
}

int gr_step_device(gr_engine* e, const void* in_space, void* out_space, uint32_t in_chunks,
                   uint32_t in_positions, uint32_t out_chunks, uint32_t out_positions, uint32_t depth,
                   uint32_t n_peers, void* stream) {
  if (!e || !in_space || !out_space || n_peers > e->cfg.max_peers || depth == 0 || depth > GR_C)
    return GR_EINVAL;
  // the mutex orders this pass after a compact _begin/_end on another thread
  // (uncontended: one lock per pass)
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);  // the pending compact pass owns the lane rows and bail lists
  const int r = step_device_locked(e, in_space, out_space, in_chunks, in_positions, out_chunks, out_positions, depth,
                                   n_peers, stream);
  if (r == GR_OK) e->lanes_by_slot = true;
  return r;
}

// A captured sequence of device-resident passes (gpuraft.h gr_graph_*).
struct gr_graph {
  gr_engine* e = nullptr;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  uint32_t n_passes = 0;
  // the engine's counter-set and hint-set parities the captured pass 0 assumes
  // (launches & 1, hint_flip & 1): a replay at any other parity would read a
  // counter set nobody zeroed and the wrong hint set, so it is refused
  uint32_t launch_par = 0, hint_par = 0;
};

int gr_graph_capture(gr_engine* e, void* space_a, void* space_b, uint32_t n_chunks, uint32_t positions,
                     uint32_t depth, uint32_t n_peers, uint32_t n_passes, gr_graph** out) {
  if (!e || !space_a || !space_b || !out || n_peers > e->cfg.max_peers || depth == 0 || depth > GR_C ||
      n_passes == 0 || (n_passes & 1))
    return GR_EINVAL;
  *out = nullptr;
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  if (e->timing) return GR_ESTATE;  // per-pass timing events are not captured
  HIPCHK(hipDeviceSynchronize());   // nothing of the engine in flight while the parities are read
  hipStream_t cs = nullptr;
  HIPCHK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
  gr_graph* g = new gr_graph();
  g->e = e;
  g->n_passes = n_passes;
  g->launch_par = (uint32_t)(e->launches & 1);
  g->hint_par = (uint32_t)(e->hint_flip & 1);
  // recording runs no pass: the engine's counters are restored afterwards on
  // every path (a failed capture must not leave the parities advanced)
  const uint64_t saved_launches = e->launches, saved_flip = e->hint_flip, saved_passes = e->passes;
  int r = GR_OK;
  if (hipStreamBeginCapture(cs, hipStreamCaptureModeRelaxed) != hipSuccess) r = GR_EDEVICE;
  // pass k reads space k % 2 and writes the other; the launch and hint parities
  // advance by n_passes (even), so every replay starts where the capture did
  for (uint32_t k = 0; k < n_passes && r == GR_OK; ++k)
    r = step_device_locked(e, (k & 1) ? space_b : space_a, (k & 1) ? space_a : space_b, n_chunks, positions,
                           n_chunks, positions, depth, n_peers, cs);
  hipGraph_t graph = nullptr;
  const hipError_t ce = hipStreamEndCapture(cs, &graph);  // ends the capture on every path
  if (r == GR_OK && (ce != hipSuccess || !graph)) r = GR_EDEVICE;
  if (r == GR_OK && hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0) != hipSuccess) r = GR_EDEVICE;
  g->graph = graph;
  (void)hipStreamDestroy(cs);
  e->launches = saved_launches;
  e->hint_flip = saved_flip;
  e->passes = saved_passes;
  if (r != GR_OK) {
    gr_graph_destroy(g);
    return r;
  }
  *out = g;
  return GR_OK;
}

int gr_graph_replay(gr_graph* g, void* stream) {
  if (!g || !g->exec) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(g->e->mu);
  GR_REFUSE_PENDING(g->e);
  gr_engine* e = g->e;
  // passes run between replays must come in even numbers (gpuraft.h)
  if ((uint32_t)(e->launches & 1) != g->launch_par || (uint32_t)(e->hint_flip & 1) != g->hint_par)
    return GR_ESTATE;
  HIPCHK(hipGraphLaunch(g->exec, (hipStream_t)stream));
  e->launches += g->n_passes;
  e->hint_flip += g->n_passes;
  e->passes += g->n_passes;
  e->lanes_by_slot = true;
  return GR_OK;
}

void gr_graph_destroy(gr_graph* g) {
  if (!g) return;
  if (g->exec) (void)hipGraphExecDestroy(g->exec);
  if (g->graph) (void)hipGraphDestroy(g->graph);
  delete g;
}

int gr_collect_results(gr_engine* e, uint32_t first, gr_peer_result* out, size_t n) {
  if (!e || (n && !out) || (uint64_t)first + n > e->cfg.max_peers) return GR_EINVAL;
  if (n == 0) return GR_OK;
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  HIPCHK(hipDeviceSynchronize());
  const size_t bytes = n * sizeof(gr_peer_result);
  int r;
  if ((r = e->d_results.grow(bytes))) return r;
  hipLaunchKernelGGL(io::pack_results, dim3(io_grid(n)), dim3(io::kIoBlock), 0, e->stream, e->ln, e->st,
                     (const uint32_t*)nullptr, first, (uint32_t)n, (gr_peer_result*)e->d_results.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, e->d_results.p, bytes, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return GR_OK;
}

// gpuraft.h gr_update_class: the rule on the host (gr_host.h update_class, which
// the classify kernel runs too).
int gr_update_class(const gr_peer_result* r, uint64_t log_applied, uint64_t first_index_m1,
                    const gr_update_state* prev, uint32_t flags) {
  if (!r || !prev || (flags & ~(uint32_t)(GR_UPD_MORE_TO_APPLY | GR_UPD_EVERY))) return GR_EINVAL;
  return update_class(update_fields(*r), log_applied, first_index_m1, *prev, flags);
}

// Peer.HasUpdate / GetUpdate for slots [first, first + n) after a device-resident
// pass (gr_io.h update_classify / update_pack): only the reported peers' records
// cross PCIe.
int gr_collect_updates(gr_engine* e, uint32_t first, uint32_t n, uint32_t flags, gr_updates* out) {
  if (!e || !out || (flags & ~(uint32_t)(GR_UPD_MORE_TO_APPLY | GR_UPD_EVERY))) return GR_EINVAL;
  if ((uint64_t)first + n > e->cfg.max_peers) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  if (!e->lanes_by_slot) return GR_ESTATE;  // the last pass was a host-path one: lanes are not slots
  memset(out, 0, sizeof(*out));
  if (n == 0) return GR_OK;
  HIPCHK(hipDeviceSynchronize());  // passes may run on the caller's streams
  const hipStream_t s = e->stream;
  const uint32_t ntiles = ((first + n - 1) >> GR_TILE_SHIFT) - (first >> GR_TILE_SHIFT) + 1;
  const dim3 grid(ntiles), blk(io::kIoBlock);
  int r;
  if ((r = ensure_update_state(e))) return r;
  if ((r = ensure_scal(e))) return r;
  if ((r = e->d_ucls.grow((size_t)ntiles * kTileW))) return r;
  if ((r = e->d_ucnt.grow((size_t)ntiles * 8))) return r;
  if ((r = e->d_uoff.grow((size_t)ntiles * 8))) return r;
  const bool timed = e->timing;
  if (timed)
    for (hipEvent_t& ev : e->upd_ev)
      if (!ev) HIPCHK(hipEventCreate(&ev));
  uint8_t* cls = e->d_ucls.as<uint8_t>();
  uint64_t* cnt = e->d_ucnt.as<uint64_t>();
  uint64_t* off = e->d_uoff.as<uint64_t>();
  uint32_t* scal = e->d_scal.as<uint32_t>();
  if (timed) HIPCHK(hipEventRecord(e->upd_ev[0], s));
  hipLaunchKernelGGL(io::update_classify, grid, blk, 0, s, e->ln, e->st, (const gr_update_state*)e->upd_state, first,
                     n, flags, cls, cnt);
  HIPCHK(hipGetLastError());
  if (timed) HIPCHK(hipEventRecord(e->upd_ev[1], s));
  if ((r = io_scan64(e, cnt, off, ntiles, s))) return r;
  hipLaunchKernelGGL(io::update_totals, dim3(1), dim3(64), 0, s, (const uint64_t*)cnt, (const uint64_t*)off, ntiles,
                     scal);
  HIPCHK(hipGetLastError());
  // every device-to-host copy of this call goes through here and is counted
  gr_updates_info info{};
  const auto down = [&](void* dst, const void* src, size_t bytes) {
    info.bytes_down += bytes;
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s);
  };
  HIPCHK(down(e->h_scal.p, scal, 8));  // the totals
  HIPCHK(hipStreamSynchronize(s));
  const uint32_t nr = e->h_scal.as<uint32_t>()[0], nx = e->h_scal.as<uint32_t>()[1];
  const size_t rbytes = (size_t)nr * sizeof(gr_cresult), xbytes = (size_t)nx * sizeof(gr_peer_result);
  if (nr) {  // no record, nothing to pack: no update state moves either
    if ((r = e->d_results.grow(rbytes))) return r;
    if ((r = e->d_resext.grow(xbytes + 1))) return r;
    if ((r = e->h_upd.grow(rbytes))) return r;
    if ((r = e->h_updext.grow(xbytes + 1))) return r;
    if (timed) HIPCHK(hipEventRecord(e->upd_ev[2], s));
    hipLaunchKernelGGL(io::update_pack, grid, blk, 0, s, e->ln, e->st, e->upd_state, first, (const uint8_t*)cls,
                       (const uint64_t*)off, e->d_results.as<gr_cresult>(), e->d_resext.as<gr_peer_result>());
    HIPCHK(hipGetLastError());
    if (timed) HIPCHK(hipEventRecord(e->upd_ev[3], s));
    HIPCHK(down(e->h_upd.p, e->d_results.p, rbytes));
    if (nx) HIPCHK(down(e->h_updext.p, e->d_resext.p, xbytes));
    HIPCHK(hipStreamSynchronize(s));
  }
  if (timed) {
    float a = 0, b = 0;
    HIPCHK(hipEventElapsedTime(&a, e->upd_ev[0], e->upd_ev[1]));
    if (nr) HIPCHK(hipEventElapsedTime(&b, e->upd_ev[2], e->upd_ev[3]));
    info.classify_ms = a;
    info.pack_ms = b;
    info.timed = 1;
  }
  info.n_results = nr;
  info.n_ext_results = nx;
  e->upd_last = info;
  out->results = nr ? e->h_upd.as<gr_cresult>() : nullptr;
  out->n_results = nr;
  out->ext_results = nx ? e->h_updext.as<gr_peer_result>() : nullptr;
  out->n_ext_results = nx;
  return GR_OK;
}

int gr_updates_last(gr_engine* e, gr_updates_info* out) {
  if (!e || !out) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  *out = e->upd_last;
  return GR_OK;
}

// A plain run-time switch of the engine (StepParams reads it at the next pass).
static int set_switch(gr_engine* e, uint8_t gr_engine::*field, int on) {
  if (!e) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  e->*field = on ? 1 : 0;
  return GR_OK;
}

int gr_set_elections(gr_engine* e, int on) { return set_switch(e, &gr_engine::elections, on); }
int gr_get_elections(const gr_engine* e) { return e ? (int)e->elections : GR_EINVAL; }

int gr_set_snapshots(gr_engine* e, int on) { return set_switch(e, &gr_engine::snapshots, on); }
int gr_get_snapshots(const gr_engine* e) { return e ? (int)e->snapshots : GR_EINVAL; }

int gr_set_config_entries(gr_engine* e, int on) { return set_switch(e, &gr_engine::config_entries, on); }
int gr_get_config_entries(const gr_engine* e) { return e ? (int)e->config_entries : GR_EINVAL; }

int gr_set_quiesce(gr_engine* e, int on) {
  if (!e) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  const uint8_t v = on ? 1 : 0;
  if (v == e->quiesce) return GR_OK;
  HIPCHK(hipDeviceSynchronize());
  if (v) {
    const int r = ensure_quiesce(e);
    if (r) return r;
  }
  e->quiesce = v;
  // bound locals mean LocalTicks on one side of the switch and a host-chosen
  // split on the other: bind again
  e->locals_set = false;
  e->locals_other = false;
  return GR_OK;
}

int gr_get_quiesce(const gr_engine* e) { return e ? (int)e->quiesce : GR_EINVAL; }

// gr_quiesce_state records <-> the device records for slots [first, first+n) or a
// slot list, as transfer() moves gr_peer records.
static int transfer_quiesce(gr_engine* e, const uint32_t* slots, uint32_t first, size_t n, gr_quiesce_state* host,
                            bool to_device) {
  if (!e || (n && !host)) return GR_EINVAL;
  const uint32_t cap = e->cfg.max_peers;
  if (!slots && (uint64_t)first + n > cap) return GR_ERANGE;
  if (n == 0) return GR_OK;
  if (n >= 0x80000000ull) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  HIPCHK(hipDeviceSynchronize());  // passes in flight on other streams own the records
  const hipStream_t s = e->stream;
  const size_t bytes = n * sizeof(gr_quiesce_state);
  int r;
  if ((r = ensure_quiesce(e))) return r;
  if ((r = e->d_peers.grow(bytes))) return r;
  if ((r = e->d_mark.grow((size_t)cap * 4))) return r;
  if ((r = ensure_scal(e))) return r;
  const uint32_t* dslots = nullptr;
  if (slots && (r = upload_slots(e, slots, n, &dslots))) return r;
  gr_quiesce_state* dq = (gr_quiesce_state*)e->d_peers.p;
  const dim3 grid(io_grid(n)), blk(io::kIoBlock);
  if (to_device) HIPCHK(hipMemcpyAsync(dq, host, bytes, hipMemcpyHostToDevice, s));
  if (to_device || slots) {  // nothing is written (or read back) when a record or the list is refused
    if (slots) HIPCHK(hipMemsetAsync(e->d_mark.p, 0, (size_t)cap * 4, s));
    HIPCHK(hipMemsetAsync(e->d_scal.p, 0, 16, s));
    hipLaunchKernelGGL(io::check_quiesce, grid, blk, 0, s, to_device ? (const gr_quiesce_state*)dq : nullptr, dslots,
                       (uint32_t)n, cap, (uint32_t*)e->d_mark.p, (uint32_t*)e->d_scal.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(e->h_scal.p, e->d_scal.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const uint32_t err = *(uint32_t*)e->h_scal.p;
    if (err & 2u) return GR_ERANGE;
    if (err & 1u) return GR_EINVAL;
  }
  if (to_device) {
    hipLaunchKernelGGL(io::quiesce_to_rows, grid, blk, 0, s, (const gr_quiesce_state*)dq, dslots, first, (uint32_t)n,
                       e->qrec, e->qcfg);
    HIPCHK(hipGetLastError());
  } else {
    hipLaunchKernelGGL(io::rows_to_quiesce, grid, blk, 0, s, (const QuiesceRec*)e->qrec, (const uint32_t*)e->qcfg,
                       dslots, first, (uint32_t)n, dq);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(host, dq, bytes, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  return GR_OK;
}

int gr_load_quiesce(gr_engine* e, uint32_t first, const gr_quiesce_state* recs, size_t n) {
  return transfer_quiesce(e, nullptr, first, n, const_cast<gr_quiesce_state*>(recs), true);
}
int gr_sync_quiesce(gr_engine* e, uint32_t first, gr_quiesce_state* out, size_t n) {
  return transfer_quiesce(e, nullptr, first, n, out, false);
}
int gr_load_quiesce_peers(gr_engine* e, const uint32_t* slots, const gr_quiesce_state* recs, size_t n) {
  if (n && !slots) return GR_EINVAL;
  return transfer_quiesce(e, slots, 0, n, const_cast<gr_quiesce_state*>(recs), true);
}
int gr_sync_quiesce_peers(gr_engine* e, const uint32_t* slots, gr_quiesce_state* out, size_t n) {
  if (n && !slots) return GR_EINVAL;
  return transfer_quiesce(e, slots, 0, n, out, false);
}

int gr_tick_all(gr_engine* e, uint32_t ticks, uint64_t rand_seed) {
  if (!e) return GR_EINVAL;
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  HIPCHK(hipDeviceSynchronize());  // a pass in flight on another stream may read the rows
  const uint32_t cap = e->cfg.max_peers;
  hipLaunchKernelGGL(io::fill_tick_all, dim3(io_grid(cap)), dim3(io::kIoBlock), 0, e->stream, cap, ticks, rand_seed,
                     e->st, e->ln, e->qraw);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  e->locals_set = true;
  e->locals_other = ticks != 0;
  return GR_OK;
}

uint64_t gr_splitmix64(uint64_t x) { return q_splitmix64(x); }

// Drain a device list (a kPromoHeader header of count and overflow flag, then
// cap_records records): all of it or, without room, nothing and the count.
static int drain_list(gr_engine* e, uint8_t* base, size_t record_size, size_t cap_records, void* out, size_t cap,
                      size_t* n) {
  if (!e || !n || (cap && !out)) return GR_EINVAL;
  *n = 0;
  std::lock_guard<std::mutex> guard(e->mu);
  GR_REFUSE_PENDING(e);
  HIPCHK(hipDeviceSynchronize());  // passes may run on the caller's streams (gr_step_device, graph replays)
  uint32_t hdr[2] = {0, 0};
  HIPCHK(hipMemcpy(hdr, base, sizeof(hdr), hipMemcpyDeviceToHost));
  const size_t have = std::min<size_t>(hdr[0], cap_records);
  if (have > cap) {  // nothing drained: the caller comes back with room
    *n = have;
    return GR_ECAPACITY;
  }
  if (have) HIPCHK(hipMemcpy(out, base + kPromoHeader, have * record_size, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(base, 0, 4));  // the count; the overflow flag stays
  *n = have;
  return hdr[1] ? GR_ECAPACITY : GR_OK;
}

int gr_promotions(gr_engine* e, gr_promotion* out, size_t cap, size_t* n) {
  return drain_list(e, e ? e->promo : nullptr, sizeof(gr_promotion), e ? e->cfg.max_peers : 0, out, cap, n);
}

int gr_restored_snapshots(gr_engine* e, gr_restored* out, size_t cap, size_t* n) {
  return drain_list(e, e ? e->rest : nullptr, sizeof(gr_restored), e ? (size_t)kRestStage * e->cfg.max_peers : 0, out,
                    cap, n);
}

#ifdef GR_COVERAGE
// Coverage build only (libgpuraft_cover.so): the per-branch hit counts of one
// table (gr_cover.h), summed over the kernel translation units: each keeps its own counters.
static int coverage_read(uint32_t table, uint64_t* out, uint32_t n) {
  const uint32_t len = cover_len(table);
  if (!out || n < len) return GR_EINVAL;
  HIPCHK(hipDeviceSynchronize());
  for (uint32_t k = 0; k < len; ++k) out[k] = 0;
  for (uint32_t S : {1u, 3u, 5u, 8u})
    HIPCHK(with_slots(S, [&](auto ss) { return cover_read<decltype(ss)::value>(table, out); }));
  return (int)len;
}
#define GR_COVER_NAME(x) #x ","
int gr_coverage_read(uint64_t* out, uint32_t n) { return coverage_read(COVER_STEP, out, n); }
const char* gr_coverage_names() { return GR_COVER_IDS(GR_COVER_NAME); }
int gr_coverage_elect_read(uint64_t* out, uint32_t n) { return coverage_read(COVER_ELECT, out, n); }
const char* gr_coverage_elect_names() { return GR_COVER_ELECT_IDS(GR_COVER_NAME); }
int gr_coverage_quiesce_read(uint64_t* out, uint32_t n) { return coverage_read(COVER_QUIESCE, out, n); }
const char* gr_coverage_quiesce_names() { return GR_COVER_QUIESCE_IDS(GR_COVER_NAME); }
int gr_coverage_snap_read(uint64_t* out, uint32_t n) { return coverage_read(COVER_SNAP, out, n); }
const char* gr_coverage_snap_names() { return GR_COVER_SNAP_IDS(GR_COVER_NAME); }
int gr_coverage_cc_read(uint64_t* out, uint32_t n) { return coverage_read(COVER_CC, out, n); }
const char* gr_coverage_cc_names() { return GR_COVER_CC_IDS(GR_COVER_NAME); }
#undef GR_COVER_NAME
#endif

}  // extern "C"

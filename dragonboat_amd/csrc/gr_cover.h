// gr_cover.h — per-branch hit counters of the lane code (coverage builds only).
//
// Every handler and branch of the device step (gr_lane.h general lane, gr_fast.h
// lean lane, gr_tick.h heartbeat/ReadIndex/tick lane) and every escalation
// reason has an id. Built with -DGR_COVERAGE (libgpuraft_cover.so, and the
// test-only host lane), GR_COVER(id) counts a hit: a device atomic on the GPU,
// a plain increment on the host. The product library is built without it and
// the macro is empty. tests/test_coverage.py drives the parity workloads through
// the coverage build and requires every id to be reached.
#pragma once
#include <stdint.h>

#include "gr_layout.h"

namespace gr {

#define GR_COVER_IDS(X)                                                                       \
  X(TERM_HIGHER) X(TERM_HIGHER_OBSERVER) X(TERM_LOWER_NOOP) X(TERM_LOWER_DROP)                  \
  X(L_RESP_NONMEMBER) X(L_REPLICATE_RESP_ACCEPT) X(L_REPLICATE_RESP_REJECT) X(L_HEARTBEAT_RESP) \
  X(L_LEADER_TRANSFER) X(L_UNREACHABLE) X(L_SNAPSHOT_STATUS) X(L_READ_INDEX_MSG)                \
  X(L_LEADER_HEARTBEAT) X(L_CHECK_QUORUM_MSG) X(L_ELECTION) X(L_PROPOSE_FWD) X(L_NIL)         \
  X(F_REPLICATE) X(F_HEARTBEAT) X(F_READ_INDEX_RESP) X(F_READ_INDEX_FWD)                        \
  X(F_LEADER_TRANSFER_FWD) X(F_ELECTION) X(F_PROPOSE_FWD) X(F_NIL)                              \
  X(O_REPLICATE) X(O_HEARTBEAT) X(O_READ_INDEX_RESP) X(O_READ_INDEX_FWD) X(O_PROPOSE_FWD)       \
  X(O_DROPPED)                                                                                  \
  X(C_PROPOSE) X(C_NIL)                                                                         \
  X(REP_EARLY_ACK) X(REP_REJECT) X(REP_MATCH_NO_APPEND) X(REP_APPEND_TAIL) X(REP_TRUNCATE)      \
  X(REP_TWO_RUNS)                                                                               \
  X(RESPONDED_RETRY) X(RESPONDED_SNAPSHOT_RETRY) X(RESPONDED_SNAPSHOT_STAY)                    \
  X(DECREASE_REPLICATE) X(DECREASE_PROBE) X(DECREASE_IGNORED)                                   \
  X(TIMEOUT_NOW_SENT) X(SEND_PAUSED) X(SEND_MULTI_ENTRY) X(SEND_TWO_RUNS) X(SEND_EMPTY)         \
  X(BCAST_OBSERVER) X(HEARTBEAT_OBSERVER)                                                       \
  X(RI_SINGLE_READY) X(RI_SINGLE_OBSERVER_RESP) X(RI_NOT_AT_TERM) X(RI_ADD) X(RI_DUP)           \
  X(RI_ACK_PENDING) X(RI_CONFIRM_RELEASE) X(RI_RESP_REMOTE) X(RI_LOCAL_FORWARD)                 \
  X(TICK_LEADER) X(TICK_CHECK_QUORUM_OK) X(TICK_STEP_DOWN) X(TICK_TRANSFER_ABORT)              \
  X(TICK_HEARTBEAT) X(TICK_FOLLOWER) X(TICK_OBSERVER) X(TICK_ELECTION_SKIPPED) X(QTICK)         \
  X(PROP_APPEND) X(PROP_DROP_SELF_REMOVED) X(PROP_DROP_TRANSFER) X(PROP_FORWARD)                \
  X(PROP_DROP_NO_LEADER) X(PROP_CANDIDATE)                                                      \
  X(FAST_LEADER) X(FAST_FOLLOWER) X(FAST_QUIESCED) X(TICKLANE_LEADER) X(TICKLANE_FOLLOWER)     \
  X(STEADY_LEADER) X(STEADY_FOLLOWER) X(QUIET_STEP)                                              \
  X(GENERAL_LANE)                                                                               \
  X(ESC_TERM_WINDOW) X(ESC_RANDOM) X(ESC_UNSUPPORTED) X(ESC_ELECTION) X(ESC_PANIC)              \
  X(ESC_CAPACITY) X(ESC_SNAPSHOT) X(ESC_ENTRY_SIZE) X(ESC_MSG_RUNS) X(ESC_NONMEMBER)            \
  X(ESC_CONFIG_CHANGE) X(ESC_WIDE_TERM)                                                          \
  X(BAD_COMMITTED_PAST_LAST) X(BAD_RUNS_NOT_ASCENDING) X(BAD_RUN_TERMS_DECREASE)                \
  X(BAD_WINDOW_PAST_LAST) X(BAD_LAST_TERM_ABOVE_TERM) X(BAD_MARKER_PAST_LAST)                   \
  X(BAD_STEADY_STATS_RANGE)

#define GR_COVER_ENUM(n) CV_##n,
enum CoverId : uint32_t { GR_COVER_IDS(GR_COVER_ENUM) CV_N };
#undef GR_COVER_ENUM
// escalation reason r (1..12) -> its id
constexpr uint32_t CV_ESC_FIRST = CV_ESC_TERM_WINDOW;
// BAD_* ids are the checked build's invariant violations (they must stay 0);
// the coverage test requires every other id to be reached.
constexpr uint32_t CV_BAD_FIRST = CV_BAD_COMMITTED_PAST_LAST;

// The election handlers' ids (gr_lane.h with StepParams::elections): a second
// table with its own counters and read-out, so the first table, which the
// election-free workloads must reach in full, stays as it is.
#define GR_COVER_ELECT_IDS(X)                                                                 \
  X(CAMPAIGN) X(CAMPAIGN_TRANSFER) X(VOTE_GRANT) X(VOTE_REJECT) X(VOTE_DROPPED_CHECK_QUORUM)     \
  X(VOTE_HIGHER_TERM) X(C_VOTE_RESP_WIN) X(C_VOTE_RESP_LOSE) X(C_VOTE_RESP_PENDING)              \
  X(C_VOTE_RESP_OBSERVER) X(C_REPLICATE) X(C_HEARTBEAT) X(F_TIMEOUT_NOW) X(PROMOTE_UNCOMMITTED)
#define GR_COVER_ENUM(n) CE_##n,
enum CoverElectId : uint32_t { GR_COVER_ELECT_IDS(GR_COVER_ENUM) CE_N };
#undef GR_COVER_ENUM

// The quiesce pass's ids (gr_kernels.h gr_quiesce_kernel and the general lane's
// sends and prefix re-run, with StepParams::quiesce): a third table, read out
// through gr_coverage_quiesce_read, so the first two stay as they are.
#define GR_COVER_QUIESCE_IDS(X)                                                               \
  X(LANE) X(UNIFORM_MAILBOX) X(FULL_MAILBOX) X(NOTICE) X(HEARTBEAT_HINT) X(READ_INDEX) X(SPLIT)  \
  X(MARK) X(SEND) X(PREFIX) X(PREFIX_SEND)
#define GR_COVER_ENUM(n) CQ_##n,
enum CoverQuiesceId : uint32_t { GR_COVER_QUIESCE_IDS(GR_COVER_ENUM) CQ_N };
#undef GR_COVER_ENUM

// The snapshot handlers' ids (gr_lane.h with StepParams::snapshots): a fourth
// table, read out through gr_coverage_snap_read, so the first three stay as they
// are.
#define GR_COVER_SNAP_IDS(X)                                                                  \
  X(SEND_INACTIVE) X(SEND_INSTALL) X(SEND_EMPTY_SNAPSHOT) X(F_INSTALL) X(O_INSTALL) X(C_INSTALL) \
  X(IGNORED_COMMITTED) X(MATCH_COMMIT) X(RESTORE) X(REJECT_PANIC)
#define GR_COVER_ENUM(n) CS_##n,
enum CoverSnapId : uint32_t { GR_COVER_SNAP_IDS(GR_COVER_ENUM) CS_N };
#undef GR_COVER_ENUM

// The config-change-entry handlers' ids (gr_lane.h with
// StepParams::config_entries, and the lean leader's hand-over in gr_fast.h): a
// fifth table, read out through gr_coverage_cc_read, so the others stay as they are.
#define GR_COVER_CC_IDS(X)                                                                        \
  X(PROPOSE_LOCAL) X(PROPOSE_FWD) X(PROPOSE_PENDING) X(PROPOSED) X(SEND_MARK) X(SEND_MARK_TWO)       \
  X(SEND_NO_MARK) X(MERGE) X(TRUNCATE_KEEP) X(TRUNCATE_DROP) X(TRUNCATE_TWO) X(PROMOTE_CLEAR)        \
  X(PROMOTE_PENDING) X(PROMOTE_PANIC) X(LEAN_HANDOVER)
#define GR_COVER_ENUM(n) CC_##n,
enum CoverCcId : uint32_t { GR_COVER_CC_IDS(GR_COVER_ENUM) CC_N };
#undef GR_COVER_ENUM

#ifdef GR_COVERAGE
// one array per code object (the kernels of each slot count are their own translation unit)
static __device__ unsigned long long gr_cover_dev[CV_N];
inline unsigned long long gr_cover_host[CV_N];
static __device__ unsigned long long gr_cover_elect_dev[CE_N];
inline unsigned long long gr_cover_elect_host[CE_N];
__host__ __device__ static inline void cover_elect_hit(uint32_t id) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(&gr_cover_elect_dev[id], 1ull);
#else
  gr_cover_elect_host[id]++;
#endif
}
#define GR_COVER_E(id) ::gr::cover_elect_hit(::gr::CE_##id)
static __device__ unsigned long long gr_cover_quiesce_dev[CQ_N];
inline unsigned long long gr_cover_quiesce_host[CQ_N];
__host__ __device__ static inline void cover_quiesce_hit(uint32_t id) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(&gr_cover_quiesce_dev[id], 1ull);
#else
  gr_cover_quiesce_host[id]++;
#endif
}
#define GR_COVER_Q(id) ::gr::cover_quiesce_hit(::gr::CQ_##id)
static __device__ unsigned long long gr_cover_snap_dev[CS_N];
inline unsigned long long gr_cover_snap_host[CS_N];
__host__ __device__ static inline void cover_snap_hit(uint32_t id) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(&gr_cover_snap_dev[id], 1ull);
#else
  gr_cover_snap_host[id]++;
#endif
}
#define GR_COVER_S(id) ::gr::cover_snap_hit(::gr::CS_##id)
static __device__ unsigned long long gr_cover_cc_dev[CC_N];
inline unsigned long long gr_cover_cc_host[CC_N];
__host__ __device__ static inline void cover_cc_hit(uint32_t id) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(&gr_cover_cc_dev[id], 1ull);
#else
  gr_cover_cc_host[id]++;
#endif
}
#define GR_COVER_C(id) ::gr::cover_cc_hit(::gr::CC_##id)
__host__ __device__ static inline void cover_hit(uint32_t id) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(&gr_cover_dev[id], 1ull);
#else
  gr_cover_host[id]++;
#endif
}
#define GR_COVER(id) ::gr::cover_hit(::gr::CV_##id)
#define GR_COVER_ESC(e) ::gr::cover_hit(::gr::CV_ESC_FIRST + (uint32_t)(e) - 1u)
#define GR_CHECK_INV(cond, id) ((cond) ? (void)0 : ::gr::cover_hit(::gr::CV_##id))
#else
#define GR_COVER(id) ((void)0)
#define GR_COVER_E(id) ((void)0)
#define GR_COVER_Q(id) ((void)0)
#define GR_COVER_S(id) ((void)0)
#define GR_COVER_C(id) ((void)0)
#define GR_COVER_ESC(e) ((void)0)
#define GR_CHECK_INV(cond, id) ((void)0)
#endif

// The checked build (-DGR_COVERAGE: libgpuraft_cover.so and the host lane):
// after a lane stores its group, the SoA rows must still describe a raft log
// (entryLog invariants): committed <= lastIndex (commitTo panics otherwise,
// logentry.go:314-323), term-run starts strictly ascending with non-decreasing
// terms (checkEntriesToAppend, entryutils.go:36-48), the newest run inside the
// log, the last entry's term at most the current term, and inMemory's marker at
// most lastIndex + 1. A violation counts its BAD_* id. BAD_STEADY_STATS_RANGE:
// a closed-form lane (gr_steady.h) counted more than the bit planes hold that
// the steady kernel sums its waves' counters in (kSteady*Bits). It sits in this
// table, not in one of its own, because every checked-build test already
// requires this table's BAD_* ids to stay 0, on the host lane and on the device.
#ifdef GR_COVERAGE
template <class StateBaseT>
__host__ __device__ inline void check_state(const StateBaseT& st, uint32_t p) {
  const uint64_t last = st.u64(SR_LAST_INDEX)[p];
  const uint64_t committed = h_committed(st.u64(SR_HDR)[p], last, st.u64(SR_COMMITTED)[p]);  // H_CL
  GR_CHECK_INV(committed <= last, BAD_COMMITTED_PAST_LAST);
  const uint64_t h = st.u64(SR_HDR)[p];
  uint32_t nr = h_nruns(h);
  if (nr > GR_K) nr = GR_K;
  uint64_t ps = 0, pt = 0;
  for (uint32_t r = 0; r < nr; ++r) {
    const uint64_t rs = st.u64(SR_RUN_START + run_row(nr, r))[p], rt = st.u64(SR_RUN_TERM + run_row(nr, r))[p];
    if (r) {
      GR_CHECK_INV(rs > ps, BAD_RUNS_NOT_ASCENDING);
      GR_CHECK_INV(rt >= pt, BAD_RUN_TERMS_DECREASE);
    }
    ps = rs;
    pt = rt;
  }
  if (nr) {
    GR_CHECK_INV(ps <= last, BAD_WINDOW_PAST_LAST);
    GR_CHECK_INV(pt <= st.u64(SR_TERM)[p], BAD_LAST_TERM_ABOVE_TERM);
  }
  GR_CHECK_INV(st.u64(SR_MARKER)[p] <= last + 1, BAD_MARKER_PAST_LAST);
}
#define GR_CHECK_STATE(st, p) ::gr::check_state((st), (p))
#else
#define GR_CHECK_STATE(st, p) ((void)0)
#endif

}  // namespace gr

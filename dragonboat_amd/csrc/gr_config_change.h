// gr_config_change.h — Peer.ApplyConfigChange / RejectConfigChange
// (peer.go:153-174) and what they call, raft.addNode / addObserver / removeNode
// (raft.go:822-861), as code shared by the device (gr_io.h config_rows, behind
// gr_apply_config_change) and the host (tests/native/config_change_host.hip).
// The call arrives between passes from the RSM's apply path, so nothing here can
// send: a change whose reference execution would send (removeNode's tryCommit
// raising committed, raft.go:857-859) is refused with GR_CC_HOST and leaves the
// peer untouched, the project's rule that an item is applied wholly on the
// device or wholly on the host.
//
// The change is applied to the peer's gr_peer record, read from the state rows
// and written back with the accessors gr_sync_peers_to_host and gr_load_peers
// use (gr_host.h set_u64_row / resolve_sync / get_u64_row / header_of), so this
// file holds no decoder of the header word: the header's summaries of remote
// rows (H_NX, H_MS, H_MP) are resolved into the record by resolve_sync, every
// row is written exact, and the bits are cleared; the next pass sets them again.
#pragma once
#include <string.h>

#include "gr_host.h"

#define GR_HD __host__ __device__ inline __attribute__((always_inline))

namespace gr {
namespace conf {

GR_HD bool known_type(uint32_t t) {  // peer.go:159-168: any other type panics
  return t == GR_CC_ADD_NODE || t == GR_CC_REMOVE_NODE || t == GR_CC_ADD_OBSERVER;
}

// The member slot of node `id` (raft.remotes / raft.observers lookups), or GR_SLOT_NONE.
GR_HD uint32_t member_slot(const gr_peer& g, uint32_t S, uint64_t id) {
  uint32_t s = GR_SLOT_NONE;
  for (uint32_t j = 0; j < S; ++j)
    if (s == GR_SLOT_NONE && g.remotes[j].kind != GR_SLOT_EMPTY && g.remote_id[j] == id) s = j;
  return s;
}

// Where a node that is no member goes: the empty slot that already carries its
// id (a re-add), else the lowest empty slot no live ReadIndex FIFO entry names.
// readStatus.confirmed is keyed by node id (readindex.go:21-26, 77-116) and the
// entry of a removed node stays in it, so its slot's ack bit still counts; a new
// node given that slot would be counted once where the reference counts two.
GR_HD uint32_t free_slot(const gr_peer& g, uint32_t S, uint64_t id) {
  uint32_t named = 0;
  for (uint32_t q = 0; q < g.read_index_count && q < (uint32_t)GR_Q; ++q) {
    named |= g.read_index[q].ack_bits;
    if (g.read_index[q].from_slot < S) named |= 1u << g.read_index[q].from_slot;
  }
  uint32_t again = GR_SLOT_NONE, fresh = GR_SLOT_NONE;
  for (uint32_t j = 0; j < S; ++j) {
    if (g.remotes[j].kind != GR_SLOT_EMPTY) continue;
    if (again == GR_SLOT_NONE && g.remote_id[j] == id) again = j;
    if (fresh == GR_SLOT_NONE && !((named >> j) & 1u)) fresh = j;
  }
  return again != GR_SLOT_NONE ? again : fresh;
}

// setRemote / setObserver (raft.go:872-889): a new remote{match: 0, next:
// lastIndex + 1}, so state Retry, inactive, snapshotIndex 0 (remote.go:47-54).
GR_HD void set_member(gr_peer& g, uint32_t j, uint64_t id, uint32_t kind) {
  g.remote_id[j] = id;
  memset(&g.remotes[j], 0, sizeof(gr_remote));
  g.remotes[j].next = g.last_index + 1;
  g.remotes[j].state = GR_RETRY;
  g.remotes[j].kind = (uint8_t)kind;
}

// deleteRemote / deleteObserver (raft.go:863-870): the slot reads as an empty
// one of a freshly loaded record; remote_id stays (free_slot's re-add).
GR_HD void drop_member(gr_peer& g, uint32_t j) {
  memset(&g.remotes[j], 0, sizeof(gr_remote));
  g.remotes[j].kind = GR_SLOT_EMPTY;
}

// gr_peer.self_slot as gpuraft.h defines it (selfRemoved, raft.go:813-820, reads it).
GR_HD void set_self_slot(gr_peer& g, uint32_t S) { g.self_slot = (uint8_t)member_slot(g, S, g.node_id); }

// entryLog.term (logentry.go:141-157) over the record's term-run window, as the
// general lane's term_of (gr_lane.h): false = the index lies below the window.
GR_HD bool term_of(const gr_peer& g, uint64_t x, uint64_t* t) {
  *t = 0;
  if (x < g.first_index_m1 || x > g.last_index) return true;
  const uint32_t n = g.n_runs <= GR_K ? g.n_runs : GR_K;
  if (n == 0 || x < g.run_start[0]) return false;
  for (uint32_t r = 0; r < n; ++r)
    if (g.run_start[r] <= x) *t = g.run_term[r];
  return true;
}

// removeNode's tail (raft.go:856-860): tryCommit (raft.go:625-641,
// logentry.go:359-374) with no state check; where it would raise committed the
// reference broadcasts Replicates, which only a pass can do.
GR_HD int32_t try_commit(const gr_peer& g, uint32_t S) {
  uint64_t m[GR_SMAX];
  uint32_t nv = 0;
  for (uint32_t j = 0; j < S; ++j)
    if (g.remotes[j].kind == GR_SLOT_VOTER) m[nv++] = g.remotes[j].match;
  if (nv == 0) return GR_CC_APPLIED;  // len(r.remotes) == 0: not evaluated
  for (uint32_t a = 1; a < nv; ++a)  // sortMatchValues, ascending
    for (uint32_t b = a; b > 0 && m[b - 1] > m[b]; --b) {
      const uint64_t v = m[b];
      m[b] = m[b - 1];
      m[b - 1] = v;
    }
  const uint64_t q = m[nv - (nv / 2 + 1)];  // matched[len(remotes) - quorum()]
  if (q <= g.committed) return GR_CC_APPLIED;
  uint64_t t;
  if (!term_of(g, q, &t)) return GR_CC_HOST;  // LogReader.Term territory
  return t == g.term ? GR_CC_HOST : GR_CC_APPLIED;
}

// becomeFollower(r.term, r.leaderID) of a promoted observer (raft.go:833-835,
// 669-674): reset(term) with the term unchanged (raft.go:704-720, so the vote
// stays) and the draw `rand`, then the leader id it had. As the general lane's
// reset() (gr_lane.h).
GR_HD int32_t become_follower(gr_peer& g, uint32_t S, uint64_t rand) {
  if (g.election_timeout == 0) return GR_CC_HOST;  // rand % electionTimeout panics (raft.go:436)
  g.state = GR_FOLLOWER;
  g.votes_granted = 0;
  g.votes_rejected = 0;
  g.election_tick = 0;
  g.heartbeat_tick = 0;
  g.randomized_election_timeout = g.election_timeout + rand % g.election_timeout;  // raft.go:435-438
  memset(g.read_index, 0, sizeof(g.read_index));  // newReadIndex()
  g.read_index_count = 0;
  g.flags &= (uint8_t)~GR_F_PENDING_CONFIG_CHANGE;
  g.leader_transfer_target = 0;
  for (uint32_t j = 0; j < S; ++j) {  // resetRemotes / resetObservers, raft.go:733-753
    if (g.remotes[j].kind == GR_SLOT_EMPTY) continue;
    const uint8_t kind = g.remotes[j].kind;
    set_member(g, j, g.remote_id[j], kind);
    if (g.remote_id[j] == g.node_id) g.remotes[j].match = g.last_index;
  }
  return GR_CC_APPLIED;
}

// One change on one record. Anything but GR_CC_APPLIED: g holds garbage and the
// caller keeps the peer as it was.
GR_HD int32_t apply(gr_peer& g, uint32_t S, const gr_config_change& c) {
  // a candidate's vote tally overlays the FIFO ack rows by slot (gr_layout.h
  // Rows::B_VOTES_*): a slot that changes hands would inherit a vote
  if (g.state == GR_CANDIDATE) return GR_CC_HOST;
  g.flags &= (uint8_t)~GR_F_PENDING_CONFIG_CHANGE;  // clearPendingConfigChange, every path
  if (c.node_id == 0) return GR_CC_APPLIED;         // peer.go:155-158, RejectConfigChange :172-174
  const uint64_t id = c.node_id;
  const uint32_t j = member_slot(g, S, id);
  int32_t rc = GR_CC_APPLIED;
  if (c.type == GR_CC_REMOVE_NODE) {  // raft.go:849-861
    if (j != GR_SLOT_NONE) drop_member(g, j);
    // leaderTransfering() && leaderTransferTarget == id: abortLeaderTransfer (raft.go:246-252)
    if (g.state == GR_LEADER && g.leader_transfer_target == id) g.leader_transfer_target = 0;
    rc = try_commit(g, S);
  } else if (c.type == GR_CC_ADD_NODE) {  // raft.go:822-839
    if (j != GR_SLOT_NONE && g.remotes[j].kind == GR_SLOT_VOTER) {
    } else if (j != GR_SLOT_NONE) {  // an observer keeps its progress
      g.remotes[j].kind = GR_SLOT_VOTER;
      if (id == g.node_id) rc = become_follower(g, S, c.rand);
    } else {
      const uint32_t f = free_slot(g, S, id);
      if (f == GR_SLOT_NONE) return GR_CC_NO_SLOT;
      set_member(g, f, id, GR_SLOT_VOTER);
    }
  } else {  // GR_CC_ADD_OBSERVER, raft.go:841-847
    if (j != GR_SLOT_NONE && g.remotes[j].kind == GR_SLOT_OBSERVER) {
    } else if (j != GR_SLOT_NONE) {
      return GR_CC_HOST;  // the reference now holds the id in both maps; a slot has one kind
    } else {
      const uint32_t f = free_slot(g, S, id);
      if (f == GR_SLOT_NONE) return GR_CC_NO_SLOT;
      set_member(g, f, id, GR_SLOT_OBSERVER);
    }
  }
  set_self_slot(g, S);
  return rc;
}

// The header word of a changed peer: header_of's (what a load of the record
// gives), except
//  - the summaries that do not depend on membership are kept as the lanes left
//    them: H_CL (neither lastIndex nor committed moves here), H_GE_LO and, where
//    the header has them, the run bits (term, committed and the window stay);
//  - the remote summaries H_NX / H_MS / H_MP are cleared (every remote row is
//    written exact beside this word);
//  - F_LSLOT does not name an empty slot: a follower whose leader was removed
//    keeps leaderID and forgets the slot (0 = none known, which every reader
//    takes as "load the remote id").
GR_HD uint64_t header_after(const gr_peer& g, uint32_t S, uint64_t old) {
  uint64_t h = host::header_of(g, S);
  const uint64_t keep = H_CL_MASK | (1ull << H_GE_LO_BIT) | (has_run_bits((int)S) ? H_RUN_MASK : 0ull);
  h = (h & ~keep) | (old & keep);
  if (has_sync_bits((int)S)) h &= ~H_SYNC_MASK;
  const uint32_t sl = (h_flags(h) & F_LSLOT) >> F_LSLOT_SHIFT;
  if (sl && g.remotes[sl - 1].kind == GR_SLOT_EMPTY) h &= ~((uint64_t)F_LSLOT << H_FLAGS_SHIFT);
  return h;
}

// One change on the state rows of peer p: the rows are read into a record as
// gr_sync_peers_to_host reads them, changed, and written back as gr_load_peers
// writes them. A refused change writes nothing.
template <int S>
GR_HD int32_t apply_rows(const StateBase& st, uint32_t p, const gr_config_change& c) {
  constexpr uint32_t n64 = SR_REMOTE + 4 * S + 3 * GR_Q, n8 = 2 * GR_Q;  // rows_u64(S), rows_u8(S)
  gr_peer g;
  memset(&g, 0, sizeof(g));
  const uint64_t old = st.u64(SR_HDR)[p];
  for (uint32_t r = 0; r < n64; ++r) host::set_u64_row(g, r, S, st.u64(r)[p]);
  host::resolve_sync(g, S, old);
  for (uint32_t r = 0; r < n8; ++r) host::set_u8_row(g, r, S, st.u8(r)[p]);
  const int32_t rc = apply(g, S, c);
  if (rc != GR_CC_APPLIED) return rc;
  for (uint32_t r = 0; r < n64; ++r) st.u64(r)[p] = r == SR_HDR ? header_after(g, S, old) : host::get_u64_row(g, r, S);
  for (uint32_t r = 0; r < n8; ++r) st.u8(r)[p] = host::get_u8_row(g, r, S);
  return rc;
}

// ---------------------------------------------------------------- restoreRemotes
// Peer.RestoreRemotes (peer.go:177-180 -> raft.restoreRemotes, raft.go:327-355)
// behind gr_restore_remotes, by the same read-record / transform / write-record
// scheme. The reference rebuilds both maps from the snapshot's membership:
// every listed id gets remote{match: 0 or lastIndex for the peer itself, next:
// lastIndex + 1}, every other member is gone. Before it sets a voter that it
// holds as an observer it runs becomeFollower(term, leaderID) (:329-333), whose
// reset() draws once: two such ids need two draws and go to the host.

// The list's length (the first GR_SLOT_EMPTY kind ends it).
GR_HD uint32_t listed(const gr_membership& m) {
  uint32_t n = 0;
  while (n < (uint32_t)GR_SMAX && m.kind[n] != GR_SLOT_EMPTY) n++;
  return n;
}
GR_HD bool known_kinds(const gr_membership& m) {
  for (uint32_t k = 0; k < listed(m); ++k)
    if (m.kind[k] != GR_SLOT_VOTER && m.kind[k] != GR_SLOT_OBSERVER) return false;
  return true;
}

// One membership on one record. Anything but GR_CC_APPLIED: g holds garbage and
// the caller keeps the peer as it was.
GR_HD int32_t restore_remotes(gr_peer& g, uint32_t S, const gr_membership& m) {
  if (g.state == GR_CANDIDATE) return GR_CC_HOST;  // as apply(): the tally overlays the ack rows by slot
  const uint32_t n = listed(m);
  uint32_t promoted = 0;
  for (uint32_t k = 0; k < n; ++k) {
    for (uint32_t x = 0; x < k; ++x)
      if (m.node_id[x] == m.node_id[k]) return GR_CC_HOST;  // an id in both maps, or twice in one
    const uint32_t j = member_slot(g, S, m.node_id[k]);
    if (m.kind[k] == GR_SLOT_VOTER && j != GR_SLOT_NONE && g.remotes[j].kind == GR_SLOT_OBSERVER) promoted++;
  }
  if (promoted > 1) return GR_CC_HOST;
  if (promoted) {
    const int32_t rc = become_follower(g, S, m.rand);  // keeps leaderID; clears the FIFO
    if (rc != GR_CC_APPLIED) return rc;
  }
  // members that are not listed go; their slots keep their ids
  for (uint32_t j = 0; j < S; ++j) {
    if (g.remotes[j].kind == GR_SLOT_EMPTY) continue;
    bool keep = false;
    for (uint32_t k = 0; k < n; ++k) keep = keep || m.node_id[k] == g.remote_id[j];
    if (!keep) drop_member(g, j);
  }
  // an id keeps the slot that carries it, live or empty: the mailbox routes
  // bound to that slot stay valid
  for (uint32_t k = 0; k < n; ++k) {
    uint32_t j = member_slot(g, S, m.node_id[k]);
    for (uint32_t x = 0; x < S; ++x)
      if (j == GR_SLOT_NONE && g.remotes[x].kind == GR_SLOT_EMPTY && g.remote_id[x] == m.node_id[k]) j = x;
    if (j == GR_SLOT_NONE) continue;
    set_member(g, j, m.node_id[k], m.kind[k]);
    if (m.node_id[k] == g.node_id) g.remotes[j].match = g.last_index;
  }
  // the others take free slots by apply()'s rule
  for (uint32_t k = 0; k < n; ++k) {
    if (member_slot(g, S, m.node_id[k]) != GR_SLOT_NONE) continue;
    const uint32_t f = free_slot(g, S, m.node_id[k]);
    if (f == GR_SLOT_NONE) return GR_CC_NO_SLOT;
    set_member(g, f, m.node_id[k], m.kind[k]);
    if (m.node_id[k] == g.node_id) g.remotes[f].match = g.last_index;
  }
  set_self_slot(g, S);
  return GR_CC_APPLIED;
}

template <int S>
GR_HD int32_t restore_rows(const StateBase& st, uint32_t p, const gr_membership& m) {
  constexpr uint32_t n64 = SR_REMOTE + 4 * S + 3 * GR_Q, n8 = 2 * GR_Q;  // rows_u64(S), rows_u8(S)
  gr_peer g;
  memset(&g, 0, sizeof(g));
  const uint64_t old = st.u64(SR_HDR)[p];
  for (uint32_t r = 0; r < n64; ++r) host::set_u64_row(g, r, S, st.u64(r)[p]);
  host::resolve_sync(g, S, old);
  for (uint32_t r = 0; r < n8; ++r) host::set_u8_row(g, r, S, st.u8(r)[p]);
  const int32_t rc = restore_remotes(g, S, m);
  if (rc != GR_CC_APPLIED) return rc;
  for (uint32_t r = 0; r < n64; ++r) st.u64(r)[p] = r == SR_HDR ? header_after(g, S, old) : host::get_u64_row(g, r, S);
  for (uint32_t r = 0; r < n8; ++r) st.u8(r)[p] = host::get_u8_row(g, r, S);
  return rc;
}

}  // namespace conf
}  // namespace gr

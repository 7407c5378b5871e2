// wire_out_san — a stand-alone CPU program (its own main; never loaded into
// Python, never run on a GPU) that drives gr_wire_out_host's implementation
// (gr_host.h wire_out_host, the code the kernels of gr_io.h share) over seeded
// outbox records, built with ASAN + UBSAN by tests/test_wire_out_host.py. Every
// output array is allocated at exactly the documented size, so a write past it is
// a sanitizer report; the rule, the order and the cuts are re-derived here with
// plain loops and compared.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "gr_host.h"

using namespace gr;

static uint64_t rng_state = 0x1234567ull;
static uint64_t rnd() { return rng_state = q_splitmix64(rng_state); }

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

struct Case {
  uint32_t n_peers, S, T, mbm;
  double host_frac, entry_frac;
};

static void run(const Case& c) {
  const size_t pairs = (size_t)c.n_peers * c.S;
  std::vector<uint64_t> cl(c.n_peers), nd(c.n_peers), rid(pairs);
  std::vector<uint32_t> tgt(pairs);
  for (uint32_t p = 0; p < c.n_peers; ++p) {
    cl[p] = 1 + p / c.S;
    nd[p] = 1 + p % c.S;
    for (uint32_t j = 0; j < c.S; ++j) {
      rid[(size_t)p * c.S + j] = 100 + j;
      tgt[(size_t)p * c.S + j] = (rnd() % 1000) < c.host_frac * 1000 ? GR_TARGET_HOST : (uint32_t)(rnd() % c.T);
    }
  }
  // outbox order: peer, slot, position; 0..GR_C messages per mailbox
  std::vector<gr_message> msgs;
  for (uint32_t p = 0; p < c.n_peers; ++p)
    for (uint32_t j = 0; j < c.S; ++j) {
      const uint32_t k = (uint32_t)(rnd() % (GR_C + 1));
      for (uint32_t q = 0; q < k; ++q) {
        gr_message m{};
        m.peer = p;
        m.slot = (uint8_t)j;
        const uint8_t types[] = {GR_REPLICATE, GR_REPLICATE_RESP, GR_HEARTBEAT, GR_HEARTBEAT_RESP, GR_REQUEST_VOTE,
                                 GR_REQUEST_VOTE_RESP, GR_TIMEOUT_NOW, GR_READ_INDEX, GR_READ_INDEX_RESP, GR_NOOP,
                                 GR_QUIESCE, GR_INSTALL_SNAPSHOT};
        m.type = types[rnd() % (sizeof(types) / sizeof(types[0]))];
        m.reject = (uint8_t)(rnd() & 1);
        m.term = rnd() % 9;
        m.log_index = rnd();
        m.log_term = rnd() % 9;
        m.commit = rnd();
        m.hint = rnd();
        m.hint_high = rnd();
        if (m.type == GR_REPLICATE && (rnd() % 1000) < c.entry_frac * 1000) {
          m.n_entries = 1 + (uint32_t)(rnd() % 3);
          m.n_runs = 1;
          m.run_term[0] = m.term;
        }
        msgs.push_back(m);
      }
    }
  const size_t n = msgs.size();
  gr_wire_out_cfg cfg{};
  cfg.deployment_id = 77;
  cfg.bin_ver = 210;
  cfg.max_batch_msgs = c.mbm;
  cfg.source_off = 3;
  cfg.source_len = 9;
  std::vector<grw_batch> bat(n);
  std::vector<grw_message> wm(n);
  std::vector<uint32_t> bt(n);
  std::vector<uint8_t> held(n);
  size_t nb = ~(size_t)0, nw = ~(size_t)0;
  CHECK(host::wire_out_host(msgs.data(), n, cl.data(), nd.data(), rid.data(), c.n_peers, c.S, tgt.data(), c.T, &cfg,
                            bat.data(), &nb, wm.data(), &nw, bt.data(), held.data()) == GR_OK);
  // the rule per mailbox, and the expected order: target, peer, slot, position
  std::map<uint32_t, std::vector<size_t>> by_target;
  for (size_t a = 0; a < n;) {
    size_t b = a;
    bool ok = true;
    while (b < n && msgs[b].peer == msgs[a].peer && msgs[b].slot == msgs[a].slot) {
      ok = ok && msgs[b].n_entries == 0 && msgs[b].type != GR_INSTALL_SNAPSHOT;
      ++b;
    }
    const uint32_t t = tgt[(size_t)msgs[a].peer * c.S + msgs[a].slot];
    const bool wire = ok && t != GR_TARGET_HOST;
    for (size_t k = a; k < b; ++k) {
      CHECK(held[k] == (wire ? 0 : 1));
      if (wire) by_target[t].push_back(k);
    }
    a = b;
  }
  size_t pos = 0, bi = 0;
  for (auto& kv : by_target) {
    const size_t first = pos, cnt = kv.second.size();
    for (size_t k : kv.second) {
      const gr_message& m = msgs[k];
      const grw_message& w = wm[pos];
      CHECK(w.to == rid[(size_t)m.peer * c.S + m.slot] && w.from == nd[m.peer] && w.cluster_id == cl[m.peer]);
      CHECK(w.type == (int32_t)m.type && w.term == m.term && w.log_term == m.log_term && w.log_index == m.log_index);
      CHECK(w.commit == m.commit && w.hint == m.hint && w.hint_high == m.hint_high && w.reject == (m.reject ? 1 : 0));
      CHECK(w.n_entries == 0 && w.first_entry == 0 && w.snapshot_len == 0 && w.snapshot_off == 0);
      CHECK(w.msg_off == 0 && w.msg_len == 0 && w.snapshot_host == 0);
      CHECK(w.batch == bi + (pos - first) / c.mbm);
      ++pos;
    }
    const size_t nbt = (cnt + c.mbm - 1) / c.mbm;
    for (size_t x = 0; x < nbt; ++x, ++bi) {
      CHECK(bi < nb && bt[bi] == kv.first);
      CHECK(bat[bi].first_msg == first + x * c.mbm);
      CHECK(bat[bi].n_msgs == (x + 1 < nbt ? c.mbm : cnt - x * c.mbm));
      CHECK(bat[bi].deployment_id == 77 && bat[bi].bin_ver == 210 && bat[bi].source_off == 3 &&
            bat[bi].source_len == 9);
      CHECK(bat[bi].frame_off == 0 && bat[bi].frame_len == 0 && bat[bi].status == 0);
    }
  }
  CHECK(pos == nw && bi == nb);

  // refusals write nothing
  nb = nw = 12345;
  std::vector<uint8_t> held0(held);
  std::vector<uint32_t> bad(tgt);
  if (!bad.empty() && n) {
    bad[pairs - 1] = c.T;  // an index out of range
    CHECK(host::wire_out_host(msgs.data(), n, cl.data(), nd.data(), rid.data(), c.n_peers, c.S, bad.data(), c.T, &cfg,
                              bat.data(), &nb, wm.data(), &nw, bt.data(), held.data()) == GR_EINVAL);
    CHECK(host::wire_out_host(msgs.data(), n, cl.data(), nd.data(), rid.data(), c.n_peers, c.S, tgt.data(), 0, &cfg,
                              bat.data(), &nb, wm.data(), &nw, bt.data(), held.data()) == GR_EINVAL);
    CHECK(host::wire_out_host(msgs.data(), n, cl.data(), nd.data(), rid.data(), c.n_peers, c.S, tgt.data(),
                              GR_MAX_TARGETS + 1, &cfg, bat.data(), &nb, wm.data(), &nw, bt.data(),
                              held.data()) == GR_EINVAL);
    gr_wire_out_cfg z = cfg;
    z.max_batch_msgs = 0;
    CHECK(host::wire_out_host(msgs.data(), n, cl.data(), nd.data(), rid.data(), c.n_peers, c.S, tgt.data(), c.T, &z,
                              bat.data(), &nb, wm.data(), &nw, bt.data(), held.data()) == GR_EINVAL);
    CHECK(host::wire_out_host(msgs.data(), n, cl.data(), nd.data(), rid.data(), c.n_peers, c.S, tgt.data(), c.T, &cfg,
                              nullptr, &nb, wm.data(), &nw, bt.data(), held.data()) == GR_EINVAL);
    CHECK(host::wire_out_host(msgs.data(), n, cl.data(), nd.data(), rid.data(), c.n_peers, c.S, tgt.data(), c.T, &cfg,
                              bat.data(), &nb, wm.data(), &nw, bt.data(), nullptr) == GR_EINVAL);
    CHECK(nb == 12345 && nw == 12345 && held == held0);
  }
}

int main() {
  const Case cases[] = {
      {1, 1, 1, 1, 0.0, 0.0},       {7, 3, 3, 1, 0.2, 0.3},    {64, 3, 3, 3, 0.1, 0.3},
      {300, 3, 5, 0x80000000u, 0.0, 0.5}, {41, 5, 256, 2, 0.3, 0.2}, {9, 8, 2, 4, 1.0, 0.2},
      {33, 5, 4, 7, 0.0, 0.0},
  };
  for (const Case& c : cases) run(c);
  // an empty outbox
  gr_wire_out_cfg cfg{};
  cfg.max_batch_msgs = 1;
  size_t nb = 9, nw = 9;
  CHECK(host::wire_out_host(nullptr, 0, nullptr, nullptr, nullptr, 0, 3, nullptr, 1, &cfg, nullptr, &nb, nullptr, &nw,
                            nullptr, nullptr) == GR_OK);
  CHECK(nb == 0 && nw == 0);
  printf("wire_out_san ok\n");
  return 0;
}

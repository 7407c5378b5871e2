// quiesce_host.cpp — the host build of dragonboat_amd/csrc/gr_quiesce.h behind a
// small C interface (tests/_build/libquiesce_host.so, test-only): the same
// functions the device kernel calls, compiled by g++, so tests/test_quiesce.py
// can compare them with the golden tables and the Python model.
#include <stdint.h>

#include "gr_quiesce.h"

using namespace gr;

extern "C" {

enum { QH_TICK = 0, QH_ACT, QH_TRY_ENTER, QH_QUIESCED, QH_NEW_TO_QUIESCE, QH_JUST_EXITED, QH_MESSAGE, QH_ENTER,
       QH_EXIT, QH_NODE_TICK };

// One manager call on the record *s with its new-state flag *flag (0/1).
// arg: the message type (QH_ACT), or type | (Hint > 0) << 8 (QH_MESSAGE).
uint64_t qh_op(gr_quiesce_state* s, uint8_t* flag, int op, uint32_t arg) {
  QuiesceMgr q = q_from_state(*s);
  q.flag = *flag != 0;
  uint64_t r = 0;
  switch (op) {
    case QH_TICK: r = q_increase_quiesce_tick(q); break;
    case QH_ACT: q_record_activity(q, arg); break;
    case QH_TRY_ENTER: q_try_enter_quiesce(q); break;
    case QH_QUIESCED: r = q_quiesced(q); break;
    case QH_NEW_TO_QUIESCE: r = q_new_to_quiesce(q); break;
    case QH_JUST_EXITED: r = q_just_exited_quiesce(q); break;
    case QH_MESSAGE: q_message(q, arg & 0xFFu, (arg >> 8) != 0); break;
    case QH_ENTER: q_enter_quiesce(q); break;
    case QH_EXIT: q_exit_quiesce(q); break;
    case QH_NODE_TICK: r = q_tick(q); break;
    default: return ~0ull;
  }
  *s = q_to_state(q);
  *flag = q.flag ? 1 : 0;
  return r;
}

// One pass each for n peers (q_run_pass): peer x has messages
// [msg_off[x], msg_off[x+1]) of types / hints (Hint > 0 flags), a ReadIndex flag,
// raw LocalTicks and an item limit; out[3x..] = ticks, quiesced_ticks, send.
void qh_run_passes(uint32_t n, gr_quiesce_state* s, const uint8_t* read_index, const uint32_t* msg_off,
                   const uint8_t* types, const uint8_t* hints, const uint32_t* raw_ticks, const uint32_t* limits,
                   uint32_t* out) {
  for (uint32_t x = 0; x < n; ++x) {
    QuiesceMgr q = q_from_state(s[x]);
    const uint32_t o = msg_off[x];
    const QuiescePass r = q_run_pass(q, read_index[x] != 0, msg_off[x + 1] - o, raw_ticks[x], limits[x],
                                     [&](uint32_t nm, auto sink) {
                                       for (uint32_t k = 0; k < nm; ++k) sink(types[o + k], hints[o + k] != 0);
                                     });
    s[x] = q_to_state(q);
    out[3 * x] = r.ticks;
    out[3 * x + 1] = r.quiesced_ticks;
    out[3 * x + 2] = r.send ? 1u : 0u;
  }
}

// The device encoding: 1 and *out = decode(encode(*in)) when it holds *in, else 0.
int qh_roundtrip(const gr_quiesce_state* in, gr_quiesce_state* out) {
  if (!q_encodable(*in)) return 0;
  const QuiesceMgr q = q_from_state(*in);
  *out = q_to_state(q_decode(q_encode(q), q_cfg(*in)));
  return 1;
}

uint64_t qh_splitmix64(uint64_t x) { return q_splitmix64(x); }
uint32_t qh_sizeof_state(void) { return (uint32_t)sizeof(gr_quiesce_state); }

}  // extern "C"

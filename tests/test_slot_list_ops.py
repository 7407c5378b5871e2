"""The slot-list operations of the C-ABI, one table: gr_compact_log,
gr_commit_update, gr_apply_config_change, gr_restore_remotes,
gr_set/get_snapshot_recs, gr_set/get_cc_indexes and gr_notify_applied.

They share one order of checks (gpuraft.h): null arguments (GR_EINVAL), an
empty list (GR_OK), a slot out of range or listed twice (GR_ERANGE, before
anything is written and before the records are looked at), a pass pending
between gr_step_compact_begin and _end (GR_ESTATE, again before the records are
looked at), then a record no reference call would take (GR_EINVAL). Every case
goes through raw library calls, so the codes are seen exactly; a refused call
leaves the peers, the side arrays and the caller's status array as they were.
One good call per operation is read back and compared with what the host build
of the same code (or the record itself) gives.
"""
import ctypes

import numpy as np
import pytest

from dragonboat_amd import abi
import config_change_common as CC
import parity
import snapshot_common as SN
from oracle.pyoracle import hostlane_commit_update
from test_config_change import _group

pytestmark = pytest.mark.gpu

N = 8                     # engine slots
EINVAL, ERANGE, ESTATE = -1, -4, -6
SENTINEL = -7             # no status any operation writes
INSTANCE = {1: 1, 3: 3, 4: 8}  # gr_config.slots -> the instantiated slot count


def _peers(slots):
    """Eight peers of groups with max(1, slots - 1) voters (so a slot is free
    wherever there is more than one): leaders in the even engine slots,
    followers (or, alone, leaders again) in the odd ones. Log 1..10 at term 5,
    committed 8."""
    nv = max(1, slots - 1)
    lead = _group(slots, 1, abi.LEADER, [10] + [8] * (nv - 1))
    foll = _group(slots, 2, abi.FOLLOWER, [0, 10] + [0] * (nv - 2)) if nv > 1 else lead
    return np.concatenate([lead, foll] * (N // 2))


def _u64(vals):
    return np.asarray(vals, np.uint64)


def _changes(n, slots):
    """A change every peer of _peers applies: a new voter into the free slot, or,
    with one slot, the removal of its only member."""
    return CC.changes(n, abi.CC_ADD_NODE, 9) if slots > 1 else CC.changes(n, abi.CC_REMOVE_NODE, 1)


def _bad_changes(n, slots):
    cc = _changes(n, slots)
    cc["type"][n - 1] = 3  # no raftpb.ConfigChangeType
    return cc


def _members(n, slots):
    nv = max(1, slots - 1)
    return np.concatenate([SN.membership([(k + 1, abi.SLOT_VOTER) for k in range(nv)])] * n)


def _bad_members(n, slots):
    ms = _members(n, slots)
    ms[n - 1]["kind"][0] = 3  # no member kind
    return ms


def _commits(n, slots):
    uc = np.zeros(n, abi.UPDATE_COMMIT)
    uc["applied_to"] = 5 + np.arange(n)
    return uc


def _snaps(n, slots):
    r = np.zeros(n, abi.SNAPSHOT_REC)
    r["index"], r["term"] = 3 + np.arange(n), 5
    return r


def _ccidx(n, slots):
    r = np.zeros(n, abi.CC_INDEX)
    r["last"], r["prev"] = 10 - np.arange(n), 9 - np.arange(n)
    return r


def _out(dtype):
    def make(n, slots):
        return np.full(n, 0xAB, np.uint8).repeat(dtype.itemsize).view(dtype)  # a get's buffer: a sentinel too
    return make


# ---- what a good call must leave behind: (engine, peers before, slot list, records, instance, status)
def _want_compact(eng, before, sl, recs, S, st):
    assert list(st) == [0] * len(sl)
    want = before.copy()
    want["first_index_m1"][sl] = recs
    after = eng.sync(N)
    assert list(after["first_index_m1"][sl]) == list(recs)
    assert not parity.compare_states(after, want, S)


def _want_commit(eng, before, sl, recs, S, st):
    want = before.copy()
    rc, hst = hostlane_commit_update(want, sl, recs, S)
    assert rc == 0 and list(st) == list(hst) == [0] * len(sl)
    after = eng.sync(N)
    assert list(after["log_applied"][sl]) == list(recs["applied_to"])
    assert not parity.compare_states(after, want, S)


def _want_change(eng, before, sl, recs, S, st):
    want = before.copy()
    rc, hst = CC.host_apply(want, sl, recs, S)
    assert rc == 0 and list(st) == list(hst) == [abi.CC_APPLIED] * len(sl)
    assert want.tobytes() != before.tobytes()
    assert not parity.compare_states(eng.sync(N), want, S)


def _want_restore(eng, before, sl, recs, S, st):
    want = before.copy()
    rc, hst = SN.host_restore(want, sl, recs, S)
    assert rc == 0 and list(st) == list(hst) == [abi.CC_APPLIED] * len(sl)
    assert not parity.compare_states(eng.sync(N), want, S)


def _want_snaps(eng, before, sl, recs, S, st):
    want = np.zeros(N, abi.SNAPSHOT_REC)
    want[sl] = recs
    assert eng.get_snapshot_recs(np.arange(N)).tobytes() == want.tobytes()
    assert eng.sync(N).tobytes() == before.tobytes()


def _want_get_snaps(eng, before, sl, recs, S, st):
    eng.set_snapshot_recs(np.arange(N), _snaps(N, S))
    assert eng.lib.gr_get_snapshot_recs(eng._h, sl.ctypes.data, recs.ctypes.data, len(sl)) == 0
    assert recs.tobytes() == _snaps(N, S)[sl].tobytes()


def _want_ccidx(eng, before, sl, recs, S, st):
    want = np.zeros(N, abi.CC_INDEX)
    want[sl] = recs
    assert eng.get_cc_indexes(np.arange(N)).tobytes() == want.tobytes()
    assert eng.sync(N).tobytes() == before.tobytes()


def _want_get_ccidx(eng, before, sl, recs, S, st):
    eng.set_cc_indexes(np.arange(N), _ccidx(N, S))
    assert eng.lib.gr_get_cc_indexes(eng._h, sl.ctypes.data, recs.ctypes.data, len(sl)) == 0
    assert recs.tobytes() == _ccidx(N, S)[sl].tobytes()


def _want_applied(eng, before, sl, recs, S, st):
    want = before.copy()
    want["applied"][sl] = recs
    after = eng.sync_peers(sl)
    assert list(after["applied"]) == list(recs)
    assert eng.sync(N).tobytes() == want.tobytes()  # no other field changes


class Op:
    def __init__(self, name, good, want, bad=None, status=False):
        self.name, self.good, self.want, self.bad, self.status = name, good, want, bad, status

    def call(self, eng, slots, recs, n, st=None):
        """The raw call: slots / recs arrays or None (a null pointer)."""
        ptr = lambda a: None if a is None else a.ctypes.data
        args = [eng._h, ptr(slots), ptr(recs), n] + ([ptr(st)] if self.status else [])
        return getattr(eng.lib, self.name)(*args)


OPS = [
    Op("gr_compact_log", lambda n, s: _u64(4 + np.arange(n)), _want_compact, status=True),
    Op("gr_commit_update", _commits, _want_commit, status=True),
    Op("gr_apply_config_change", _changes, _want_change, bad=_bad_changes, status=True),
    Op("gr_restore_remotes", _members, _want_restore, bad=_bad_members, status=True),
    Op("gr_set_snapshot_recs", _snaps, _want_snaps),
    Op("gr_get_snapshot_recs", _out(abi.SNAPSHOT_REC), _want_get_snaps),
    Op("gr_set_cc_indexes", _ccidx, _want_ccidx),
    Op("gr_get_cc_indexes", _out(abi.CC_INDEX), _want_get_ccidx),
    Op("gr_notify_applied", lambda n, s: _u64(6 + np.arange(n)), _want_applied),
]
BY_NAME = {op.name: op for op in OPS}
OP_IDS = [op.name[3:] for op in OPS]


def _engine(slots):
    from dragonboat_amd.engine import Engine
    eng = Engine(N, slots, elections=True, snapshots=True, config_entries=True)
    eng.load(_peers(slots))
    return eng


def _everything(eng):
    """The peers and both side arrays, as bytes."""
    a = np.arange(N)
    return eng.sync(N).tobytes(), eng.get_snapshot_recs(a).tobytes(), eng.get_cc_indexes(a).tobytes()


def _slots(*v):
    return np.asarray(v, np.uint32)


@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
def test_refusals_write_nothing(built, gpu, op):
    """Null records, an empty list, a slot out of range, a slot listed twice, and
    either of the last two together with a record that would be refused on its own."""
    eng = _engine(3)
    try:
        before = _everything(eng)
        cases = [("null records", _slots(0, 1), None, 2, EINVAL),
                 ("null slots", None, op.good(2, 3), 2, EINVAL),
                 ("empty", None, None, 0, 0),
                 ("out of range", _slots(N), op.good(1, 3), 1, ERANGE),
                 ("out of range, last", _slots(0, N), op.good(2, 3), 2, ERANGE),
                 ("listed twice", _slots(1, 1), op.good(2, 3), 2, ERANGE)]
        if op.bad:
            cases += [("out of range and a bad record", _slots(N), op.bad(1, 3), 1, ERANGE),
                      ("listed twice and a bad record", _slots(1, 1), op.bad(2, 3), 2, ERANGE),
                      ("a bad record", _slots(0, 1), op.bad(2, 3), 2, EINVAL)]
        for what, sl, recs, n, want in cases:
            st = np.full(max(n, 1), SENTINEL, np.int32)
            given = None if recs is None else recs.tobytes()
            assert op.call(eng, sl, recs, n, st) == want, what
            assert np.all(st == SENTINEL), what
            assert _everything(eng) == before, what
            assert recs is None or recs.tobytes() == given, what  # a get's buffer too
    finally:
        eng.close()


@pytest.mark.parametrize("op", OPS, ids=OP_IDS)
def test_pending_pass_then_taken(built, gpu, op):
    """Between gr_step_compact_begin and _end every call is GR_ESTATE, a call
    whose only defect is a bad record too; after _end that call is GR_EINVAL and
    the good one is taken and does what the host side expects."""
    eng = _engine(3)
    try:
        loc = np.zeros(1, abi.LOCAL)
        loc["peer"], loc["ticks"], loc["rand"] = N - 1, 1, 77  # a follower far from its election timeout
        cm, xm = eng.pack_messages(np.zeros(0, abi.MESSAGE))
        cl, xl = eng.pack_locals(loc)
        ib, ob = abi.cinbox_of(cm, xm, cl, xl), abi.COutbox()
        sl = _slots(2, 5)
        good = op.good(2, 3)
        assert eng.lib.gr_step_compact_begin(eng._h, ctypes.byref(ib)) == 0
        for recs in [good] + ([op.bad(2, 3)] if op.bad else []):
            st = np.full(2, SENTINEL, np.int32)
            given = recs.tobytes()
            assert op.call(eng, sl, recs, 2, st) == ESTATE
            assert np.all(st == SENTINEL) and recs.tobytes() == given
        assert eng.lib.gr_step_compact_end(eng._h, ctypes.byref(ob)) == 0
        assert eng.lib.gr_release_coutbox(eng._h, ctypes.byref(ob)) == 0
        before = eng.sync(N)
        if op.bad:
            st = np.full(2, SENTINEL, np.int32)
            assert op.call(eng, sl, op.bad(2, 3), 2, st) == EINVAL and np.all(st == SENTINEL)
            assert eng.sync(N).tobytes() == before.tobytes()
        st = np.full(2, SENTINEL, np.int32)
        assert op.call(eng, sl, good, 2, st) == 0
        op.want(eng, before, sl, good, 3, st)
    finally:
        eng.close()


@pytest.mark.parametrize("slots", [1, 4])
@pytest.mark.parametrize("name", ["gr_compact_log", "gr_apply_config_change", "gr_restore_remotes"])
def test_slot_count_instances(built, gpu, name, slots):
    """The operations whose kernels are instantiated per slot count, on an engine
    of one slot and on one of four (which runs the eight-slot instance)."""
    op = BY_NAME[name]
    eng = _engine(slots)
    try:
        before = eng.sync(N)
        sl = _slots(6, 1, 3)
        recs = op.good(3, slots)
        st = np.full(3, SENTINEL, np.int32)
        assert op.call(eng, sl, recs, 3, st) == 0
        op.want(eng, before, sl, recs, INSTANCE[slots], st)
    finally:
        eng.close()

"""The bounds behind the steady kernel's bit-plane stats (gr_kernels.h
steady_stats sums a wave's counters one ballot per bit; gr_steady.h
kSteady*Bits): on the host build of the lane code, which is a checked build
(GR_COVERAGE), every lane a closed form finishes must count within them
(BAD_STEADY_STATS_RANGE stays 0) over populations that drive the counters to
their largest values: steady proposals, acks dropped and then arriving two per
follower, one follower's acks a pass late, two-entry proposals, idle passes."""
import ctypes

import numpy as np
import pytest

from dragonboat_amd import populations as P
from test_commit_lag import _HostDriver, _peers, _scenario_lag_range


def _coverage():
    from oracle.pyoracle import hostlane_lib
    lib = hostlane_lib()
    lib.hl_coverage_names.restype = ctypes.c_char_p
    names = [n for n in lib.hl_coverage_names().decode().split(",") if n]
    c = np.zeros(len(names), np.uint64)
    lib.hl_coverage(c.ctypes.data_as(ctypes.c_void_p), len(names))
    return dict(zip(names, c.tolist()))


def _two_entries(drv):
    G, R = drv.G, drv.R
    for k in range(10):
        two = k in (4, 5, 7)
        drv.step(P.propose_locals(R * G, np.arange(0, G, 3) if two else np.arange(G), entries=2 if two else 1,
                                  pass_index=k))


@pytest.mark.parametrize("workload", [_scenario_lag_range, _two_entries], ids=["lag_range", "two_entries"])
@pytest.mark.parametrize("G", [128, 192])
def test_closed_form_lanes_count_within_the_bit_planes(built, workload, G):
    from oracle.pyoracle import hostlane_steady_lanes
    before, s0 = _coverage(), hostlane_steady_lanes()
    assert "BAD_STEADY_STATS_RANGE" in before
    drv = _HostDriver(_peers(G, 3, 31), G, 3)
    try:
        workload(drv)
    finally:
        drv.close()
    after = _coverage()
    assert after["BAD_STEADY_STATS_RANGE"] == before["BAD_STEADY_STATS_RANGE"]
    assert hostlane_steady_lanes() - s0 > 3 * G
    assert after["STEADY_LEADER"] > before["STEADY_LEADER"] and after["STEADY_FOLLOWER"] > before["STEADY_FOLLOWER"]

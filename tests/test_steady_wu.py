"""The steady kernel's wave-uniform addressing (gr_steady.h WaveAddr), CPU tier.

The device kernel takes the instance when gr_layout.h steady_wu_routes and
steady_wu_space hold. Here the predicate's truth table, the compare chain that
replaces replica_of's division, and every address WaveAddr forms against the
per-lane policy's (LaneAddr, the addressing every other kernel uses), all through
the host build of those headers (tests/native/steady_wu_host.hip). The address
comparison also checks that each address lies inside its region, so a wrong
offset shows here and not as a stray store on a device.
"""
import ctypes

import numpy as np
import pytest

from dragonboat_amd import build

NOPOS = 0xFFFFFFFF
SMAX = 8           # GR_SMAX
RT_TABLE, RT_AFFINE, RT_LOOPBACK = 1, 2, 3
TILE = 256         # gr_layout.h kTileW


@pytest.fixture(scope="module")
def wu():
    lib = ctypes.CDLL(build.build_steady_wu_host())
    lib.wu_routes.argtypes = [ctypes.c_uint32] * 4 + [ctypes.c_void_p]
    lib.wu_space.argtypes = [ctypes.c_uint32, ctypes.c_uint64]
    lib.wu_replica_chain.argtypes = [ctypes.c_uint32] * 3
    lib.wu_replica_chain.restype = ctypes.c_uint32
    lib.wu_addr_mismatches.argtypes = [ctypes.c_uint32] * 7 + [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    lib.wu_addr_mismatches.restype = ctypes.c_int64
    return lib


def _bases(R, S, fn):
    """[2][SMAX][SMAX] block bases: fn(dir, r, j) or NOPOS."""
    b = np.full((2, SMAX, SMAX), NOPOS, np.uint32)
    for d in range(2):
        for r in range(R):
            for j in range(S):
                b[d, r, j] = fn(d, r, j)
    return b


def _ring(G, R, S, shift=0):
    """Affine bases of a replica-major exchange: block (r, j) at ((r * S + j) * G + shift)."""
    return _bases(R, S, lambda d, r, j: NOPOS if j == r else (r * S + j) * G + shift)


def _routes(wu, mode, S, G, R, base=None):
    return wu.wu_routes(mode, S, G, R, base.ctypes.data if base is not None else None)


def test_predicate_loopback(wu):
    for G, want in [(64, 1), (128, 1), (192, 1), (320, 1), (1 << 20, 1), (130, 0), (20000, 0), (32, 0), (63, 0),
                    (65, 0), (0, 0)]:
        assert _routes(wu, RT_LOOPBACK, 3, G, 3) == want, G
    # route_r * route_g is then a multiple of 64 too, for every replica count
    for R in (1, 2, 3, 5):
        assert _routes(wu, RT_LOOPBACK, 5, 64, R) == 1


def test_predicate_other_modes(wu):
    assert _routes(wu, 0, 3, 64, 3) == 0          # RT_IDENTITY
    assert _routes(wu, RT_TABLE, 3, 64, 3) == 0
    assert _routes(wu, RT_AFFINE, 3, 64, 3, None) == 0  # affine without its bases


def test_predicate_affine_bases(wu):
    G, R, S = 128, 3, 3
    assert _routes(wu, RT_AFFINE, S, G, R, _ring(G, R, S)) == 1
    assert _routes(wu, RT_AFFINE, S, G, R, _ring(G, R, S, shift=64)) == 1
    assert _routes(wu, RT_AFFINE, S, G, R, _ring(G, R, S, shift=32)) == 0
    assert _routes(wu, RT_AFFINE, S, 130, R, _ring(130, R, S)) == 0  # route_g itself
    # one unaligned base, in either direction, any block, refuses
    for d, r, j in [(0, 0, 1), (1, 2, 0), (0, 1, 2)]:
        b = _ring(G, R, S)
        b[d, r, j] += 8
        assert _routes(wu, RT_AFFINE, S, G, R, b) == 0, (d, r, j)
    # NOPOS is no base; blocks past route_r or S are not read
    b = _ring(G, R, S)
    b[0, 0, 1] = NOPOS
    b[1, 5, 5] = 7
    b[0, 1, 6] = 7
    assert _routes(wu, RT_AFFINE, S, G, R, b) == 1


def test_predicate_space_4gib_edge(wu):
    assert wu.wu_space(1, 1 << 32) == 1
    assert wu.wu_space(1, (1 << 32) + 256) == 0
    assert wu.wu_space(4, 1 << 30) == 1
    assert wu.wu_space(4, (1 << 30) + 256) == 0
    assert wu.wu_space(1, 4352) == 1


def test_replica_chain_is_the_division(wu):
    rng = np.random.default_rng(5)
    for nr in (1, 3, 5, 8):
        for G in (1, 64, 130, 192, 1 << 20, (1 << 32) // nr - 1):
            edge = [r * G + d for r in range(nr) for d in (0, 1, G - 1) if 0 <= r * G + d < nr * G]
            for i in edge + rng.integers(0, nr * G, 50).tolist():
                assert wu.wu_replica_chain(nr, i, G) == i // G, (nr, G, i)


def _mismatches(wu, S, mode, G, R, n_chunks, pc, depth, base=None):
    checked = ctypes.c_uint64(0)
    bad = wu.wu_addr_mismatches(S, mode, G, R, n_chunks, pc, depth, base.ctypes.data if base is not None else None,
                                ctypes.byref(checked))
    return bad, checked.value


@pytest.mark.parametrize("G", [64, 192, 320, 1024])
@pytest.mark.parametrize("S,R", [(3, 3), (5, 5), (5, 3), (8, 8), (1, 1)])
def test_addresses_loopback(wu, S, R, G):
    """Loopback spaces hold S * n positions in one chunk; depths 1 and GR_C."""
    pc = -(-(S * R * G) // TILE) * TILE
    for depth in (1, 2, 4):
        bad, checked = _mismatches(wu, S, RT_LOOPBACK, G, R, 1, pc, depth)
        assert bad == 0 and checked > R * G * 10, (bad, checked)


@pytest.mark.parametrize("n_chunks,pc", [(1, 4096), (3, 1024), (4, 768)])
def test_addresses_affine(wu, n_chunks, pc):
    """Affine bases over one and several chunks (a wave's run lies in one chunk:
    pc is a multiple of the tile), blocks at every 64-phase of a tile."""
    G, R, S = 192, 3, 3
    for shift in (0, 64, 128):
        base = _ring(G, R, S, shift)
        assert int(base[base != NOPOS].max()) + G <= n_chunks * pc
        bad, checked = _mismatches(wu, S, RT_AFFINE, G, R, n_chunks, pc, 2, base)
        assert bad == 0 and checked > 0, (bad, checked)


def test_addresses_at_the_4gib_edge(wu):
    """The last tiles of a hot region that ends just below 4 GiB (17 bytes per
    position at depth 1): the 32-bit offsets neither wrap nor leave the region."""
    pc = ((1 << 32) // 17) // TILE * TILE
    assert wu.wu_space(1, pc * 17) == 1
    G, R, S = 64, 3, 3
    k = iter(range(1, 100))
    base = _bases(R, S, lambda d, r, j: NOPOS if j == r else pc - 64 * next(k))
    bad, checked = _mismatches(wu, S, RT_AFFINE, G, R, 1, pc, 1, base)
    assert bad == 0 and checked > 0, (bad, checked)
    # a region past 4 GiB is refused, not addressed
    assert _mismatches(wu, S, RT_AFFINE, G, R, 1, pc + TILE, 1, base)[0] == -1


def test_unaligned_routes_are_refused_not_addressed(wu):
    assert _mismatches(wu, 3, RT_LOOPBACK, 130, 3, 1, 1280, 2)[0] == -1

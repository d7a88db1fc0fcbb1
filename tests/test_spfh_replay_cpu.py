"""spfh_replay (csrc/spfh_replay.hpp), the O(binades) form of an SPFH bin's float chain "v = 0; repeat hits: v = v + incr", against
the plain loop in numpy float32 -- bit for bit, through the host-only hook mm3d_debug_spfh_replay (no GPU).

The reference is taken incrementally: one pass of n additions gives the chain's value for every hits <= n."""
import ctypes as C

import numpy as np
import pytest


def replay(mm, incr, hits):
    incr = np.ascontiguousarray(incr, dtype=np.float32)
    hits = np.ascontiguousarray(hits, dtype=np.uint32)
    assert incr.shape == hits.shape
    out = np.empty(len(incr), dtype=np.float32)
    f = mm.lib().mm3d_debug_spfh_replay
    f.restype = None
    f(incr.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p), C.c_int(len(incr)), out.ctypes.data_as(C.c_void_p))
    return out


def chains(incr, n):
    """[len(incr), n + 1] float32: column h = the chain of h additions, every row's chain advanced by one numpy float32 addition
    per column."""
    incr = np.asarray(incr, dtype=np.float32)
    out = np.empty((len(incr), n + 1), dtype=np.float32)
    v = np.zeros(len(incr), dtype=np.float32)
    out[:, 0] = v
    with np.errstate(over="ignore", invalid="ignore"):
        for h in range(1, n + 1):
            v = v + incr
            out[:, h] = v
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_every_neighbour_count_and_every_hit_count(mm):
    """incr = float32(100) / float32(cnt - 1) for every cnt in 2 .. 4096, every hits in 0 .. cnt: about 8.4 M chains."""
    cnt = np.arange(2, 4097)
    incr = np.float32(100.0) / (cnt - 1).astype(np.float32)
    ref = chains(incr, 4096)
    rows, cols = np.nonzero(np.arange(4097)[None, :] <= cnt[:, None])
    got = replay(mm, incr[rows], cols)
    bad = np.flatnonzero(bits(got) != bits(ref[rows, cols]))
    assert len(bad) == 0, f"{len(bad)} of {len(rows)} chains differ; first: cnt {cnt[rows[bad[0]]]}, hits {cols[bad[0]]}: " \
                          f"{got[bad[0]]!r} vs {ref[rows[bad[0]], cols[bad[0]]]!r}"


HAND_PICKED = [
    1.5, 0.75, 3 * 2.0 ** -25,                  # the remainder is exactly half an ulp from the second binade on (odd mantissas)
    1.0 + 2.0 ** -23, 5 * 2.0 ** -10, 7.0, 2.0 ** -126 * 1.75, 0.1, 100.0, 1.0 / 3.0, 33.333332, 2.0 ** -24 * 11,
    1e-45, 3e-45, 2.0 ** -130, 2.0 ** -127 * 3,  # denormals (and the way out of them)
    1.0, 2.0 ** 20,                              # powers of two: never a rounding
    3e38 / 400, 3.4e38 / 65535, 2.0 ** 127, 3.0e38,   # overflow to inf within 65 535 additions
    float("inf"), 0.0,
]


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_hand_picked_increments(mm, sign):
    """Ties, denormals, overflow, inf, zero: every hits in 0 .. 65 535, both signs."""
    incr = (np.array(HAND_PICKED, dtype=np.float64) * sign).astype(np.float32)
    n = 65535
    ref = chains(incr, n)
    rows = np.repeat(np.arange(len(incr)), n + 1)
    cols = np.tile(np.arange(n + 1), len(incr))
    got = replay(mm, incr[rows], cols)
    bad = np.flatnonzero(bits(got) != bits(ref[rows, cols]))
    assert len(bad) == 0, f"{len(bad)} chains differ; first: incr {incr[rows[bad[0]]]!r}, hits {cols[bad[0]]}: " \
                          f"{got[bad[0]]!r} vs {ref[rows[bad[0]], cols[bad[0]]]!r}"
    # the set holds what it says: a tie, a saturating overflow, a denormal
    assert np.isinf(ref[incr == np.float32(sign * 3e38 / 400), n]).all()
    assert (np.abs(incr[np.abs(incr) > 0]).min() < np.float32(2.0 ** -126))


def test_a_chain_that_stands_still(mm):
    """x < U/2 after 2^24 additions of 1: 2^24 + 1 rounds back to 2^24 (a tie to even), and 0.75 stalls at 2^24 too -- far more
    additions than a bin can hold; checked against the closed form."""
    got = replay(mm, [1.0, 1.0, 1.0], [2 ** 24 - 1, 2 ** 24, 2 ** 25])
    assert list(got) == [2.0 ** 24 - 1, 2.0 ** 24, 2.0 ** 24]


def test_nan_increment(mm):
    incr = np.array([np.nan], dtype=np.float32)
    assert replay(mm, incr, [0])[0] == 0.0
    assert np.isnan(replay(mm, incr, [1])[0]) and np.isnan(replay(mm, incr, [7])[0])

"""The wave-wide reductions and scans of csrc/device_util.hpp run on the DPP / permlane network; until they did, each was a
loop of shuffles through the LDS pipe.  The test hook mm3d_debug_wave_primitives (csrc/libm_debug.hip, which keeps the
shuffle loops' text) runs both forms on the same input, 4 blocks x 256 threads = 16 waves, and returns what every lane holds.
Bit-equal in every lane a caller reads: lane 0 for the sums (the kernels' double and float sums must not move by a bit: the
new form adds the same pairs in the same order), every lane for minima, maxima and the scan.  The inputs are chosen so that
another pairing, a lost lane or a wrong row boundary shows: sums of mixed signs with exponents spread over 2^+-40 (also replayed
in numpy, pair by pair), float minima over +-0, +-inf and NaN, integer extremes, scan counts of 0 and of more than 2^16."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 4 * 256
WAVES = N // 64


def _bits(a):
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _shuffle_down_tree(x):
    """v += shuffle_down(v, o) for o = 32 .. 1 as lane 0 sees it, in the input's own float format."""
    v = x.reshape(WAVES, 64).copy()
    for o in (32, 16, 8, 4, 2, 1):
        v[:, :o] = v[:, :o] + v[:, o:2 * o]
    return v[:, 0]


def _spread(rng, dtype):
    sign = rng.choice([-1.0, 1.0], N)
    return (sign * rng.uniform(1.0, 2.0, N) * np.exp2(rng.integers(-40, 41, N))).astype(dtype)


@pytest.mark.parametrize("op,dtype", [(0, np.float64), (1, np.float32)])
def test_float_sums_keep_their_pairs_and_order(ctx, op, dtype):
    rng = np.random.default_rng(11 + op)
    x = _spread(rng, dtype)
    x[64:128] = np.abs(x[64:128])                       # one wave of one sign
    x[128:192] = dtype(0.0)
    x[128 + 37] = dtype(-3.5)                           # one wave with a single term, in the last row
    # one wave that tells pairings apart by construction: 1 and 63 half-ulps of 1.  Added in lane order every half-ulp is a
    # tie that rounds back to 1 (ties to even), so that sum is 1 exactly; the tree first adds half-ulps to each other, which is
    # exact, and 1 meets sums of two and more of them, so its result lies above 1
    half_ulp = dtype(np.finfo(dtype).eps / 2)
    x[192:256] = half_ulp
    x[192] = dtype(1.0)
    new, old = ctx.debugWavePrimitives(op, x)
    lane0_new, lane0_old = _bits(new)[::64], _bits(old)[::64]
    assert np.array_equal(lane0_old, _bits(_shuffle_down_tree(x))), "the predecessor is not the tree this test replays"
    assert np.array_equal(lane0_new, lane0_old)
    seq = dtype(0.0)
    for v in x[192:256]:
        seq = dtype(seq + v)
    assert seq == dtype(1.0) and new[192] > dtype(1.0)


def _float_extremes(rng):
    x = rng.normal(0.0, 100.0, N).astype(np.float32)
    w = x.reshape(WAVES, 64)
    w[0] = 0.0; w[0, ::3] = -0.0                        # zeros of both signs only
    w[1] = 0.0; w[1, 63] = -0.0                         # a single -0, in the last lane
    w[2] = -0.0; w[2, 16] = 0.0                         # a single +0, first lane of the second row
    w[3, ::2] = np.nan                                  # NaN against numbers
    w[4] = np.nan                                       # NaN only
    w[5] = np.nan; w[5, 47] = 2.5                       # one number among NaN
    w[6, 5] = np.inf; w[6, 33] = -np.inf
    w[7] = np.inf; w[8] = -np.inf
    w[9] = np.inf; w[9, 31] = -0.0; w[9, 32] = 0.0      # the two zeros on either side of the half-wave boundary
    w[10, 15] = -1e30; w[10, 16] = 1e30                 # the extremes on either side of a row boundary
    w[11, 0] = 1e30; w[11, 63] = -1e30
    return x


@pytest.mark.parametrize("op", [5, 6])
def test_float_min_max_over_zeros_infinities_and_nan(ctx, op):
    x = _float_extremes(np.random.default_rng(5))
    new, old = ctx.debugWavePrimitives(op, x)
    assert np.array_equal(_bits(new), _bits(old))       # every lane
    w = x.reshape(WAVES, 64)
    ref = (np.fmin if op == 5 else np.fmax).reduce(w, axis=1)
    got = new.reshape(WAVES, 64)
    assert np.array_equal(np.isnan(got[:, 0]), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.array_equal(got[ok, 0], ref[ok])
    # -0 is below +0
    assert np.signbit(got[0, 0]) == (op == 5) and np.signbit(got[1, 0]) == (op == 5) and np.signbit(got[2, 0]) == (op == 5)
    if op == 5:
        assert np.signbit(got[9, 0])                    # ... across the half-wave boundary too


def _int_extremes(rng):
    x = rng.integers(-1 << 31, 1 << 31, N, dtype=np.int64).astype(np.int32)
    w = x.reshape(WAVES, 64)
    w[0] = 0
    w[1] = np.iinfo(np.int32).max; w[1, 63] = np.iinfo(np.int32).min
    w[2] = np.iinfo(np.int32).min; w[2, 0] = np.iinfo(np.int32).max
    w[3] = 7; w[3, 16] = np.iinfo(np.int32).min; w[3, 47] = np.iinfo(np.int32).max
    w[4] = -1
    return x


@pytest.mark.parametrize("op", [3, 4])
def test_int_min_max(ctx, op):
    x = _int_extremes(np.random.default_rng(8))
    new, old = ctx.debugWavePrimitives(op, x)
    assert np.array_equal(new, old)                     # every lane
    ref = (np.min if op == 3 else np.max)(x.reshape(WAVES, 64), axis=1)
    assert np.array_equal(new.reshape(WAVES, 64), np.repeat(ref[:, None], 64, axis=1))


def test_int_sum(ctx):
    x = _int_extremes(np.random.default_rng(9))
    new, old = ctx.debugWavePrimitives(2, x)
    assert np.array_equal(new[::64], old[::64])         # lane 0
    ref = (x.reshape(WAVES, 64).astype(np.int64).sum(axis=1) & 0xffffffff).astype(np.uint32).view(np.int32)   # wraps like the adder
    assert np.array_equal(new[::64], ref)


def test_inclusive_scan_with_empty_and_large_counts(ctx):
    rng = np.random.default_rng(10)
    x = rng.integers(0, 100, N).astype(np.int32)
    w = x.reshape(WAVES, 64)
    w[0] = 0
    w[1] = 70000                                        # more than 2^16 in every lane
    w[2] = 0; w[2, 15] = 1 << 20; w[2, 16] = 3; w[2, 32] = 1 << 17; w[2, 63] = 5
    w[3] = rng.choice([0, 65537, 1 << 18], 64)
    w[4] = 0; w[4, 0] = 1
    w[5] = 0; w[5, 63] = 1
    new, old = ctx.debugWavePrimitives(7, x)
    assert np.array_equal(new, old)                     # every lane
    assert np.array_equal(new.reshape(WAVES, 64), np.cumsum(w, axis=1, dtype=np.int64).astype(np.int32))


def test_u64_key_min(ctx):
    rng = np.random.default_rng(12)
    x = rng.integers(0, 1 << 63, N, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, N).astype(np.uint64)
    w = x.reshape(WAVES, 64)
    w[0] = np.uint64(0xffffffffffffffff)                # "no key" everywhere
    w[1] = np.uint64(0xffffffffffffffff); w[1, 63] = np.uint64(5)
    w[2] = (np.uint64(0x3f800000) << np.uint64(32)) | np.arange(64, dtype=np.uint64)[::-1]   # equal high words: the low word decides
    w[3] = (np.arange(64, dtype=np.uint64) << np.uint64(32)) | np.uint64(0xffffffff)
    w[3, 40] = np.uint64(0xfffffffe)                    # high word 0, like lane 0's key, and a lower low word
    new, old = ctx.debugWavePrimitives(8, x)
    assert np.array_equal(new, old)                     # every lane
    assert np.array_equal(new.reshape(WAVES, 64), np.repeat(w.min(axis=1)[:, None], 64, axis=1))

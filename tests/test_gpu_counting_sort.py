"""The counting sort behind the voxel filter (csrc/grid.hip) through the test hook mm3d_debug_counting_sort, against
numpy.argsort(kind="stable"): the sorted keys and their indices entry for entry.  Bin = key / ceil(key_range / 2^22); a bin of more
than kCountSortBinMax = 1024 keys makes the sort give up and write nothing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF
BIN_MAX = 1024


def check(ctx, keys, key_range, no_invalid_keys=False):
    keys = np.asarray(keys, dtype=np.uint32)
    ko, io, too_long = ctx.debugCountingSort(keys, key_range, no_invalid_keys)
    assert not too_long
    valid = np.flatnonzero(keys != INVALID)
    ref_idx = valid[np.argsort(keys[valid], kind="stable")]
    m = len(valid)
    assert np.array_equal(ko[:m], keys[ref_idx]), "sorted keys differ"
    bad = np.flatnonzero(io[:m] != ref_idx)
    assert len(bad) == 0, "index differs at %d of %d places, first %d: device %d, numpy %d" % (len(bad), m, bad[0], io[bad[0]], ref_idx[bad[0]])
    assert (ko[m:] == INVALID).all(), "entries behind the valid keys must read 0xFFFFFFFF"


def test_one_key(ctx):
    check(ctx, [5], 10)
    check(ctx, [0], 1, no_invalid_keys=True)


def test_bin_at_its_limit(ctx):
    """1 024 equal keys fill a bin to kCountSortBinMax and are placed by index; one more and the sort reports too_long and
    leaves both outputs untouched"""
    rng = np.random.default_rng(1)
    others = rng.integers(0, 5000, 700).astype(np.uint32)
    others[others == 777] = 778
    for no_invalid in (False, True):
        keys = np.concatenate([np.full(BIN_MAX, 777, dtype=np.uint32), others])
        check(ctx, keys[rng.permutation(len(keys))], 5000, no_invalid)
        keys = np.concatenate([np.full(BIN_MAX + 1, 777, dtype=np.uint32), others])
        ko, io, too_long = ctx.debugCountingSort(keys[rng.permutation(len(keys))], 5000, no_invalid)
        assert too_long
        assert (ko == INVALID).all() and (io == INVALID).all(), "a sort that gave up must write nothing"


def test_invalid_keys_stay_out(ctx):
    rng = np.random.default_rng(2)
    keys = rng.integers(0, 200000, 3000).astype(np.uint32)            # several blocks, bins mostly of one key
    clean = keys.copy()
    keys[rng.choice(len(keys), 400, replace=False)] = INVALID
    check(ctx, keys, 200000)
    check(ctx, clean, 200000, no_invalid_keys=False)
    check(ctx, clean, 200000, no_invalid_keys=True)
    check(ctx, np.full(70, INVALID, dtype=np.uint32), 9)              # nothing valid at all


def test_neighbouring_keys_share_a_bin(ctx):
    """key_range = 2^24: the divisor is 4, so keys 4 b .. 4 b + 3 meet in bin b -- equal keys (ordered by index) among unequal
    ones (ordered by key)"""
    rng = np.random.default_rng(3)
    key_range = 1 << 24
    dense = rng.integers(1000, 1064, 900).astype(np.uint32)           # 16 bins of four keys, ~56 members each, every key many times
    wide = rng.integers(0, key_range, 1500).astype(np.uint32)
    edge = np.array([0, 1, 2, 3, 3, 0, key_range - 1, key_range - 4, key_range - 1], dtype=np.uint32)
    keys = np.concatenate([dense, wide, edge])
    keys = keys[rng.permutation(len(keys))]
    bins = keys // 4
    shared = [b for b in np.unique(bins) if len(np.unique(keys[bins == b])) > 1 and len(keys[bins == b]) > len(np.unique(keys[bins == b]))]
    assert len(shared) >= 16, "the input must hold bins with both equal and unequal keys"
    check(ctx, keys, key_range)
    with_invalid = keys.copy()
    with_invalid[::17] = INVALID
    check(ctx, with_invalid, key_range)

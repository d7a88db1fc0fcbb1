"""The inputs of tests/test_gpu_nn_search.py, checked without a GPU (tests/nn_cases.py).

Every case is aimed at one mechanism of the ICP / score nearest-neighbour search, and only tests it if its points actually get
there: each case counts, from the brute-force reference and the grid geometry alone, how many of its points take the branch
it is for, and fails below the minimum.  The float32 brute force itself is checked against a float64 one, and the one-iteration
ICP comparison is shown to be able to see ONE wrong correspondence."""
import numpy as np
import pytest

import nn_cases as nc
from nn_cases import ICP_STEP_TOLERANCE


@pytest.fixture(scope="module")
def cases(po, synth):
    return nc.all_cases(po, synth)


def test_every_case_reaches_what_it_is_aimed_at(cases):
    missed = []
    for c in cases:
        cov = c.check_coverage()
        print(c.name, "(%d source, %d target points; %s)" % (len(c.src), len(c.tgt), c.aimed_at), {k: v[0] for k, v in cov.items()})
        missed += ["%s: %s = %s, at least %s wanted" % (c.name, k, got, least) for k, (got, least) in cov.items() if not got >= least]
    assert not missed, "\n".join(missed)
    names = [c.name for c in cases]
    assert len(set(names)) == len(names) and len(names) >= 30


def test_the_large_split1_case_reaches_what_it_is_aimed_at(synth):
    c = nc.split1_case(synth)
    cov = c.check_coverage()
    print(c.name, {k: v[0] for k, v in cov.items()})
    assert all(got >= least for got, least in cov.values()), cov


def test_max_d2_is_the_largest_float_in_range():
    for conv, v in ((0, 0.3), (0, 0.5), (0, 1.0), (1, 0.1), (1, 0.3), (1, 0.25), (1, 1.0), (0, 0.003)):
        lim = v * v if conv == 0 else v
        m = nc.max_d2_of(conv, v)
        assert float(m) <= lim < float(np.nextafter(m, np.float32(np.inf))), (conv, v, m)
    # 0.1 and 0.3 are no floats, and the float nearest to either lies ABOVE it: the bound is the float below that one
    assert nc.max_d2_of(1, 0.1) == np.nextafter(np.float32(0.1), np.float32(0)) and nc.max_d2_of(1, 0.3) == np.nextafter(np.float32(0.3), np.float32(0))
    assert nc.max_d2_of(1, 0.25) == np.float32(0.25) and nc.max_d2_of(0, 0.5) == np.float32(0.25)


def test_float32_brute_force_against_float64(cases):
    """The same index wherever the float64 gap between the two nearest exceeds what float32 rounding can move their d2 by; d2
    itself within that rounding.  (Sources beyond 3 000 are sampled at a fixed stride: the float64 pass is the slow one.)"""
    checked = decided = 0
    for c in cases:
        if len(c.src) == 0 or len(c.tgt) == 0:
            continue
        nn = c.nn()
        sel = np.flatnonzero(np.isfinite(c.src).all(axis=1))
        sel = sel[::max(1, len(sel) // 3000)]
        i64, d64, s64, scale = nc.brute_nn64(c.src[sel], c.tgt, c.T)
        err1, err2 = nc.d2_rounding(d64, scale), nc.d2_rounding(s64, scale) if len(c.tgt) > 1 else 0.0
        assert (np.abs(nn["d2"][sel].astype(np.float64) - d64) <= err1).all(), c.name
        clear = (s64 - d64) > (err1 + err2)
        assert (nn["idx"][sel][clear] == i64[clear]).all(), c.name
        checked += len(sel)
        decided += int(clear.sum())
    print("float64 check: %d points, %d with a gap that rounding cannot close" % (checked, decided))
    assert decided >= 0.5 * checked


def test_reference_takes_the_lower_index_on_a_tie_and_the_bound_as_in_range():
    tgt = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 1, 0]], np.float32)
    nn = nc.brute_nn(np.zeros((1, 3), np.float32), tgt[::-1].copy(), np.eye(4), want_ties=True, want_second=True)
    assert nn["idx"][0] == 0 and nn["ties"][0] == 4 and nn["d2"][0] == 1.0 and nn["second"][0] == 1
    idx, d2 = nc.in_range(nn, 0, 1.0)
    assert idx[0] == 0 and d2[0] == 1.0
    idx, d2 = nc.in_range(nn, 1, float(np.nextafter(np.float32(1.0), np.float32(0))))
    assert idx[0] == -1 and np.isinf(d2[0])


def test_one_swapped_correspondence_is_visible_to_the_icp_clause(cases):
    """Clause 4 of the GPU test compares one ICP iteration with a float64 Umeyama over the reference correspondences, within
    ICP_STEP_TOLERANCE.  Here: ONE correspondence swapped for that point's second-nearest target moves the float64 result by
    more than the tolerance, for every case the clause keeps."""
    kept = nc.icp_clause_cases(cases)
    print("cases of the ICP clause:", [c.name for c, _ in kept])
    assert len(kept) >= 8
    for c, max_corr in kept:
        ref = nc.icp_step64(c, max_corr)
        shifted = nc.icp_step64(c, max_corr, swap=nc.swap_candidate(c, max_corr))
        shift = np.linalg.norm(shifted - ref)
        print("%-28s one swap moves the transform by %.3g (tolerance %.3g)" % (c.name, shift, ICP_STEP_TOLERANCE))
        assert shift > ICP_STEP_TOLERANCE, (c.name, shift)

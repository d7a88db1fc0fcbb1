"""The ICP / score nearest-neighbour search (csrc/nn_search_body.hpp) point by point: the test hook mm3d_debug_nn_search against
a float32 brute force that rounds every step as the device does (tests/nn_cases.py), on inputs aimed at the search's bounds --
ties, the range limit to the ulp, cell faces, the distance transform's rings, the corner filter, queries outside the grid,
mixed rings in one wave, dense cells, wide boxes, degenerate clouds, the cell regimes, a real transform.  No tolerance: index
and d2 bits.  The hook is its own compile of the shared body, so three more tests tie the production kernels to it: the score
is the sum of the probed distances to the last bits a double sum allows, one ICP iteration is the Umeyama of the reference
correspondences, and a source large enough for the library's own SPLIT 1 launch scores like the brute force.

tests/test_nn_cases_cpu.py checks on the CPU that each input reaches the branch it is aimed at."""
import time

import numpy as np
import pytest

import nn_cases as nc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(po, synth):
    return nc.all_cases(po, synth)


@pytest.fixture(scope="module")
def probed(ctx, cases):
    """{(case name, range index, split): (idx, d2, info)} over every case, every range and both splits, and the device clouds."""
    out, clouds, t_probe = {}, {}, 0.0
    for c in cases:
        clouds[c.name] = (ctx.cloud(nc.points(c.src)), ctx.cloud(nc.points(c.tgt)))
        for k, (conv, value) in enumerate(c.ranges):
            for split in (1, 4):
                t0 = time.perf_counter()
                out[c.name, k, split] = ctx.debugNnSearch(*clouds[c.name], c.T, value, conv, split)
                t_probe += time.perf_counter() - t0
    print("probe: %d searches in %.2f s (the first of a cloud builds its grid and Hilbert order)" % (len(out), t_probe))
    return out, clouds


def score_bound(count):
    """A double sum of `count` non-negative terms in any order, then one division: (count + 2) 2^-53 relative at worst."""
    return (count + 2) * 2.0 ** -53


def test_index_and_d2_bits_of_every_point(cases, probed):
    """Clauses 1 and 2: idx and the bits of d2 equal the brute force's everywhere (-1 / +inf included), for SPLIT 1 and SPLIT 4,
    which therefore agree with each other; and the grid the library derived is the one the cases' coverage was counted on."""
    out, _ = probed
    wrong, points = [], 0
    for c in cases:
        nn = c.nn()
        for k, (conv, value) in enumerate(c.ranges):
            ref_idx, ref_d2 = nc.in_range(nn, conv, value)
            for split in (1, 4):
                idx, d2, info = out[c.name, k, split]
                points += len(idx)
                bad = np.flatnonzero((idx != ref_idx) | (d2.view(np.uint32) != ref_d2.view(np.uint32)))
                if len(bad):
                    i = int(bad[0])
                    wrong.append("%s range %s split %d: %d of %d points differ; first: point %d at %s, device (%d, %r), reference (%d, %r)"
                                 % (c.name, (conv, value), split, len(bad), len(idx), i, nn["p"][i], idx[i], d2[i], ref_idx[i], ref_d2[i]))
                if len(c.src) and len(c.tgt):
                    g = nc.geometry(c.tgt, conv, value, dense_limit=0)
                    got = (info["cell"], info["dims"], info["max_ring"], info["max_d2"], info["rmax"], tuple(info["origin"]))
                    want = (g["cell"], g["dims"], g["max_ring"], g["max_d2"], g["rmax"], tuple(g["origin"]))
                    if got != want:
                        wrong.append("%s range %s: the library's grid %s is not the restated one %s" % (c.name, (conv, value), got, want))
                    if info["n_items"] != len(nc.hilbert_items(c.src)[1]):
                        wrong.append("%s: %d work items, %d restated" % (c.name, info["n_items"], len(nc.hilbert_items(c.src)[1])))
            a, b = out[c.name, k, 1], out[c.name, k, 4]
            if not (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))):
                wrong.append("%s range %s: SPLIT 1 and SPLIT 4 differ" % (c.name, (conv, value)))
    print("%d points compared over %d cases" % (points, len(cases)))
    assert not wrong, "\n".join(wrong)


def test_transform_score_is_the_sum_of_the_probed_distances(ctx, cases, probed):
    """Clause 3: score_nn_reduce (MODE 1, the split the library picks) against the probe.  transformScore equals
    fsum(d2 in range) / count within (count + 2) 2^-53 relative, and DBL_MAX exactly where nothing is in range."""
    out, clouds = probed
    wrong, worst = [], 0.0
    for c in cases:
        for k, (conv, value) in enumerate(c.ranges):
            if conv != 1:
                continue
            want, count = nc.score_of(out[c.name, k, 4][1])
            got = ctx.transformScore(*clouds[c.name], c.T, value)
            if count == 0:
                ok = got == nc.DBL_MAX
            else:
                rel = abs(got - want) / want if want > 0 else abs(got - want)
                worst = max(worst, rel / score_bound(count))
                ok = rel <= score_bound(count)
            if not ok:
                wrong.append("%s max_distance %r: score %r, sum of the probed distances %r over %d points" % (c.name, value, got, want, count))
    print("largest |score - fsum / count| / ((count + 2) 2^-53): %.3f" % worst)
    assert not wrong, "\n".join(wrong)


def test_one_icp_iteration_is_the_umeyama_of_the_reference_correspondences(ctx, cases, probed):
    """Clause 4: icp_corr_reduce + icp_finalize against the reference.  estimateTransformICP with max_iterations = 1 from the
    case's transform, against a float64 Umeyama (numpy SVD) over the brute force's correspondences composed with the guess.

    Cases: nn_cases.icp_clause_cases -- at most 2 000 source points, everything within 30 m of the origin, an ICP range, at least
    ten correspondences: lattice_ties, wide_items, 63 / 64 / 65_source_points, range_3mm_cell_clamped, range_50m_few_cells and
    lattice_ties_moved.  Left out of THIS clause only: planar_target, collinear_target and one_target_point (a flat moment matrix:
    the rotation is then the SVD's rank handling, not the search), non_finite_source_points, one_source_point and the empty
    clouds (fewer than three correspondences), the cases of more than 2 000 source points (the parity poses, the faces,
    sparse, outside, patch, dense-cell and grown-cell cases and their moved copies) and the boundary cases (pairs laid out over
    1.2 km).

    MEASURED on an MI355X (Frobenius norm of device - reference): 4.1e-8 lattice_ties, 2.1e-7 wide_items, 5.6e-8 / 4.3e-8 / 8.4e-8
    for 63 / 64 / 65 points, 1.1e-9 range_3mm, 1.5e-7 range_50m, 5.58e-7 lattice_ties_moved (a 25 m translation: one float ulp of
    it is 1.9e-6).  Tolerance nn_cases.ICP_STEP_TOLERANCE = 2.24e-6 = 4 x the largest: the output is a float matrix and the margin
    only has to cover its rounding.  tests/test_nn_cases_cpu.py shows that ONE swapped correspondence moves the float64 result
    by 3.2e-4 .. 1.3e-2 in these cases, at least 140 x the tolerance."""
    _, clouds = probed
    kept = nc.icp_clause_cases(cases)
    assert len(kept) >= 8
    worst, wrong = 0.0, []
    for c, max_corr in kept:
        ref = nc.icp_step64(c, max_corr)
        got = ctx.estimateTransformICP(*clouds[c.name], c.T, max_corr, 0.5, 1, 0.0)
        dist = float(np.linalg.norm(got.astype(np.float64) - ref))
        print("%-28s %5d source points: |device - float64 Umeyama| = %.3g" % (c.name, len(c.src), dist))
        worst = max(worst, dist)
        if not dist <= nc.ICP_STEP_TOLERANCE:
            wrong.append((c.name, dist))
    print("largest distance %.3g, tolerance %.3g" % (worst, nc.ICP_STEP_TOLERANCE))
    assert not wrong, wrong


def test_the_librarys_own_split1_launch_scores_like_the_brute_force(ctx, synth):
    """Clause 5: a source of more than 4096 work items (nn_split_items then picks SPLIT 1) against a 4 000 point target:
    transformScore against fsum(brute-force d2 in range) / count within the bound of clause 3."""
    c = nc.split1_case(synth)
    src, tgt = ctx.cloud(nc.points(c.src)), ctx.cloud(nc.points(c.tgt))
    conv, value = c.ranges[0]
    idx, d2, info = ctx.debugNnSearch(src, tgt, c.T, value, conv, 1)
    assert len(c.src) >= 300000 and len(c.tgt) <= 4000 and info["n_items"] > 4096, info
    ref_idx, ref_d2 = nc.in_range(c.nn(), conv, value)
    bad = np.flatnonzero((idx != ref_idx) | (d2.view(np.uint32) != ref_d2.view(np.uint32)))
    assert len(bad) == 0, (len(bad), bad[:5])
    want, count = nc.score_of(ref_d2)
    got = ctx.transformScore(src, tgt, c.T, value)
    print("score %r, reference %r over %d points: %.3f of the bound" % (got, want, count, abs(got - want) / want / score_bound(count)))
    assert count > 30000 and abs(got - want) <= score_bound(count) * want

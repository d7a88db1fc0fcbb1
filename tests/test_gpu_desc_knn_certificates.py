"""The descriptor k-NN's certificate where it matters (tests/knn_cases.py, checked on the CPU by tests/test_knn_cases_cpu.py):
exact tie blocks larger than a query's candidate set, near-tie shells the matrix-core expansion misranks, the same at
magnitudes from 2^-32 to 2^50 and on a common offset of 4096, and benign rows at every size edge of the dispatch -- on each route
of csrc/desc_knn.hip, which every test asserts it took (mm3d_debug_knn_paths).

The criterion is the project's: indices equal and distance words bit-equal to the oracle's brute force, ties to the lower index,
-1 / +inf tails where there are fewer targets than k.  No tolerance anywhere.  For the tie blocks the fallback count is asserted
too: a target at exactly the k-th exact distance that is no candidate (pigeonhole: the block is larger than the candidate set)
makes every certified row a false certificate, whatever the index order happens to give.  For the other families the count is
printed, not asserted (at 2^-32 the absolute terms of the bound send every row to the exact search: sound)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import knn_cases as kc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_IDS = sorted(kc.ROUTES)


def _direct(ctx, mm, po, name, A, B, k, bit):
    """One mm3d_debug_desc_knn call (targets built per call) against the oracle; returns the fallback count."""
    idx, d2, fb, paths = kc.gpu_desc_knn(ctx, mm.lib(), A, B, k)
    ref_idx, ref_d2 = po.desc_knn(A, B, k)
    bad = kc.mismatching_rows(idx, d2, ref_idx, ref_d2)
    print(f"{name}: {fb} of {len(A)} rows took the exact fallback, route mask {paths}")
    assert paths == bit, (name, paths, bit)
    assert len(bad) == 0, (name, bad[:8].tolist(), idx[bad[:2]].tolist(), ref_idx[bad[:2]].tolist())
    return fb


def _matched(ctx, mm, po, name, A, B, k, bit):
    """The same rows as descriptor sets through findFeatureCorrespondences: both directions, B -> A against len(A) targets."""
    dim = A.shape[1]
    if dim not in kc.DESCRIPTOR_OF:
        return
    L = mm.lib()
    kc.bind_debug(L)
    da, db = ctx.descriptors(A, kc.DESCRIPTOR_OF[dim]), ctx.descriptors(B, kc.DESCRIPTOR_OF[dim])
    L.mm3d_set_debug(ctx._h, 1)
    try:
        got = ctx.findFeatureCorrespondences(da, db, k)
        paths = mm.knn_paths(ctx)
    finally:
        L.mm3d_set_debug(ctx._h, 0)
    ref = po.find_correspondences(A, B, k)
    back = bit if bit in (kc.PATH_LIST_WIDE, kc.PATH_WIDE_BF16) else kc.PATH_LIST           # 80 targets: never the filter
    assert paths == bit | back, (name, paths)
    assert np.array_equal(got["index_query"], ref["index_query"]), name
    assert np.array_equal(got["index_match"], ref["index_match"]), name
    assert np.array_equal(got["distance"].view(np.uint32), ref["distance"].view(np.uint32)), name


@pytest.mark.parametrize("route", ROUTE_IDS)
def test_tie_blocks(ctx, mm, po, route):
    bit = kc.ROUTES[route][3]
    for name, make in kc.family_cases("T", route):
        A, B, k, adv, _ = make()
        fb = _direct(ctx, mm, po, name, A, B, k, bit)
        assert fb >= len(adv), (name, fb)              # a certified row here is a false certificate
        _matched(ctx, mm, po, name, A, B, k, bit)


@pytest.mark.parametrize("route", ROUTE_IDS)
def test_near_tie_shells(ctx, mm, po, route):
    bit = kc.ROUTES[route][3]
    for name, make in kc.family_cases("S", route):
        A, B, k, adv, _ = make()
        _direct(ctx, mm, po, name, A, B, k, bit)
        _matched(ctx, mm, po, name, A, B, k, bit)


@pytest.mark.parametrize("route", ROUTE_IDS)
def test_magnitudes(ctx, mm, po, route):
    """s = +50 on a list route (nb = 1000: 24 padding rows in the last target tile) is the case in which real squared distances
    exceed 1e30: padding targets with that finite distance came ahead of real rows, filled the lists of the wave that owns the
    last tile and were then dropped, so full lists passed for empty ones and 37 to 53 of the 80 rows came out wrong.  Padding
    targets are at +inf now and enter no list; the fallback counts at 2^50 are those at 2^0."""
    bit = kc.ROUTES[route][3]
    for name, make in kc.family_cases("M", route):
        A, B, k, adv, _ = make()
        _direct(ctx, mm, po, name, A, B, k, bit)


@pytest.mark.parametrize("route", ROUTE_IDS)
def test_common_offset(ctx, mm, po, route):
    bit = kc.ROUTES[route][3]
    for name, make in kc.family_cases("O", route):
        A, B, k, adv, _ = make()
        _direct(ctx, mm, po, name, A, B, k, bit)


@pytest.mark.parametrize("dim,na,nb,k,bit", kc.EDGES, ids=lambda v: str(v))
def test_size_edges(ctx, mm, po, dim, na, nb, k, bit):
    A, B, k, _, note = kc.edge(dim, na, nb, k)
    _direct(ctx, mm, po, note, A, B, k, bit)


@pytest.mark.parametrize("which", sorted(kc.CHILD_RUNS))
def test_selectors_read_from_the_environment(which):
    """MM3D_KNN_WIDE_BF16=0 (the f32 wide selector) and MM3D_KNN_NO_FILTER=1 (lists for every shape) are read once per process:
    one fresh child each, T and S, zero mismatching rows and the route the switch selects."""
    env_add, routes, bit = kc.CHILD_RUNS[which]
    env = dict(os.environ)
    env.update(env_add)
    out = subprocess.run([sys.executable, os.path.join("tests", "knn_cases.py"), "--run", which], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    print(res)
    assert res["run"] == which and res["paths"] == bit, res
    assert len(res["cases"]) == 5 * len(routes)
    for case in res["cases"]:
        assert case["mismatches"] == 0, case

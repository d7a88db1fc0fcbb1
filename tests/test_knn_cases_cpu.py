"""The inputs of tests/test_gpu_desc_knn_certificates.py, checked without a GPU (tests/knn_cases.py): oracle and numpy only.

A case the expansion ranks correctly anyway is no test of the certificate.  So: every T case is counted (targets at exactly the
k-th oracle distance: at least m, more than a query has candidates), every S case is measured (the float64 gap between the k-th
and (k+1)-th distance, and the float32-emulated expansion's top-k against the oracle's: it must differ on at least 90 % of the
adversarial rows at every width), M's scaling property is shown on the oracle for every scale used, and the route record the
GPU tests rely on is declared and exported."""
import os
import re

import numpy as np
import pytest

import knn_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_IDS = sorted(kc.ROUTES)


def _float64_sorted_d2(A, B, rows):
    a, b = A[rows].astype(np.float64), B.astype(np.float64)
    return np.sort(((a[:, None, :] - b[None]) ** 2).sum(axis=2), axis=1)


@pytest.mark.parametrize("route", ROUTE_IDS)
def test_tie_blocks_hold_their_ties(po, route):
    dim, nb, m, _ = kc.ROUTES[route]
    for name, make in kc.family_cases("T", route):
        A, B, k, adv, note = make()
        assert A.dtype == B.dtype == np.float32 and A.shape == (kc.NA, dim) and B.shape == (nb, dim) and len(adv) == kc.N_ADV
        whole = (A == np.rint(A)).all() and ((B == np.rint(B)) | (dim == 2)).all()
        assert whole and (2 * B == np.rint(2 * B)).all(), name                     # integer rows (width 2: and the halves)
        idx, d2 = po.desc_knn(A, B, k)
        exact = ((A[adv].astype(np.float64)[:, None, :] - B.astype(np.float64)[None]) ** 2).sum(axis=2)
        tied = (exact.astype(np.float32) == d2[adv, k - 1][:, None]).sum(axis=1)    # (integers and quarters: exact in both)
        print(note, "targets at the k-th distance:", tied.tolist())
        assert (tied >= m).all(), (name, tied)
        assert (d2[adv, k - 1] == (1.0 if dim == 2 else 2.0)).all(), name
        # the index decides: the k-th neighbour is the lowest-indexed members of the block
        for a, row in zip(adv, exact):
            block = np.flatnonzero(row.astype(np.float32) == d2[a, k - 1])
            nearer = int((row.astype(np.float32) < d2[a, k - 1]).sum())
            assert np.array_equal(idx[a, nearer:], block[:k - nearer]), name


@pytest.mark.parametrize("route", ROUTE_IDS)
def test_near_tie_shells_are_misranked_by_the_expansion(po, route):
    dim, nb, m, _ = kc.ROUTES[route]
    for (name, make), g in zip(kc.family_cases("S", route), kc.GAPS):
        A, B, k, adv, note = make()
        assert A.dtype == B.dtype == np.float32 and A.shape == (kc.NA, dim) and B.shape == (nb, dim)
        d = _float64_sorted_d2(A, B, adv)
        gap = (d[:, k] - d[:, k - 1]) / d[:, k - 1]
        idx, _ = po.desc_knn(A, B, k)
        emu = kc.emulated_topk(A[adv], B, k)
        differ = sum(not np.array_equal(np.sort(e), np.sort(idx[a])) for e, a in zip(emu, adv))
        print(note, "relative gap k / k+1: %.3g" % gap.max(), "emulated top-k differs on", differ, "of", len(adv))
        assert (gap >= 0).all() and gap.max() <= 2 * g + 1e-6, (name, gap)
        assert differ >= 0.9 * len(adv), (name, differ)


@pytest.mark.parametrize("route", ROUTE_IDS)
def test_magnitudes_scale_exactly_on_the_oracle(po, route):
    dim, nb, m, _ = kc.ROUTES[route]
    cases = dict(zip(kc.SCALES, kc.family_cases("M", route)))
    A0, B0, k, adv0, _ = cases[0][1]()
    idx0, d0 = po.desc_knn(A0, B0, k)
    for s, (name, make) in cases.items():
        A, B, k_s, adv, note = make()
        assert k_s == k and np.array_equal(adv, adv0)
        assert np.isfinite(A).all() and np.isfinite(B).all()
        assert np.array_equal(A.astype(np.float64), A0.astype(np.float64) * 2.0 ** s), name          # nothing rounded, nothing lost
        idx, d = po.desc_knn(A, B, k)
        assert np.array_equal(idx, idx0), name
        assert np.isfinite(d).all() and (d[d0 > 0] > 0).all(), name
        assert np.array_equal(d.astype(np.float64), d0.astype(np.float64) * 4.0 ** s), name
    # the case that decides about the padding targets: real squared distances beyond 1e30 (a padding row's distance has to lie
    # behind them: +inf), a list path, and a last target tile that is partly padding
    if kc.ROUTES[route][3] != kc.PATH_FILTER:
        _, d50 = po.desc_knn(*cases[50][1]()[:3])
        assert nb % 32 != 0 and 64 <= nb <= 2016 and d50[adv0].min() > 1e30


def test_offset_and_edge_cases_are_well_formed(po):
    for route in ROUTE_IDS:
        dim, nb, m, _ = kc.ROUTES[route]
        (name, make), = kc.family_cases("O", route)
        A, B, k, adv, note = make()
        assert A.dtype == np.float32 and A.shape == (kc.NA, dim) and B.shape == (nb, dim) and B.min() > kc.OFFSET - 40
    seen = set()
    for dim, na, nb, k, bit in kc.EDGES:
        A, B, k_, zero, note = kc.edge(dim, na, nb, k)
        assert A.shape == (na, dim) and B.shape == (nb, dim) and k_ == k and A.dtype == B.dtype == np.float32
        # the route the dispatch of csrc/desc_knn.hip takes, restated: a change of its thresholds has to show up here too
        if na * nb < 65536 or nb < 64:
            want = kc.PATH_SMALL
        elif dim > 128:
            want = kc.PATH_WIDE_BF16
        elif dim == 125:
            want = kc.PATH_LIST_WIDE
        else:
            want = kc.PATH_FILTER if (nb + 31) // 32 >= 64 else kc.PATH_LIST
        assert bit == want, note
        seen.add((dim, na, nb, k))
    table = {(33, 1, 70000, 10), (33, 1024, 64, 1), (33, 1009, 65, 16), (33, 255, 257, 5), (33, 256, 256, 5), (33, 31, 2200, 10),
             (33, 33, 2016, 10), (33, 33, 2017, 10), (2, 700, 6000, 10), (125, 32, 2048, 16), (250, 64, 1100, 5), (352, 64, 1100, 5),
             (1344, 64, 1100, 5), (1980, 64, 1100, 5), (33, 7, 3, 5), (1344, 7, 3, 5)}
    assert seen == table
    # one edge case through the oracle: duplicates tie to the lower index, zero-distance queries come first, short sets end in -1 / +inf
    A, B, k, zero, _ = kc.edge(33, 256, 256, 5)
    idx, d2 = po.desc_knn(A, B, k)
    assert (d2[zero, 0] == 0).all()
    A, B, k, zero, _ = kc.edge(33, 7, 3, 5)
    idx, d2 = po.desc_knn(A, B, k)
    assert (idx[:, 3:] == -1).all() and np.isinf(d2[:, 3:]).all() and (idx[:, :3] >= 0).all()


def test_route_record_is_declared_and_exported(mm):
    hdr = open(os.path.join(ROOT, "include", "mm3d.h")).read()
    assert re.search(r"\bmm3d_debug_knn_paths\s*\(", hdr)
    for name in ("SMALL", "LIST", "FILTER", "LIST_WIDE", "WIDE_BF16", "WIDE_F32", "ANY"):
        value = re.search(r"#define\s+MM3D_KNN_PATH_%s\s+(\d+)u" % name, hdr)
        assert value and int(value.group(1)) == getattr(kc, "PATH_" + name), name
    L = mm.lib()
    assert hasattr(L, "mm3d_debug_knn_paths")
    L.mm3d_debug_knn_paths.restype = __import__("ctypes").c_uint
    assert L.mm3d_debug_knn_paths(None) == 0
    assert callable(getattr(mm, "knn_paths", None))

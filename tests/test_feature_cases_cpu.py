"""The inputs of tests/test_gpu_feature_ties.py, checked without a GPU (tests/feature_cases.py): oracle and numpy only.

A case that tie order cannot change is no test of tie order.  So every cloud is counted by a float32 brute force -- neighbourhoods
with equal d2, pairs at exactly d2 == r2, keypoints whose nearest neighbour is shared -- and the oracle is run on the cloud and on
its index-reversed copy (normals and colours reversed alike, the same keypoints), which flips exactly the order of tied
neighbours and nothing else; compare(), the very function the GPU test uses, must tell the two apart on at least the stated
number of points or rows for every (stage, case) that feature_cases.TIE_ORDER_CHECKS names."""
import numpy as np
import pytest

import feature_cases as fc


@pytest.fixture(scope="module")
def cases(po):
    return fc.reference(po)


@pytest.fixture(scope="module")
def reversed_runs(po, cases):
    """The oracle on every cloud stored back to front; per-point results mapped back to the cloud's own order."""
    out = []
    for c, _ in cases:
        rev, _ = fc.oracle_all(po, c.cloud[::-1].copy(), {k: v[::-1].copy() for k, v in c.normals.items()}, c.keypoints)
        for key in list(rev):
            if key[0] in ("normals", "harris_response"):
                rev[key] = rev[key][::-1].copy()
        out.append(rev)
    return out


def test_the_clouds_are_what_they_claim(cases):
    for c, _ in cases:
        t = fc.tie_counts(c)
        print(c.name, t)
        n = t["points"]
        assert n == len(c.cloud) <= 650 and t["largest neighbourhood"] < 300
        for label in ("normals", "descriptors"):
            assert t["neighbourhoods of the %s radius with two equal d2" % label] >= 0.9 * n
            assert t["pairs at exactly d2 == r2, %s radius" % label] >= 500
        assert t["off-cloud keypoints whose minimum d2 is shared"] >= 100
        assert t["neighbour counts of the special keypoints, off"] == [0, 1, 2, 3]
        assert t["neighbour counts of the special keypoints, on"] == [0, 1, 2, 3]
        p = c.xyz()
        for i, j in c.dup:                                      # coincident points at distinct indices, with different colours
            assert (p[i] == p[j]).all() and c.cloud["rgba"][i] != c.cloud["rgba"][j]
        kp = c.keypoints["on"]
        assert sum((kp["x"] == kp["x"][0]) & (kp["y"] == kp["y"][0]) & (kp["z"] == kp["z"][0])) == 2      # both copies of a point
        # 15 to 17 significant bits in every coordinate (odd multiples of 2^-10 of magnitude >= 16), all of them on the lattice
        q = p.astype(np.float64) * 1024
        assert (q == np.round(q)).all() and (np.abs(q) % 2 == 1).any(axis=0).all() and np.abs(p).min() >= 16
        # points exactly on faces of the search grids' cells (cell r / 2, origin the bounding box's minimum)
        for r in (fc.R_NRM, fc.R_DESC):
            f = (p.astype(np.float64) - p.min(axis=0)) / (r / 2)
            assert ((f == np.round(f)).any(axis=1)).sum() >= 100
        rnd = c.normals["random"]
        nan = np.isnan(rnd["nx"])
        assert nan.sum() == len(range(0, n, 17)) and np.isnan(rnd["ny"][nan]).all() and np.isnan(rnd["nz"][nan]).all()
        v = np.stack([rnd["nx"], rnd["ny"], rnd["nz"]], 1)[~nan].astype(np.float64)
        assert np.abs(np.linalg.norm(v, axis=1) - 1).max() < 1e-6


def test_compare_sees_what_it_should():
    a = np.arange(12, dtype=np.float32).reshape(4, 3)
    b = a.copy()
    b[2, 1] = np.nextafter(b[2, 1], np.float32(np.inf))
    assert list(fc.compare("pfh", b, a)) == [2] and list(fc.compare("harris_keypoints", b, a)) == [2]
    assert len(fc.compare("pfh", a[:3], a)) == 4                  # a different count fails every row
    z = np.zeros((3, 4), np.float32)
    assert list(fc.compare("rsd", z + np.float32(2e-6), z)) == [0, 1, 2] and len(fc.compare("rsd", z + np.float32(5e-7), z)) == 0
    assert list(fc.compare("shot", z + np.float32(3e-6), z)) == [0, 1, 2] and len(fc.compare("shot", z + np.float32(1e-6), z)) == 0
    n = np.zeros(3, dtype=fc.NORMAL)
    m = n.copy()
    n["nx"][1] = np.nan
    m["nx"][1] = -np.float32(np.nan)                              # NaNs of different sign match; a NaN against a number does not
    assert len(fc.compare("normals", m, n)) == 0
    m["nx"][1] = 0.0
    assert list(fc.compare("normals", m, n)) == [1]
    m["nx"][1], m["nz"][0] = np.nan, -0.0                         # -0.0 is not +0.0
    assert list(fc.compare("normals", m, n)) == [0]
    ref = np.ones((2, 1980), np.float32)
    got = ref.copy()
    got[0, :8] += 1e-3
    assert len(fc.compare("sc3d", got, ref)) == 0
    got[0, 8] += 1e-3
    assert list(fc.compare("sc3d", got, ref)) == [0]
    got = ref.copy()
    got[1, :4] += 30.0                                            # 4 bins, but 6 % of the mass
    assert list(fc.compare("sc3d", got, ref)) == [1]
    k = np.zeros(5, dtype=fc.POINT)
    k["x"] = np.arange(5)
    assert list(fc.survivors(k, k[[0, 2, 3]])) == [True, False, True, True, False]


def test_a_wrong_tie_order_is_visible(cases, reversed_runs):
    """compare(reversed, forward) fails on at least TIE_ORDER_CHECKS' number of points / rows, cloud by cloud; SHOT's rows are
    counted over the three clouds together; PFHRGB does not depend on the order at all."""
    short, shot = [], {k: 0 for k in fc.SHOT_TIE_ORDER_CHECKS}
    for (c, ref), rev in zip(cases, reversed_runs):
        for key, least in fc.TIE_ORDER_CHECKS.items():
            bad = len(fc.compare(key[0], rev[key], ref[key]))
            print("%-7s %-44s %4d of %4d differ (at least %d wanted)" % (c.name, key, bad, len(ref[key]), least))
            if bad < least:
                short.append((c.name, key, bad, least))
        for key in shot:
            bad = len(fc.compare("shot", rev[key], ref[key]))
            print("%-7s %-44s %4d of %4d differ" % (c.name, key, bad, len(ref[key])))
            shot[key] += bad
        for ns in fc.NORMAL_SETS:
            for ks in fc.KEYPOINT_SETS:
                assert len(fc.compare("pfhrgb", rev["pfhrgb", ns, ks], ref["pfhrgb", ns, ks])) == 0
                for name in fc.DESCRIPTORS:                       # the same keypoints survive either way
                    assert len(fc.compare("keypoints", rev["keypoints", name, ns, ks], ref["keypoints", name, ns, ks])) == 0
    short += [("three clouds", k, v, fc.SHOT_TIE_ORDER_CHECKS[k]) for k, v in shot.items() if v < fc.SHOT_TIE_ORDER_CHECKS[k]]
    assert not short, short


def test_rows_are_finite_and_pruning_is_what_the_oracle_documents(cases):
    for c, ref in cases:
        assert np.isnan(ref["normals", None, None]["nx"]).sum() >= 1          # (the clusters of 1 and 2 points at least)
        for ns in fc.NORMAL_SETS:
            assert np.isfinite(ref["harris_response", ns, None]).all()
            for ks in fc.KEYPOINT_SETS:
                kp = c.keypoints[ks]
                far, one, two, three = c.special[ks]
                n = len(kp)
                # the far keypoint goes from PFH, FPFH, SC3D and SHOT; PFHRGB and RSD keep it with a zero row; SHOT also drops
                # the keypoints with fewer than 5 neighbours
                want = {"pfh": n - 1, "fpfh": n - 1, "sc3d": n - 1, "pfhrgb": n, "rsd": n, "shot": n - 4}
                for name in fc.DESCRIPTORS:
                    rows, kept = ref[name, ns, ks], ref["keypoints", name, ns, ks]
                    assert len(rows) == len(kept) == want[name], (c.name, name, ns, ks, len(rows))
                    assert np.isfinite(rows).all(), (c.name, name, ns, ks)
                    keep = fc.survivors(kp, kept)
                    assert not keep[far] or name in ("pfhrgb", "rsd")
                    if name == "shot":
                        assert not keep[[one, two, three]].any() and keep.sum() == n - 4
                        assert ref["shot_frames", ns, ks].shape == (n - 4, 9) and np.isfinite(ref["shot_frames", ns, ks]).all()
                # the row kinds of 0, 1, 2 and 3 neighbours (positions in the unpruned order; PFH's far row is gone)
                rsd, pfh, rgb, sc = ref["rsd", ns, ks], ref["pfh", ns, ks], ref["pfhrgb", ns, ks], ref["sc3d", ns, ks]
                assert not rsd[far].any() and not rsd[one].any()                        # fewer than 2 neighbours: (0, 0)
                assert not pfh[one - 1].any()                                           # one neighbour, no pair: zeros, kept
                assert pfh[two - 1].max() == 100.0 and (pfh[two - 1] > 0).sum() == 1    # one pair: 100 in one bin
                assert abs(float(pfh[three - 1].sum()) - 100.0) < 1e-3 and pfh[three - 1].max() <= 100.0
                assert not rgb[far].any() and not rgb[one].any()
                assert abs(float(rgb[two, :125].sum()) - 200.0) < 1e-3                  # both ordered pairs
                if ks == "on":
                    assert not sc[one - 1].any()                                        # the only neighbour is the keypoint itself
                else:
                    assert (sc[one - 1] > 0).sum() == 1                                 # one vote


def test_the_degenerate_harris_cases_on_the_plane(cases):
    """With exactly vertical normals every response is 0.0f, every point is a corner at threshold 0.0 (equal responses keep
    each other) and every refinement matrix is singular, so the corners stay where they are."""
    c, ref = cases[0]
    assert c.name == "plane"
    flat = c.normals["flat"]
    ok = ~np.isnan(flat["nx"])
    assert ok.sum() == len(flat) - 3 and (flat["nx"][ok] == 0).all() and (flat["ny"][ok] == 0).all() and (np.abs(flat["nz"][ok]) == 1).all()
    assert len(np.unique(ref["harris_response", "flat", None])) == 1
    for thr in fc.HARRIS_THRESHOLDS:
        assert np.array_equal(ref["harris_kept", "flat", thr], np.arange(len(c.cloud)))
        assert len(fc.compare("harris_keypoints", ref["harris_keypoints", "flat", thr], c.xyz())) == 0
    # the oracle's normals of the translated plane are not exactly vertical, but equal responses among neighbours abound
    resp = ref["harris_response", "oracle", None]
    assert len(np.unique(resp)) <= 16
    near = fc.d2_matrix(c.xyz(), c.xyz()) < np.float32(fc.R_NRM * fc.R_NRM)
    shared = sum(int((resp[near[i]] == resp[i]).sum() >= 2) for i in range(len(resp)))
    assert shared >= 500, shared
    # corners that move: on `corner` some refined keypoint leaves its cloud point
    c2, ref2 = cases[2]
    kept = ref2["harris_kept", "random", 0.0]
    assert len(fc.compare("harris_keypoints", ref2["harris_keypoints", "random", 0.0], c2.xyz()[kept])) >= 1


def test_prefixes_of_the_keypoints_give_prefixes_of_the_rows(po, cases):
    """RSD, SHOT and PFH rows depend on their own keypoint only, so the first n keypoints give the first rows of the full run; SC3D
    draws from one mt19937 in keypoint order, and a pruned keypoint takes no draw, so it holds there too -- the GPU test still
    compares SC3D with the oracle run on the same prefix."""
    c, ref = cases[1]
    kp, nrm = c.keypoints["off"], c.normals["random"]
    for name, fn in (("rsd", po.descriptors_rsd), ("shot", po.descriptors_shot), ("pfh", po.descriptors_pfh), ("sc3d", po.descriptors_sc3d)):
        keep = fc.survivors(kp, ref["keypoints", name, "random", "off"])
        for n in fc.PREFIXES:
            _, rows = fn(c.cloud, nrm, kp[:n], fc.R_DESC)
            assert len(fc.compare("pfh", rows, ref[name, "random", "off"][:keep[:n].sum()])) == 0, (name, n)

"""The inputs of tests/test_gpu_feature_scratch.py, checked without a GPU (tests/overflow_cases.py): oracle and numpy only.

A test of the scratch pass that never reaches the scratch pass is no test.  So a float32 brute force that forms d2 as the kernels do
counts every keypoint's neighbours, the kernels' own comparison with their capacity is read from their source (m > cap sends a
neighbourhood away, so m == cap stays), and the number of rows each family must send to scratch follows; the GPU test holds the
library's counters against these numbers."""
import os
import re

import numpy as np
import pytest

import feature_cases as fc
import overflow_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "map-merge_amd", "csrc")


@pytest.fixture(scope="module")
def blob(po):
    return oc.blob_reference(po)


@pytest.fixture(scope="module")
def scene(po, synth):
    return oc.scene_reference(po, synth)


def test_the_kernels_compare_as_the_cases_assume():
    """Capacities, the strict comparison and the host's sizing rule, as the four files state them."""
    for name, const, cap in (("pfh", "kPfhCap", 1024), ("shot", "kShotCap", 1024), ("sc3d", "kScCap", 1024), ("harris", "kHarrisCap", 2048)):
        src = open(os.path.join(CSRC, name + ".hip")).read()
        assert re.search(r"constexpr int %s = %d;" % (const, cap), src), name
        assert oc.LDS_CAP[name] == cap
        assert len(re.findall(r"if \(m > cap\) \{", src)) == 1 and "m >= cap" not in src, name       # m == cap stays in LDS
        assert len(re.findall(r"if \(slot < cap\)", src)) == 1, name
        assert "feature_lds_cap(%s)" % const in src, name
    assert "scratch(c, (size_t)n_over * max_m)" in open(os.path.join(CSRC, "pfh.hip")).read()
    for name, const in (("shot", "kShotCap"), ("sc3d", "kScCap")):
        assert re.search(r"int cap = %s;\s*while \(cap < h\[1\]\) cap <<= 1;" % const, open(os.path.join(CSRC, name + ".hip")).read()), name
    assert re.search(r"int cap = kHarrisCap;\s*while \(cap < 2 \* h\[1\]\) cap <<= 1;", open(os.path.join(CSRC, "harris.hip")).read())
    assert oc.scratch_cap("pfh", 2300) == 2300 and oc.scratch_cap("shot", 1025) == 2048 and oc.scratch_cap("sc3d", 2300) == 4096
    assert oc.scratch_cap("harris", 65) == 2048 and oc.scratch_cap("harris", 2049) == 8192 and oc.scratch_cap("shot", 65) == 1024
    assert oc.first_cap("pfh", 0) == 1024 and oc.first_cap("pfh", 64) == 64 and oc.first_cap("pfh", 2048) == 1024 and oc.first_cap("harris", 1024) == 1024


def test_the_blob_cloud_is_what_it_claims(blob):
    b, ref = blob
    p = oc.xyz(b.cloud).astype(np.float64)
    assert len(b.cloud) == sum(oc.BLOB_SIZES) + oc.N_SPARSE
    for i, size in enumerate(oc.BLOB_SIZES):
        mine = p[b.label == i]
        assert len(mine) == size
        assert np.linalg.norm(mine - b.centres[i], axis=1).max() < oc.BLOB_RADIUS                    # so the diameter is below R
        assert len(mine) - len(np.unique(mine, axis=0)) == oc.DUPLICATED.get(size, 0)                # points stored twice
    gaps = np.linalg.norm(b.centres[:, None] - b.centres[None], axis=2)
    assert gaps[gaps > 0].min() >= 3 * oc.R
    sparse = p[b.label < 0]
    assert np.linalg.norm(sparse[:, None] - b.centres[None], axis=2).min() > oc.R + oc.BLOB_RADIUS   # further than R from every blob point
    assert not (np.diff(b.label) == 0).all() and (b.label[:50] != b.label[0]).any()                  # shuffled
    nan = np.isnan(b.normals["nx"])
    assert nan.sum() == len(range(0, len(p), 17)) and np.isnan(b.normals["nz"][nan]).all()
    # keypoints: every centre has exactly its blob, the far and the non-finite one nothing, the sparse ones a handful
    counts = b.counts()
    print(list(zip(b.kinds.tolist(), counts.tolist())))
    blobs = b.kinds > 0
    assert sorted(b.kinds[blobs]) == list(oc.BLOB_SIZES) and (counts[blobs] == b.kinds[blobs]).all()
    assert (counts[b.kinds == 0] == 0).all() and (counts[b.kinds == -1] == 0).all() and (b.kinds == 0).sum() == (b.kinds == -1).sum() == 1
    assert np.isnan(oc.xyz(b.keypoints[b.kinds == -1])).any()
    sp = counts[b.kinds == -2]
    assert len(sp) == oc.N_SPARSE_KEYPOINTS and sp.min() >= 1 and sp.max() < 64
    d2 = fc.d2_matrix(oc.xyz(b.keypoints[blobs]), oc.xyz(b.cloud))
    r2 = np.float32(oc.R * oc.R)
    assert not ((d2 >= 0.25 * r2) & (d2 < 2.5 * r2)).any()                                           # nothing near d2 == r2
    # overflowing, fitting and pruned rows alternate: no two neighbours in the list are both overflowing blobs
    over = counts > 1024
    assert not (over[1:] & over[:-1]).any() and over[0] and (~over[-1:]).all()
    # (d2, index) ties among an overflowing keypoint's neighbours
    for size in oc.DUPLICATED:
        row = d2[list(b.kinds[blobs]).index(size)]
        v = row[row < r2]
        assert len(v) - len(np.unique(v)) >= oc.DUPLICATED[size]
    # the rows each family sends to scratch at the true capacities
    for fam in ("pfh", "shot", "sc3d"):
        assert oc.expected_overflow(counts, fam) == (6, {"pfh": 2300, "shot": 4096, "sc3d": 4096}[fam])
    assert oc.expected_overflow(counts[counts != 1025], "shot") == (5, 4096)                         # 1024 stays, 1025 leaves


def test_what_the_oracle_keeps_of_the_blob_keypoints(blob):
    b, ref = blob
    n = len(b.keypoints)
    # PFH and SC3D drop the far and the non-finite keypoint, PFHRGB keeps both with a zero row, SHOT also drops fewer than 5 neighbours
    counts = b.counts()
    assert len(ref["pfh"][0]) == len(ref["sc3d"][0]) == n - 2 and len(ref["pfhrgb"][0]) == n
    # (a sparse keypoint is a cloud point and does not count itself)
    assert len(ref["shot"][0]) == (counts - (b.kinds == -2) >= 5).sum() and len(ref["shot_frames"]) == len(ref["shot"][0])
    for name in ("pfh", "pfhrgb", "shot", "sc3d"):
        kept, rows = ref[name]
        assert np.isfinite(rows).all() and len(rows) == len(kept)
        keep = fc.survivors(b.keypoints, kept)
        assert keep[b.kinds > 0].all(), name                                                        # every blob row is compared


def test_harris_on_the_blob_cloud(blob):
    """Corners on both sides of 2048, and the replay of the refinement is the oracle's, bit for bit -- so its counts are the
    neighbour counts the oracle's searches saw."""
    b, ref = blob
    pos, kept = ref["harris"]
    assert len(fc.compare("harris_keypoints", ref["harris_replayed"], pos)) == 0
    label = b.label[kept]
    size = np.array([oc.BLOB_SIZES[i] if i >= 0 else 0 for i in label])
    print("corners per blob size:", {s: int((size == s).sum()) for s in sorted(set(size))})
    assert (size > 2048).sum() >= 1 and ((size > 1024) & (size <= 2048)).sum() >= 1
    assert (size == 2047).sum() + (size == 2048).sum() >= 1 and (size == 2049).sum() >= 1
    first = np.array([c[0] for c in ref["harris_counts"]])
    assert (first[size > 0] == size[size > 0]).all()                                                # a blob's corner sees its blob
    n_over, cap = oc.harris_expected_overflow(ref["harris_counts"])
    print("corners sent to scratch:", n_over, "capacity", cap)
    assert n_over >= (size > 2048).sum() and cap == 8192
    # the corners of the 2047 and 2048 blobs stay in LDS throughout
    for c, s in zip(ref["harris_counts"], size):
        if s in (2047, 2048):
            assert c.max() <= 2048


def test_the_scene_populates_both_routes(scene):
    for s in scene:
        n = len(s.keypoints)
        assert n >= 125 and np.isnan(oc.xyz(s.keypoints)).any(axis=1).sum() == 1 and (s.counts == 0).sum() == 2
        assert s.counts.max() < 1024
        sides = {cap: ((s.counts > cap).sum(), (s.counts <= cap).sum()) for cap in oc.HOOK_CAPS}
        print(n, sides, [oc.harris_expected_overflow(s.harris_counts, cap) for cap in oc.HOOK_CAPS])
        # at least a quarter of the keypoints on each side at one of the hook's values.  On this scene that value is 128 (41 of 162
        # and 46 of 131 overflow); 64 leaves 29 and 22 keypoints in LDS, under a quarter, and nothing exceeds 256 (the largest
        # neighbourhood has 202 points), so 256 is the case "the hook is set and nothing leaves"
        assert any(min(sides[cap]) >= 0.25 * n for cap in oc.HOOK_CAPS)
        assert sides[64][0] > sides[128][0] > 0 and min(sides[64]) >= 20 and sides[256][0] == 0
        # Harris: corners on both routes, and one that fits a capacity at its first search and exceeds it later
        assert len(s.harris_counts) >= 10 and len(fc.compare("harris_keypoints", s.harris_replayed, s.harris)) == 0
        assert any(0 < oc.harris_expected_overflow(s.harris_counts, cap)[0] < len(s.harris_counts) for cap in oc.HOOK_CAPS)
        assert any(c[0] <= cap < c.max() for c in s.harris_counts for cap in oc.HOOK_CAPS)

"""The cluster filter, everything a machine without a GPU can check: the header and the library's exports, the numpy restatement
of the rule (tests/cluster_cases.py) against a second formulation and the cases worked by hand, and the shim's MM3D_CLUSTERS
parser."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FUNCTIONS = ("mm3d_cluster_options_default", "mm3d_set_cluster_filter", "mm3d_get_cluster_filter", "mm3d_last_cluster_stats",
             "mm3d_cluster_labels", "mm3d_remove_small_clusters")


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


def test_header_declares_the_cluster_filter():
    h = _read("include", "mm3d.h")
    assert re.search(r"MM3D_CLUSTERS_OFF\s*=\s*0\s*,\s*MM3D_CLUSTERS_MIN_SIZE\s*=\s*1\s*,\s*MM3D_CLUSTERS_LARGEST\s*=\s*2\s*}\s*mm3d_cluster_method;", h)
    assert re.search(r"typedef struct mm3d_cluster_options\s*{\s*int method;[^}]*int min_size;[^}]*double tolerance;[^}]*}\s*mm3d_cluster_options;", h)
    assert re.search(r"typedef struct mm3d_cluster_stats\s*{\s*long long points, valid, kept;[^}]*long long clusters, kept_clusters;[^}]*long long largest;[^}]*}", h)
    for decl in (r"void mm3d_cluster_options_default\(mm3d_cluster_options \*o\);",
                 r"int mm3d_set_cluster_filter\(mm3d_ctx \*ctx, const mm3d_cluster_options \*options\);",
                 r"int mm3d_get_cluster_filter\(const mm3d_ctx \*ctx, mm3d_cluster_options \*options\);",
                 r"int mm3d_last_cluster_stats\(const mm3d_ctx \*ctx, mm3d_cluster_stats \*stats\);",
                 r"int mm3d_cluster_labels\(mm3d_ctx \*ctx, const mm3d_cloud \*points, double tolerance, int \*labels, size_t capacity, mm3d_cluster_stats \*stats\);",
                 r"int mm3d_remove_small_clusters\(mm3d_ctx \*ctx, const mm3d_cloud \*in, double tolerance, int method, int min_size, mm3d_cloud \*\*out\);"):
        assert re.search(decl, h), decl
    # the rule is stated to the operation, and what it is no copy of
    for text in ("(double)d2 <= tolerance * tolerance", "d2 = (dx * dx + dy * dy) + dz * dz in float", "smallest record index",
                 "EuclideanClusterExtraction", "quadratic"):
        assert text in h, text
    body = h[:h.index("} mm3d_params;")]                                      # mm3d_params carries nothing of it
    assert "min_size" not in body[body.rindex("typedef struct"):]


def test_library_exports_mirror_and_defaults(mm):
    """A test that fails without the feature: the names are in libmm3d.so."""
    L = mm.lib()
    for name in FUNCTIONS:
        assert hasattr(L, name), name
    o = mm.ClusterOptions()
    assert C.sizeof(o) == 16 and o.as_tuple() == (mm.ClusterMethod.OFF, 100, 0.0)
    assert C.sizeof(mm.ClusterStats) == 48
    assert (int(mm.ClusterMethod.OFF), int(mm.ClusterMethod.MIN_SIZE), int(mm.ClusterMethod.LARGEST)) == (0, 1, 2) == (cc.OFF, cc.MIN_SIZE, cc.LARGEST)
    for method in ("setClusterFilter", "getClusterFilter", "clusterLabels", "removeSmallClusters"):
        assert callable(getattr(mm.Context, method))
    assert isinstance(mm.Context.last_cluster_stats, property)
    L.mm3d_cluster_options_default(None)                                      # a NULL is ignored
    with pytest.raises(TypeError):
        mm.ClusterOptions(size=3)
    out = C.c_void_p()
    assert L.mm3d_set_cluster_filter(None, C.byref(o)) == EINVAL and L.mm3d_get_cluster_filter(None, C.byref(o)) == EINVAL
    assert L.mm3d_remove_small_clusters(None, None, C.c_double(0.2), 1, 100, C.byref(out)) == EINVAL
    assert L.mm3d_cluster_labels(None, None, C.c_double(0.2), None, C.c_size_t(0), None) == EINVAL
    assert L.mm3d_last_cluster_stats(None, None) == EINVAL


def test_sources_carry_the_stage():
    """The plumbing of DESIGN.md section 7h, as the other stages' tests read it."""
    assert "clusters_euclidean.hip" in _read("map-merge_amd", "build.sh")
    assert "clusters_euclidean" not in _read("map-merge_amd", "csrc", "host_sources.sh")      # it holds kernels
    t = _read("map-merge_amd", "csrc", "types.hpp")
    assert "struct ClusterFilterBase" in t and "const ClusterFilterBase *clusters = nullptr;" in t and "last_cluster_stats" in t
    assert "sel.clusters->filter(" in _read("map-merge_amd", "csrc", "pair_estimate.cpp")
    assert "cluster_options" in _read("map-merge_amd", "csrc", "map_cache.cpp")
    d = _read("DESIGN.md")
    assert "thirteen stages" in d and re.search(r"^#+ 7o\b", d, re.M)


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", sorted(cc.cases()))
def test_restatement_equals_a_second_formulation(name):
    xyz, tol = cc.cases()[name]
    ref = cc.reference(name)
    adj, valid = cc.adjacency(xyz, tol)
    other, rounds = cc.labels_min_propagation(adj, valid)
    print(name, len(xyz), "points", ref["stats"], "min-propagation rounds", rounds)
    assert np.array_equal(valid, np.isfinite(xyz).all(axis=1)) and np.array_equal(valid, ref["valid"])
    assert np.array_equal(ref["labels"], other)
    lab = ref["labels"]
    assert (lab[~valid] == -1).all() and (lab[valid] >= 0).all() and (lab[valid] <= np.nonzero(valid)[0]).all()
    assert (lab[lab[valid]] == lab[valid]).all()                                # a label is a member of its own cluster, its first
    assert not (adj & (lab[:, None] != lab[None, :])).any()                    # no edge leaves a cluster
    assert np.array_equal(adj, adj.T)
    st = ref["stats"]
    assert st["points"] == len(xyz) and st["valid"] == int(valid.sum()) == st["kept"] and st["clusters"] == st["kept_clusters"] == len(cc.partition(lab))


def test_chain_is_one_cluster():
    xyz, tol = cc.cases()["a_chain"]
    ref = cc.reference("a_chain")
    assert len(xyz) == 3000 and (ref["labels"] == 0).all() and ref["stats"]["largest"] == 3000
    adj, _ = cc.adjacency(xyz, tol)
    deg = adj.sum(axis=1)
    assert sorted(np.unique(deg).tolist()) == [1, 2] and (deg == 1).sum() == 2   # a path: nothing but the curve joins it
    cells = np.unique(np.floor(xyz.astype(np.float64) / (1.01 * tol)).astype(np.int64), axis=0)
    assert len(cells) >= 500                                                     # through hundreds of cells


def test_threshold_case_by_hand():
    xyz, tol = cc.cases()["b_threshold"]
    assert tol == 0.5 and len(xyz) == 38
    lattice = xyz[:36].astype(np.float64) * 64.0
    assert np.array_equal(lattice, np.rint(lattice))                             # multiples of 2^-6: every d2 is exact
    d = (xyz[1::2].astype(np.float64) - xyz[0::2].astype(np.float64))
    assert (np.linalg.norm(d[:8], axis=1) == 0.5).all() and (np.linalg.norm(d[8:16], axis=1) == 0.5 + 2.0 ** -6).all()
    assert np.linalg.norm(d[16]) == 0.5 and np.linalg.norm(d[17]) == 0.5
    a, b = xyz[37, 0], xyz[37, 2]
    assert a * a + b * b == np.float32(0.25) and float(a) ** 2 + float(b) ** 2 > 0.25 and abs(a - 0.3) < 1e-5 and abs(b - 0.4) < 1e-5
    for cell in (0.5, 0.505, 0.51):                                              # pairs on both sides of a cell border, adjacent and not
        c = np.floor((xyz[:32, 0].astype(np.float64) - xyz[:, 0].min()) / cell)
        split = c[0::2] != c[1::2]
        assert split[:8].any() and split[8:].any()
    assert cc.reference("b_threshold")["labels"].tolist() == cc.THRESHOLD_LABELS
    assert cc.THRESHOLD_LABELS == [0, 0, 2, 2, 4, 4, 6, 6, 8, 8, 10, 10, 12, 12, 14, 14, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28,
                                   29, 30, 31, 32, 32, 34, 34, 36, 36]


def test_sizes_case_by_hand():
    xyz, blob = cc.sizes()
    assert cc.SIZES_BLOBS == (30, 19, 20, 21, 30, 1, 1, 1, 1, 1) and cc.SIZES_MIN == 20 and len(xyz) == 125
    assert blob[:10].tolist() == list(range(10))                                 # blob b's first record is record b
    lab = cc.reference("c_sizes")["labels"]
    assert np.array_equal(lab, blob)                                             # so every record's label is its blob's number
    assert np.bincount(lab).tolist() == [30, 19, 20, 21, 30, 1, 1, 1, 1, 1]
    keep, st = cc.reference_filter("c_sizes", cc.MIN_SIZE, cc.SIZES_MIN)
    assert np.array_equal(keep, np.isin(blob, (0, 2, 3, 4))) and st == dict(points=125, valid=125, kept=101, clusters=10, kept_clusters=4, largest=30)
    keep, st = cc.reference_filter("c_sizes", cc.LARGEST, 1)
    assert np.array_equal(keep, blob == 0) and st["kept"] == 30 and st["kept_clusters"] == 1     # the tie goes to the smaller label
    keep, st = cc.reference_filter("c_sizes", cc.MIN_SIZE, 1)
    assert keep.all() and st["kept_clusters"] == 10
    keep, st = cc.reference_filter("c_sizes", cc.MIN_SIZE, 31)
    assert not keep.any() and st["kept_clusters"] == 0
    far = np.linalg.norm(xyz[:10, None, :] - xyz[None, :10, :], axis=2)[~np.eye(10, dtype=bool)].min()
    assert far >= 30.0                                                           # tens of metres apart: most cells are empty


def test_the_other_cases_are_what_they_are_for():
    dense, tol = cc.cases()["d_dense_blob"]
    adj, _ = cc.adjacency(dense, tol)
    assert len(dense) == 5000 and adj.sum() == 5000 * 4999                      # all mutually adjacent
    assert (dense.max(axis=0) - dense.min(axis=0)).max() < tol                  # inside one cell, whatever the cell above the tolerance
    inv, _ = cc.cases()["e_invalid_and_duplicates"]
    bad = ~np.isfinite(inv).all(axis=1)
    assert bad[0] and bad[-1] and bad.sum() == 10
    for col in range(3):
        assert np.isnan(inv[:, col]).any() and (inv[:, col] == np.inf).any() and (inv[:, col] == -np.inf).any()
    good = inv[~bad]
    assert len(np.unique(good, axis=0)) < len(good) - 30                        # exact duplicates, and they share a cluster
    lab = cc.reference("e_invalid_and_duplicates")["labels"]
    assert lab[200] == lab[10] and lab[230] == lab[10]
    assert (cc.reference("f_all_invalid")["labels"] == -1).all() and cc.reference("f_all_invalid")["stats"]["clusters"] == 0
    assert cc.reference_filter("f_all_invalid", cc.LARGEST, 1)[0].sum() == 0
    assert len(cc.reference("g_empty")["labels"]) == 0 and cc.reference("h_one_point")["labels"].tolist() == [0]
    for name in ("i_random_1", "j_random_2", "k_random_at_1km", "l_random_at_10km"):
        st = cc.reference(name)["stats"]
        sizes = np.bincount(cc.reference(name)["labels"])
        print(name, st, "sizes present", len(np.unique(sizes[sizes > 0])))
        assert st["clusters"] >= 300 and st["largest"] >= 50 and len(np.unique(sizes[sizes > 0])) >= 10     # many clusters of many sizes
    assert cc.cases()["l_random_at_10km"][0][:, 0].min() >= 10000.0


# ---------------------------------------------------------------- the shim
SHIM_CASES = r"""
#include <cstdio>
#include <cstring>
#include "map_merge_3d_shim.hpp"
using map_merge_3d::mm3d_shim::parse_clusters;
static int refused(const char *v) { try { (void)parse_clusters(v); } catch (const std::runtime_error &e) { return std::strstr(e.what(), "MM3D_CLUSTERS") != nullptr; } return 0; }
static int is(const mm3d_cluster_options &o, int m, int k, double t) { return o.method == m && o.min_size == k && o.tolerance == t; }
int main()
{
  if (!is(parse_clusters(nullptr), MM3D_CLUSTERS_OFF, 100, 0.0)) return 1;
  if (!is(parse_clusters(""), MM3D_CLUSTERS_OFF, 100, 0.0)) return 2;
  if (!is(parse_clusters("off"), MM3D_CLUSTERS_OFF, 100, 0.0)) return 3;
  if (!is(parse_clusters("min_size:200"), MM3D_CLUSTERS_MIN_SIZE, 200, 0.0)) return 4;
  if (!is(parse_clusters("min_size:200:0.25"), MM3D_CLUSTERS_MIN_SIZE, 200, 0.25)) return 5;
  if (!is(parse_clusters("largest"), MM3D_CLUSTERS_LARGEST, 100, 0.0)) return 6;
  if (!is(parse_clusters("largest:.5"), MM3D_CLUSTERS_LARGEST, 100, 0.5)) return 7;
  if (!is(parse_clusters("min_size"), MM3D_CLUSTERS_MIN_SIZE, 100, 0.0)) return 8;
  if (!is(parse_clusters("min_size:1:2"), MM3D_CLUSTERS_MIN_SIZE, 1, 2.0)) return 9;
  const char *bad[] = {"garbage", "min_size:", "min_size:abc", "min_size:0", "min_size:-3", "min_size:200:", "min_size:200:0", "min_size:200:-1",
                       "min_size:200:nan", "min_size:200:inf", "min_size:200:0.25x", "min_size:200:0.25:1", "min_size:1.5", "min_size: 200",
                       "min_sizes", "Largest", "largest:", "largest:0", "largest:abc", "largest:0.2:3", "on", "min_size::1", "min_size:99999999999"};
  for (const char *b : bad) if (!refused(b)) { std::printf("accepted '%s'\n", b); return 10; }
  std::puts("shim clusters: ok");
  return 0;
}
"""


def test_shim_parses_mm3d_clusters(tmp_path):
    """Compiled with the flags tests/shim/build.sh compiles the shim with; the parser lies outside the header's PCL guard."""
    src = tmp_path / "shim_clusters.cpp"
    src.write_text(SHIM_CASES)
    exe = tmp_path / "shim_clusters"
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0 and "shim clusters: ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    s = _read("include", "map_merge_3d_shim.hpp")
    assert 'parse_clusters(std::getenv("MM3D_CLUSTERS"))' in s and "mm3d_set_cluster_filter(e, &clusters)" in s

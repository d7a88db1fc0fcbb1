"""Statistical outlier removal, everything a machine without a GPU can check: the header and the library's exports, the numpy
restatement of the rule (tests/outlier_cases.py) against independent forms and a vector worked by hand, the conditions the GPU
comparisons rest on, the sparse maps the filter is for, and the shim's MM3D_OUTLIERS parser."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import outlier_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FUNCTIONS = ("mm3d_outlier_options_default", "mm3d_set_outlier_filter", "mm3d_get_outlier_filter", "mm3d_knn_mean_distances",
             "mm3d_remove_outliers_statistical", "mm3d_last_outlier_stats", "mm3d_debug_outlier_search")
TIED = ("e_integer_lattice", "d_duplicates")                   # exact ties: scipy's tree may pick other, equally near neighbours


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


def test_header_declares_the_outlier_filter():
    h = _read("include", "mm3d.h")
    assert re.search(r"MM3D_OUTLIERS_RADIUS\s*=\s*0\s*,\s*MM3D_OUTLIERS_STATISTICAL\s*=\s*1\s*}\s*mm3d_outlier_method;", h)
    assert re.search(r"typedef struct mm3d_outlier_options\s*{\s*int method;[^}]*int mean_k;[^}]*double stddev_mult;[^}]*}\s*mm3d_outlier_options;", h)
    assert re.search(r"typedef struct mm3d_outlier_stats\s*{\s*long long points, valid, kept;[^}]*int k;[^}]*double mean, stddev, threshold;[^}]*}", h)
    for decl in (r"void mm3d_outlier_options_default\(mm3d_outlier_options \*o\);",
                 r"int mm3d_set_outlier_filter\(mm3d_ctx \*ctx, const mm3d_outlier_options \*options\);",
                 r"int mm3d_get_outlier_filter\(const mm3d_ctx \*ctx, mm3d_outlier_options \*options\);",
                 r"int mm3d_knn_mean_distances\(mm3d_ctx \*ctx, const mm3d_cloud \*points, int mean_k, double \*out, size_t capacity\);",
                 r"int mm3d_remove_outliers_statistical\(mm3d_ctx \*ctx, const mm3d_cloud \*in, int mean_k, double stddev_mult, mm3d_cloud \*\*out\);",
                 r"int mm3d_last_outlier_stats\(const mm3d_ctx \*ctx, mm3d_outlier_stats \*stats\);",
                 r"void mm3d_debug_outlier_search\(long long out\[3\], int reset\);"):
        assert re.search(decl, h), decl
    assert "one wave's width" in h and "StatisticalOutlierRemoval" in h       # why 64, and what it is no copy of
    body = h[:h.index("} mm3d_params;")]                                      # mm3d_params carries nothing of it
    assert "mean_k" not in body[body.rindex("typedef struct"):]


def test_library_exports_mirror_and_defaults(mm):
    """The test that fails without the feature: the names are in libmm3d.so."""
    L = mm.lib()
    for name in FUNCTIONS + ("mm3d_remove_outliers",):
        assert hasattr(L, name), name
    o = mm.OutlierOptions()
    assert C.sizeof(o) == 16 and o.as_tuple() == (mm.OutlierMethod.RADIUS, 16, 2.0)
    assert int(mm.OutlierMethod.STATISTICAL) == 1 and C.sizeof(mm.OutlierStats) == 56
    for method in ("setOutlierFilter", "getOutlierFilter", "removeOutliersStatistical", "knnMeanDistances"):
        assert callable(getattr(mm.Context, method))
    assert isinstance(mm.Context.last_outlier_stats, property)
    L.mm3d_outlier_options_default(None)                                      # a NULL is ignored
    with pytest.raises(TypeError):
        mm.OutlierOptions(k=3)
    out = C.c_void_p()
    assert L.mm3d_set_outlier_filter(None, C.byref(o)) == EINVAL and L.mm3d_get_outlier_filter(None, C.byref(o)) == EINVAL
    assert L.mm3d_remove_outliers_statistical(None, None, 16, C.c_double(1.0), C.byref(out)) == EINVAL
    assert L.mm3d_knn_mean_distances(None, None, 16, None, C.c_size_t(0)) == EINVAL
    assert L.mm3d_last_outlier_stats(None, None) == EINVAL


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", sorted(oc.cases()))
def test_restatement_equals_an_independent_form(name):
    xyz = oc.cases()[name][0]
    p = xyz[np.isfinite(xyz).all(axis=1)]
    if len(p) <= 1:
        d, valid, k = oc.reference_distances(name, 16)
        assert k == 0 and np.isnan(d).all() and int(valid.sum()) == len(p)
        return
    kmax = min(max(oc.MEAN_KS), len(p) - 1)
    # np.partition on the brute-force matrix: the same numbers, bit for bit
    other = oc.nearest_d2(p, kmax, select="partition")
    for mean_k in oc.MEAN_KS:
        d, valid, k = oc.reference_distances(name, mean_k)
        d2, _, k2 = oc.mean_distances(xyz, mean_k, near=other)
        assert k == k2 == min(mean_k, len(p) - 1) and np.array_equal(valid, np.isfinite(xyz).all(axis=1))
        assert np.array_equal(d[valid], d2[valid]) and np.isnan(d[~valid]).all() and (d[valid] >= 0).all()
    if name in TIED:
        return
    # scipy's k-d tree picks the neighbours in double: the same up to what float32 d2 rounds (2e-7 relative), ties of that size aside
    tree = oc.nearest_d2_tree(p, kmax)
    for mean_k in oc.MEAN_KS:
        d, valid, _ = oc.reference_distances(name, mean_k)
        d3, _, _ = oc.mean_distances(xyz, mean_k, near=tree)
        assert np.allclose(d[valid], d3[valid], rtol=1e-6, atol=0.0), (name, mean_k)


def test_restatement_reproduces_the_vector_worked_by_hand():
    """x = 0, 1, 3, 7 on a line, mean_k 2: the two nearest are (1, 3), (1, 2), (2, 3), (4, 6) away."""
    xyz = np.zeros((4, 3), dtype=np.float32)
    xyz[:, 0] = [0, 1, 3, 7]
    r = oc.restate(xyz, 2, 1.0)
    assert r["d"].tolist() == [2.0, 1.5, 2.5, 5.0] and r["k"] == 2
    assert r["mean"] == 2.75 and abs(r["stddev"] ** 2 - 29.0 / 12.0) < 1e-15
    assert abs(r["threshold"] - (2.75 + np.sqrt(29.0 / 12.0))) < 1e-15 and abs(r["threshold"] - 4.3046) < 1e-4
    assert r["keep"].tolist() == [True, True, True, False]
    assert oc.restate(xyz, 2, 2.0)["keep"].all()
    # an invalid row is nobody's neighbour and is never kept; a duplicate is a neighbour at distance 0
    more = np.concatenate([xyz, [[np.nan, 0, 0]], xyz[:1]]).astype(np.float32)
    r = oc.restate(more, 2, 1.0)
    assert np.isnan(r["d"][4]) and not r["keep"][4] and r["d"][0] == r["d"][5] == 0.5 and r["valid"].sum() == 5
    assert oc.restate(more, 64, 1.0)["k"] == 4


# ---------------------------------------------------------------- what the GPU tests rest on
@pytest.mark.parametrize("name", sorted(n for n, (_, keep) in oc.cases().items() if keep))
def test_no_point_sits_on_the_threshold(name):
    """Double rounding moves t by about 1e-13 relative, so with every |d_i - t| / t >= 1e-9 the device's summation order cannot
    flip a point.  Two points alone are the exception by construction: d_0 = d_1 = mu, var = 0 and t = mu exactly in any order."""
    xyz = oc.cases()[name][0]
    for mean_k, mult in oc.FILTER_PARAMS:
        r = oc.reference_filter(name, mean_k, mult)
        print(name, mean_k, mult, "k'", r["k"], "kept", int(r["keep"].sum()), "of", len(xyz), "margin", r["margin"])
        if name == "c_two_points":
            assert r["stddev"] == 0.0 and r["threshold"] == r["mean"] == r["d"][0] == r["d"][1] == 0.5 and r["keep"].all()
            continue
        assert r["margin"] >= oc.MARGIN, (name, mean_k, mult, r["margin"])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_defaults_remove_the_planted_points_and_keep_the_room(seed):
    xyz, planted = oc.room_with_planted(seed)
    assert planted.sum() == 150 and len(xyz) == 4150
    rows = []
    for mean_k, mult in ((16, 2.0), (16, 1.0), (50, 1.0)):
        r = oc.restate(xyz, mean_k, mult)
        rows.append((mean_k, mult, 1.0 - r["keep"][planted].mean(), r["keep"][~planted].mean()))
        print("seed", seed, "mean_k", mean_k, "stddev_mult", mult, "planted removed %.4f room kept %.4f" % rows[-1][2:])
    assert rows[0][2] >= 0.95 and rows[0][3] >= 0.99
    assert all(r[2] >= 0.95 for r in rows)


@pytest.mark.parametrize("family,n_points,window", [("lattice", 20000, 40.0), ("independent", 20000, 40.0), ("lattice", 12000, 30.0),
                                                    ("independent", 12000, 30.0)])
def test_sparse_maps_survive_the_statistical_rule_only(synth, family, n_points, window):
    """Maps of about 12.5 points per square metre behind a 0.1 m voxel filter: the reference's radius filter at its defaults deletes
    them, the statistical rule keeps them."""
    make = synth.lattice_maps if family == "lattice" else synth.synth_maps
    _, maps = make(3, n_points, window=window, overlap_step=0.25)
    for x, _, _ in maps:
        down = oc.first_point_per_voxel(x, 0.1)
        radius = oc.radius_rule_keeps(down, 0.8, 50)
        stat = oc.restate(down, 16, 1.0, nearest=oc.nearest_d2_tree)["keep"].mean()
        print(family, n_points, "down-sampled", len(down), "radius rule keeps %.4f statistical keeps %.4f" % (radius, stat))
        assert radius <= 0.02 and stat >= 0.75


# ---------------------------------------------------------------- the shim
SHIM_CASES = r"""
#include <cstdio>
#include <cstring>
#include "map_merge_3d_shim.hpp"
using map_merge_3d::mm3d_shim::parse_outliers;
static int refused(const char *v) { try { (void)parse_outliers(v); } catch (const std::runtime_error &e) { return std::strstr(e.what(), "MM3D_OUTLIERS") != nullptr; } return 0; }
static int is(const mm3d_outlier_options &o, int m, int k, double s) { return o.method == m && o.mean_k == k && o.stddev_mult == s; }
int main()
{
  if (!is(parse_outliers(nullptr), MM3D_OUTLIERS_RADIUS, 16, 2.0)) return 1;
  if (!is(parse_outliers(""), MM3D_OUTLIERS_RADIUS, 16, 2.0)) return 2;
  if (!is(parse_outliers("reference"), MM3D_OUTLIERS_RADIUS, 16, 2.0)) return 3;
  if (!is(parse_outliers("statistical"), MM3D_OUTLIERS_STATISTICAL, 16, 2.0)) return 4;
  if (!is(parse_outliers("statistical:50"), MM3D_OUTLIERS_STATISTICAL, 50, 2.0)) return 5;
  if (!is(parse_outliers("statistical:8:1.5"), MM3D_OUTLIERS_STATISTICAL, 8, 1.5)) return 6;
  if (!is(parse_outliers("statistical:64:0"), MM3D_OUTLIERS_STATISTICAL, 64, 0.0)) return 7;
  if (!is(parse_outliers("statistical:1:.5"), MM3D_OUTLIERS_STATISTICAL, 1, 0.5)) return 8;
  const char *bad[] = {"garbage", "statistical:", "statistical:abc", "statistical:0", "statistical:65", "statistical:-3", "statistical:16:",
                       "statistical:16:-1", "statistical:16:nan", "statistical:16:inf", "statistical:16:1.0x", "statistical:16:1:2",
                       "statistical:1.5", "statistical: 16", "statistically", "Statistical", "radius", "statistical::1"};
  for (const char *b : bad) if (!refused(b)) { std::printf("accepted '%s'\n", b); return 9; }
  std::puts("shim outliers: ok");
  return 0;
}
"""


def test_shim_parses_mm3d_outliers(tmp_path):
    """Compiled with the flags tests/shim/build.sh compiles the shim with; the parser lies outside the header's PCL guard."""
    src = tmp_path / "shim_outliers.cpp"
    src.write_text(SHIM_CASES)
    exe = tmp_path / "shim_outliers"
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0 and "shim outliers: ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    s = _read("include", "map_merge_3d_shim.hpp")
    assert 'parse_outliers(std::getenv("MM3D_OUTLIERS"))' in s and "mm3d_set_outlier_filter(e, &outliers)" in s

"""Consistency-graph estimation (mm3d_set_estimator) without a GPU: the numpy restatement of consistency_cases.py alone on the
scenes where the reference's RANSAC goes blind, the oracle's RANSAC on the same inputs, the declared and exported surface, and
the shim's MM3D_ESTIMATOR parser compiled on its own."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from consistency_cases import DEFAULTS, THRESHOLD, identity_corr, meets_the_conditions, points, restate, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


# ---------------------------------------------------------------- the rule against the oracle's RANSAC
@pytest.fixture(scope="module")
def low_share():
    """The restatement on scene(seed, 1500, frac), seeds 1 to 5 at 3 % and 5 %: computed once."""
    out = {}
    for frac in (0.03, 0.05):
        for seed in range(1, 6):
            p, q, inl, R, t = scene(seed, 1500, frac)
            out[frac, seed] = (p, q, inl, R, t, restate(p, q, identity_corr(1500, _corr_dtype()), THRESHOLD))
    return out


def _corr_dtype():
    return np.dtype([("index_query", "<i4"), ("index_match", "<i4"), ("distance", "<f4")])


@pytest.mark.parametrize("frac", [0.03, 0.05])
def test_restatement_keeps_the_inliers_at_low_shares(low_share, frac):
    for seed in range(1, 6):
        p, q, inl, R, t, r = low_share[frac, seed]
        held, others = meets_the_conditions(r["inliers"], inl)
        err_R, err_t = np.abs(r["T"][:3, :3] - R).max(), np.abs(r["T"][:3, 3] - t).max()
        print("share", frac, "seed", seed, "true", int(inl.sum()), "held", held, "others", others, "edges", int(r["deg"].sum()) // 2,
              "winner rank", r["winner"], "|R - R_true|", err_R, "|t - t_true|", err_t)
        # at most 10 % others, each less than the threshold of 0.5 m off: the centroid moves by at most 0.05 m, the rotation by
        # about that over the inliers' spread of some 5 m = 0.01, which the centroid's 12.6 m from the origin turns into another
        # 0.13 m of translation; the noise of 0.02 m over 40 pairs is small beside both
        assert err_R < 0.02 and err_t < 0.2


def test_oracle_ransac_is_blind_at_three_percent(po, low_share):
    """pcl's CorrespondenceRejectorSampleConsensus at its 1 000 iterations on the same inputs: the most it held was 6 of 45."""
    for seed in range(1, 6):
        p, q, inl, _, _, r = low_share[0.03, seed]
        _, inl_ref, _, _ = po.ransac(points(p, po.POINT), points(q, po.POINT), identity_corr(1500, po.CORR), THRESHOLD)
        held = int(inl[inl_ref["index_query"]].sum())
        print("seed", seed, "oracle RANSAC held", held, "of", int(inl.sum()), "; the restatement", int(inl[r["inliers"]].sum()))
        assert held < 0.5 * inl.sum()


def test_both_estimators_hold_everything_at_twenty_percent(po):
    for seed in range(1, 6):
        p, q, inl, _, _ = scene(seed, 1500, 0.2)
        r = restate(p, q, identity_corr(1500, po.CORR), THRESHOLD)
        _, inl_ref, _, _ = po.ransac(points(p, po.POINT), points(q, po.POINT), identity_corr(1500, po.CORR), THRESHOLD)
        assert inl[r["inliers"]].sum() == inl.sum() == 300
        assert inl[inl_ref["index_query"]].sum() == 300


def test_restatement_degenerate_inputs():
    dt = _corr_dtype()
    p, q, _, _, _ = scene(1, 40, 0.5)
    for n in (0, 2):
        r = restate(p, q, identity_corr(n, dt), THRESHOLD)
        assert r["winner"] == -1 and not r["T"].any() and len(r["inliers"]) == 0
    # every target the same point: db = 0 fails db > t2 everywhere
    r = restate(p, np.tile(q[:1], (40, 1)), identity_corr(40, dt), THRESHOLD)
    assert not r["A"].any() and len(r["seeds"]) == 0 and r["winner"] == -1 and not r["T"].any()
    # the matrix is symmetric with a zero diagonal, and the bit rows are its bits
    r = restate(p, q, identity_corr(40, dt), THRESHOLD)
    assert np.array_equal(r["A"], r["A"].T) and not r["A"].diagonal().any()
    assert r["rows"].shape == (40, 1) and all(int(r["rows"][i, 0]) == sum(1 << j for j in np.flatnonzero(r["A"][i])) for i in range(40))


# ---------------------------------------------------------------- the surface
def test_header_declares_the_estimator():
    h = _read("include", "mm3d.h")
    assert re.search(r"typedef enum \{ MM3D_ESTIMATOR_RANSAC = 0, MM3D_ESTIMATOR_CONSISTENCY = 1 \} mm3d_estimator_method;", h)
    m = re.search(r"typedef struct mm3d_estimator_options \{(.*?)\} mm3d_estimator_options;", h, re.S)
    assert m, "mm3d_estimator_options is not declared"
    assert re.findall(r"^\s*(int|double)\s+(\w+);", m.group(1), re.M) == [("int", "method"), ("double", "tolerance"), ("int", "seeds"),
                                                                         ("int", "consensus")]
    m = re.search(r"typedef struct mm3d_estimator_stats \{(.*?)\} mm3d_estimator_stats;", h, re.S)
    assert m, "mm3d_estimator_stats is not declared"
    assert re.findall(r"^\s*(int|long long)\s+(\w+);", m.group(1), re.M) == [
        ("long long", "correspondences"), ("long long", "edges"), ("long long", "seeds"), ("long long", "hypotheses"),
        ("int", "winner_index"), ("int", "winner_rank"), ("int", "winner_inliers")]
    for decl in ("void mm3d_estimator_options_default(mm3d_estimator_options *o);",
                 "int mm3d_set_estimator(mm3d_ctx *ctx, const mm3d_estimator_options *options);",
                 "int mm3d_get_estimator(const mm3d_ctx *ctx, mm3d_estimator_options *options);",
                 "int mm3d_last_estimator_stats(const mm3d_ctx *ctx, mm3d_estimator_stats *stats);",
                 "int mm3d_estimate_transform_consistency(mm3d_ctx *ctx, const mm3d_cloud *source_keypoints, const mm3d_cloud *target_keypoints,",
                 "int mm3d_debug_consistency(mm3d_ctx *ctx, const mm3d_cloud *source_keypoints, const mm3d_cloud *target_keypoints,"):
        assert decl in h, decl
    # what the restatement restates
    assert "e e <= 4.0 (da db) with e = (da + db) - t2" in h and "(deg descending, i ascending)" in h and "ties to the lower j" in h


def test_library_exports_the_estimator(mm):
    lib = mm.lib()
    for name in ("mm3d_estimator_options_default", "mm3d_set_estimator", "mm3d_get_estimator", "mm3d_last_estimator_stats",
                 "mm3d_estimate_transform_consistency", "mm3d_debug_consistency"):
        assert hasattr(lib, name), name
    for name in ("EstimatorMethod", "EstimatorOptions", "EstimatorStats"):
        assert hasattr(mm, name), name
    for name in ("setEstimator", "getEstimator", "lastEstimatorStats", "estimateTransformConsistency", "consistencyGraph"):
        assert callable(getattr(mm.Context, name)), name
    assert (mm.EstimatorMethod.RANSAC, mm.EstimatorMethod.CONSISTENCY) == (0, 1)
    assert C.sizeof(mm.EstimatorOptions) == 24 and C.sizeof(mm.EstimatorStats) == 48
    assert mm.EstimatorOptions().as_tuple() == DEFAULTS
    lib.mm3d_estimator_options_default(None)               # a no-op, not a crash
    # what is checked before anything touches a device or the handle: a context that is never dereferenced shows it
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    o = mm.EstimatorOptions()
    T = (C.c_float * 16)()
    corr = (C.c_char * 12)()

    def stage(ctx, s, t, cr, opt, out=T):
        return lib.mm3d_estimate_transform_consistency(ctx, s, t, cr, C.c_size_t(1), C.c_double(0.5), opt, out, None, C.c_size_t(0), None, None)

    def hook(ctx, s, t, cr, opt):
        return lib.mm3d_debug_consistency(ctx, s, t, cr, C.c_size_t(1), C.c_double(0.5), opt, None, None, None, None, None, None, None)

    assert lib.mm3d_set_estimator(None, C.byref(o)) == EINVAL and lib.mm3d_set_estimator(fake, None) == EINVAL
    assert lib.mm3d_get_estimator(None, C.byref(o)) == EINVAL and lib.mm3d_get_estimator(fake, None) == EINVAL
    assert lib.mm3d_last_estimator_stats(None, C.byref(mm.EstimatorStats())) == EINVAL and lib.mm3d_last_estimator_stats(fake, None) == EINVAL
    for bad in (dict(method=2), dict(method=-1), dict(tolerance=-0.1), dict(tolerance=float("nan")), dict(seeds=0), dict(seeds=4097),
                dict(consensus=2), dict(consensus=65)):
        for method in (0, 1):
            b = mm.EstimatorOptions(**{"method": method, **bad})
            assert lib.mm3d_set_estimator(fake, C.byref(b)) == EINVAL, bad
            assert stage(fake, fake, fake, corr, C.byref(b)) == EINVAL and hook(fake, fake, fake, corr, C.byref(b)) == EINVAL
    for args in ((None, fake, fake, corr, C.byref(o)), (fake, None, fake, corr, C.byref(o)), (fake, fake, None, corr, C.byref(o)),
                 (fake, fake, fake, None, C.byref(o)), (fake, fake, fake, corr, None)):
        assert stage(*args) == EINVAL and hook(*args) == EINVAL
    assert stage(fake, fake, fake, corr, C.byref(o), out=None) == EINVAL


SHIM_CASES = r"""
#include <cstdio>
#include <cstring>
#include "map_merge_3d_shim.hpp"
using map_merge_3d::mm3d_shim::parse_estimator;
using map_merge_3d::mm3d_shim::check_estimator_devices;
static int refused(const char *v)
{
  try { (void)parse_estimator(v); } catch (const std::runtime_error &e) { return std::strstr(e.what(), "MM3D_ESTIMATOR") != nullptr; }
  return 0;
}
static int devices_refused(const char *v, const char *d)
{
  try { check_estimator_devices(parse_estimator(v), d); }
  catch (const std::runtime_error &e) { return std::strstr(e.what(), "MM3D_ESTIMATOR") != nullptr && std::strstr(e.what(), "MM3D_DEVICES") != nullptr; }
  return 0;
}
static int is(const mm3d_estimator_options &o, int method, int seeds)
{
  return o.method == method && o.tolerance == 0.0 && o.seeds == seeds && o.consensus == 20;
}
int main()
{
  if (!is(parse_estimator(nullptr), MM3D_ESTIMATOR_RANSAC, 64) || !is(parse_estimator(""), MM3D_ESTIMATOR_RANSAC, 64)) return 1;
  if (!is(parse_estimator("ransac"), MM3D_ESTIMATOR_RANSAC, 64)) return 2;
  if (!is(parse_estimator("consistency"), MM3D_ESTIMATOR_CONSISTENCY, 64)) return 3;
  if (!is(parse_estimator("consistency:1"), MM3D_ESTIMATOR_CONSISTENCY, 1) || !is(parse_estimator("consistency:256"), MM3D_ESTIMATOR_CONSISTENCY, 256) ||
      !is(parse_estimator("consistency:4096"), MM3D_ESTIMATOR_CONSISTENCY, 4096))
    return 4;
  const char *bad[] = {"consistency:", "consistency:0", "consistency:4097", "consistency:-3", "consistency:12x", "consistency:1.5", "consistency: 8",
                       "consistency:+8", "consistent", "consistencyx", "RANSAC", "1", "on", " "};
  for (const char *b : bad) if (!refused(b)) { std::printf("accepted '%s'\n", b); return 5; }
  if (!devices_refused("consistency", "0,1") || !devices_refused("consistency:8", "all")) return 6;
  if (devices_refused("consistency", nullptr) || devices_refused("consistency", "") || devices_refused("ransac", "0,1") || devices_refused(nullptr, "all")) return 7;
  std::puts("shim estimator: ok");
  return 0;
}
"""


def test_shim_parses_mm3d_estimator(tmp_path):
    """Compiled with the flags tests/shim/build.sh compiles the shim with; the parser lies outside the header's PCL guard."""
    src = tmp_path / "shim_estimator.cpp"
    src.write_text(SHIM_CASES)
    exe = tmp_path / "shim_estimator"
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0 and "shim estimator: ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    s = _read("include", "map_merge_3d_shim.hpp")
    assert 'parse_estimator(std::getenv("MM3D_ESTIMATOR"))' in s and "mm3d_set_estimator(e, &estimator)" in s
    assert 'check_estimator_devices(estimator, std::getenv("MM3D_DEVICES"))' in s

"""ICP correspondence rejection (mm3d_set_icp_rejection) without a GPU: the declared and exported surface, defaults and ranges, the
shim's MM3D_ICP_REJECT parser compiled on its own, and the numpy restatement of the rule that include/mm3d.h states -- checked
against literal vectors and on the cabinet scene, and read by test_gpu_icp_rejection.py."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_icp_plane import _ldlt_solve, _nearest, _problem, _xform_f32, construct_transform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NONE, TRIMMED, MEDIAN = 0, 1, 2

Opt = collections.namedtuple("Opt", "one_to_one distance overlap_ratio min_correspondences median_factor")
DEFAULT = Opt(0, NONE, 0.5, 0, 1.0)


def opt(**kw):
    return DEFAULT._replace(**kw)


# the rejecting variants measured on the cabinet scene
VARIANTS = {"trimmed 0.7": opt(distance=TRIMMED, overlap_ratio=0.7), "trimmed 0.5": opt(distance=TRIMMED, overlap_ratio=0.5),
            "median x 1.5": opt(distance=MEDIAN, median_factor=1.5), "median x 4": opt(distance=MEDIAN, median_factor=4.0),
            "one-to-one": opt(one_to_one=1), "one-to-one + trimmed 0.7": opt(one_to_one=1, distance=TRIMMED, overlap_ratio=0.7)}


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


# ---------------------------------------------------------------- the restatement
def max_d2_of(max_corr):
    """The largest float d2 the ICP accepts: the largest float not above max_corr^2 (in double)."""
    m = np.float32(max_corr * max_corr)
    if float(m) > max_corr * max_corr:
        m = np.nextafter(m, np.float32(-np.inf))
    return m


def restate_rejection(idx, d2, o, max_d2):
    """Steps 1 - 3 of the rule for one iteration.  idx / d2: every source point's nearest target point and float d2 in the
    caller's order (-1 / +inf: none).  Returns (kept mask, stats dict, rank gap): the rank gap is the smallest relative distance of
    the threshold's two rank neighbours from it (inf where there is no threshold).  A neighbour that EQUALS the threshold bit for
    bit is a tie, which the rule keeps whole, and does not count: on a noise-free scene the last iteration's d2 are rounding
    residue (1e-13) with dozens of exact repeats, +0 among them, so a gap that counted ties would be 0 for every seed."""
    idx = np.asarray(idx, dtype=np.int64)
    d2 = np.asarray(d2, dtype=np.float32)
    matched = (idx >= 0) & (d2 <= max_d2)
    surv = matched.copy()
    if o.one_to_one:
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(idx), dtype=np.uint64)
        m = np.flatnonzero(matched)
        order = m[np.lexsort((key[m], idx[m]))]                      # by target, then by key
        first = np.r_[True, idx[order][1:] != idx[order][:-1]] if len(order) else np.zeros(0, dtype=bool)
        surv = np.zeros(len(idx), dtype=bool)
        surv[order[first]] = True
    n = int(surv.sum())
    sd = np.sort(d2[surv])
    kept, thr, gap = surv.copy(), np.float32(np.inf), np.inf
    rank = None
    if o.distance == TRIMMED:
        k = max(int(o.min_correspondences), int(o.overlap_ratio * float(n)))
        if k >= n:
            pass
        elif k == 0:
            kept, thr = np.zeros(len(idx), dtype=bool), np.float32(-1.0)
        else:
            rank = k - 1
            thr = sd[rank]
            kept = surv & (d2 <= thr)
    elif o.distance == MEDIAN and n > 0:
        rank = n // 2
        thr = sd[rank]
        kept = surv & (d2.astype(np.float64) <= float(thr) * o.median_factor)
    if rank is not None:
        near = [float(sd[r]) for r in (rank - 1, rank + 1) if 0 <= r < n and sd[r] != thr]
        gap = min([abs(v - float(thr)) / max(float(thr), 1e-300) for v in near], default=np.inf)
    stats = dict(matched=int(matched.sum()), after_one_to_one=n, kept=int(kept.sum()), threshold_d2=np.float32(thr))
    return kept, stats, gap


def _umeyama(p, q):
    """k_icp_finalize's estimate: the rigid transform of the double moments, R rounded to float before t is formed."""
    mp, mq = p.mean(axis=0), q.mean(axis=0)
    sigma = (q.T @ p) / len(p) - np.outer(mq, mp)
    U, _, Vt = np.linalg.svd(sigma)
    S = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0 else -1.0])
    R = (U @ S @ Vt).astype(np.float32)
    Ti = np.eye(4, dtype=np.float32)
    Ti[:3, :3] = R
    Ti[:3, 3] = (mq - R.astype(np.float64) @ mp).astype(np.float32)
    return Ti


def restate_icp_rejecting(src, tgt, nrm, guess, max_corr, max_iter, eps, o, tau=1e-12):
    """The whole loop in numpy: float32 transforms and distances, the rejection above, double sums over the kept
    correspondences, the point-to-point (nrm None) or point-to-plane estimate, DefaultConvergenceCriteria.  Non-finite source
    points match nothing.  Returns (T, iterations, converged, margins, smallest rank gap, last iteration's stats)."""
    max_d2 = max_d2_of(max_corr)
    T = np.asarray(guess, dtype=np.float32).copy()
    fin = np.isfinite(src).all(axis=1)
    prev_mse, iters, margins, min_gap, stats = np.finfo(np.float64).max, 0, [], np.inf, None
    while True:
        s = _xform_f32(T, src)
        idx = np.full(len(src), -1, dtype=np.int64)
        d2 = np.full(len(src), np.inf, dtype=np.float32)
        idx[fin], d2[fin] = _nearest(s[fin], tgt)
        kept, stats, gap = restate_rejection(idx, d2, o, max_d2)
        min_gap = min(min_gap, gap)
        cnt = int(kept.sum())
        if cnt < 3:
            return T, iters, 0, margins, min_gap, stats
        sd, d = s[kept].astype(np.float64), tgt[idx[kept]].astype(np.float64)
        if nrm is None:
            Ti = _umeyama(sd, d)
        else:
            n = nrm[idx[kept]].astype(np.float64)
            ok = np.isfinite(n).all(axis=1)
            sr, dr, n = sd[ok], d[ok], n[ok]
            sx, sy, sz = sr[:, 0], sr[:, 1], sr[:, 2]
            nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
            A = np.stack([nz * sy - ny * sz, nx * sz - nz * sx, ny * sx - nx * sy, nx, ny, nz], axis=1)
            r = (nx * dr[:, 0] + ny * dr[:, 1] + nz * dr[:, 2]) - (nx * sx + ny * sy + nz * sz)
            AtA, Atr = A.T @ A, A.T @ r
            floor = tau * np.trace(AtA) / 6.0
            x, pivots = _ldlt_solve(AtA, Atr, floor) if len(A) >= 6 else (None, [])
            margins += [abs(p - floor) / max(abs(floor), 1e-300) for p in pivots]
            if x is None:
                return T, iters, 0, margins, min_gap, stats
            Ti = construct_transform(*x).astype(np.float32)
        Tn = np.zeros((4, 4), dtype=np.float32)
        for rr in range(4):
            for c in range(4):
                a = np.float32(0.0)
                for k in range(4):
                    a = np.float32(a + Ti[rr, k] * T[k, c])
                Tn[rr, c] = a
        T = Tn
        iters += 1
        if iters >= max_iter:
            return T, iters, 1, margins, min_gap, stats
        cos_angle = 0.5 * ((float(Ti[0, 0]) + float(Ti[1, 1]) + float(Ti[2, 2])) - 1.0)
        t2 = float(Ti[0, 3]) * float(Ti[0, 3]) + float(Ti[1, 3]) * float(Ti[1, 3]) + float(Ti[2, 3]) * float(Ti[2, 3])
        margins += [abs((1.0 - cos_angle) - eps) / eps, abs(t2 - eps) / eps]
        if cos_angle >= 1.0 - eps and t2 <= eps:
            return T, iters, 1, margins, min_gap, stats
        mse = float(d2[kept].astype(np.float64).sum()) / cnt
        if iters > 1:                                   # (the first compares with DBL_MAX)
            margins.append(abs(abs(mse - prev_mse) - 1e-12) / 1e-12)
        if abs(mse - prev_mse) < 1e-12:
            return T, iters, 1, margins, min_gap, stats
        prev_mse = mse


# ---------------------------------------------------------------- the cabinet scene
def cabinet(seed, n=3000):
    """_problem(seed, n) plus 1200 source-only points: a flat cabinet front 0.5 m before the target's wall x = 8."""
    tgt, nrm, src, T_true, guess = _problem(seed, n)
    rng = np.random.default_rng(seed + 500)
    cab = np.c_[np.full(1200, 7.5), rng.uniform(1, 5, 1200), rng.uniform(0, 2.5, 1200)]
    cab_src = (np.linalg.inv(T_true) @ np.c_[cab, np.ones(len(cab))].T).T[:, :3].astype(np.float32)
    return tgt, nrm, np.concatenate([src, cab_src]), T_true, guess


# ---------------------------------------------------------------- surface
def test_header_declares_the_surface():
    h = _read("include", "mm3d.h")
    assert re.search(r"typedef enum \{ MM3D_REJECT_NONE = 0, MM3D_REJECT_TRIMMED = 1, MM3D_REJECT_MEDIAN = 2 \} mm3d_reject_distance;", h)
    assert re.search(r"typedef struct mm3d_icp_rejection_options \{\s*int one_to_one;[^}]*int distance;[^}]*double overlap_ratio;"
                     r"[^}]*int min_correspondences;[^}]*double median_factor;[^}]*\} mm3d_icp_rejection_options;", h)
    assert re.search(r"typedef struct mm3d_icp_rejection_stats \{[^}]*long long matched;[^}]*long long after_one_to_one;[^}]*long long kept;"
                     r"[^}]*float threshold_d2;[^}]*int iterations, converged;\s*\} mm3d_icp_rejection_stats;", h)
    for decl in (r"void mm3d_icp_rejection_options_default\(mm3d_icp_rejection_options \*o\);",
                 r"int mm3d_set_icp_rejection\(mm3d_ctx \*ctx, const mm3d_icp_rejection_options \*options\);",
                 r"int mm3d_get_icp_rejection\(const mm3d_ctx \*ctx, mm3d_icp_rejection_options \*options\);",
                 r"int mm3d_last_icp_rejection_stats\(const mm3d_ctx \*ctx, mm3d_icp_rejection_stats \*stats\);",
                 r"int mm3d_estimate_transform_icp_rejecting\(mm3d_ctx \*ctx, const mm3d_cloud \*source, const mm3d_cloud \*target,",
                 r"int mm3d_debug_icp_rejection\(mm3d_ctx \*ctx, const mm3d_cloud \*source, const mm3d_cloud \*target, const float T\[16\],",
                 r"int mm3d_debug_icp_rejection_split\(int split\);"):
        assert re.search(decl, h), decl


def test_library_exports_and_mirror_binds(mm):
    lib = mm.lib()
    for name in ("mm3d_icp_rejection_options_default", "mm3d_set_icp_rejection", "mm3d_get_icp_rejection", "mm3d_last_icp_rejection_stats",
                 "mm3d_estimate_transform_icp_rejecting", "mm3d_debug_icp_rejection", "mm3d_debug_icp_rejection_split"):
        assert getattr(lib, name)
    for name in ("setIcpRejection", "getIcpRejection", "estimateTransformICPRejecting", "debugIcpRejection"):
        assert callable(getattr(mm.Context, name))
    assert isinstance(mm.Context.last_icp_rejection_stats, property)
    assert (mm.RejectDistance.NONE, mm.RejectDistance.TRIMMED, mm.RejectDistance.MEDIAN) == (NONE, TRIMMED, MEDIAN)
    assert C.sizeof(mm.IcpRejectionOptions) == 32 and C.sizeof(mm.IcpRejectionStats) == 40


def test_defaults_and_null_handling(mm):
    o = mm.IcpRejectionOptions()
    assert o.as_tuple() == tuple(DEFAULT)
    lib = mm.lib()
    lib.mm3d_icp_rejection_options_default(None)          # a no-op, not a crash
    st = mm.IcpRejectionStats()
    T = (C.c_float * 16)()
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    assert lib.mm3d_set_icp_rejection(None, C.byref(o)) == EINVAL and lib.mm3d_set_icp_rejection(fake, None) == EINVAL
    assert lib.mm3d_get_icp_rejection(None, C.byref(o)) == EINVAL and lib.mm3d_get_icp_rejection(fake, None) == EINVAL
    assert lib.mm3d_last_icp_rejection_stats(None, C.byref(st)) == EINVAL and lib.mm3d_last_icp_rejection_stats(fake, None) == EINVAL
    assert lib.mm3d_estimate_transform_icp_rejecting(fake, None, None, None, T, C.c_double(1.0), C.byref(o), 10, C.c_double(0.0), T, None) == EINVAL
    assert lib.mm3d_estimate_transform_icp_rejecting(fake, fake, fake, None, T, C.c_double(1.0), None, 10, C.c_double(0.0), T, None) == EINVAL
    assert lib.mm3d_debug_icp_rejection(fake, None, None, T, C.c_double(1.0), C.byref(o), 1, None, None, None, None) == EINVAL
    assert lib.mm3d_debug_icp_rejection(fake, fake, fake, T, C.c_double(1.0), C.byref(o), 2, None, None, None, None) == EINVAL   # split
    # the split hook: negative asks, anything but 0 / 1 / 4 changes nothing
    assert lib.mm3d_debug_icp_rejection_split(-1) == 0
    assert lib.mm3d_debug_icp_rejection_split(3) == 0


BAD = [dict(one_to_one=2), dict(one_to_one=-1), dict(distance=-1), dict(distance=3), dict(overlap_ratio=0.0), dict(overlap_ratio=-0.5),
       dict(overlap_ratio=1.5), dict(overlap_ratio=float("nan")), dict(min_correspondences=-1), dict(median_factor=0.0),
       dict(median_factor=-1.0), dict(median_factor=float("inf")), dict(median_factor=float("nan"))]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
@pytest.mark.parametrize("distance", [NONE, TRIMMED, MEDIAN])
def test_out_of_range_options_are_refused_whatever_the_selection(mm, bad, distance):
    """The check comes before anything touches a device or the handle: a context that is never dereferenced shows it."""
    o = mm.IcpRejectionOptions(**{"distance": distance, **bad})
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)      # never read: the options are checked first
    T = (C.c_float * 16)()
    assert mm.lib().mm3d_set_icp_rejection(fake, C.byref(o)) == EINVAL
    assert mm.lib().mm3d_estimate_transform_icp_rejecting(fake, fake, fake, None, T, C.c_double(1.0), C.byref(o), 10, C.c_double(0.0), T, None) == EINVAL


SHIM_CASES = r"""
#include <cstdio>
#include <cstring>
#include "map_merge_3d_shim.hpp"
using map_merge_3d::mm3d_shim::parse_icp_reject;
using map_merge_3d::mm3d_shim::check_icp_reject_devices;
static int refused(const char *v) { try { (void)parse_icp_reject(v); } catch (const std::runtime_error &e) { return std::strstr(e.what(), "MM3D_ICP_REJECT") != nullptr; } return 0; }
static int devices_refused(const char *v, const char *d) { try { check_icp_reject_devices(parse_icp_reject(v), d); } catch (const std::runtime_error &) { return 1; } return 0; }
static int is(const mm3d_icp_rejection_options &o, int one, int dist, double ratio, int minc, double factor)
{
  return o.one_to_one == one && o.distance == dist && o.overlap_ratio == ratio && o.min_correspondences == minc && o.median_factor == factor;
}
int main()
{
  if (!is(parse_icp_reject(nullptr), 0, MM3D_REJECT_NONE, 0.5, 0, 1.0)) return 1;
  if (!is(parse_icp_reject(""), 0, MM3D_REJECT_NONE, 0.5, 0, 1.0) || !is(parse_icp_reject("none"), 0, MM3D_REJECT_NONE, 0.5, 0, 1.0)) return 2;
  if (!is(parse_icp_reject("one_to_one"), 1, MM3D_REJECT_NONE, 0.5, 0, 1.0)) return 3;
  if (!is(parse_icp_reject("trimmed"), 0, MM3D_REJECT_TRIMMED, 0.5, 0, 1.0) || !is(parse_icp_reject("trimmed:0.7"), 0, MM3D_REJECT_TRIMMED, 0.7, 0, 1.0)) return 4;
  if (!is(parse_icp_reject("trimmed:1"), 0, MM3D_REJECT_TRIMMED, 1.0, 0, 1.0)) return 5;
  if (!is(parse_icp_reject("median"), 0, MM3D_REJECT_MEDIAN, 0.5, 0, 1.0) || !is(parse_icp_reject("median:4"), 0, MM3D_REJECT_MEDIAN, 0.5, 0, 4.0)) return 6;
  if (!is(parse_icp_reject("one_to_one+trimmed:0.7"), 1, MM3D_REJECT_TRIMMED, 0.7, 0, 1.0)) return 7;
  if (!is(parse_icp_reject("median:1.5+one_to_one"), 1, MM3D_REJECT_MEDIAN, 0.5, 0, 1.5)) return 8;
  const char *bad[] = {"trimmed+median", "median:2+trimmed:0.5", "trimmed+trimmed", "one_to_one+one_to_one", "one_to_one:1", "trimmed:", "trimmed:0",
                       "trimmed:1.5", "trimmed:-0.2", "trimmed:abc", "trimmed:0.7x", "median:0", "median:-1", "median:inf", "median:nan", "sorted",
                       "Trimmed", "one_to_one+", "+one_to_one", "one_to_one++median", "none+trimmed", " trimmed", "trimmed:0.7 "};
  for (const char *b : bad) if (!refused(b)) { std::printf("accepted '%s'\n", b); return 9; }
  if (!devices_refused("one_to_one", "0,1") || !devices_refused("trimmed:0.7", "all") || !devices_refused("median", "0")) return 10;
  if (devices_refused("trimmed", nullptr) || devices_refused("trimmed", "") || devices_refused("none", "0,1") || devices_refused(nullptr, "0,1")) return 11;
  std::puts("shim icp reject: ok");
  return 0;
}
"""


def test_shim_parses_mm3d_icp_reject(tmp_path):
    """Compiled with the flags tests/shim/build.sh compiles the shim with; the parser lies outside the header's PCL guard."""
    src = tmp_path / "shim_icp_reject.cpp"
    src.write_text(SHIM_CASES)
    exe = tmp_path / "shim_icp_reject"
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0 and "shim icp reject: ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    s = _read("include", "map_merge_3d_shim.hpp")
    assert 'parse_icp_reject(std::getenv("MM3D_ICP_REJECT"))' in s and "mm3d_set_icp_rejection(e, &reject)" in s
    assert 'check_icp_reject_devices(reject, std::getenv("MM3D_DEVICES"))' in s
    # the parser's defaults are the library's
    assert "0, NONE, 0.5, 0, 1.0" in _read("include", "mm3d.h")


# ---------------------------------------------------------------- the restatement against literal vectors
F = np.float32
MAX_D2 = F(1.0)


def test_one_to_one_key_literal():
    # target 5 is shared by sources 0, 2 and 3: 2 and 3 tie on d2 (the lower index wins); target 7 by 1 and 4; source 5 is alone,
    # source 6 has no match, source 7 is beyond max_d2
    idx = [5, 7, 5, 5, 7, 9, -1, 9]
    d2 = np.array([0.5, 0.25, 0.125, 0.125, 0.0, 1.0, np.inf, 1.5], dtype=F)
    kept, st, _ = restate_rejection(idx, d2, opt(one_to_one=1), MAX_D2)
    assert kept.tolist() == [False, False, True, False, True, True, False, False]
    assert (st["matched"], st["after_one_to_one"], st["kept"]) == (6, 3, 3) and np.isinf(st["threshold_d2"])
    # a smaller d2 beats a smaller index: the key's high word is the distance
    kept, _, _ = restate_rejection([3, 3], np.array([0.5, 0.25], dtype=F), opt(one_to_one=1), MAX_D2)
    assert kept.tolist() == [False, True]
    # +0 keys order below every positive distance
    kept, _, _ = restate_rejection([3, 3, 3], np.array([1e-30, 0.0, 0.0], dtype=F), opt(one_to_one=1), MAX_D2)
    assert kept.tolist() == [False, True, False]


def test_trimmed_k_and_ties_literal():
    idx = np.arange(10)
    d2 = np.array([0.9, 0.1, 0.2, 0.3, 0.3, 0.3, 0.4, 0.5, 0.0, 0.8], dtype=F)
    # k = (long long)(0.4 * 10) = 4: tau = the 4th smallest = 0.3, and the three 0.3 are all kept: kept = 6 >= k
    kept, st, gap = restate_rejection(idx, d2, opt(distance=TRIMMED, overlap_ratio=0.4), MAX_D2)
    assert st["threshold_d2"] == F(0.3) and st["kept"] == 6
    assert abs(gap - (0.3 - 0.2) / 0.3) < 1e-6            # (rank neighbours 0.2 and 0.3: the tie does not count)
    assert kept.tolist() == [False, True, True, True, True, True, False, False, True, False]
    # truncation, not rounding: 0.39 * 10 = 3.9 -> 3
    _, st, _ = restate_rejection(idx, d2, opt(distance=TRIMMED, overlap_ratio=0.39), MAX_D2)
    assert st["threshold_d2"] == F(0.2) and st["kept"] == 3
    # ratio 1.0: k = n, nothing is cut
    _, st, _ = restate_rejection(idx, d2, opt(distance=TRIMMED, overlap_ratio=1.0), MAX_D2)
    assert st["kept"] == 10 and np.isinf(st["threshold_d2"])
    # min_correspondences lifts k: above n nothing is cut, below n it is the rank
    _, st, _ = restate_rejection(idx, d2, opt(distance=TRIMMED, overlap_ratio=0.1, min_correspondences=50), MAX_D2)
    assert st["kept"] == 10 and np.isinf(st["threshold_d2"])
    _, st, _ = restate_rejection(idx, d2, opt(distance=TRIMMED, overlap_ratio=0.1, min_correspondences=2), MAX_D2)
    assert st["kept"] == 2 and st["threshold_d2"] == F(0.1)
    # k = 0: everything is cut
    kept, st, _ = restate_rejection(idx, d2, opt(distance=TRIMMED, overlap_ratio=0.05), MAX_D2)
    assert st["kept"] == 0 and not kept.any() and st["threshold_d2"] == F(-1.0) and st["after_one_to_one"] == 10
    # nothing matched: k = 0 >= n = 0, nothing is cut, +inf
    _, st, _ = restate_rejection([-1, -1], np.array([np.inf, np.inf], dtype=F), opt(distance=TRIMMED, overlap_ratio=0.5), MAX_D2)
    assert (st["matched"], st["kept"]) == (0, 0) and np.isinf(st["threshold_d2"])


def test_median_rank_literal():
    # even n: rank n / 2 = 2 of [0.1, 0.2, 0.3, 0.4] is 0.3 (the upper median)
    d2 = np.array([0.4, 0.1, 0.3, 0.2], dtype=F)
    kept, st, _ = restate_rejection(np.arange(4), d2, opt(distance=MEDIAN, median_factor=1.0), MAX_D2)
    assert st["threshold_d2"] == F(0.3) and kept.tolist() == [False, True, True, True]
    # odd n: rank 2 of five
    d2 = np.array([0.5, 0.1, 0.3, 0.2, 0.9], dtype=F)
    kept, st, _ = restate_rejection(np.arange(5), d2, opt(distance=MEDIAN, median_factor=2.0), MAX_D2)
    assert st["threshold_d2"] == F(0.3) and kept.tolist() == [True, True, True, True, False]      # 0.5 <= 0.6 < 0.9
    # the product is taken in double: float(0.3f) * 3 is above float(0.9f) by an ulp of float, so 0.9f is kept
    kept, _, _ = restate_rejection(np.arange(5), d2, opt(distance=MEDIAN, median_factor=3.0), MAX_D2)
    assert bool(kept[4]) == (float(F(0.9)) <= float(F(0.3)) * 3.0)
    # one-to-one comes first: the median is over the survivors
    kept, st, _ = restate_rejection([1, 1, 2, 3], np.array([0.5, 0.1, 0.2, 0.3], dtype=F), opt(one_to_one=1, distance=MEDIAN), MAX_D2)
    assert st["after_one_to_one"] == 3 and st["threshold_d2"] == F(0.2) and kept.tolist() == [False, True, True, False]


# ---------------------------------------------------------------- the cabinet scene is honest before the GPU sees it
@pytest.fixture(scope="module", params=[7, 8, 9])
def scene(request):
    return cabinet(request.param)


def _err(T, T_true):
    return float(np.abs(T.astype(np.float64) - T_true).max())


def test_cabinet_shape(scene):
    tgt, nrm, src, _, _ = scene
    assert len(tgt) == 3000 and len(src) == 4200 and src.dtype == np.float32


def test_plain_icp_is_pulled_off_by_the_cabinet(scene):
    """0.2 is 60 % of the smallest error measured for plain ICP (0.327)."""
    tgt, _, src, T_true, guess = scene
    T, _, _, _, _, st = restate_icp_rejecting(src, tgt, None, guess, 1.0, 50, 1e-10, DEFAULT)
    assert _err(T, T_true) > 0.2, _err(T, T_true)
    assert st["kept"] == st["matched"] and np.isinf(st["threshold_d2"])


@pytest.mark.parametrize("name", list(VARIANTS))
def test_every_rejecting_variant_recovers_the_pose(scene, name):
    """1e-5 is 15 x the largest error measured for a rejecting variant (below 7e-7)."""
    tgt, _, src, T_true, guess = scene
    T, iters, conv, _, _, _ = restate_icp_rejecting(src, tgt, None, guess, 1.0, 50, 1e-10, VARIANTS[name])
    assert conv == 1 and iters < 50
    assert _err(T, T_true) < 1e-5, _err(T, T_true)

"""The overlap confidence without a GPU: the header declares it, the library exports it and the ctypes mirror binds it, the
defaults, the NULL and range handling of the entry points that touch no device, the shim's MM3D_CONFIDENCE, and the numpy
restatement of include/mm3d.h's rule -- the one tests/test_gpu_confidence.py holds the device to, integer for integer --
against literal vectors and on a planted split room."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_icp_plane import _xform_f32, box_room

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
REFERENCE, OVERLAP = 0, 1
INDEX_LIMIT = np.float32(2.0 ** 30)


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


# ---------------------------------------------------------------- the restatement (also read by test_gpu_confidence.py)
def voxel_of(xyz, voxel):
    """(int)floorf(x * inv) with inv = 1.0f / (float)voxel, every step one float operation."""
    inv = np.float32(1.0) / np.float32(voxel)
    return np.floor((np.asarray(xyz, dtype=np.float32) * inv).astype(np.float32)).astype(np.int64)


_FIELD = 1 << 20          # the restatement keys a voxel as three 21-bit fields: every table here lies far inside


def _key(v):
    v = np.asarray(v, dtype=np.int64).reshape(-1, 3)
    inside = (np.abs(v) < _FIELD - 2).all(axis=1)
    k = ((v[:, 0] + _FIELD) << 42) | ((v[:, 1] + _FIELD) << 21) | (v[:, 2] + _FIELD)
    return np.where(inside, k, -1)


_OFF27 = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.int64)


class Table:
    """The table of a map as sets: occ / near voxels, cnt per view cell, seen / view cells; and its dense form."""

    def __init__(self, pts, voxel, min_points=8, view_margin=0):
        pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
        self.voxel, self.min_points, self.view_margin = voxel, min_points, view_margin
        fin = pts[np.isfinite(pts).all(axis=1)]
        self.n_finite = len(fin)
        v = voxel_of(fin, voxel)
        assert (_key(v) >= 0).all()
        self.occ = np.unique(v, axis=0).reshape(-1, 3)
        self.near = np.unique((self.occ[:, None, :] + _OFF27[None]).reshape(-1, 3), axis=0)
        cells, cnt = np.unique(v >> 3, axis=0, return_counts=True)
        self.cnt = {tuple(int(x) for x in c): int(n) for c, n in zip(cells.reshape(-1, 3), cnt)}
        self.seen = cells.reshape(-1, 3)[cnt >= min_points]
        self.view = np.unique((self.seen[:, None, :] + _OFF27[None]).reshape(-1, 3), axis=0) if view_margin else self.seen
        self._near_keys = np.sort(_key(self.near))
        self._view_keys = np.sort(_key(self.view))
        if self.n_finite:
            # the boxes, from the voxels of the bounding box's corners (floorf(x * inv) is monotone)
            v_lo, v_hi = voxel_of(fin.min(axis=0), voxel), voxel_of(fin.max(axis=0), voxel)
            assert np.array_equal(v_lo, v.min(axis=0)) and np.array_equal(v_hi, v.max(axis=0))
            self.b0 = (v_lo - 1) >> 2
            b1 = (v_hi + 1) >> 2
            self.nb = b1 - self.b0 + 1
            self.c0 = (self.b0 >> 1) - view_margin
            self.nc = ((b1 >> 1) + view_margin) - self.c0 + 1
        else:
            self.b0 = self.nb = self.c0 = self.nc = np.zeros(3, dtype=np.int64)

    def has_near(self, v):
        return np.isin(_key(v), self._near_keys) & (_key(v) >= 0)

    def has_view(self, c):
        return np.isin(_key(c), self._view_keys) & (_key(c) >= 0)

    def dense(self):
        """(words uint64 [nb], view uint8 [nc]) as mm3d_debug_overlap_table lays them out."""
        words = np.zeros(tuple(int(x) for x in self.nb), dtype=np.uint64)
        view = np.zeros(tuple(int(x) for x in self.nc), dtype=np.uint8)
        if self.n_finite:
            b = (self.near >> 2) - self.b0
            assert (b >= 0).all() and (b < self.nb).all()
            bit = (self.near[:, 0] & 3) | ((self.near[:, 1] & 3) << 2) | ((self.near[:, 2] & 3) << 4)
            np.bitwise_or.at(words, (b[:, 0], b[:, 1], b[:, 2]), np.uint64(1) << bit.astype(np.uint64))
            c = self.view - self.c0
            assert (c >= 0).all() and (c < self.nc).all()
            view[c[:, 0], c[:, 1], c[:, 2]] = 1
        return words, view


def inverse_rule(T):
    """R' = R^T, t'_r = -((R_0r t_0 + R_1r t_1) + R_2r t_2) in double from T's float entries, rounded to float once."""
    T = np.asarray(T, dtype=np.float32).astype(np.float64)
    out = np.zeros((4, 4))
    out[:3, :3] = T[:3, :3].T
    for r in range(3):
        out[r, 3] = -((T[0, r] * T[0, 3] + T[1, r] * T[1, 3]) + T[2, r] * T[2, 3])
    out[3, 3] = 1.0
    return out.astype(np.float32)


def count_direction(a_pts, M, b_table):
    """(in, hit) of the finite points of A under the float matrix M against B's table."""
    p = np.asarray(a_pts, dtype=np.float32).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    inv = np.float32(1.0) / np.float32(b_table.voxel)
    with np.errstate(all="ignore"):
        f = (_xform_f32(np.asarray(M, dtype=np.float32), p) * inv).astype(np.float32)
        ok = (np.abs(f) < INDEX_LIMIT).all(axis=1)               # false for NaN and infinities
    v = np.floor(f[ok]).astype(np.int64)
    inside = b_table.has_view(v >> 3)
    hit = inside & b_table.has_near(v)
    return int(inside.sum()), int(hit.sum())


def confidence_of(n_s, in_st, hit_st, n_t, in_ts, hit_ts, min_overlap):
    if in_st == 0 or in_ts == 0 or float(in_st) < min_overlap * float(n_s) or float(in_ts) < min_overlap * float(n_t):
        return 0.0
    return min(float(hit_st) / float(in_st), float(hit_ts) / float(in_ts))


def restate_overlap(src, tgt, T, voxel, min_points=8, min_overlap=0.05, view_margin=0, tables=None):
    """mm3d_transform_overlap in numpy: the dict of mm3d_overlap_stats.  T is the 4 x 4 matrix (row, column)."""
    ts, tt = tables if tables is not None else (Table(src, voxel, min_points, view_margin), Table(tgt, voxel, min_points, view_margin))
    T = np.asarray(T, dtype=np.float32).reshape(4, 4)
    out = dict(points_st=ts.n_finite, in_st=0, hit_st=0, points_ts=tt.n_finite, in_ts=0, hit_ts=0, confidence=0.0)
    if np.isfinite(T).all() and T.any():
        out["in_st"], out["hit_st"] = count_direction(src, T, tt)
        out["in_ts"], out["hit_ts"] = count_direction(tgt, inverse_rule(T), ts)
    out["confidence"] = confidence_of(out["points_st"], out["in_st"], out["hit_st"], out["points_ts"], out["in_ts"], out["hit_ts"], min_overlap)
    return out


# ---------------------------------------------------------------- surface
def test_header_declares_the_surface():
    h = _read("include", "mm3d.h")
    assert re.search(r"typedef enum \{ MM3D_CONFIDENCE_REFERENCE = 0, MM3D_CONFIDENCE_OVERLAP = 1 \} mm3d_confidence_method;", h)
    assert re.search(r"typedef struct mm3d_confidence_options \{\s*int method;[^}]*double voxel;[^}]*int min_points;[^}]*double min_overlap;"
                     r"[^}]*int view_margin;[^}]*\} mm3d_confidence_options;", h)
    assert re.search(r"typedef struct mm3d_overlap_stats \{\s*long long points_st, in_st, hit_st;[^}]*long long points_ts, in_ts, hit_ts;"
                     r"[^}]*double confidence;\s*\} mm3d_overlap_stats;", h)
    for decl in (r"void mm3d_confidence_options_default\(mm3d_confidence_options \*o\);",
                 r"int mm3d_set_confidence\(mm3d_ctx \*ctx, const mm3d_confidence_options \*options\);",
                 r"int mm3d_get_confidence\(const mm3d_ctx \*ctx, mm3d_confidence_options \*options\);",
                 r"int mm3d_last_confidence_stats\(const mm3d_ctx \*ctx, mm3d_overlap_stats \*stats\);",
                 r"int mm3d_transform_overlap\(mm3d_ctx \*ctx, const mm3d_cloud \*source, const mm3d_cloud \*target, const float T\[16\],",
                 r"int mm3d_debug_overlap_table\(mm3d_ctx \*ctx, const mm3d_cloud \*cloud, const mm3d_confidence_options \*options, int box\[12\],"):
        assert re.search(decl, h), decl
    # the header says where the number lives, and what that does to the threshold
    assert "LIVES IN [0, 1]" in h and re.search(r"confidence_threshold is then a fraction", h)
    assert "2^30" in h and "2^24" in h


def test_library_exports_and_mirror_binds(mm):
    lib = mm.lib()
    for name in ("mm3d_confidence_options_default", "mm3d_set_confidence", "mm3d_get_confidence", "mm3d_last_confidence_stats",
                 "mm3d_transform_overlap", "mm3d_debug_overlap_table"):
        assert getattr(lib, name)
    for name in ("setConfidence", "getConfidence", "lastConfidenceStats", "transformOverlap", "debugOverlapTable"):
        assert callable(getattr(mm.Context, name))
    assert (mm.ConfidenceMethod.REFERENCE, mm.ConfidenceMethod.OVERLAP) == (REFERENCE, OVERLAP)
    assert C.sizeof(mm.OverlapStats) == 56 and C.sizeof(mm.ConfidenceOptions) == 40


def test_defaults_and_null_handling(mm):
    o = mm.ConfidenceOptions()
    assert o.as_tuple() == (REFERENCE, 0.0, 8, 0.05, 0)
    lib = mm.lib()
    lib.mm3d_confidence_options_default(None)             # a no-op, not a crash
    st = mm.OverlapStats()
    T = (C.c_float * 16)()
    box = (C.c_int * 12)()
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    assert lib.mm3d_set_confidence(None, C.byref(o)) == EINVAL and lib.mm3d_set_confidence(fake, None) == EINVAL
    assert lib.mm3d_get_confidence(None, C.byref(o)) == EINVAL and lib.mm3d_get_confidence(fake, None) == EINVAL
    assert lib.mm3d_last_confidence_stats(None, C.byref(st)) == EINVAL and lib.mm3d_last_confidence_stats(fake, None) == EINVAL
    assert lib.mm3d_transform_overlap(None, None, None, T, C.byref(o), C.byref(st)) == EINVAL
    assert lib.mm3d_debug_overlap_table(None, None, C.byref(o), box, None, C.c_size_t(0), None, C.c_size_t(0)) == EINVAL
    # the stage-level calls want a voxel of their own: 0 is refused before the handles are read
    assert lib.mm3d_transform_overlap(fake, fake, fake, T, C.byref(o), C.byref(st)) == EINVAL
    assert lib.mm3d_debug_overlap_table(fake, fake, C.byref(o), box, None, C.c_size_t(0), None, C.c_size_t(0)) == EINVAL


BAD = [dict(method=-1), dict(method=2), dict(voxel=-0.1), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(voxel=1e-45),
       dict(min_points=0), dict(min_points=-3), dict(min_overlap=1.5), dict(min_overlap=-0.01), dict(min_overlap=float("nan")),
       dict(view_margin=2), dict(view_margin=-1)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
@pytest.mark.parametrize("method", [REFERENCE, OVERLAP])
def test_out_of_range_options_are_refused_whatever_the_method(mm, bad, method):
    """The check comes before anything touches a device or the handle: a context that is never dereferenced shows it."""
    o = mm.ConfidenceOptions(**{"method": method, **bad})
    fake = C.create_string_buffer(1 << 16)                 # never read: the options are checked first
    assert mm.lib().mm3d_set_confidence(C.cast(fake, C.c_void_p), C.byref(o)) == EINVAL


SHIM_CASES = r"""
#include <cstdio>
#include <cstring>
#include "map_merge_3d_shim.hpp"
using map_merge_3d::mm3d_shim::parse_confidence;
using map_merge_3d::mm3d_shim::check_confidence_devices;
static int refused(const char *v) { try { (void)parse_confidence(v); } catch (const std::runtime_error &e) { return std::strstr(e.what(), "MM3D_CONFIDENCE") != nullptr; } return 0; }
static int devices_refused(const char *v, const char *d) { try { check_confidence_devices(parse_confidence(v), d); } catch (const std::runtime_error &e) { return std::strstr(e.what(), "MM3D_DEVICES") != nullptr; } return 0; }
int main()
{
  mm3d_confidence_options o = parse_confidence(nullptr);
  if (o.method != MM3D_CONFIDENCE_REFERENCE || o.voxel != 0.0 || o.min_points != 8 || o.min_overlap != 0.05 || o.view_margin != 0) return 1;
  o = parse_confidence("");
  if (o.method != MM3D_CONFIDENCE_REFERENCE) return 2;
  o = parse_confidence("none");
  if (o.method != MM3D_CONFIDENCE_REFERENCE) return 3;
  o = parse_confidence("overlap");
  if (o.method != MM3D_CONFIDENCE_OVERLAP || o.voxel != 0.0 || o.min_points != 8 || o.min_overlap != 0.05 || o.view_margin != 0) return 4;
  o = parse_confidence("overlap:0.2");
  if (o.method != MM3D_CONFIDENCE_OVERLAP || o.voxel != 0.2) return 5;
  const char *bad[] = {"garbage", "overlap:", "overlap:abc", "overlap:0.2m", "overlap:-1", "overlap:0", "overlap:nan", "overlap:inf",
                       "overlapping", "Overlap", "reference"};
  for (const char *b : bad) if (!refused(b)) { std::printf("accepted '%s'\n", b); return 6; }
  if (!devices_refused("overlap", "0,1") || !devices_refused("overlap:0.2", "all")) return 7;
  if (devices_refused("overlap", nullptr) || devices_refused("overlap", "") || devices_refused("none", "0,1")) return 8;
  std::puts("shim confidence: ok");
  return 0;
}
"""


def test_shim_parses_mm3d_confidence(tmp_path):
    """Compiled with the flags tests/shim/build.sh compiles the shim with; the parser lies outside the header's PCL guard."""
    src = tmp_path / "shim_confidence.cpp"
    src.write_text(SHIM_CASES)
    exe = tmp_path / "shim_confidence"
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0 and "shim confidence: ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    s = _read("include", "map_merge_3d_shim.hpp")
    assert 'parse_confidence(std::getenv("MM3D_CONFIDENCE"))' in s and "mm3d_set_confidence(e, &confidence)" in s
    assert 'check_confidence_devices(confidence, std::getenv("MM3D_DEVICES"))' in s
    # the parser's defaults are the library's
    assert "REFERENCE, 0, 8, 0.05, 0" in _read("include", "mm3d.h")


# ---------------------------------------------------------------- the restatement against literal vectors
def _bits(word):
    return {b for b in range(64) if (int(word) >> b) & 1}


def test_one_point_dilates_over_eight_bricks():
    t = Table(np.array([[0.05, 0.05, 0.05]], dtype=np.float32), 0.1, min_points=1)
    assert t.occ.tolist() == [[0, 0, 0]]
    assert sorted(map(tuple, t.near.tolist())) == sorted((i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1))
    assert t.b0.tolist() == [-1, -1, -1] and t.nb.tolist() == [2, 2, 2]
    words, view = t.dense()
    assert _bits(words[1, 1, 1]) == {0, 1, 4, 5, 16, 17, 20, 21}        # brick (0, 0, 0)
    assert _bits(words[0, 0, 0]) == {63}                                # brick (-1, -1, -1)
    assert _bits(words[0, 1, 1]) == {3, 7, 19, 23}                      # brick (-1, 0, 0): i = 3, j and k in {0, 1}
    assert _bits(words[1, 0, 1]) == {12, 13, 28, 29}                    # brick (0, -1, 0): j = 3
    assert _bits(words[1, 1, 0]) == {48, 49, 52, 53}                    # brick (0, 0, -1): k = 3
    assert _bits(words[0, 0, 1]) == {15, 31}                            # an edge: i = j = 3, k in {0, 1}
    assert sum(len(_bits(w)) for w in words.ravel()) == 27
    # view cells: the brick box touches cells -1 and 0 per axis; the point's cell (0, 0, 0) has one point
    assert t.c0.tolist() == [-1, -1, -1] and t.nc.tolist() == [2, 2, 2]
    assert view[1, 1, 1] == 1 and view.sum() == 1
    assert Table(np.array([[0.05, 0.05, 0.05]], dtype=np.float32), 0.1, min_points=2).dense()[1].sum() == 0
    m = Table(np.array([[0.05, 0.05, 0.05]], dtype=np.float32), 0.1, min_points=1, view_margin=1)
    assert m.c0.tolist() == [-2, -2, -2] and m.nc.tolist() == [4, 4, 4]
    assert m.dense()[1].sum() == 27 and m.dense()[1][1:, 1:, 1:].all()


def test_voxels_on_lattice_planes_and_negative_shifts():
    p = np.array([[0.0, -0.0, 1.0], [-1.0, -1e-7, 0.99999994], [2.5, -2.5, 3.0]], dtype=np.float32)
    v = voxel_of(p, 1.0)
    assert v.tolist() == [[0, 0, 1], [-1, -1, 0], [2, -3, 3]]
    assert (v >> 2).tolist() == [[0, 0, 0], [-1, -1, 0], [0, -1, 0]]   # arithmetic shift: floor division
    assert (np.array([-1, -4, -5, -8, -9, 7, 8]) >> 3).tolist() == [-1, -1, -1, -1, -2, 0, 1]


def test_inverse_rule_on_a_hand_made_transform():
    T = np.array([[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0], [0.0, 0.0, 0.0, 1.0]], dtype=np.float32)
    inv = inverse_rule(T)
    # R^T, and t' = -R^T t = -(2, -1, 3)
    assert inv.tolist() == [[0.0, 1.0, 0.0, -2.0], [-1.0, 0.0, 0.0, 1.0], [0.0, 0.0, 1.0, -3.0], [0.0, 0.0, 0.0, 1.0]]
    assert inv.dtype == np.float32
    # the order of the sum is the rule's: (a + b) + c in double, rounded once
    T = np.eye(4, dtype=np.float32)
    T[:3, 0] = [np.float32(0.1), np.float32(0.2), np.float32(0.3)]
    T[:3, 3] = [np.float32(1e8), np.float32(-1e8), np.float32(1.0)]
    a, b, c = float(np.float32(0.1)) * 1e8, float(np.float32(0.2)) * -1e8, float(np.float32(0.3)) * 1.0
    assert inverse_rule(T)[0, 3] == np.float32(-((a + b) + c))


def test_gate_at_exactly_min_overlap_times_n():
    # 10 / 40 points in view: the gate is `in < min_overlap * n`, so exactly 0.25 passes and anything above refuses
    assert confidence_of(40, 10, 5, 40, 10, 10, 0.25) == 0.5
    assert confidence_of(40, 10, 5, 40, 10, 10, np.nextafter(0.25, 1.0)) == 0.0
    assert confidence_of(40, 10, 5, 41, 10, 10, 0.25) == 0.0            # the other direction gates too
    assert confidence_of(40, 0, 0, 40, 10, 10, 0.0) == 0.0 and confidence_of(40, 10, 10, 40, 0, 0, 0.0) == 0.0
    assert confidence_of(40, 10, 10, 40, 10, 7, 0.0) == 0.7


def test_counts_of_a_small_hand_made_pair():
    # target: 8 points in voxel (0, 0, 0) of side 1 -> its view cell (0, 0, 0) is seen; near = (-1..1)^3
    tgt = np.tile(np.array([[0.5, 0.5, 0.5]], dtype=np.float32), (8, 1))
    src = np.array([[0.5, 0.5, 0.5], [1.5, 1.5, 1.5], [2.5, 0.5, 0.5], [7.5, 7.5, 7.5], [8.5, 0.5, 0.5], [-0.5, 0.5, 0.5],
                    [np.nan, 0.0, 0.0]], dtype=np.float32)
    r = restate_overlap(src, tgt, np.eye(4), 1.0, min_points=8, min_overlap=0.0)
    # in view: the four source points with every coordinate in [0, 8); near the target: the first two
    assert (r["points_st"], r["in_st"], r["hit_st"]) == (6, 4, 2)
    # the other way round no source view cell holds 8 points
    assert (r["points_ts"], r["in_ts"], r["hit_ts"]) == (8, 0, 0) and r["confidence"] == 0.0
    r = restate_overlap(src, tgt, np.eye(4), 1.0, min_points=1, min_overlap=0.0)
    assert (r["in_ts"], r["hit_ts"]) == (8, 8) and r["confidence"] == 0.5
    # the margin lets the point in view cell (-1, 0, 0) and the one in (1, 0, 0) in as well
    r = restate_overlap(src, tgt, np.eye(4), 1.0, min_points=8, min_overlap=0.0, view_margin=1)
    assert (r["in_st"], r["hit_st"]) == (6, 3)
    for T in (np.zeros((4, 4)), np.full((4, 4), np.nan), np.diag([1.0, 1.0, np.inf, 1.0])):
        r = restate_overlap(src, tgt, T, 1.0, min_points=1, min_overlap=0.0)
        assert (r["in_st"], r["hit_st"], r["in_ts"], r["hit_ts"], r["confidence"]) == (0, 0, 0, 0, 0.0)
    # a transform that sends a point beyond 2^30 voxels: that point counts for nothing
    far = np.eye(4, dtype=np.float32)
    far[0, 3] = 2.0 ** 31
    assert restate_overlap(src, tgt, far, 1.0, min_points=1, min_overlap=0.0)["in_st"] == 0


# ---------------------------------------------------------------- a planted case
@pytest.fixture(scope="module")
def split_room():
    xyz = box_room(3, 120000)[0]
    _, first = np.unique(voxel_of(xyz, 0.05), axis=0, return_index=True)
    xyz = xyz[np.sort(first)]                                # one point per 0.05 m voxel
    a, b = xyz[xyz[:, 0] < 5.5], xyz[xyz[:, 0] > 2.5]
    return a, b, (Table(a, 0.1), Table(b, 0.1))


def _ratios(r):
    return r["hit_st"] / r["in_st"], r["hit_ts"] / r["in_ts"]


def test_planted_room_true_pose_scores_one(split_room):
    a, b, tables = split_room
    r = restate_overlap(a, b, np.eye(4), 0.1, tables=tables)
    print(r)
    assert r["in_st"] > 0.3 * len(a) and r["in_ts"] > 0.3 * len(b)
    assert _ratios(r) == (1.0, 1.0) and r["confidence"] == 1.0


@pytest.mark.parametrize("name", ["slide", "yaw"])
def test_planted_room_wrong_poses_score_at_most_0_9(split_room, name):
    a, b, tables = split_room
    T = np.eye(4)
    if name == "slide":
        T[1, 3] = 1.0                                        # 1 m across the room
    else:
        c, s = np.cos(np.radians(5.0)), np.sin(np.radians(5.0))
        T[:2, :2] = [[c, -s], [s, c]]
    r = restate_overlap(a, b, T, 0.1, tables=tables)
    print(name, r, _ratios(r))
    assert max(_ratios(r)) <= 0.9
    assert 0.0 < r["confidence"] <= 0.9

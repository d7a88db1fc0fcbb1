"""Uniform keypoints without a GPU: the header, the library and the Python mirror carry the surface, the NULL paths return
MM3D_EINVAL, the numpy restatement of tests/test_gpu_uniform_keypoints.py (the judge of the device's rows there) reproduces
vectors worked out by hand and a brute-force form, and the shim reads MM3D_KEYPOINTS."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_uniform_keypoints import (LITERAL_LEAF, LITERAL_POINTS, LITERAL_WINNERS, extent_overflows, restate, restate_brute,
                                        voxel_terms)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


def test_header_declares_the_keypoint_source():
    h = _read("include", "mm3d.h")
    assert re.search(r"MM3D_KEYPOINTS_REFERENCE\s*=\s*0\s*,\s*MM3D_KEYPOINTS_UNIFORM\s*=\s*1", h)
    for decl in (r"int mm3d_uniform_keypoints\(mm3d_ctx \*ctx, const mm3d_cloud \*points, double leaf, mm3d_cloud \*\*out\);",
                 r"void mm3d_keypoint_options_default\(mm3d_keypoint_options \*o\);",
                 r"int mm3d_set_keypoints\(mm3d_ctx \*ctx, const mm3d_keypoint_options \*options\);",
                 r"int mm3d_get_keypoints\(const mm3d_ctx \*ctx, mm3d_keypoint_options \*options\);"):
        assert re.search(decl, h), decl
    assert "pcl::UniformSampling" in h and "__fmul_rn" not in h      # the rule is stated in C terms, and says what it is not
    body = h[:h.index("} mm3d_params;")]                              # mm3d_params carries nothing of it
    assert "leaf" not in body[body.rindex("typedef struct"):]


def test_library_exports_mirror_and_defaults(mm):
    L = mm.lib()
    for name in ("mm3d_uniform_keypoints", "mm3d_keypoint_options_default", "mm3d_set_keypoints", "mm3d_get_keypoints"):
        assert hasattr(L, name), name
    o = mm.KeypointOptions()
    assert C.sizeof(o) == 16 and (o.source, o.leaf) == (mm.KeypointSource.REFERENCE, 0.0)
    assert int(mm.KeypointSource.UNIFORM) == 1
    for method in ("setKeypoints", "getKeypoints", "uniformKeypoints"):
        assert callable(getattr(mm.Context, method))
    L.mm3d_keypoint_options_default(None)                              # a NULL is ignored
    with pytest.raises(TypeError):
        mm.KeypointOptions(spacing=1.0)


def test_null_arguments_are_einval(mm):
    L = mm.lib()
    o = mm.KeypointOptions()
    out = C.c_void_p()
    assert L.mm3d_set_keypoints(None, C.byref(o)) == EINVAL
    assert L.mm3d_get_keypoints(None, C.byref(o)) == EINVAL
    assert L.mm3d_uniform_keypoints(None, None, C.c_double(1.0), C.byref(out)) == EINVAL


def test_restatement_reproduces_the_hand_computed_vectors():
    xyz = np.array([p for p, _ in LITERAL_POINTS], dtype=np.float32)
    idx, f, d2 = voxel_terms(xyz, LITERAL_LEAF)
    finite = [i for i, (_, v) in enumerate(LITERAL_POINTS) if v is not None]
    assert idx.tolist() == finite and len(LITERAL_POINTS) >= 12
    for row, i in enumerate(finite):
        assert tuple(int(v) for v in f[row]) == LITERAL_POINTS[i][1], i
    assert not np.signbit(f).any() or (f[np.signbit(f)] < 0).all()       # -0.0f counts as voxel 0
    by = dict(zip(idx.tolist(), d2.tolist()))
    assert by[0] == 0.0 and by[3] == by[4] and by[5] == by[6] == 0.015625 and by[12] < by[11]
    assert restate(xyz, LITERAL_LEAF).tolist() == LITERAL_WINNERS
    assert restate_brute(xyz, LITERAL_LEAF).tolist() == LITERAL_WINNERS
    # truncation instead of floor would merge point 2 into voxel (0, 0, 0), where point 0 beats it
    assert 2 in LITERAL_WINNERS and int(np.trunc(np.float32(-0.1) * np.float32(2.0))) == 0
    # the extent rule: 3001^3 voxels between two points
    far = np.array([[0, 0, 0], [3000, 3000, 3000], [0.1, 0.1, 0.1], [np.nan, 0, 0]], dtype=np.float32)
    assert extent_overflows(voxel_terms(far, 1.0)[1]) and restate(far, 1.0).tolist() == [0, 1, 2]
    assert restate(far, 4.0).tolist() == [1, 2]                         # 751^3 fits: (0.1, 0.1, 0.1) is nearer the centre (2, 2, 2) than the origin
    assert restate(np.full((3, 3), np.nan, dtype=np.float32), 1.0).tolist() == []


def test_restatement_equals_the_brute_force_form_on_seeded_points():
    rng = np.random.default_rng(20261016)
    xyz = rng.uniform(-4, 4, (10000, 3)).astype(np.float32)
    xyz[::501, 1] = np.nan
    xyz[7::997] = np.round(xyz[7::997] * 2) / 2                          # points on voxel faces and corners
    for leaf in (0.5, 1.0, 3.7):
        a, b = restate(xyz, leaf), restate_brute(xyz, leaf)
        assert np.array_equal(a, b), leaf
        assert (np.diff(a) > 0).all() and np.isfinite(xyz[a]).all()
        _, f, _ = voxel_terms(xyz, leaf)
        assert len(a) == len(np.unique(f, axis=0))                       # one keypoint per occupied voxel


SHIM_CASES = r"""
#include <cstdio>
#include <cstring>
#include "map_merge_3d_shim.hpp"
using map_merge_3d::mm3d_shim::parse_keypoints;
static int refused(const char *v) { try { (void)parse_keypoints(v); } catch (const std::runtime_error &e) { return std::strstr(e.what(), "MM3D_KEYPOINTS") != nullptr; } return 0; }
int main()
{
  mm3d_keypoint_options o = parse_keypoints(nullptr);
  if (o.source != MM3D_KEYPOINTS_REFERENCE || o.leaf != 0.0) return 1;
  o = parse_keypoints("");
  if (o.source != MM3D_KEYPOINTS_REFERENCE) return 2;
  o = parse_keypoints("reference");
  if (o.source != MM3D_KEYPOINTS_REFERENCE) return 3;
  o = parse_keypoints("uniform");
  if (o.source != MM3D_KEYPOINTS_UNIFORM || o.leaf != 0.0) return 4;
  o = parse_keypoints("uniform:0.4");
  if (o.source != MM3D_KEYPOINTS_UNIFORM || o.leaf != 0.4) return 5;
  const char *bad[] = {"garbage", "uniform:", "uniform:abc", "uniform:0.4m", "uniform:-1", "uniform:0", "uniform:nan", "uniform:inf",
                       "uniformly", "Uniform", "sift"};
  for (const char *b : bad) if (!refused(b)) { std::printf("accepted '%s'\n", b); return 6; }
  std::puts("shim keypoints: ok");
  return 0;
}
"""


def test_shim_parses_mm3d_keypoints(tmp_path):
    """Compiled with the flags tests/shim/build.sh compiles the shim with; the parser lies outside the header's PCL guard."""
    src = tmp_path / "shim_keypoints.cpp"
    src.write_text(SHIM_CASES)
    exe = tmp_path / "shim_keypoints"
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0 and "shim keypoints: ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    s = _read("include", "map_merge_3d_shim.hpp")
    assert 'parse_keypoints(std::getenv("MM3D_KEYPOINTS"))' in s and "mm3d_set_keypoints(e, &keypoints)" in s

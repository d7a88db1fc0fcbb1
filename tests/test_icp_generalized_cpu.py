"""Generalized ICP (mm3d_set_icp_generalized) without a GPU: the declared and exported surface, the shim's MM3D_ICP_GENERALIZED
parser compiled on its own, and the numpy restatement of test_gpu_icp_generalized.py alone on two independent samplings of one
room -- it ends two orders of magnitude closer to the truth than point-to-plane's restatement, which the sampling pulls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from test_gpu_icp_generalized import DEFAULTS, ROOM, generalized_system, resampled_room, restate_icp_generalized, unit_normals
from test_gpu_icp_plane import restate_icp_plane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


def test_header_declares_the_generalized_icp():
    h = _read("include", "mm3d.h")
    m = re.search(r"typedef struct mm3d_icp_generalized_options \{(.*?)\} mm3d_icp_generalized_options;", h, re.S)
    assert m, "mm3d_icp_generalized_options is not declared"
    fields = re.findall(r"^\s*(int|double)\s+(\w+);", m.group(1), re.M)
    assert fields == [("int", "enabled"), ("double", "epsilon")]
    for decl in ("void mm3d_icp_generalized_options_default(mm3d_icp_generalized_options *o);",
                 "int mm3d_set_icp_generalized(mm3d_ctx *ctx, const mm3d_icp_generalized_options *options);",
                 "int mm3d_get_icp_generalized(const mm3d_ctx *ctx, mm3d_icp_generalized_options *options);",
                 "int mm3d_estimate_transform_icp_generalized(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_normals *source_normals,",
                 "int mm3d_debug_icp_generalized_split(int split);"):
        assert decl in h, decl
    # the setter is enum-free, and the ICP method's enum stays as it was
    assert re.search(r"typedef enum \{ MM3D_ICP_POINT_TO_POINT = 0, MM3D_ICP_POINT_TO_PLANE = 1 \} mm3d_icp_method;", h)
    # what the restatement restates
    assert "Sigma = 2 I - (1 - epsilon) (n_t n_t^T + m m^T)" in h and "J = [-[s]x | I3]" in h and "0, 1e-3" in h


def test_library_exports_the_generalized_icp(mm):
    lib = mm.lib()
    for name in ("mm3d_icp_generalized_options_default", "mm3d_set_icp_generalized", "mm3d_get_icp_generalized",
                 "mm3d_estimate_transform_icp_generalized", "mm3d_debug_icp_generalized_split"):
        assert hasattr(lib, name), name
    for name in ("IcpGeneralizedOptions", "icp_generalized_split"):
        assert hasattr(mm, name), name
    for name in ("setIcpGeneralized", "getIcpGeneralized", "estimateTransformICPGeneralized"):
        assert callable(getattr(mm.Context, name)), name
    assert C.sizeof(mm.IcpGeneralizedOptions) == 16
    assert mm.IcpGeneralizedOptions().as_tuple() == DEFAULTS
    lib.mm3d_icp_generalized_options_default(None)         # a no-op, not a crash
    # what is checked before anything touches a device or the handle: a context that is never dereferenced shows it
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    o = mm.IcpGeneralizedOptions()
    T = (C.c_float * 16)()

    def stage(s, sn, t, tn, opt):
        return lib.mm3d_estimate_transform_icp_generalized(fake, s, sn, t, tn, T, C.c_double(1.0), opt, 10, C.c_double(0.0), T)

    assert lib.mm3d_set_icp_generalized(None, C.byref(o)) == EINVAL and lib.mm3d_set_icp_generalized(fake, None) == EINVAL
    assert lib.mm3d_get_icp_generalized(None, C.byref(o)) == EINVAL and lib.mm3d_get_icp_generalized(fake, None) == EINVAL
    for bad in (dict(enabled=2), dict(epsilon=0.0), dict(epsilon=-0.5), dict(epsilon=1.0001), dict(epsilon=float("nan")),
                dict(epsilon=float("inf"))):
        for enabled in (0, 1):
            b = mm.IcpGeneralizedOptions(**{"enabled": enabled, **bad})
            assert lib.mm3d_set_icp_generalized(fake, C.byref(b)) == EINVAL, bad
            assert stage(fake, fake, fake, fake, C.byref(b)) == EINVAL
    for args in ((None, fake, fake, fake, C.byref(o)), (fake, None, fake, fake, C.byref(o)), (fake, fake, None, fake, C.byref(o)),
                 (fake, fake, fake, None, C.byref(o)), (fake, fake, fake, fake, None)):
        assert stage(*args) == EINVAL
    assert lib.mm3d_debug_icp_generalized_split(-1) == 0 and lib.mm3d_debug_icp_generalized_split(3) == 0


SHIM_CASES = r"""
#include <cstdio>
#include <cstring>
#include "map_merge_3d_shim.hpp"
using map_merge_3d::mm3d_shim::parse_icp_generalized;
using map_merge_3d::mm3d_shim::parse_icp_color;
using map_merge_3d::mm3d_shim::parse_icp_reject;
using map_merge_3d::mm3d_shim::check_icp_generalized_combinations;
static int refused(const char *v)
{
  try { (void)parse_icp_generalized(v); } catch (const std::runtime_error &e) { return std::strstr(e.what(), "MM3D_ICP_GENERALIZED") != nullptr; }
  return 0;
}
// 1: refused, and the message names both variables; 0: accepted
static int combination_refused(const char *v, const char *reject, const char *color, const char *d, const char *other)
{
  try { check_icp_generalized_combinations(parse_icp_generalized(v), parse_icp_reject(reject), parse_icp_color(color), d); }
  catch (const std::runtime_error &e) { return std::strstr(e.what(), "MM3D_ICP_GENERALIZED") != nullptr && std::strstr(e.what(), other) != nullptr; }
  return 0;
}
static int is(const mm3d_icp_generalized_options &o, int enabled, double epsilon) { return o.enabled == enabled && o.epsilon == epsilon; }
int main()
{
  if (!is(parse_icp_generalized(nullptr), 0, 1e-3) || !is(parse_icp_generalized(""), 0, 1e-3)) return 1;
  if (!is(parse_icp_generalized("0"), 0, 1e-3) || !is(parse_icp_generalized("none"), 0, 1e-3)) return 2;
  if (!is(parse_icp_generalized("1"), 1, 1e-3)) return 3;
  if (!is(parse_icp_generalized("0.01"), 1, 0.01) || !is(parse_icp_generalized("1.0"), 1, 1.0) || !is(parse_icp_generalized("1e-4"), 1, 1e-4)) return 4;
  const char *bad[] = {"2", "1.5", "-0.5", "0.0", "abc", "0.5x", "0.5:", "0.5:0.3", "nan", "inf", "on", " "};
  for (const char *b : bad) if (!refused(b)) { std::printf("accepted '%s'\n", b); return 5; }
  if (!combination_refused("1", nullptr, nullptr, "0,1", "MM3D_DEVICES") || !combination_refused("0.01", "none", "0", "all", "MM3D_DEVICES")) return 6;
  if (!combination_refused("1", "trimmed:0.7", nullptr, nullptr, "MM3D_ICP_REJECT") || !combination_refused("1", "one_to_one", "0", "", "MM3D_ICP_REJECT")) return 7;
  if (!combination_refused("1", nullptr, "1", nullptr, "MM3D_ICP_COLOR") || !combination_refused("0.5", "none", "0.9:0.3", "", "MM3D_ICP_COLOR")) return 8;
  if (combination_refused("1", nullptr, nullptr, nullptr, "MM3D") || combination_refused("1", "none", "0", "", "MM3D") ||
      combination_refused(nullptr, "trimmed", "1", "0,1", "MM3D") || combination_refused("0", "median", "1", "0", "MM3D"))
    return 9;
  std::puts("shim icp generalized: ok");
  return 0;
}
"""


def test_shim_parses_mm3d_icp_generalized(tmp_path):
    """Compiled with the flags tests/shim/build.sh compiles the shim with; the parser lies outside the header's PCL guard."""
    src = tmp_path / "shim_icp_generalized.cpp"
    src.write_text(SHIM_CASES)
    exe = tmp_path / "shim_icp_generalized"
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0 and "shim icp generalized: ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    s = _read("include", "map_merge_3d_shim.hpp")
    assert 'parse_icp_generalized(std::getenv("MM3D_ICP_GENERALIZED"))' in s and "mm3d_set_icp_generalized(e, &generalized)" in s
    assert 'check_icp_generalized_combinations(generalized, reject, color, std::getenv("MM3D_DEVICES"))' in s


def test_unit_normals_and_the_system():
    u, ok = unit_normals(np.float32([[0, 0, 2], [3, 4, 0], [0, 0, 0], [np.nan, 0, 1], [np.inf, 0, 0], [1e-30, 0, 0]]))
    assert ok.tolist() == [True, True, False, False, False, True]
    assert np.array_equal(u[0], [0, 0, 1]) and np.allclose(u[1], [0.6, 0.8, 0], rtol=1e-15) and np.array_equal(u[2:5], np.zeros((3, 3)))
    # epsilon 1: both covariances are I, W = I / 2, and the system is point-to-point's linearisation at half weight
    rng = np.random.default_rng(3)
    s, q = rng.normal(size=(50, 3)), rng.normal(size=(50, 3))
    n = rng.normal(size=(50, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    AtA, Atr = generalized_system(s, q, n, n[::-1].copy(), 1.0)
    J = np.zeros((50, 3, 6))
    for k in range(50):
        x, y, z = s[k]
        J[k, :, :3] = -np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
        J[k, :, 3:] = np.eye(3)
    assert np.allclose(AtA, 0.5 * np.einsum("kai,kaj->ij", J, J), rtol=1e-12)
    assert np.allclose(Atr, 0.5 * np.einsum("kai,ka->i", J, q - s), rtol=1e-12, atol=1e-12)
    # two parallel planes with epsilon -> 0: only the offset along the common normal is weighted
    z = np.tile([0.0, 0.0, 1.0], (50, 1))
    AtA, _ = generalized_system(s, q, z, z, 1e-9)
    assert AtA[5, 5] > 1e7 * AtA[3, 3] and AtA[5, 5] > 1e7 * AtA[4, 4]


def test_restatement_on_the_resampled_room():
    """Seed 1 of the issue's table: two independent samplings of the room, 3 000 points each.  Generalized ICP ends within 1e-4 of
    the truth and at least 100 times closer than point-to-plane's restatement on the same inputs."""
    tgt, nrm, src, s_nrm, T_true, guess = resampled_room(1)
    T, iters, conv, margins = restate_icp_generalized(src, s_nrm, tgt, nrm, guess, ROOM["max_corr"], ROOM["max_iter"], ROOM["eps"], ROOM["epsilon"])
    err = np.abs(T - T_true).max()
    Tp, it_p, conv_p, _ = restate_icp_plane(src, tgt, nrm, guess, ROOM["max_corr"], ROOM["max_iter"], ROOM["eps"])
    err_plane = np.abs(Tp - T_true).max()
    print("generalized: iterations", iters, "max|T - T_true|", err, "smallest margin", min(margins), "; point-to-plane: iterations", it_p,
          "max|T - T_true|", err_plane)
    assert conv == 1 and iters >= 2
    assert err < 1e-4, err
    assert conv_p == 1 and 100.0 * err <= err_plane, (err, err_plane)

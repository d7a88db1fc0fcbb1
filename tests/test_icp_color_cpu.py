"""Coloured ICP (mm3d_set_icp_color) without a GPU: the declared and exported surface, the shim's MM3D_ICP_COLOR parser compiled on
its own, and the numpy restatement of test_gpu_icp_color.py alone on a small textured corridor -- it recovers the slide along
the axis that point-to-plane's terms (lambda 1) leave singular."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from test_gpu_icp_color import DEFAULTS, _ldlt3, corridor_pair, intensity_of, restate_gradients, restate_icp_color

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


def test_header_declares_the_coloured_icp():
    h = _read("include", "mm3d.h")
    m = re.search(r"typedef struct mm3d_icp_color_options \{(.*?)\} mm3d_icp_color_options;", h, re.S)
    assert m, "mm3d_icp_color_options is not declared"
    fields = re.findall(r"^\s*(int|double)\s+(\w+);", m.group(1), re.M)
    assert fields == [("int", "enabled"), ("double", "lambda_geometric"), ("double", "gradient_radius"), ("int", "min_neighbours")]
    for decl in ("void mm3d_icp_color_options_default(mm3d_icp_color_options *o);",
                 "int mm3d_set_icp_color(mm3d_ctx *ctx, const mm3d_icp_color_options *options);",
                 "int mm3d_get_icp_color(const mm3d_ctx *ctx, mm3d_icp_color_options *options);",
                 "int mm3d_estimate_transform_icp_color(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target,",
                 "int mm3d_debug_color_gradients(mm3d_ctx *ctx, const mm3d_cloud *points, const mm3d_normals *normals,",
                 "int mm3d_debug_icp_color_split(int split);"):
        assert decl in h, decl
    # the setter is enum-free, and the ICP method's enum stays as it was
    assert re.search(r"typedef enum \{ MM3D_ICP_POINT_TO_POINT = 0, MM3D_ICP_POINT_TO_PLANE = 1 \} mm3d_icp_method;", h)
    assert "0, 0.968, 0, 4" in h


def test_library_exports_the_coloured_icp(mm):
    lib = mm.lib()
    for name in ("mm3d_icp_color_options_default", "mm3d_set_icp_color", "mm3d_get_icp_color", "mm3d_estimate_transform_icp_color",
                 "mm3d_debug_color_gradients", "mm3d_debug_icp_color_split"):
        assert hasattr(lib, name), name
    for name in ("IcpColorOptions", "icp_color_split"):
        assert hasattr(mm, name), name
    for name in ("setIcpColor", "getIcpColor", "estimateTransformICPColor", "debugColorGradients"):
        assert callable(getattr(mm.Context, name)), name
    assert C.sizeof(mm.IcpColorOptions) == 32
    assert mm.IcpColorOptions().as_tuple() == DEFAULTS
    lib.mm3d_icp_color_options_default(None)               # a no-op, not a crash
    # what is checked before anything touches a device or the handle: a context that is never dereferenced shows it
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    o = mm.IcpColorOptions()
    T = (C.c_float * 16)()
    assert lib.mm3d_set_icp_color(None, C.byref(o)) == EINVAL and lib.mm3d_set_icp_color(fake, None) == EINVAL
    assert lib.mm3d_get_icp_color(None, C.byref(o)) == EINVAL and lib.mm3d_get_icp_color(fake, None) == EINVAL
    for bad in (dict(enabled=2), dict(lambda_geometric=0.0), dict(lambda_geometric=1.0001), dict(lambda_geometric=float("nan")),
                dict(gradient_radius=-1.0), dict(gradient_radius=float("inf")), dict(min_neighbours=3)):
        for enabled in (0, 1):
            b = mm.IcpColorOptions(**{"enabled": enabled, **bad})
            assert lib.mm3d_set_icp_color(fake, C.byref(b)) == EINVAL, bad
            assert lib.mm3d_estimate_transform_icp_color(fake, fake, fake, fake, T, C.c_double(1.0), C.byref(b), 10, C.c_double(0.0), T) == EINVAL
    assert lib.mm3d_estimate_transform_icp_color(fake, fake, fake, fake, T, C.c_double(1.0), C.byref(o), 10, C.c_double(0.0), T) == EINVAL   # radius 0
    assert lib.mm3d_estimate_transform_icp_color(fake, None, fake, fake, T, C.c_double(1.0), C.byref(o), 10, C.c_double(0.0), T) == EINVAL
    assert lib.mm3d_debug_color_gradients(fake, None, None, C.byref(o), None) == EINVAL
    assert lib.mm3d_debug_icp_color_split(-1) == 0 and lib.mm3d_debug_icp_color_split(3) == 0


SHIM_CASES = r"""
#include <cstdio>
#include <cstring>
#include "map_merge_3d_shim.hpp"
using map_merge_3d::mm3d_shim::parse_icp_color;
using map_merge_3d::mm3d_shim::parse_icp_reject;
using map_merge_3d::mm3d_shim::check_icp_color_combinations;
static int refused(const char *v) { try { (void)parse_icp_color(v); } catch (const std::runtime_error &e) { return std::strstr(e.what(), "MM3D_ICP_COLOR") != nullptr; } return 0; }
static int combination_refused(const char *v, const char *reject, const char *d)
{
  try { check_icp_color_combinations(parse_icp_color(v), parse_icp_reject(reject), d); } catch (const std::runtime_error &e) { return std::strstr(e.what(), "MM3D_ICP_COLOR") != nullptr; }
  return 0;
}
static int is(const mm3d_icp_color_options &o, int enabled, double lambda, double radius, int minn)
{
  return o.enabled == enabled && o.lambda_geometric == lambda && o.gradient_radius == radius && o.min_neighbours == minn;
}
int main()
{
  if (!is(parse_icp_color(nullptr), 0, 0.968, 0.0, 4) || !is(parse_icp_color(""), 0, 0.968, 0.0, 4)) return 1;
  if (!is(parse_icp_color("0"), 0, 0.968, 0.0, 4) || !is(parse_icp_color("none"), 0, 0.968, 0.0, 4)) return 2;
  if (!is(parse_icp_color("1"), 1, 0.968, 0.0, 4)) return 3;
  if (!is(parse_icp_color("0.5"), 1, 0.5, 0.0, 4) || !is(parse_icp_color("1.0"), 1, 1.0, 0.0, 4)) return 4;
  if (!is(parse_icp_color("0.9:0.3"), 1, 0.9, 0.3, 4) || !is(parse_icp_color("1:0.25"), 1, 1.0, 0.25, 4)) return 5;
  const char *bad[] = {"2", "1.5", "-0.5", "0.0", "abc", "0.5x", "0.5:", "0.5:0", "0.5:-1", "0.5:inf", "0.5:nan", "0.5:0.3x", ":0.3", "nan", "on", "0.5:0.3:1"};
  for (const char *b : bad) if (!refused(b)) { std::printf("accepted '%s'\n", b); return 6; }
  if (!combination_refused("1", nullptr, "0,1") || !combination_refused("0.5:0.3", "none", "all")) return 7;
  if (!combination_refused("1", "trimmed:0.7", nullptr) || !combination_refused("1", "one_to_one", "")) return 8;
  if (combination_refused("1", nullptr, nullptr) || combination_refused("1", "none", "") || combination_refused(nullptr, "trimmed", "0,1") ||
      combination_refused("0", "median", "0"))
    return 9;
  std::puts("shim icp color: ok");
  return 0;
}
"""


def test_shim_parses_mm3d_icp_color(tmp_path):
    """Compiled with the flags tests/shim/build.sh compiles the shim with; the parser lies outside the header's PCL guard."""
    src = tmp_path / "shim_icp_color.cpp"
    src.write_text(SHIM_CASES)
    exe = tmp_path / "shim_icp_color"
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0 and "shim icp color: ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    s = _read("include", "map_merge_3d_shim.hpp")
    assert 'parse_icp_color(std::getenv("MM3D_ICP_COLOR"))' in s and "mm3d_set_icp_color(e, &color)" in s
    assert 'check_icp_color_combinations(color, reject, std::getenv("MM3D_DEVICES"))' in s


def test_intensity_and_the_small_solve():
    h = _read("include", "mm3d.h")
    assert "I = (float)((double)(299 r + 587 g + 114 b) / 255000.0)" in h and "1e-12 trace(M) / 3" in h     # what is restated here
    assert intensity_of(np.uint32([0xff000000, 0xffffffff, 0x00ff0000, 0x0000ff00, 0x000000ff])).tolist() == \
        [0.0, 1.0, np.float32(299 * 255 / 255000.0), np.float32(587 * 255 / 255000.0), np.float32(114 * 255 / 255000.0)]
    M = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.2], [0.5, 0.2, 2.0]])
    b = np.array([1.0, -2.0, 0.5])
    assert np.allclose(_ldlt3(M, b, 1e-12), np.linalg.solve(M, b), rtol=1e-13)
    assert _ldlt3(np.diag([1.0, 0.0, 1.0]), b, 1e-12) is None


def test_restatement_recovers_the_corridor_slide_and_is_singular_without_colour(mm):
    default = mm.IcpColorOptions()
    tgt, rgba, nrm, src, s_rgba, T_true = corridor_pair(1500)
    rec, cond = restate_gradients(tgt, rgba, nrm, 0.3, default.min_neighbours)
    assert np.abs(rec[:, :3]).max() > 0.1 and 0 < cond.max() < 1e6
    # a gradient lies in its tangent plane (the soft constraint weighs k^2)
    assert np.abs((rec[:, :3] * nrm).sum(axis=1)).max() < 1e-3
    guess = np.eye(4, dtype=np.float32)
    for lam in (default.lambda_geometric, 0.5):
        T, iters, conv, _, singular = restate_icp_color(src, s_rgba, tgt, nrm, rec, guess, 0.5, 50, 1e-10, lam)
        err = np.abs(T - T_true).max()
        assert conv == 1 and not singular and iters >= 2, (lam, iters, conv)
        # the GPU test's 6 000-point scene is held to 5e-3; a quarter of the points leaves a quarter of the neighbours per
        # gradient, so twice its sampling noise: 1e-2, against a slide of 0.25
        assert err < 1e-2, (lam, err)
    T, iters, conv, _, singular = restate_icp_color(src, s_rgba, tgt, nrm, rec, guess, 0.5, 50, 1e-10, 1.0)
    assert singular and conv == 0 and iters == 0 and np.array_equal(T, guess)

"""The geometric ICP rejectors (mm3d_set_icp_geometry_rejection, mm3d_boundary_points) without a GPU: the declared and exported
surface, defaults and ranges, the shim's MM3D_ICP_REJECT_GEOMETRY parser compiled on its own, and the numpy restatement of the
rule that include/mm3d.h states (icp_geometry_cases.py) -- on literal vectors, on the half-overlapping height field and on the
slanted cabinet -- which test_gpu_icp_geometry.py reads."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import icp_geometry_cases as G
from test_icp_rejection_cpu import VARIANTS, cabinet, restate_icp_rejecting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


# ---------------------------------------------------------------- surface
def test_header_declares_the_surface():
    h = _read("include", "mm3d.h")
    assert re.search(r"typedef struct mm3d_icp_geometry_options \{\s*int boundary;[^}]*double boundary_radius;[^}]*double boundary_angle_deg;"
                     r"[^}]*int boundary_min_neighbours;[^}]*int normals;[^}]*double normal_angle_deg;[^}]*\} mm3d_icp_geometry_options;", h)
    assert re.search(r"typedef struct mm3d_icp_geometry_stats \{[^}]*long long matched, on_boundary, normal_mismatch, passed;"
                     r"[^}]*long long target_boundary_points;[^}]*\} mm3d_icp_geometry_stats;", h)
    for decl in (r"void mm3d_icp_geometry_options_default\(mm3d_icp_geometry_options \*o\);",
                 r"int mm3d_set_icp_geometry_rejection\(mm3d_ctx \*ctx, const mm3d_icp_geometry_options \*options\);",
                 r"int mm3d_get_icp_geometry_rejection\(const mm3d_ctx \*ctx, mm3d_icp_geometry_options \*options\);",
                 r"int mm3d_last_icp_geometry_stats\(const mm3d_ctx \*ctx, mm3d_icp_geometry_stats \*stats\);",
                 r"int mm3d_boundary_points\(mm3d_ctx \*ctx, const mm3d_cloud \*points, const mm3d_normals \*normals, double radius, double angle_deg,",
                 r"int mm3d_estimate_transform_icp_rejecting_geometry\(mm3d_ctx \*ctx, const mm3d_cloud \*source, const mm3d_normals \*source_normals,",
                 r"int mm3d_debug_icp_geometry\(mm3d_ctx \*ctx, const mm3d_cloud \*source, const mm3d_normals \*source_normals, const mm3d_cloud \*target,",
                 r"int mm3d_debug_boundary_lds_cap\(int cap\);"):
        assert re.search(decl, h), decl
    # the rule is stated where the operation is declared
    for phrase in ("FILLS THE WEDGE", "cross > 0 || (cross == 0 && dot < 0)", "exactly 0 at 90 and exactly -1 at 180", "Step 1b"):
        assert phrase in h, phrase


def test_library_exports_and_mirror_binds(mm):
    lib = mm.lib()
    for name in ("mm3d_icp_geometry_options_default", "mm3d_set_icp_geometry_rejection", "mm3d_get_icp_geometry_rejection",
                 "mm3d_last_icp_geometry_stats", "mm3d_boundary_points", "mm3d_estimate_transform_icp_rejecting_geometry",
                 "mm3d_debug_icp_geometry", "mm3d_debug_boundary_lds_cap"):
        assert getattr(lib, name)
    for name in ("setIcpGeometryRejection", "getIcpGeometryRejection", "boundaryPoints", "estimateTransformICPRejectingGeometry",
                 "debugIcpGeometry"):
        assert callable(getattr(mm.Context, name))
    assert isinstance(mm.Context.last_icp_geometry_stats, property) and callable(mm.boundary_lds_cap)
    assert C.sizeof(mm.IcpGeometryOptions) == 40 and C.sizeof(mm.IcpGeometryStats) == 40


def test_defaults_and_null_handling(mm):
    o = mm.IcpGeometryOptions()
    assert o.as_tuple() == tuple(G.GEO_DEFAULT) == (0, 0.0, 90.0, 3, 0, 45.0)
    lib = mm.lib()
    lib.mm3d_icp_geometry_options_default(None)          # a no-op, not a crash
    ro, st = mm.IcpRejectionOptions(), mm.IcpGeometryStats()
    T = (C.c_float * 16)()
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    assert lib.mm3d_set_icp_geometry_rejection(None, C.byref(o)) == EINVAL and lib.mm3d_set_icp_geometry_rejection(fake, None) == EINVAL
    assert lib.mm3d_get_icp_geometry_rejection(None, C.byref(o)) == EINVAL and lib.mm3d_get_icp_geometry_rejection(fake, None) == EINVAL
    assert lib.mm3d_last_icp_geometry_stats(None, C.byref(st)) == EINVAL and lib.mm3d_last_icp_geometry_stats(fake, None) == EINVAL
    d, k = C.c_double, C.c_size_t
    assert lib.mm3d_boundary_points(None, fake, fake, d(0.3), d(90.0), 3, fake, k(0), None) == EINVAL
    assert lib.mm3d_boundary_points(fake, None, fake, d(0.3), d(90.0), 3, fake, k(0), None) == EINVAL
    assert lib.mm3d_boundary_points(fake, fake, None, d(0.3), d(90.0), 3, fake, k(0), None) == EINVAL
    assert lib.mm3d_boundary_points(fake, fake, fake, d(0.3), d(90.0), 3, None, k(0), None) == EINVAL
    for r, a, m in ((0.0, 90.0, 3), (-1.0, 90.0, 3), (float("inf"), 90.0, 3), (float("nan"), 90.0, 3), (0.3, 0.0, 3), (0.3, 180.5, 3),
                    (0.3, float("nan"), 3), (0.3, 90.0, 2)):
        assert lib.mm3d_boundary_points(fake, fake, fake, d(r), d(a), m, fake, k(0), None) == EINVAL, (r, a, m)
    args = (T, d(1.0), C.byref(ro), C.byref(o), 10, d(0.0), T, None, None)
    assert lib.mm3d_estimate_transform_icp_rejecting_geometry(fake, None, None, fake, None, 0, *args) == EINVAL
    assert lib.mm3d_estimate_transform_icp_rejecting_geometry(fake, fake, None, None, None, 0, *args) == EINVAL
    assert lib.mm3d_estimate_transform_icp_rejecting_geometry(fake, fake, None, fake, None, 2, *args) == EINVAL       # point_to_plane
    assert lib.mm3d_estimate_transform_icp_rejecting_geometry(fake, fake, None, fake, None, 1, *args) == EINVAL       # plane without normals
    assert lib.mm3d_estimate_transform_icp_rejecting_geometry(fake, fake, None, fake, None, 0, T, d(1.0), None, C.byref(o), 10, d(0.0), T, None,
                                                              None) == EINVAL
    assert lib.mm3d_estimate_transform_icp_rejecting_geometry(fake, fake, None, fake, None, 0, T, d(1.0), C.byref(ro), None, 10, d(0.0), T, None,
                                                              None) == EINVAL
    # normals == 1 without the source's normals, boundary == 1 without the target's, boundary == 1 with radius 0
    n1, b1, b0 = mm.IcpGeometryOptions(normals=1), mm.IcpGeometryOptions(boundary=1, boundary_radius=0.3), mm.IcpGeometryOptions(boundary=1)
    for go in (n1, b1, b0):
        assert lib.mm3d_estimate_transform_icp_rejecting_geometry(fake, fake, None, fake, None, 0, T, d(1.0), C.byref(ro), C.byref(go), 10, d(0.0),
                                                                  T, None, None) == EINVAL
    assert lib.mm3d_debug_icp_geometry(fake, None, None, fake, None, T, d(1.0), C.byref(ro), C.byref(o), 1, None, None, None, None, None) == EINVAL
    assert lib.mm3d_debug_icp_geometry(fake, fake, None, fake, None, T, d(1.0), C.byref(ro), C.byref(o), 2, None, None, None, None, None) == EINVAL
    # the arena hook: negative asks, a value outside 0 .. 512 changes nothing
    assert lib.mm3d_debug_boundary_lds_cap(-1) == 512 and lib.mm3d_debug_boundary_lds_cap(513) == 512
    assert lib.mm3d_debug_boundary_lds_cap(64) == 64 and lib.mm3d_debug_boundary_lds_cap(0) == 512


BAD = [dict(boundary=2), dict(boundary=-1), dict(normals=2), dict(normals=-1), dict(boundary_radius=-0.1), dict(boundary_radius=float("inf")),
       dict(boundary_radius=float("nan")), dict(boundary_angle_deg=0.0), dict(boundary_angle_deg=180.5), dict(boundary_angle_deg=float("nan")),
       dict(boundary_min_neighbours=2), dict(normal_angle_deg=0.0), dict(normal_angle_deg=90.5), dict(normal_angle_deg=float("nan"))]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
@pytest.mark.parametrize("bits", [(0, 0), (1, 0), (0, 1)])
def test_out_of_range_options_are_refused_whatever_the_bits(mm, bad, bits):
    """The check comes before anything touches a device or the handle: a context that is never dereferenced shows it."""
    o = mm.IcpGeometryOptions(**{"boundary": bits[0], "normals": bits[1], "boundary_radius": 0.3, **bad})
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)      # never read: the options are checked first
    ro = mm.IcpRejectionOptions()
    T = (C.c_float * 16)()
    assert mm.lib().mm3d_set_icp_geometry_rejection(fake, C.byref(o)) == EINVAL
    assert mm.lib().mm3d_estimate_transform_icp_rejecting_geometry(fake, fake, fake, fake, fake, 0, T, C.c_double(1.0), C.byref(ro), C.byref(o), 10,
                                                                   C.c_double(0.0), T, None, None) == EINVAL


SHIM_CASES = r"""
#include <cstdio>
#include <cstring>
#include "map_merge_3d_shim.hpp"
using map_merge_3d::mm3d_shim::parse_icp_reject_geometry;
using map_merge_3d::mm3d_shim::check_icp_reject_geometry_devices;
static int refused(const char *v) { try { (void)parse_icp_reject_geometry(v); } catch (const std::runtime_error &e) { return std::strstr(e.what(), "MM3D_ICP_REJECT_GEOMETRY") != nullptr; } return 0; }
static int devices_refused(const char *v, const char *d) { try { check_icp_reject_geometry_devices(parse_icp_reject_geometry(v), d); } catch (const std::runtime_error &) { return 1; } return 0; }
static int is(const mm3d_icp_geometry_options &o, int b, double r, int n, double a)
{
  return o.boundary == b && o.boundary_radius == r && o.boundary_angle_deg == 90.0 && o.boundary_min_neighbours == 3 && o.normals == n &&
         o.normal_angle_deg == a;
}
int main()
{
  if (!is(parse_icp_reject_geometry(nullptr), 0, 0.0, 0, 45.0) || !is(parse_icp_reject_geometry(""), 0, 0.0, 0, 45.0)) return 1;
  if (!is(parse_icp_reject_geometry("none"), 0, 0.0, 0, 45.0)) return 2;
  if (!is(parse_icp_reject_geometry("boundary"), 1, 0.0, 0, 45.0) || !is(parse_icp_reject_geometry("boundary:0.35"), 1, 0.35, 0, 45.0)) return 3;
  if (!is(parse_icp_reject_geometry("normals"), 0, 0.0, 1, 45.0) || !is(parse_icp_reject_geometry("normals:30"), 0, 0.0, 1, 30.0)) return 4;
  if (!is(parse_icp_reject_geometry("normals:90"), 0, 0.0, 1, 90.0)) return 5;
  if (!is(parse_icp_reject_geometry("boundary:0.35+normals:30"), 1, 0.35, 1, 30.0)) return 6;
  if (!is(parse_icp_reject_geometry("normals:30+boundary"), 1, 0.0, 1, 30.0)) return 7;
  const char *bad[] = {"boundary+boundary", "normals:30+normals:20", "boundary:", "boundary:0", "boundary:-1", "boundary:inf", "boundary:nan",
                       "boundary:abc", "boundary:0.3x", "normals:0", "normals:90.5", "normals:-30", "edges", "Boundary", "boundary+", "+boundary",
                       "boundary++normals", "none+boundary", " boundary", "normals:30 "};
  for (const char *b : bad) if (!refused(b)) { std::printf("accepted '%s'\n", b); return 8; }
  if (!devices_refused("boundary", "0,1") || !devices_refused("normals:30", "all")) return 9;
  if (devices_refused("boundary", nullptr) || devices_refused("boundary", "") || devices_refused("none", "0,1") || devices_refused(nullptr, "0,1")) return 10;
  std::puts("shim icp reject geometry: ok");
  return 0;
}
"""


def test_shim_parses_mm3d_icp_reject_geometry(tmp_path):
    """Compiled with the flags tests/shim/build.sh compiles the shim with; the parser lies outside the header's PCL guard."""
    src = tmp_path / "shim_icp_reject_geometry.cpp"
    src.write_text(SHIM_CASES)
    exe = tmp_path / "shim_icp_reject_geometry"
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0 and "shim icp reject geometry: ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    s = _read("include", "map_merge_3d_shim.hpp")
    assert 'parse_icp_reject_geometry(std::getenv("MM3D_ICP_REJECT_GEOMETRY"))' in s and "mm3d_set_icp_geometry_rejection(e, &reject_geometry)" in s
    assert 'check_icp_reject_geometry_devices(reject_geometry, std::getenv("MM3D_DEVICES"))' in s
    assert "0, 0.0, 90, 3, 0, 45" in _read("include", "mm3d.h")          # the parser's defaults are the library's


# ---------------------------------------------------------------- the restatement against literal vectors
F = np.float32
UP = np.array([0, 0, 1], dtype=F)
RING = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]          # every 45 degrees, counter-clockwise


def _flag(offsets, theta=90.0, k=3, normal=UP, centre=(2.0, -1.5, 0.75), extra=()):
    """The flag of a point at `centre` with neighbours at centre + 0.25 * offset (offsets (dx, dy) or (dx, dy, dz))."""
    c = np.asarray(centre, dtype=np.float64)
    rows = [c] + [c + 0.25 * np.asarray(tuple(o) + (0,) * (3 - len(o)), dtype=np.float64) for o in offsets] + [np.asarray(e, dtype=np.float64) for e in extra]
    pts = np.asarray(rows, dtype=F)
    nrm = np.tile(np.asarray(normal, dtype=F), (len(pts), 1))
    flags, counts = G.restate_boundary(pts, nrm, 0.4, theta, k)
    return bool(flags[0]), int(counts[0])


def test_boundary_rule_literal():
    assert _flag(RING) == (False, 8)                                    # a closed ring: every wedge of 90 is filled (by the next at 45)
    assert _flag([RING[i] for i in (0, 1, 2, 3, 4)]) == (True, 5)       # three consecutive neighbours removed: a gap of 180
    assert _flag([(1, 0), (0, 1), (-1, 0), (0, -1)]) == (False, 4)      # gaps of exactly 90: no boundary at theta = 90
    assert _flag([(1, 0), (0, 1), (-1, 0), (0, -1)], theta=89.0) == (True, 4)
    assert _flag([(1, 0), (0, 1)]) == (False, 2)                        # two neighbours: never a boundary at k = 3
    assert _flag([(1, 0), (0, 1)], k=3)[0] is False and _flag([(1, 0), (0, 1), (-1, 0)]) == (True, 3)
    # a duplicate of the point and a neighbour straight up the normal are no directions
    assert _flag(RING + [(0, 0), (0, 0, 1)]) == (False, 8)
    assert _flag([(1, 0), (0, 1), (0, 0), (0, 0, 1)]) == (False, 2)
    # a neighbour beyond r = 0.4 is none: (2, 0) * 0.25 = 0.5
    assert _flag([(1, 0), (0, 1), (-2, 0)]) == (False, 2)
    # a non-finite row is nobody's neighbour and gets no flag; a point with a non-finite or zero normal gets none
    flag, n = _flag([RING[i] for i in (0, 1, 2, 3, 4)], extra=[(np.nan, 0, 0), (2.0, np.inf, 0.75)])
    assert (flag, n) == (True, 5)
    pts = np.array([[0, 0, 0], [0.25, 0, 0], [0, 0.25, 0], [-0.25, 0, 0], [np.nan, 0, 0]], dtype=F)
    nrm = np.tile(UP, (5, 1))
    # (rows 1 and 3 see two neighbours only, rows 0 and 2 three on one side)
    assert G.restate_boundary(pts, nrm, 0.4)[0].tolist() == [True, False, True, False, False]
    for bad in ((np.nan, 0, 1), (0, 0, 0), (np.inf, 0, 0)):
        nb = nrm.copy()
        nb[0] = bad
        assert not G.restate_boundary(pts, nb, 0.4)[0][0]
    # theta = 180: a boundary only when every direction lies in one closed half-plane
    assert _flag([(1, 0), (0, 1), (-1, 0)], theta=180.0) == (False, 3)           # a half-plane closed by both ends: the gap is exactly 180
    assert _flag([(1, 0), (0, 1), (-1, 0), (0, -1)], theta=180.0) == (False, 4)
    assert _flag([(1, 0), (1, 1), (0, 1)], theta=180.0) == (True, 3)
    assert _flag([(1, 0), (0, 1), (-1, -1)], theta=180.0) == (False, 3)
    # the frame follows the normal: the same ring in the plane x = const, seen along (1, 0, 0)
    ring_yz = [(0, a, b) for a, b in RING]
    assert _flag(ring_yz, normal=(1, 0, 0)) == (False, 8)
    assert _flag([ring_yz[i] for i in (0, 1, 2, 3, 4)], normal=(-1, 0, 0)) == (True, 5)
    # seen along UP the ring in x = const collapses onto one line: two rows lie along the normal, six on the two opposite rays
    assert _flag(ring_yz, normal=UP) == (True, 6)


# ---------------------------------------------------------------- the scenes are honest before the GPU sees them
@pytest.mark.parametrize("seed", G.HF_SEEDS)
def test_height_field_plain_icp_slides_and_the_boundary_rejector_holds(seed):
    """Every source point beyond the target's edge finds an edge point within a metre and pulls: the plain ICP slides the source on
    top of the target.  Measured with this restatement (Frobenius distance from the truth, seeds 1 / 3 / 4): plain 3.95 / 4.03 / 4.01,
    boundary rejector 0.034 / 0.019 / 0.108."""
    src, _, tgt, tn, T_true, guess = G.height_field_pair(seed)
    flags, counts = G.restate_boundary(tgt, tn, G.HF_RADIUS)
    share = flags.mean()
    plain = G.restate_icp_geometry(src, tgt, None, guess, G.HF_MAX_CORR, G.HF_ITER, G.HF_EPS)
    held = G.restate_icp_geometry(src, tgt, None, guess, G.HF_MAX_CORR, G.HF_ITER, G.HF_EPS, g=G.geo(boundary=1, boundary_radius=G.HF_RADIUS),
                                  flags=flags)
    e_plain, e_held = G.frobenius(plain[0], T_true), G.frobenius(held[0], T_true)
    print(f"height field {seed}: flagged {share:.3f}, directions {counts.min()} .. {counts.max()}, plain {e_plain:.3f} ({plain[1]} it), "
          f"boundary {e_held:.3f} ({held[1]} it), last iteration {held[6]}")
    assert 0.04 < share < 0.10
    assert e_plain > 1.0, e_plain
    assert e_held < 0.25, e_held
    gs = held[6]
    assert gs["on_boundary"] > 0 and gs["passed"] == gs["matched"] - gs["on_boundary"] and gs["target_boundary_points"] == int(flags.sum())


@pytest.mark.parametrize("seed", [7, 8, 9])
def test_slanted_cabinet_pulls_the_plain_icp_and_the_normal_rejector_holds(seed):
    """The front leaves the wall at 40 degrees, so a 30 degree agreement test drops every correspondence between the front and
    the wall or the floor.  Measured with this restatement (Frobenius distance from the truth, seeds 7 / 8 / 9): plain 0.079 /
    0.095 / 0.074, normals: 30 below 1e-6.  The margin asserted is 0.03: less than half the smallest difference measured."""
    tgt, nrm, src, src_n, T_true, guess = G.slanted_cabinet(seed)
    plain = G.restate_icp_geometry(src, tgt, None, guess, 1.0, 50, 1e-10)
    held = G.restate_icp_geometry(src, tgt, None, guess, 1.0, 50, 1e-10, g=G.geo(normals=1, normal_angle_deg=30.0), src_nrm=src_n, tgt_nrm=nrm)
    e_plain, e_held = G.frobenius(plain[0], T_true), G.frobenius(held[0], T_true)
    print(f"slanted cabinet {seed}: plain {e_plain:.3g}, normals 30 {e_held:.3g}, last iteration {held[6]}")
    assert e_plain > e_held + 0.03, (e_plain, e_held)
    assert e_held < 1e-4
    assert held[6]["normal_mismatch"] > 0 and held[6]["on_boundary"] == 0


def test_nothing_dropped_is_the_restated_rejection():
    """With no bit set, and with normals at 90 degrees on finite normals, the loop is restate_icp_rejecting's, bit for bit."""
    tgt, nrm, src, _, guess = cabinet(7)
    o = VARIANTS["one-to-one + trimmed 0.7"]
    ref = restate_icp_rejecting(src, tgt, None, guess, 1.0, 30, 1e-9, o)
    src_n = np.tile(np.array([0.6, 0.0, 0.8], dtype=np.float32), (len(src), 1))
    for g in (G.GEO_DEFAULT, G.geo(normals=1, normal_angle_deg=90.0)):
        got = G.restate_icp_geometry(src, tgt, None, guess, 1.0, 30, 1e-9, o, g, src_nrm=src_n, tgt_nrm=nrm)
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)) and got[1:3] == ref[1:3] and got[5] == ref[5]
        assert got[6]["passed"] == got[6]["matched"] and got[6]["normal_mismatch"] == 0

"""The MLS smoothing, everything a machine without a GPU can check: the header and the library's exports, the plumbing of the
stage, the shim's MM3D_SMOOTH parser, the numpy restatement of the rule (tests/smooth_cases.py) against second formulations,
that every case is what it is for, and the claims the stage was added on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import smooth_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FUNCTIONS = ("mm3d_smooth_options_default", "mm3d_set_smoothing", "mm3d_get_smoothing", "mm3d_last_smooth_stats",
             "mm3d_smooth_displacements", "mm3d_smooth_cloud")


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


def test_header_declares_the_smoothing():
    h = _read("include", "mm3d.h")
    assert re.search(r"MM3D_SMOOTH_OFF\s*=\s*0\s*,\s*MM3D_SMOOTH_MLS\s*=\s*1\s*}\s*mm3d_smooth_method;", h)
    assert re.search(r"enum\s*{\s*MM3D_SMOOTH_MAPS\s*=\s*1\s*,\s*MM3D_SMOOTH_COMPOSED\s*=\s*2\s*};", h)
    assert re.search(r"typedef struct mm3d_smooth_options\s*{\s*int method;[^}]*int order;[^}]*int min_neighbours;[^}]*int where;[^}]*double radius;[^}]*}"
                     r"\s*mm3d_smooth_options;", h)
    assert re.search(r"typedef struct mm3d_smooth_stats\s*{\s*long long points, valid, few, degenerate, plane, polynomial;[^}]*double max_displacement;[^}]*}", h)
    for decl in (r"void mm3d_smooth_options_default\(mm3d_smooth_options \*o\);",
                 r"int mm3d_set_smoothing\(mm3d_ctx \*ctx, const mm3d_smooth_options \*options\);",
                 r"int mm3d_get_smoothing\(const mm3d_ctx \*ctx, mm3d_smooth_options \*options\);",
                 r"int mm3d_last_smooth_stats\(const mm3d_ctx \*ctx, mm3d_smooth_stats \*stats\);",
                 r"int mm3d_smooth_displacements\(mm3d_ctx \*ctx, const mm3d_cloud \*points, double radius, int order, int min_neighbours,\s*"
                 r"double \*disp, int \*state, int \*neighbours, size_t capacity, mm3d_smooth_stats \*stats\);",
                 r"int mm3d_smooth_cloud\(mm3d_ctx \*ctx, const mm3d_cloud \*in, double radius, int order, int min_neighbours, mm3d_cloud \*\*out\);"):
        assert re.search(decl, h), decl
    # the rule is stated to the operation, and what it is no copy of
    for text in ("(double)d2 <= r * r", "d2 = (dx * dx + dy * dy) + dz * dz in float", "w_j = exp(-(double)d2_j / (r * r))", "o = (mu . n) n",
                 "lambda1 - lambda0 <= 1e-6 * trace", "1e-9 * trace(M) / 6", "(float)((double)p + displacement)", "pcl::MovingLeastSquares",
                 "downsample(smooth(downsample(cat, res), radius), res)"):
        assert text in h, text
    body = h[:h.index("} mm3d_params;")]                                      # mm3d_params carries nothing of it
    assert "smooth" not in body[body.rindex("typedef struct"):]


def test_library_exports_mirror_and_defaults(mm):
    """A test that fails without the feature: the names are in libmm3d.so."""
    L = mm.lib()
    for name in FUNCTIONS:
        assert hasattr(L, name), name
    o = mm.SmoothOptions()
    assert C.sizeof(o) == 24 and o.as_tuple() == (mm.SmoothMethod.OFF, 2, 6, mm.SmoothWhere.MAPS | mm.SmoothWhere.COMPOSED, 0.0)
    assert C.sizeof(mm.SmoothStats) == 56
    assert (int(mm.SmoothMethod.OFF), int(mm.SmoothMethod.MLS), int(mm.SmoothWhere.MAPS), int(mm.SmoothWhere.COMPOSED)) == (0, 1, 1, 2)
    assert [int(s) for s in mm.SmoothState] == [sc.INVALID, sc.FEW, sc.DEGENERATE, sc.PLANE, sc.POLYNOMIAL] == [0, 1, 2, 3, 4]
    for method in ("setSmoothing", "getSmoothing", "smoothDisplacements", "smoothCloud"):
        assert callable(getattr(mm.Context, method))
    assert isinstance(mm.Context.last_smooth_stats, property)
    L.mm3d_smooth_options_default(None)                                       # a NULL is ignored
    with pytest.raises(TypeError):
        mm.SmoothOptions(size=3)
    out = C.c_void_p()
    assert L.mm3d_set_smoothing(None, C.byref(o)) == EINVAL and L.mm3d_get_smoothing(None, C.byref(o)) == EINVAL
    assert L.mm3d_smooth_cloud(None, None, C.c_double(0.3), 2, 6, C.byref(out)) == EINVAL
    assert L.mm3d_smooth_displacements(None, None, C.c_double(0.3), 2, 6, None, None, None, C.c_size_t(0), None) == EINVAL
    assert L.mm3d_last_smooth_stats(None, None) == EINVAL


def test_sources_carry_the_stage():
    """The plumbing of DESIGN.md section 7h, as the other stages' tests read it."""
    assert "smooth_mls.hip" in _read("map-merge_amd", "build.sh")
    assert "smooth_mls" not in _read("map-merge_amd", "csrc", "host_sources.sh")              # it holds kernels
    t = _read("map-merge_amd", "csrc", "types.hpp")
    assert "struct SmootherBase" in t and "const SmootherBase *smoother = nullptr;" in t and "mm3d_smooth_options smooth_options;" in t
    assert "last_smooth_stats" in t
    pe = _read("map-merge_amd", "csrc", "pair_estimate.cpp")
    assert "sel.smoother->smooth(" in pe and "MM3D_SMOOTH_MAPS" in pe
    assert pe.index("sel.clusters->filter(") < pe.index("sel.smoother->smooth(") < pe.index("compute_normals(")     # after the filters, before the normals
    capi = _read("map-merge_amd", "csrc", "capi.cpp")
    assert "sel.smoother->smooth(" in capi and "MM3D_SMOOTH_COMPOSED" in capi and "mm3d_smooth_options_default(&smooth_options)" in capi
    assert "smooth_options" in _read("map-merge_amd", "csrc", "map_cache.cpp")
    k = _read("map-merge_amd", "csrc", "smooth_mls.hip")
    assert "select_stage(ctx, Stage::Smoothing" in k and "wave_sum" in k and "solve6_ldlt(" in k and "sym_eig3(" in k
    # the stage travels in the bundles (the peers of a device list follow): its row of the stage table gives no reason to stay home
    rules = _read("map-merge_amd", "csrc", "stage_rules.cpp")
    assert re.search(r'\{"mm3d_set_smoothing",[^\n]*\n[^\n]*"the MLS smoothing is selected", nullptr\},', rules)
    assert "voxel_leaf =" not in k                                             # the smoothed cloud is no voxel grid's output
    assert '#include "sym_eig3.hpp"' in _read("map-merge_amd", "csrc", "shot.hip")            # one text for both eigen-solves
    assert "rand(" not in k
    d = _read("DESIGN.md")
    assert "thirteen stages" in d and re.search(r"^#+ 7p\b", d, re.M)
    assert "mm3d_set_smoothing" in _read("README.md") and "MM3D_SMOOTH" in _read("INTEGRATION.md")


# ---------------------------------------------------------------- the shim
SHIM_CASES = r"""
#include <cstdio>
#include <cstring>
#include "map_merge_3d_shim.hpp"
using map_merge_3d::mm3d_shim::parse_smooth;
static int refused(const char *v) { try { (void)parse_smooth(v); } catch (const std::runtime_error &e) { return std::strstr(e.what(), "MM3D_SMOOTH") != nullptr; } return 0; }
static int is(const mm3d_smooth_options &o, int m, int order, int where, double r) { return o.method == m && o.order == order && o.min_neighbours == 6 && o.where == where && o.radius == r; }
int main()
{
  const int both = MM3D_SMOOTH_MAPS | MM3D_SMOOTH_COMPOSED;
  if (!is(parse_smooth(nullptr), MM3D_SMOOTH_OFF, 2, both, 0.0)) return 1;
  if (!is(parse_smooth(""), MM3D_SMOOTH_OFF, 2, both, 0.0)) return 2;
  if (!is(parse_smooth("off"), MM3D_SMOOTH_OFF, 2, both, 0.0)) return 3;
  if (!is(parse_smooth("mls"), MM3D_SMOOTH_MLS, 2, both, 0.0)) return 4;
  if (!is(parse_smooth("mls:1"), MM3D_SMOOTH_MLS, 1, both, 0.0)) return 5;
  if (!is(parse_smooth("mls:2:0.25"), MM3D_SMOOTH_MLS, 2, both, 0.25)) return 6;
  if (!is(parse_smooth("mls@maps"), MM3D_SMOOTH_MLS, 2, MM3D_SMOOTH_MAPS, 0.0)) return 7;
  if (!is(parse_smooth("mls:1:.5@composed"), MM3D_SMOOTH_MLS, 1, MM3D_SMOOTH_COMPOSED, 0.5)) return 8;
  if (!is(parse_smooth("mls:2@composed"), MM3D_SMOOTH_MLS, 2, MM3D_SMOOTH_COMPOSED, 0.0)) return 9;
  const char *bad[] = {"garbage", "mls:", "mls:0", "mls:3", "mls:-1", "mls:abc", "mls:2:", "mls:2:0", "mls:2:-1", "mls:2:nan", "mls:2:inf",
                       "mls:2:0.25x", "mls:2:0.25:1", "mls:1.5", "mls: 2", "mlss", "MLS", "on", "mls::1", "mls@", "mls@both", "mls@maps@composed",
                       "mls:2@Maps", "@maps", "off@maps", "mls:12", "mls:2: 0.3"};
  for (const char *b : bad) if (!refused(b)) { std::printf("accepted '%s'\n", b); return 10; }
  std::puts("shim smooth: ok");
  return 0;
}
"""


def test_shim_parses_mm3d_smooth(tmp_path):
    """Compiled with the flags tests/shim/build.sh compiles the shim with; the parser lies outside the header's PCL guard."""
    src = tmp_path / "shim_smooth.cpp"
    src.write_text(SHIM_CASES)
    exe = tmp_path / "shim_smooth"
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0 and "shim smooth: ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    s = _read("include", "map_merge_3d_shim.hpp")
    assert s.count('parse_smooth(std::getenv("MM3D_SMOOTH"))') == 2 and "mm3d_set_smoothing(e, &smooth)" in s     # the estimation and the compositing context


# ---------------------------------------------------------------- the restatement
def _some(name):
    """At most 150 records of a case, spread over it: the second formulations run on these."""
    n = len(sc.cases()[name][0])
    return np.arange(n) if n <= 150 else np.unique(np.linspace(0, n - 1, 150).astype(np.int64))


@pytest.mark.parametrize("name", sorted(sc.cases()))
def test_restatement_equals_its_second_formulations(name):
    """The neighbour order permuted, np.longdouble throughout (with a Jacobi solver in eigh's place), and another u, v frame:
    the same states and counts, the displacements within 1e-13 r."""
    xyz, r, min_nb = sc.cases()[name]
    q = _some(name)
    ref = sc.reference(name)
    worst = 0.0
    for label, kw in (("permuted", dict(shuffle=np.random.default_rng(7))), ("longdouble", dict(dtype=np.longdouble)), ("frame", dict(frame=0.7))):
        other = sc.smooth(xyz, r, min_nb, queries=q, **kw)
        for key in ("count", "state1", "state2"):
            assert np.array_equal(other[key], ref[key][q]), (name, label, key)
        for key in ("disp1", "disp2"):
            diff = float(np.abs(other[key] - ref[key][q]).max()) if len(q) else 0.0
            worst = max(worst, diff / r)
            assert diff <= 1e-13 * r, (name, label, key, diff / r)
    print(name, "records", len(q), "worst difference / r", worst)


@pytest.mark.parametrize("name", sorted(sc.cases()))
def test_every_case_is_what_it_is_for(name):
    """The conditions that give the device's tolerance its meaning (test_gpu_smoothing.py): away from the planted cases the
    plane is well separated, every pivot is far above its floor, no displacement is long, and no d2 is near r * r."""
    xyz, r, min_nb = sc.cases()[name]
    ref = sc.reference(name)
    valid = sc.valid_rows(xyz)
    assert np.array_equal(ref["state2"] == sc.INVALID, ~valid) and np.array_equal(ref["state1"] == sc.INVALID, ~valid)
    assert (ref["count"][~valid] == 0).all() and (ref["count"][valid] >= 1).all()
    assert np.array_equal(ref["state1"] == sc.FEW, valid & (ref["count"] < min_nb)) and np.array_equal(ref["state2"] == sc.FEW, ref["state1"] == sc.FEW)
    assert (ref["state1"] != sc.POLYNOMIAL).all() and ((ref["state2"] == sc.POLYNOMIAL) <= (ref["count"] >= sc.POLY_MIN)).all()
    assert (ref["disp2"][ref["state2"] <= sc.DEGENERATE] == 0).all() and (ref["disp1"][ref["state1"] <= sc.DEGENERATE] == 0).all()
    assert (ref["margin"] >= 4.0).all(), ref["margin"].min()                  # no d2 within 4 ulps of r * r but the planted exact ones
    fitted = ref["state1"] >= sc.DEGENERATE
    tried = np.isfinite(ref["pivot"])
    length = max(np.sqrt((ref["disp1"] ** 2).sum(axis=1)).max(), np.sqrt((ref["disp2"] ** 2).sum(axis=1)).max()) if len(xyz) else 0.0
    print(name, "records", len(xyz), "order 1", ref["stats1"], "order 2", ref["stats2"], "smallest gap", ref["gap"][fitted].min() if fitted.any() else None,
          "smallest pivot / floor", ref["pivot"][tried].min() if tried.any() else None, "longest / r", length / r)
    assert length <= r / 2
    if name == "e_collinear":
        assert fitted.all() and (ref["gap"][:30] == 0.0).all() and np.isnan(ref["gap"][30:]).all()      # the lines: exactly zero; the repeated point: no trace
        assert (ref["state1"] == sc.DEGENERATE).all() and (ref["state2"] == sc.DEGENERATE).all() and (ref["count"][30:] == 5).all()
    elif name == "f_conic_ring":
        assert (ref["count"] == 12).all() and tried.all() and (ref["pivot"] <= 1e-3).all()           # singular: rounding noise under the floor
        assert (ref["state2"] == sc.PLANE).all() and (ref["gap"] >= 1e-3).all() and np.array_equal(ref["disp1"], ref["disp2"])
    else:
        assert name not in sc.PLANTED
        assert (ref["gap"][fitted] >= 1e-3).all() and (ref["pivot"][tried] >= 1e3).all()
        assert (ref["state1"][fitted] == sc.PLANE).all()
        assert np.array_equal(ref["state2"] == sc.POLYNOMIAL, fitted & (ref["count"] >= sc.POLY_MIN))


def test_the_cases_by_hand():
    c = sc.cases()
    assert len(c["a_sphere_cap"][0]) == 750 and c["a_sphere_cap"][1] == 0.3
    lattice = c["b_plane_lattice"][0].astype(np.float64) * 16.0
    assert np.array_equal(lattice, np.rint(lattice))                             # multiples of 2^-4
    assert np.abs(sc.reference("b_plane_lattice")["disp2"]).max() <= 1e-15 and np.abs(sc.reference("b_plane_lattice")["disp1"]).max() <= 1e-15
    thr = c["c_threshold"][0].astype(np.float64)
    assert np.array_equal(thr * 64.0, np.rint(thr * 64.0)) and c["c_threshold"][1] == 0.5
    d = np.linalg.norm(thr[1::2] - thr[0::2], axis=1)
    assert (d[:8] == 0.5).all() and (d[8:16] == 0.5 + 2.0 ** -6).all() and (d[16:] == 0.5).all()
    for cell in (0.5, 0.505, 0.51):                                              # pairs on both sides of a cell border, neighbours and not
        k = np.floor((thr[:32, 0] - thr[:, 0].min()) / cell)
        split = k[0::2] != k[1::2]
        assert split[:8].any() and split[8:].any()
    assert sc.reference("c_threshold")["count"].tolist() == sc.THRESHOLD_COUNTS
    cb = sc.reference("d_count_boundaries")
    sizes = np.repeat(sc.COUNTS_SIZES, sc.COUNTS_SIZES)
    assert sc.COUNTS_SIZES == (sc.COUNTS_MIN - 1, sc.COUNTS_MIN, 5, 6, 7) and np.array_equal(cb["count"], sizes)
    assert np.array_equal(cb["state1"], np.where(sizes < sc.COUNTS_MIN, sc.FEW, sc.PLANE))
    assert np.array_equal(cb["state2"], np.where(sizes < sc.COUNTS_MIN, sc.FEW, np.where(sizes < 6, sc.PLANE, sc.POLYNOMIAL)))
    inv = c["g_invalid_and_duplicates"][0]
    bad = ~np.isfinite(inv).all(axis=1)
    assert bad[0] and bad[-1] and bad.sum() == 10
    for col in range(3):
        assert np.isnan(inv[:, col]).any() and (inv[:, col] == np.inf).any() and (inv[:, col] == -np.inf).any()
    assert len(np.unique(inv[~bad], axis=0)) < len(inv[~bad]) - 30               # exact duplicates
    dense, r, _ = c["h_dense_blob"]
    assert len(dense) == 5000 and (sc.reference("h_dense_blob")["count"] == 5000).all()
    assert np.linalg.norm(dense.astype(np.float64) - dense.astype(np.float64).mean(axis=0), axis=1).max() < r / 2
    for name, base in sc.TRANSLATED.items():                                     # exact translations: the same neighbours, the same fit
        a, b = sc.reference(name), sc.reference(base)
        for key in ("count", "state1", "state2"):
            assert np.array_equal(a[key], b[key]), (name, key)
        assert np.abs(a["disp2"] - b["disp2"]).max() <= 1e-13 * c[name][1]
    assert c["m_room_1_at_10km"][0][:, 0].min() >= 9999.9 and 3500 <= len(c["n_room_2"][0]) <= 4500
    assert len(sc.reference("p_empty")["state2"]) == 0 and sc.reference("p_empty")["stats2"]["max_displacement"] == 0.0
    assert sc.reference("q_one_point")["state2"].tolist() == [sc.FEW] and sc.reference("q_one_point")["count"].tolist() == [1]


# ---------------------------------------------------------------- the claims the stage was added on
def _rms(xyz, centre, R):
    return float(np.sqrt(np.mean((np.linalg.norm(xyz.astype(np.float64) - centre, axis=1) - R) ** 2)))


def test_double_wall_is_fused():
    """Two noisy copies of a cap 0.04 m apart: voxel pass, smoothing at r = 0.15 m, voxel pass again.  The RMS distance to the
    surface between them at most halves (measured 0.15 - 0.29 of what it was) and the doubled layer becomes one: at least a
    fifth fewer points (measured about a third)."""
    a, b, centre, R = sc.double_wall_layers()
    first = sc.double_wall()
    ref = sc.reference("o_double_wall")
    fused = sc.voxel_centroids(sc.apply(first, ref["disp2"], ref["state2"]), sc.WALL_LEAF)
    before, after = _rms(first, centre, R), _rms(fused, centre, R)
    print("double wall: points", len(first), "->", len(fused), "rms", before, "->", after, "ratio", after / before)
    assert 0.015 <= before <= 0.025
    assert after / before <= 0.5
    assert len(fused) <= 0.8 * len(first)


def test_one_noisy_surface_is_smoothed():
    """The sphere cap at sigma = 0.02, r = 0.3: away from the rim the order-2 RMS surface error falls to at most 0.6 of what it
    was (measured 0.25 - 0.42), and the order-1 plane projection is biased towards the centre of curvature: its mean signed
    error is negative, which is why order 2 is the default."""
    xyz, r, _ = sc.cases()["a_sphere_cap"]
    centre, R = np.array([5.0, -3.0, 1.0]), sc.SPHERE_R
    ref = sc.reference("a_sphere_cap")
    p = xyz.astype(np.float64)
    cos_max = 1.0 - (750 / 100.0) / (2.0 * np.pi * R * R)
    inner = np.arccos(np.clip((p[:, 2] - centre[2]) / np.linalg.norm(p - centre, axis=1), -1, 1)) <= np.arccos(cos_max) - r / R     # a radius from the rim
    err0 = np.linalg.norm(p - centre, axis=1) - R
    err1 = np.linalg.norm(p + ref["disp1"] - centre, axis=1) - R
    err2 = np.linalg.norm(p + ref["disp2"] - centre, axis=1) - R
    rms = lambda e: float(np.sqrt(np.mean(e[inner] ** 2)))
    print("sphere: inner points", int(inner.sum()), "rms", rms(err0), "order 1", rms(err1), "bias", float(err1[inner].mean()), "order 2", rms(err2),
          "bias", float(err2[inner].mean()))
    assert inner.sum() >= 200 and 0.015 <= rms(err0) <= 0.025
    assert rms(err2) / rms(err0) <= 0.6
    assert err1[inner].mean() < 0.0 and abs(err2[inner].mean()) < abs(err1[inner].mean())

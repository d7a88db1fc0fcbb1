"""NDT refinement without a GPU: the header declares it, the ctypes mirror binds it, the defaults and the NULL handling of the
entry points that touch no device, and the numpy restatement of tests/test_gpu_ndt.py -- voxel table plus loop -- pulls a
displaced box room back towards the truth."""
import ctypes as C
import os
import re

import numpy as np

from test_gpu_icp_plane import _problem
from test_gpu_ndt import restate_ndt, restate_table, voxel_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


def test_header_declares_the_refinement():
    h = _read("include", "mm3d.h")
    assert re.search(r"MM3D_REFINE_ICP\s*=\s*0\s*,\s*MM3D_REFINE_NDT\s*=\s*1", h)
    assert re.search(r"typedef struct mm3d_refine_options \{\s*int method;[^}]*double resolution;[^}]*int neighbours;[^}]*int min_points;"
                     r"[^}]*double regularisation;[^}]*\} mm3d_refine_options;", h)
    assert re.search(r"void mm3d_refine_options_default\(mm3d_refine_options \*o\);", h)
    assert re.search(r"int mm3d_set_refinement\(mm3d_ctx \*ctx, const mm3d_refine_options \*options\);", h)
    assert re.search(r"int mm3d_get_refinement\(const mm3d_ctx \*ctx, mm3d_refine_options \*options\);", h)
    assert re.search(r"int mm3d_estimate_transform_ndt\(mm3d_ctx \*ctx, const mm3d_cloud \*source, const mm3d_cloud \*target, "
                     r"const float initial_guess\[16\],\s*const mm3d_refine_options \*options, int max_iterations, "
                     r"double transformation_epsilon,\s*float T\[16\]\);", h)
    assert re.search(r"int mm3d_debug_ndt_voxels\(mm3d_ctx \*ctx, const mm3d_cloud \*target, const mm3d_refine_options \*options,", h)
    # the ICP method's enum did not grow: NDT is not an ICP method
    assert re.search(r"typedef enum \{ MM3D_ICP_POINT_TO_POINT = 0, MM3D_ICP_POINT_TO_PLANE = 1 \} mm3d_icp_method;", h)
    assert "2^26" in h and "2^26" in _read("INTEGRATION.md")      # the index limit is stated in both


def test_mirror_binds_the_entry_points(mm):
    for name in ("setRefinement", "getRefinement", "estimateTransformNDT", "ndtVoxels"):
        assert callable(getattr(mm.Context, name))
    lib = mm.lib()
    for name in ("mm3d_refine_options_default", "mm3d_set_refinement", "mm3d_get_refinement", "mm3d_estimate_transform_ndt",
                 "mm3d_debug_ndt_voxels"):
        assert getattr(lib, name)
    assert (mm.RefineMethod.ICP, mm.RefineMethod.NDT) == (0, 1)


def test_defaults_and_null_handling(mm):
    o = mm.RefineOptions()
    assert o.as_tuple() == (0, 0.0, 7, 6, 0.01)
    lib = mm.lib()
    lib.mm3d_refine_options_default(None)                # a no-op, not a crash
    assert lib.mm3d_set_refinement(None, C.byref(o)) == EINVAL
    assert lib.mm3d_get_refinement(None, C.byref(o)) == EINVAL
    T = (C.c_float * 16)()
    n = C.c_size_t()
    assert lib.mm3d_estimate_transform_ndt(None, None, None, T, C.byref(o), 10, C.c_double(1e-9), T) == EINVAL
    assert lib.mm3d_debug_ndt_voxels(None, None, C.byref(o), None, None, None, None, None, C.c_size_t(0), C.byref(n)) == EINVAL


def test_shim_selects_the_refinement_from_the_environment():
    s = _read("include", "map_merge_3d_shim.hpp")
    assert 'std::getenv("MM3D_REFINE")' in s
    assert "mm3d_set_refinement(e, &refine)" in s
    assert re.search(r"ndt.*MM3D_DEVICES", s)


def test_voxels_of_points_on_lattice_planes():
    p = np.array([[0.0, -0.0, 1.0], [-1.0, -1e-7, 0.99999994], [2.5, -2.5, 3.0]], dtype=np.float32)
    assert voxel_of(p, 1.0).tolist() == [[0, 0, 1], [-1, -1, 0], [2, -3, 3]]
    assert voxel_of(p, 0.5).tolist() == [[0, 0, 2], [-2, -1, 1], [5, -5, 6]]


def test_restatement_table_is_the_sample_covariance_inverted():
    rng = np.random.default_rng(1)
    pts = (rng.normal(size=(400, 3)) * [0.2, 0.1, 0.05] + [0.5, 0.5, 0.5]).astype(np.float32)
    pts = pts[(voxel_of(pts, 1.0) == 0).all(axis=1)]
    (key, (cnt, mu, P)), = restate_table(pts, 1.0, 6, 0.01).items()
    assert key == (0, 0, 0) and cnt == len(pts)
    S = np.cov(pts.astype(np.float64).T)
    S += 0.01 * np.trace(S) / 3.0 * np.eye(3)
    Pm = np.array([[P[0], P[1], P[2]], [P[1], P[3], P[4]], [P[2], P[4], P[5]]])
    assert np.allclose(mu, pts.astype(np.float64).mean(axis=0), rtol=0, atol=1e-14)
    assert np.allclose(Pm @ S, np.eye(3), atol=1e-10)
    assert restate_table(pts[:5], 1.0, 6, 0.01)[(0, 0, 0)][2] is None            # fewer than min_points
    assert restate_table(np.tile(pts[:1], (8, 1)), 1.0, 6, 0.01)[(0, 0, 0)][2] is None   # coincident: trace 0


def test_restatement_pulls_the_box_room_towards_the_truth():
    tgt, _, src, T_true, guess = _problem(7, 5000)
    T, it, conv, margins, n_pts = restate_ndt(src, tgt, guess, 1.0)
    assert it >= 2
    assert min(margins) > 0.01
    assert n_pts > 4000
    e0, e1 = np.abs(guess - T_true).max(), np.abs(T - T_true).max()
    print("iterations", it, "converged", conv, "pose error", e0, "->", e1, "smallest margin", min(margins))
    assert e1 <= 0.25 * e0, (e0, e1)

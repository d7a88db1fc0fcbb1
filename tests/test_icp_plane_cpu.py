"""Point-to-plane ICP without a GPU: the header declares it, the numpy restatement of tests/test_gpu_icp_plane.py composes its
increment in PCL's order, and the shim's MM3D_ICP handling is there (the shim itself compiles in test_shim_cpu.py)."""
import os
import re

import numpy as np

from test_gpu_icp_plane import construct_transform, restate_icp_plane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


def test_header_declares_the_icp_method():
    h = _read("include", "mm3d.h")
    assert re.search(r"MM3D_ICP_POINT_TO_POINT\s*=\s*0\s*,\s*MM3D_ICP_POINT_TO_PLANE\s*=\s*1", h)
    assert re.search(r"int mm3d_set_icp_method\(mm3d_ctx \*ctx, int method\);", h)
    assert re.search(r"int mm3d_get_icp_method\(const mm3d_ctx \*ctx\);", h)
    assert re.search(r"int mm3d_estimate_transform_icp_plane\(mm3d_ctx \*ctx, const mm3d_cloud \*source, const mm3d_cloud \*target,\s*"
                     r"const mm3d_normals \*target_normals, const float initial_guess\[16\],\s*double max_correspondence_distance, "
                     r"int max_iterations, double transformation_epsilon,\s*float T\[16\]\);", h)


def test_library_exports_the_icp_method():
    lib = os.path.join(ROOT, "map-merge_amd", "libmm3d.so")
    data = open(lib, "rb").read()
    for name in (b"mm3d_set_icp_method", b"mm3d_get_icp_method", b"mm3d_estimate_transform_icp_plane"):
        assert name in data


def test_composition_is_rz_ry_rx():
    def rx(a):
        c, s = np.cos(a), np.sin(a)
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])

    def ry(a):
        c, s = np.cos(a), np.sin(a)
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])

    def rz(a):
        c, s = np.cos(a), np.sin(a)
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])

    rng = np.random.default_rng(0)
    for _ in range(20):
        a, b, g = rng.uniform(-0.5, 0.5, 3)
        t = rng.normal(size=3)
        T = construct_transform(a, b, g, *t)
        assert np.allclose(T[:3, :3], rz(g) @ ry(b) @ rx(a), atol=1e-14)
        assert np.allclose(T[:3, 3], t) and np.array_equal(T[3], [0, 0, 0, 1])


def test_restatement_recovers_a_small_motion():
    # two orthogonal planes plus a third: the restatement converges to the motion that made the source
    rng = np.random.default_rng(3)
    n = 600
    a, b = rng.uniform(0, 2, (n, 1)), rng.uniform(0, 2, (n, 1))
    z0 = np.c_[a, b, np.zeros((n, 1))]
    y0 = np.c_[a, np.zeros((n, 1)), b]
    x0 = np.c_[np.zeros((n, 1)), a, b]
    tgt = np.concatenate([z0, y0, x0]).astype(np.float32)
    nrm = np.concatenate([np.tile([0, 0, 1.0], (n, 1)), np.tile([0, 1.0, 0], (n, 1)), np.tile([1.0, 0, 0], (n, 1))]).astype(np.float32)
    T_true = construct_transform(0.01, -0.02, 0.015, 0.03, -0.02, 0.01)
    src = (np.linalg.inv(T_true) @ np.c_[tgt.astype(np.float64), np.ones(len(tgt))].T).T[:, :3].astype(np.float32)
    T, it, conv, _ = restate_icp_plane(src, tgt, -nrm, np.eye(4, dtype=np.float32), 0.5, 30, 1e-10)   # (normal sign: irrelevant)
    assert conv == 1 and it >= 2
    assert np.abs(T - T_true).max() < 1e-4


def test_shim_selects_the_icp_method_from_the_environment():
    s = _read("include", "map_merge_3d_shim.hpp")
    assert 'std::getenv("MM3D_ICP")' in s
    assert "mm3d_set_icp_method(e, MM3D_ICP_POINT_TO_PLANE)" in s
    assert re.search(r"point_to_plane.*MM3D_DEVICES", s)

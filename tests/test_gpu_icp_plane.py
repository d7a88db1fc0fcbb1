"""Point-to-plane ICP (mm3d_set_icp_method, mm3d_estimate_transform_icp_plane): the surface, a known answer, a numpy restatement
of the loop the header states, non-finite normals, a degenerate system, bit-identical results across the drivers, and the
default path untouched (cache key included)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POINT_TO_POINT, POINT_TO_PLANE = 0, 1
SAC_IA, MATCHING = 1, 0
EINVAL, EUNSUPPORTED = -1, -4


# ---------------------------------------------------------------- the restatement (also read by test_icp_plane_cpu.py)
def construct_transform(alpha, beta, gamma, tx, ty, tz):
    """PCL's constructTransformationMatrix, written out: [Rz(gamma) Ry(beta) Rx(alpha) | t] (double)."""
    sa, ca, sb, cb, sg, cg = np.sin(alpha), np.cos(alpha), np.sin(beta), np.cos(beta), np.sin(gamma), np.cos(gamma)
    T = np.eye(4)
    T[0, :3] = [cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca]
    T[1, :3] = [sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca]
    T[2, :3] = [-sb, cb * sa, cb * ca]
    T[:3, 3] = [tx, ty, tz]
    return T


def _xform_f32(T, xyz):
    """device_util.hpp xform: ((T00 x + T01 y) + T02 z) + T03 in float, no fusion."""
    T = T.astype(np.float32)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1).astype(np.float32)


def _nearest(q, tgt, chunk=512):
    """Exact float nearest neighbour (d2 = (dx dx + dy dy) + dz dz in float, lowest index on ties)."""
    idx = np.empty(len(q), dtype=np.int64)
    d2 = np.empty(len(q), dtype=np.float32)
    for a in range(0, len(q), chunk):
        b = q[a:a + chunk]
        dx = b[:, None, 0] - tgt[None, :, 0]
        dy = b[:, None, 1] - tgt[None, :, 1]
        dz = b[:, None, 2] - tgt[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        k = np.argmin(d, axis=1)
        idx[a:a + chunk] = k
        d2[a:a + chunk] = d[np.arange(len(b)), k]
    return idx, d2


def _ldlt_solve(A, b, floor):
    L, D = np.eye(6), np.zeros(6)
    pivots = []
    for j in range(6):
        d = A[j, j] - sum(L[j, k] * L[j, k] * D[k] for k in range(j))
        pivots.append(d)
        if not d > floor:
            return None, pivots
        D[j] = d
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - sum(L[i, k] * L[j, k] * D[k] for k in range(j))) / d
    y = np.zeros(6)
    for i in range(6):
        y[i] = b[i] - sum(L[i, k] * y[k] for k in range(i))
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = y[i] / D[i] - sum(L[k, i] * x[k] for k in range(i + 1, 6))
    return x, pivots


def restate_icp_plane(src, tgt, nrm, guess, max_corr, max_iter, eps, tau=1e-12):
    """The loop of include/mm3d.h (mm3d_set_icp_method) in numpy: float32 transforms and distances, double sums and solve.
    Returns (T, iterations, converged, margins): margins = the relative distances of every convergence test from its
    threshold, and of every pivot from the degeneracy floor."""
    max_d2 = np.float32(max_corr * max_corr)
    if float(max_d2) > max_corr * max_corr:
        max_d2 = np.nextafter(max_d2, np.float32(-np.inf))
    T = np.asarray(guess, dtype=np.float32).copy()
    prev_mse, iters, margins = np.finfo(np.float64).max, 0, []
    while True:
        s = _xform_f32(T, src)
        idx, d2 = _nearest(s, tgt)
        ok = d2 <= max_d2
        cnt = int(ok.sum())
        if cnt < 3:
            return T, iters, 0, margins
        sd, d, n = s[ok].astype(np.float64), tgt[idx[ok]].astype(np.float64), nrm[idx[ok]].astype(np.float64)
        fin = np.isfinite(n).all(axis=1)
        sd, d, n = sd[fin], d[fin], n[fin]
        sx, sy, sz = sd[:, 0], sd[:, 1], sd[:, 2]
        nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
        A = np.stack([nz * sy - ny * sz, nx * sz - nz * sx, ny * sx - nx * sy, nx, ny, nz], axis=1)
        r = (nx * d[:, 0] + ny * d[:, 1] + nz * d[:, 2]) - (nx * sx + ny * sy + nz * sz)
        AtA, Atr = A.T @ A, A.T @ r
        floor = tau * np.trace(AtA) / 6.0
        x, pivots = _ldlt_solve(AtA, Atr, floor) if len(A) >= 6 else (None, [])
        margins += [abs(p - floor) / max(abs(floor), 1e-300) for p in pivots]
        if x is None:
            return T, iters, 0, margins
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
            return T, iters, 1, margins
        cos_angle = 0.5 * ((float(Ti[0, 0]) + float(Ti[1, 1]) + float(Ti[2, 2])) - 1.0)
        t2 = float(Ti[0, 3]) * float(Ti[0, 3]) + float(Ti[1, 3]) * float(Ti[1, 3]) + float(Ti[2, 3]) * float(Ti[2, 3])
        margins += [abs((1.0 - cos_angle) - eps) / eps, abs(t2 - eps) / eps]
        if cos_angle >= 1.0 - eps and t2 <= eps:
            return T, iters, 1, margins
        mse = float(d2[ok].astype(np.float64).sum()) / cnt
        if iters > 1:                                   # (the first compares with DBL_MAX)
            margins.append(abs(abs(mse - prev_mse) - 1e-12) / 1e-12)
        if abs(mse - prev_mse) < 1e-12:
            return T, iters, 1, margins
        prev_mse = mse


# ---------------------------------------------------------------- scenes
def box_room(seed, n, size=(8.0, 6.0, 3.0)):
    """Points on the six faces of a room and on one box inside it, with their exact normals."""
    rng = np.random.default_rng(seed)
    X, Y, Z = size
    faces = [((0, 0, 0), (X, 0, 0), (0, Y, 0), (0, 0, 1)), ((0, 0, Z), (X, 0, 0), (0, Y, 0), (0, 0, -1)),
             ((0, 0, 0), (X, 0, 0), (0, 0, Z), (0, 1, 0)), ((0, Y, 0), (X, 0, 0), (0, 0, Z), (0, -1, 0)),
             ((0, 0, 0), (0, Y, 0), (0, 0, Z), (1, 0, 0)), ((X, 0, 0), (0, Y, 0), (0, 0, Z), (-1, 0, 0)),
             ((2.0, 1.5, 0), (1.2, 0, 0), (0, 0, 1.0), (0, -1, 0)), ((2.0, 1.5, 0), (0, 0.8, 0), (0, 0, 1.0), (-1, 0, 0)),
             ((2.0, 1.5, 1.0), (1.2, 0, 0), (0, 0.8, 0), (0, 0, 1))]
    area = np.array([np.linalg.norm(np.cross(u, v)) for _, u, v, _ in faces])
    counts = rng.multinomial(n, area / area.sum())
    pts, nrm = [], []
    for (o, u, v, nn), k in zip(faces, counts):
        a, b = rng.random((k, 1)), rng.random((k, 1))
        pts.append(np.asarray(o) + a * np.asarray(u) + b * np.asarray(v))
        nrm.append(np.tile(np.asarray(nn, dtype=np.float64), (k, 1)))
    return np.concatenate(pts).astype(np.float32), np.concatenate(nrm).astype(np.float32)


def _rot(rx, ry, rz):
    return construct_transform(np.radians(rx), np.radians(ry), np.radians(rz), 0, 0, 0)[:3, :3]


def _pose(rx, ry, rz, t):
    T = np.eye(4)
    T[:3, :3] = _rot(rx, ry, rz)
    T[:3, 3] = t
    return T


def _records(xyz):
    out = np.zeros(len(xyz), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")])
    out["x"], out["y"], out["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out["rgba"] = 0xff808080
    return out


def _normals(nrm):
    out = np.zeros(len(nrm), dtype=[("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("curvature", "<f4")])
    out["nx"], out["ny"], out["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    return out


def _problem(seed, n):
    """(target points, their normals, source = the target moved by T_true^-1, T_true, a guess 2 degrees / 0.1 m off)."""
    tgt, nrm = box_room(seed, n)
    rng = np.random.default_rng(seed + 100)
    T_true = _pose(*rng.uniform(-10, 10, 3), rng.uniform(-0.5, 0.5, 3))
    src = (np.linalg.inv(T_true) @ np.c_[tgt.astype(np.float64), np.ones(len(tgt))].T).T[:, :3].astype(np.float32)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    off = _pose(*(2.0 * axis), 0.1 * axis[::-1])
    return tgt, nrm, src, T_true, (off @ T_true).astype(np.float32)


# ---------------------------------------------------------------- 1. surface
def test_surface(mm):
    c = mm.Context(0)
    assert c.getIcpMethod() == POINT_TO_POINT
    c.setIcpMethod(POINT_TO_PLANE)
    assert c.getIcpMethod() == POINT_TO_PLANE
    c.setIcpMethod(POINT_TO_POINT)
    assert c.getIcpMethod() == POINT_TO_POINT
    lib = mm.lib()
    for bad in (-1, 2, 99):
        assert lib.mm3d_set_icp_method(c._h, bad) == EINVAL
    assert lib.mm3d_set_icp_method(None, POINT_TO_PLANE) == EINVAL
    assert lib.mm3d_get_icp_method(None) == EINVAL
    assert c.getIcpMethod() == POINT_TO_POINT
    d = mm.Context(devices=[0])
    assert lib.mm3d_set_icp_method(d._h, POINT_TO_PLANE) == EUNSUPPORTED
    assert d.getIcpMethod() == POINT_TO_POINT
    d.close()
    c.setIcpMethod(POINT_TO_PLANE)
    cloud = _records(box_room(1, 2000)[0])
    with pytest.raises(mm.Mm3dError) as e:
        c.shardBegin([cloud, cloud], mm.MapMergingParams(descriptor_type=2), 0, 1)
    assert e.value.status == EUNSUPPORTED
    c.close()


def test_stage_rejects_mismatched_normals(mm):
    c = mm.Context(0)
    tgt, nrm, src, _, guess = _problem(3, 3000)
    with pytest.raises(mm.Mm3dError):
        c.estimateTransformICPPlane(c.cloud(_records(src)), c.cloud(_records(tgt)), c.normals(_normals(nrm[:-1])), guess, 1.0, 30, 1e-8)
    c.close()


# ---------------------------------------------------------------- 2. known answer
def test_known_answer_box_room(mm):
    c = mm.Context(0)
    tgt, _, src, T_true, guess = _problem(7, 30000)
    t_cloud = c.cloud(_records(tgt))
    normals = c.computeSurfaceNormals(t_cloud, 0.3)
    T = c.estimateTransformICPPlane(c.cloud(_records(src)), t_cloud, normals, guess, 1.0, 50, 1e-10)
    assert c.last_icp_converged == 1
    assert np.abs(T - T_true).max() < 1e-4, np.abs(T - T_true).max()
    c.close()


# ---------------------------------------------------------------- 3 / 4. against the restatement
def _against_restatement(mm, seed, n, nan_rows=0):
    tgt, nrm, src, _, guess = _problem(seed, n)
    if nan_rows:
        rng = np.random.default_rng(seed + 7)
        nrm = nrm.copy()
        nrm[rng.choice(len(nrm), nan_rows, replace=False)] = np.nan
    max_corr, max_iter, eps = 1.0, 30, 1e-9
    T_ref, it_ref, conv_ref, margins = restate_icp_plane(src, tgt, nrm, guess, max_corr, max_iter, eps)
    assert it_ref >= 2
    assert min(margins) > 0.01, "the restatement sits within 1 % of a threshold: the comparison would be borderline"
    c = mm.Context(0)
    T = c.estimateTransformICPPlane(c.cloud(_records(src)), c.cloud(_records(tgt)), c.normals(_normals(nrm)), guess, max_corr, max_iter, eps)
    assert (c.last_icp_iterations, c.last_icp_converged) == (it_ref, conv_ref)
    assert np.abs(T - T_ref).max() < 1e-4, np.abs(T - T_ref).max()
    c.close()


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_against_restatement(mm, seed):
    _against_restatement(mm, seed, 5000)


def test_non_finite_normals_are_skipped(mm):
    _against_restatement(mm, 21, 5000, nan_rows=300)


# ---------------------------------------------------------------- 5. degenerate
def test_single_plane_is_degenerate_not_nan(mm):
    rng = np.random.default_rng(5)
    tgt = np.c_[rng.uniform(0, 5, (4000, 2)), np.zeros(4000)].astype(np.float32)
    src = (tgt + np.array([0.05, -0.03, 0.02], dtype=np.float32)).astype(np.float32)
    guess = np.eye(4, dtype=np.float32)
    guess[:3, 3] = [0.01, 0.01, -0.01]
    c = mm.Context(0)
    t_cloud = c.cloud(_records(tgt))
    T = c.estimateTransformICPPlane(c.cloud(_records(src)), t_cloud, c.computeSurfaceNormals(t_cloud, 0.3), guess, 1.0, 30, 1e-9)
    assert c.last_icp_converged == 0
    assert np.isfinite(T).all()
    assert np.array_equal(T, guess)
    c.close()


# ---------------------------------------------------------------- 6 - 8. drivers, cache, default path
@pytest.fixture(scope="module")
def clouds(synth):
    _, maps = synth.synth_maps(7, 30000, overlap_step=0.4)
    return [synth.pack_points(x, col) for x, col, _ in maps]


def _params(mm, method=SAC_IA, **kw):
    return mm.MapMergingParams(descriptor_type=2, estimation_method=method, **kw)


def _ctx(mm, streams=1, method=POINT_TO_PLANE, cache=0, method_first=True):
    c = mm.Context(0)
    if method_first:
        c.setIcpMethod(method)
    c.setStreams(streams)
    if not method_first:
        c.setIcpMethod(method)
    if cache:
        c.setMapCache(cache)
    return c


def _run(c, clouds, p, seed=1):
    c.srand(seed)
    T, pairs = c.estimateMapsTransforms(clouds, p, return_pairs=True)
    return np.stack(T), pairs


def _same(a, b):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8))


def test_drivers_and_stage_agree_bit_for_bit(mm, clouds):
    cs = clouds[:6]
    p = _params(mm)
    one = _run(_ctx(mm, 1), cs, p)
    assert one[1]["icp_iterations"].max() > 0
    _same(one, _run(_ctx(mm, 4), cs, p))
    _same(one, _run(_ctx(mm, 4, method_first=False), cs, p))       # set after mm3d_set_streams: the helpers follow
    # the stage-level entry point from each pair's pre-ICP guess (refine off), with the target map's own normals
    c = _ctx(mm, 1)
    guesses = _run(c, cs, _params(mm, refine_transform=0))[1]
    maps = [c.mapFeatures(c.cloud(x), p) for x in cs]
    for g, r in zip(guesses, one[1]):
        s, t = int(r["source_idx"]), int(r["target_idx"])
        assert (int(g["source_idx"]), int(g["target_idx"])) == (s, t)
        guess = g["transform"].reshape(4, 4).T
        nt = c.computeSurfaceNormals(maps[t].points, p.normal_radius)
        T = c.estimateTransformICPPlane(maps[s].points, maps[t].points, nt, guess, p.max_correspondence_distance, p.max_iterations,
                                        p.transform_epsilon)
        assert np.array_equal(T.T.reshape(16).view(np.uint32), r["transform"].view(np.uint32))
        assert c.last_icp_iterations == int(r["icp_iterations"])


@pytest.mark.parametrize("streams", [1, 4])
def test_cache_lockstep(mm, clouds, streams):
    p = _params(mm)
    cached, plain = _ctx(mm, streams, cache=64), _ctx(mm, streams)
    cs = clouds[:6]
    _same(_run(cached, cs, p), _run(plain, cs, p))
    _same(_run(cached, cs, p), _run(plain, cs, p))
    st = cached.mapCacheStats(reset=True)
    assert st["pairs_reused"] > 0 and st["device_bytes"] > 0
    changed = cs[:5] + [clouds[6]]
    _same(_run(cached, changed, p), _run(plain, changed, p))


def test_default_untouched_and_methods_never_share_records(mm, clouds):
    cs = clouds[:6]
    p = _params(mm, MATCHING)
    fresh = _ctx(mm, 1, POINT_TO_POINT)
    back = _ctx(mm, 1, POINT_TO_PLANE)
    back.setIcpMethod(POINT_TO_POINT)
    _same(_run(fresh, cs, p), _run(back, cs, p))
    _same(_run(fresh, cs, p), _run(back, cs, p))
    plane_ref = _run(_ctx(mm, 1, POINT_TO_PLANE), cs, p)
    assert not np.array_equal(plane_ref[0], _run(fresh, cs, p)[0])
    c = _ctx(mm, 1, POINT_TO_POINT, cache=64)
    p2p = _run(c, cs, p)
    n_pairs = len(p2p[1])
    c.mapCacheStats(reset=True)
    # the cache key: a point-to-point record is never reused for point-to-plane (this call hits every map, reuses no pair)
    c.setIcpMethod(POINT_TO_PLANE)
    _same(_run(c, cs, p), plane_ref)
    st = c.mapCacheStats(reset=True)
    assert st["map_hits"] == 6 and st["pairs_reused"] == 0 and st["pairs_computed"] == n_pairs
    c.setIcpMethod(POINT_TO_POINT)
    _same(_run(c, cs, p), p2p)
    st = c.mapCacheStats(reset=True)
    assert st["pairs_reused"] == n_pairs

"""Generalized ICP (mm3d_set_icp_generalized, mm3d_estimate_transform_icp_generalized): the surface and its refusals, a numpy
restatement of the rule the header states, a known answer on two independent samplings of one room (where point-to-plane is
pulled by the sampling), unusable normals, split invariance, the whole-map drivers with the cache, and the batch's edges."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_icp_plane import _ldlt_solve, _nearest, _normals, _problem, _records, _xform_f32, box_room, construct_transform

POINT_TO_POINT, POINT_TO_PLANE = 0, 1
SAC_IA, MATCHING = 1, 0
EINVAL, EUNSUPPORTED = -1, -4
TRIMMED = 1
DEFAULTS = (0, 1e-3)


# ---------------------------------------------------------------- the restatement (also read by test_icp_generalized_cpu.py)
def unit_normals(nrm):
    """(n / sqrt(n.n) in double, usable): usable = three finite components and n.n = (nx nx + ny ny) + nz nz > 0."""
    n = np.asarray(nrm, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        ok = np.isfinite(n).all(axis=1) & (nn > 0.0)
        u = n / np.sqrt(nn)[:, None]
    u[~ok] = 0.0
    return u, ok


def _adjugate_inverse(S):
    """Symmetric 3x3 inverses, the adjugate over the determinant; S is [k, 3, 3]."""
    a, b, c, d, e, f = S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    det = (a * c00 + b * c01) + c * c02
    W = np.empty_like(S)
    W[:, 0, 0], W[:, 0, 1], W[:, 0, 2] = c00 / det, c01 / det, c02 / det
    W[:, 1, 1], W[:, 1, 2], W[:, 2, 2] = (a * f - c * c) / det, (b * c - a * e) / det, (a * d - b * b) / det
    W[:, 1, 0], W[:, 2, 0], W[:, 2, 1] = W[:, 0, 1], W[:, 0, 2], W[:, 1, 2]
    return W


def generalized_system(s, q, m, nt, epsilon):
    """(AtA, Atr) of correspondences with both normals usable, in double: s the transformed source points, q their targets, m the
    rotated source normals, nt the targets' unit normals.  J = [-[s]x | I3], W = (2 I - (1 - epsilon)(nt nt^T + m m^T))^-1."""
    k = len(s)
    S = 2.0 * np.eye(3)[None] - (1.0 - epsilon) * (nt[:, :, None] * nt[:, None, :] + m[:, :, None] * m[:, None, :])
    W = _adjugate_inverse(S)
    J = np.zeros((k, 3, 6))
    sx, sy, sz = s[:, 0], s[:, 1], s[:, 2]
    J[:, 0, 1], J[:, 0, 2] = sz, -sy                     # -[s]x
    J[:, 1, 0], J[:, 1, 2] = -sz, sx
    J[:, 2, 0], J[:, 2, 1] = sy, -sx
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
    e = q - s
    return np.einsum("kai,kab,kbj->ij", J, W, J), np.einsum("kai,kab,kb->i", J, W, e)


def restate_icp_generalized(src, src_nrm, tgt, tgt_nrm, guess, max_corr, max_iter, eps, epsilon=1e-3, tau=1e-12):
    """The loop of include/mm3d.h (mm3d_set_icp_generalized) in numpy: float32 transforms and distances, double sums and solve.
    Returns (T, iterations, converged, margins): margins = the relative distances of every convergence test from its
    threshold, and of every pivot from the degeneracy floor."""
    max_d2 = np.float32(max_corr * max_corr)
    if float(max_d2) > max_corr * max_corr:
        max_d2 = np.nextafter(max_d2, np.float32(-np.inf))
    us, s_ok = unit_normals(src_nrm)
    ut, t_ok = unit_normals(tgt_nrm)
    T = np.asarray(guess, dtype=np.float32).copy()
    prev_mse, iters, margins = np.finfo(np.float64).max, 0, []
    while True:
        s = _xform_f32(T, src)
        idx, d2 = _nearest(s, tgt)
        ok = d2 <= max_d2
        cnt = int(ok.sum())
        if cnt < 3:
            return T, iters, 0, margins
        R = T[:3, :3].astype(np.float64)
        m = np.stack([(R[r, 0] * us[:, 0] + R[r, 1] * us[:, 1]) + R[r, 2] * us[:, 2] for r in range(3)], axis=1)
        use = ok & s_ok & t_ok[idx]
        AtA, Atr = generalized_system(s[use].astype(np.float64), tgt[idx[use]].astype(np.float64), m[use], ut[idx[use]], epsilon)
        floor = tau * np.trace(AtA) / 6.0
        x, pivots = _ldlt_solve(AtA, Atr, floor) if 3 * int(use.sum()) >= 6 else (None, [])
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
def _moved(xyz, T):
    return (T @ np.c_[xyz.astype(np.float64), np.ones(len(xyz))].T).T[:, :3].astype(np.float32)


def _rotated(nrm, T):
    return (T[:3, :3] @ nrm.astype(np.float64).T).T.astype(np.float32)


def same_points_problem(seed, n=5000):
    """_problem(seed, n) with the source's normals: the target's, rotated by T_true^-1 (the source is the target moved point for
    point)."""
    tgt, nrm, src, T_true, guess = _problem(seed, n)
    return tgt, nrm, src, _rotated(nrm, np.linalg.inv(T_true)), T_true, guess


def resampled_room(seed, n=3000):
    """Target box_room(seed); source box_room(seed + 1), an independent sampling of the same surfaces, moved by _problem(seed)'s
    T_true^-1; its guess.  Exact normals on both sides."""
    tgt, nrm, _, T_true, guess = _problem(seed, n)
    s_in_t, s_nrm = box_room(seed + 1, n)
    inv = np.linalg.inv(T_true)
    return tgt, nrm, _moved(s_in_t, inv), _rotated(s_nrm, inv), T_true, guess


ROOM = dict(max_corr=0.5, max_iter=50, eps=1e-10, epsilon=1e-3)          # the settings of the known answer


def _bits(T):
    return np.ascontiguousarray(T, dtype=np.float32).view(np.uint32)


def _stage(mm, src, s_nrm, tgt, t_nrm, guess, max_corr, max_iter, eps, epsilon=None):
    c = mm.Context(0)
    T = c.estimateTransformICPGeneralized(c.cloud(_records(src)), c.normals(_normals(s_nrm)), c.cloud(_records(tgt)), c.normals(_normals(t_nrm)),
                                          guess, max_corr, max_iterations=max_iter, transformation_epsilon=eps, epsilon=epsilon)
    out = (T, c.last_icp_iterations, c.last_icp_converged)
    c.close()
    return out


# ---------------------------------------------------------------- 1. surface
@pytest.mark.gpu
def test_surface(mm):
    lib = mm.lib()
    c = mm.Context(0)
    assert mm.IcpGeneralizedOptions().as_tuple() == DEFAULTS
    assert c.getIcpGeneralized().as_tuple() == DEFAULTS
    c.setIcpMethod(POINT_TO_PLANE)
    c.setIcpGeneralized(enabled=1, epsilon=0.01)
    assert c.getIcpGeneralized().as_tuple() == (1, 0.01)
    assert c.getIcpMethod() == POINT_TO_PLANE             # keeps answering its own value
    assert lib.mm3d_set_icp_method(c._h, 2) == EINVAL      # and its enum stays as it is
    c.setIcpMethod(POINT_TO_POINT)
    assert c.getIcpMethod() == POINT_TO_POINT and c.getIcpGeneralized().as_tuple() == (1, 0.01)
    c.setIcpGeneralized(enabled=0)
    assert c.getIcpGeneralized().as_tuple() == DEFAULTS
    c.setIcpGeneralized(enabled=1, epsilon=1.0)           # the upper end is in
    c.setIcpGeneralized(enabled=0)
    o = mm.IcpGeneralizedOptions()
    assert lib.mm3d_set_icp_generalized(None, C.byref(o)) == EINVAL and lib.mm3d_set_icp_generalized(c._h, None) == EINVAL
    assert lib.mm3d_get_icp_generalized(None, C.byref(o)) == EINVAL and lib.mm3d_get_icp_generalized(c._h, None) == EINVAL
    bad = [dict(enabled=2), dict(enabled=-1), dict(epsilon=0.0), dict(epsilon=-1e-3), dict(epsilon=1.0001), dict(epsilon=float("nan")),
           dict(epsilon=float("inf"))]
    for b in bad:
        for enabled in (0, 1):
            assert lib.mm3d_set_icp_generalized(c._h, C.byref(mm.IcpGeneralizedOptions(**{"enabled": enabled, **b}))) == EINVAL, (enabled, b)
    assert c.getIcpGeneralized().as_tuple() == DEFAULTS
    # the stage entry point: NULL arguments, epsilon out of range, normals of another count on either side
    tgt, nrm, src, s_nrm, _, guess = same_points_problem(21, 600)
    s_c, t_c = c.cloud(_records(src)), c.cloud(_records(tgt))
    sn_c, tn_c = c.normals(_normals(s_nrm)), c.normals(_normals(nrm))
    short = c.normals(_normals(nrm[:-1]))
    T = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16))
    good = mm.IcpGeneralizedOptions()

    def stage(s, sn, t, tn, g, opt, out):
        return lib.mm3d_estimate_transform_icp_generalized(c._h, s, sn, t, tn, g, C.c_double(0.5), opt, 10, C.c_double(1e-9), out)

    assert stage(s_c._h, sn_c._h, t_c._h, tn_c._h, T, C.byref(good), T) == 0        # enabled == 0: it runs whatever that says
    for args in [(None, sn_c._h, t_c._h, tn_c._h, T, C.byref(good), T), (s_c._h, None, t_c._h, tn_c._h, T, C.byref(good), T),
                 (s_c._h, sn_c._h, None, tn_c._h, T, C.byref(good), T), (s_c._h, sn_c._h, t_c._h, None, T, C.byref(good), T),
                 (s_c._h, sn_c._h, t_c._h, tn_c._h, None, C.byref(good), T), (s_c._h, sn_c._h, t_c._h, tn_c._h, T, None, T),
                 (s_c._h, sn_c._h, t_c._h, tn_c._h, T, C.byref(good), None),
                 (s_c._h, short._h, t_c._h, tn_c._h, T, C.byref(good), T), (s_c._h, sn_c._h, t_c._h, short._h, T, C.byref(good), T)] + \
                [(s_c._h, sn_c._h, t_c._h, tn_c._h, T, C.byref(mm.IcpGeneralizedOptions(**b)), T) for b in bad]:
        assert stage(*args) == EINVAL
    # device lists and shards
    d = mm.Context(devices=[0])
    assert lib.mm3d_set_icp_generalized(d._h, C.byref(mm.IcpGeneralizedOptions(enabled=1))) == EUNSUPPORTED
    assert b"device-list" in lib.mm3d_last_error(d._h)
    assert lib.mm3d_set_icp_generalized(d._h, C.byref(mm.IcpGeneralizedOptions(enabled=0))) == 0
    assert d.getIcpGeneralized().as_tuple() == DEFAULTS
    d.close()
    c.setIcpGeneralized(enabled=1)
    cloud = _records(tgt)
    with pytest.raises(mm.Mm3dError) as e:
        c.shardBegin([cloud, cloud], mm.MapMergingParams(descriptor_type=2), 0, 1)
    assert e.value.status == EUNSUPPORTED
    # rejection and colour under it ...
    rej = mm.IcpRejectionOptions(distance=TRIMMED, overlap_ratio=0.7)
    assert lib.mm3d_set_icp_rejection(c._h, C.byref(rej)) == EUNSUPPORTED
    assert b"mm3d_set_icp_generalized" in lib.mm3d_last_error(c._h)
    assert lib.mm3d_set_icp_rejection(c._h, C.byref(mm.IcpRejectionOptions())) == 0         # (an inactive selection is fine)
    assert lib.mm3d_set_icp_color(c._h, C.byref(mm.IcpColorOptions(enabled=1))) == EUNSUPPORTED
    assert b"mm3d_set_icp_generalized" in lib.mm3d_last_error(c._h)
    assert lib.mm3d_set_icp_color(c._h, C.byref(mm.IcpColorOptions(enabled=0, lambda_geometric=0.5))) == 0
    # ... and it under each of them
    c.setIcpGeneralized(enabled=0)
    c.setIcpRejection(rej)
    assert lib.mm3d_set_icp_generalized(c._h, C.byref(mm.IcpGeneralizedOptions(enabled=1))) == EUNSUPPORTED
    assert b"mm3d_set_icp_rejection" in lib.mm3d_last_error(c._h)
    assert lib.mm3d_set_icp_generalized(c._h, C.byref(mm.IcpGeneralizedOptions(enabled=0, epsilon=0.5))) == 0
    c.setIcpRejection(mm.IcpRejectionOptions())
    c.setIcpColor(enabled=1)
    assert lib.mm3d_set_icp_generalized(c._h, C.byref(mm.IcpGeneralizedOptions(enabled=1))) == EUNSUPPORTED
    assert b"mm3d_set_icp_color" in lib.mm3d_last_error(c._h)
    assert lib.mm3d_set_icp_generalized(c._h, C.byref(mm.IcpGeneralizedOptions(enabled=0))) == 0
    c.setIcpColor(enabled=0)
    c.setIcpGeneralized(enabled=1)
    assert c.getIcpGeneralized().enabled == 1
    c.close()


# ---------------------------------------------------------------- 2. against the restatement
def _against_restatement(mm, tgt, nrm, src, s_nrm, guess):
    max_corr, max_iter, eps, epsilon = 1.0, 30, 1e-9, 1e-3
    T_ref, it_ref, conv_ref, margins = restate_icp_generalized(src, s_nrm, tgt, nrm, guess, max_corr, max_iter, eps, epsilon)
    assert it_ref >= 2
    assert min(margins) > 0.01, "the restatement sits within 1 % of a threshold: the comparison would be borderline"
    T, iters, conv = _stage(mm, src, s_nrm, tgt, nrm, guess, max_corr, max_iter, eps, epsilon)
    print("iterations", iters, it_ref, "smallest margin", min(margins), "max|T - T_ref|", np.abs(T - T_ref).max())
    assert (iters, conv) == (it_ref, conv_ref)
    assert np.abs(T - T_ref).max() < 1e-4, np.abs(T - T_ref).max()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [21, 22, 23])
def test_against_restatement(mm, seed):
    tgt, nrm, src, s_nrm, _, guess = same_points_problem(seed)
    _against_restatement(mm, tgt, nrm, src, s_nrm, guess)


# ---------------------------------------------------------------- 3. known answer
@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 3, 5])
def test_known_answer_resampled_room(mm, seed):
    tgt, nrm, src, s_nrm, T_true, guess = resampled_room(seed)
    T, iters, conv = _stage(mm, src, s_nrm, tgt, nrm, guess, ROOM["max_corr"], ROOM["max_iter"], ROOM["eps"], ROOM["epsilon"])
    err = np.abs(T - T_true).max()
    c = mm.Context(0)
    Tp = c.estimateTransformICPPlane(c.cloud(_records(src)), c.cloud(_records(tgt)), c.normals(_normals(nrm)), guess, ROOM["max_corr"],
                                     ROOM["max_iter"], ROOM["eps"])
    err_plane = np.abs(Tp - T_true).max()
    Tq = c.estimateTransformICP(c.cloud(_records(src)), c.cloud(_records(tgt)), guess, ROOM["max_corr"], ROOM["max_iter"], ROOM["eps"])
    err_point = np.abs(Tq - T_true).max()
    c.close()
    print("seed", seed, "generalized: iterations", iters, "converged", conv, "max|T - T_true|", err, "point-to-plane", err_plane,
          "point-to-point", err_point)
    assert conv == 1
    assert err < 1e-4, err
    assert 5.0 * err <= err_plane, (err, err_plane)


# ---------------------------------------------------------------- 4. unusable normals
def _with_unusable(nrm, step, zeros):
    out = nrm.copy()
    out[::step] = np.nan
    out[zeros] = 0.0
    return out


@pytest.mark.gpu
def test_unusable_normals_are_skipped(mm):
    tgt, nrm, src, s_nrm, _, guess = same_points_problem(24)
    nrm, s_nrm = _with_unusable(nrm, 97, [3, 1001, 4002]), _with_unusable(s_nrm, 89, [7, 2003, 4999])
    nrm[5, 1], s_nrm[11, 2] = np.inf, -np.inf
    _against_restatement(mm, tgt, nrm, src, s_nrm, guess)


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["source", "target"])
def test_one_side_without_normals_is_degenerate(mm, side):
    tgt, nrm, src, s_nrm, _, guess = same_points_problem(25, 2000)
    if side == "source":
        s_nrm = np.full_like(s_nrm, np.nan)
    else:
        nrm = np.full_like(nrm, np.nan)
    T, iters, conv = _stage(mm, src, s_nrm, tgt, nrm, guess, 1.0, 30, 1e-9)
    assert np.array_equal(_bits(T), _bits(guess))
    assert (iters, conv) == (0, 0)


# ---------------------------------------------------------------- 5. split invariance
@pytest.mark.gpu
def test_split_invariance(mm):
    a, b = same_points_problem(22), resampled_room(3)

    def both():
        ra = _stage(mm, a[2], a[3], a[0], a[1], a[5], 1.0, 30, 1e-9)
        rb = _stage(mm, b[2], b[3], b[0], b[1], b[5], ROOM["max_corr"], ROOM["max_iter"], ROOM["eps"])
        return (_bits(ra[0]).copy(),) + ra[1:], (_bits(rb[0]).copy(),) + rb[1:]

    assert mm.icp_generalized_split() == 0
    try:
        assert mm.icp_generalized_split(1) == 1
        one = both()
        assert mm.icp_generalized_split(4) == 4
        four = both()
        assert mm.icp_generalized_split(3) == 4                # anything but 0 / 1 / 4 changes nothing
    finally:
        assert mm.icp_generalized_split(0) == 0
    for x, y in zip(one, four):
        assert np.array_equal(x[0], y[0]) and x[1:] == y[1:]
        assert x[1] >= 2


# ---------------------------------------------------------------- 6. whole-map calls
@pytest.fixture(scope="module")
def clouds(synth):
    _, maps = synth.synth_maps(7, 30000, overlap_step=0.4)
    return [synth.pack_points(x, col) for x, col, _ in maps]


def _params(mm, method=SAC_IA, **kw):
    return mm.MapMergingParams(descriptor_type=2, estimation_method=method, **kw)


def _ctx(mm, streams=1, enabled=1, cache=0, first=True, **kw):
    c = mm.Context(0)
    if first:
        c.setIcpGeneralized(enabled=enabled, **kw)
    c.setStreams(streams)
    if not first:
        c.setIcpGeneralized(enabled=enabled, **kw)
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


def _pairs_equal_the_stage(mm, c, cs, p, records):
    """every pair record = the stage entry point from the pair's pre-ICP guess (refine off), with both maps' own normals, bit for
    bit; returns the source sizes of the pairs that iterated"""
    p_off = _params(mm, refine_transform=0)
    guesses = _run(c, cs, p_off)[1]
    maps = [c.mapFeatures(c.cloud(x), p) for x in cs]
    normals = [c.computeSurfaceNormals(m.points, p.normal_radius) for m in maps]
    iterated = set()
    for g, r in zip(guesses, records):
        s, t = int(r["source_idx"]), int(r["target_idx"])
        assert (int(g["source_idx"]), int(g["target_idx"])) == (s, t)
        T = c.estimateTransformICPGeneralized(maps[s].points, normals[s], maps[t].points, normals[t], g["transform"].reshape(4, 4).T,
                                              p.max_correspondence_distance, max_iterations=p.max_iterations,
                                              transformation_epsilon=p.transform_epsilon)
        assert np.array_equal(T.T.reshape(16).view(np.uint32), r["transform"].view(np.uint32))
        assert c.last_icp_iterations == int(r["icp_iterations"])
        if int(r["icp_iterations"]) > 0:
            iterated.add(len(maps[s].points))
    return iterated


@pytest.mark.gpu
def test_drivers_and_stage_agree_bit_for_bit(mm, clouds):
    cs = clouds[:6]
    p = _params(mm)
    one = _run(_ctx(mm, 1), cs, p)
    assert one[1]["icp_iterations"].max() > 0
    _same(one, _run(_ctx(mm, 4), cs, p))
    _same(one, _run(_ctx(mm, 4, first=False), cs, p))       # set after mm3d_set_streams: the helpers follow
    c = _ctx(mm, 1)
    _pairs_equal_the_stage(mm, c, cs, p, one[1])
    c.close()


@pytest.mark.gpu
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


@pytest.mark.gpu
def test_default_untouched_and_generalized_never_shares_records(mm, clouds):
    cs = clouds[:6]
    p = _params(mm, MATCHING)
    fresh = _ctx(mm, 1, enabled=0)
    back = _ctx(mm, 1, enabled=1)
    back.setIcpGeneralized(enabled=0)
    _same(_run(fresh, cs, p), _run(back, cs, p))                  # switched on and off again: the untouched default records
    _same(_run(fresh, cs, p), _run(back, cs, p))
    gen_ref = _run(_ctx(mm, 1), cs, p)
    assert not np.array_equal(gen_ref[0], _run(fresh, cs, p)[0])
    c = _ctx(mm, 1, enabled=0, cache=64)
    plain = _run(c, cs, p)
    _same(plain, _run(fresh, cs, p))
    n_pairs = len(plain[1])
    c.mapCacheStats(reset=True)
    # the cache key: a plain record is never reused under the selection (this call hits every map, reuses no pair)
    c.setIcpGeneralized(enabled=1)
    _same(_run(c, cs, p), gen_ref)
    st = c.mapCacheStats(reset=True)
    assert st["map_hits"] == 6 and st["pairs_reused"] == 0 and st["pairs_computed"] == n_pairs
    # ... nor a record of another epsilon, nor a generalized one by a plain context
    c.setIcpGeneralized(enabled=1, epsilon=0.05)
    _run(c, cs, p)
    st = c.mapCacheStats(reset=True)
    assert st["map_hits"] == 6 and st["pairs_reused"] == 0 and st["pairs_computed"] == n_pairs
    c.setIcpGeneralized(enabled=1)
    _same(_run(c, cs, p), gen_ref)
    st = c.mapCacheStats(reset=True)
    assert st["pairs_reused"] == n_pairs and st["pairs_computed"] == 0
    c.setIcpGeneralized(enabled=0)
    _same(_run(c, cs, p), plain)
    st = c.mapCacheStats(reset=True)
    assert st["pairs_reused"] == n_pairs


# ---------------------------------------------------------------- 7. batch edges
THINNING = (1, 2, 3, 4)      # every k-th point of the fixture's maps: four maps of clearly different size


@pytest.fixture(scope="module")
def unequal_clouds(synth):
    _, maps = synth.synth_maps(4, 30000, overlap_step=0.4)
    return [synth.pack_points(x, col)[::k].copy() for (x, col, _), k in zip(maps, THINNING)]


@pytest.mark.gpu
def test_unequal_sources_in_one_batch(mm, unequal_clouds):
    """Pairs of different source and target sizes in one batch (every per-pair offset into the batch's arrays differs from its
    neighbours'): one and four streams and the forced split give the same bytes, and every pair is the stage entry point's
    result from the pair's pre-ICP guess, bit for bit."""
    p = _params(mm)
    c, four = _ctx(mm, 1), _ctx(mm, 4)
    one = _run(c, unequal_clouds, p)
    _same(one, _run(four, unequal_clouds, p))
    mm.icp_generalized_split(1)
    try:
        _same(one, _run(c, unequal_clouds, p))
    finally:
        mm.icp_generalized_split(0)
    iterated = _pairs_equal_the_stage(mm, c, unequal_clouds, p, one[1])
    assert len(iterated) >= 3          # at least three pairs that iterate, their sources of pairwise different size
    c.close()
    four.close()


@pytest.mark.gpu
@pytest.mark.parametrize("empty", ["source", "target"])
def test_nothing_to_search(mm, empty):
    """An empty source, or an empty target: MM3D_OK, the guess bit for bit and no iteration."""
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-2.0, 2.0, (300, 3)).astype(np.float32)
    full = _records(xyz)
    c = mm.Context(0)
    clouds = dict(source=c.cloud(full), target=c.cloud(full))
    clouds[empty] = c.cloud(full[:0])
    normals = {k: c.computeSurfaceNormals(v, 0.5) for k, v in clouds.items()}
    guess = np.eye(4, dtype=np.float32)
    guess[:3, :3] = [[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]]
    guess[:3, 3] = [0.1, -0.2, 0.3]
    T = c.estimateTransformICPGeneralized(clouds["source"], normals["source"], clouds["target"], normals["target"], guess, 0.5,
                                          max_iterations=30, transformation_epsilon=1e-9)
    assert np.array_equal(np.asarray(T, dtype=np.float32).view(np.uint32), guess.view(np.uint32))
    assert c.last_icp_iterations == 0
    c.close()

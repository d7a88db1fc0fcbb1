"""Coloured ICP (mm3d_set_icp_color, mm3d_estimate_transform_icp_color): the surface, the gradient records and the loop against a
numpy restatement of the rule include/mm3d.h states, a textured corridor that point-to-plane cannot register, lambda == 1 as
point-to-plane bit for bit, split invariance, grey clouds, and the whole-map drivers and cache.  The restatement and the scenes
are also read by test_icp_color_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_icp_plane import _ldlt_solve, _nearest, _normals, _pose, _problem, _xform_f32, construct_transform

POINT_TO_POINT, POINT_TO_PLANE = 0, 1
SAC_IA, MATCHING = 1, 0
EINVAL, EUNSUPPORTED = -1, -4
TRIMMED = 1
DEFAULTS = (0, 0.968, 0.0, 4)


# ---------------------------------------------------------------- the restatement
def intensity_of(rgba):
    """I = (float)((double)(299 r + 587 g + 114 b) / 255000.0) of rgba words."""
    c = np.asarray(rgba, dtype=np.uint32).astype(np.int64)
    r, g, b = (c >> 16) & 255, (c >> 8) & 255, c & 255
    return ((299 * r + 587 * g + 114 * b).astype(np.float64) / 255000.0).astype(np.float32)


def _ldlt3(M, b, floor):
    """The unpivoted 3x3 LDLt of the rule; None when a pivot is at or below `floor`."""
    L, D = np.eye(3), np.zeros(3)
    for j in range(3):
        d = M[j, j] - sum(L[j, k] * L[j, k] * D[k] for k in range(j))
        if not d > floor:
            return None
        D[j] = d
        for i in range(j + 1, 3):
            L[i, j] = (M[i, j] - sum(L[i, k] * L[j, k] * D[k] for k in range(j))) / d
    y = np.zeros(3)
    for i in range(3):
        y[i] = b[i] - sum(L[i, k] * y[k] for k in range(i))
    x = np.zeros(3)
    for i in range(2, -1, -1):
        x[i] = y[i] / D[i] - sum(L[k, i] * x[k] for k in range(i + 1, 3))
    return x


def restate_gradients(xyz, rgba, nrm, radius, min_neighbours=4, chunk=512):
    """The gradient records of the rule: (records float32 [n][4] = gx gy gz I, cond(M) per point, 0 where no system was solved)."""
    xyz = np.asarray(xyz, dtype=np.float32)
    nrm = np.asarray(nrm, dtype=np.float32)
    n = len(xyz)
    inten = intensity_of(rgba)
    thr = np.float32(radius * radius)
    if float(thr) > radius * radius:
        thr = np.nextafter(thr, np.float32(-np.inf))
    fin_p = np.isfinite(xyz).all(axis=1)
    fin_n = np.isfinite(nrm[:, :3]).all(axis=1)
    rec = np.zeros((n, 4), dtype=np.float32)
    rec[:, 3] = inten
    cond = np.zeros(n)
    with np.errstate(invalid="ignore"):
        for a in range(0, n, chunk):
            q = xyz[a:a + chunk]
            dx, dy, dz = q[:, None, 0] - xyz[None, :, 0], q[:, None, 1] - xyz[None, :, 1], q[:, None, 2] - xyz[None, :, 2]
            near = ((dx * dx + dy * dy) + dz * dz <= thr) & fin_p[None, :]
            for r in range(len(q)):
                i = a + r
                if not (fin_p[i] and fin_n[i]):
                    continue
                js = np.flatnonzero(near[r])
                js = js[js != i]
                k = len(js)
                if k < min_neighbours:
                    continue
                nn = nrm[i, :3].astype(np.float64)
                e = xyz[js].astype(np.float64) - xyz[i].astype(np.float64)
                u = e - (e @ nn)[:, None] * nn[None, :]
                w = inten[js].astype(np.float64) - float(inten[i])
                M = u.T @ u + float(k) * float(k) * np.outer(nn, nn)
                g = _ldlt3(M, u.T @ w, 1e-12 * np.trace(M) / 3.0)
                cond[i] = np.linalg.cond(M)
                if g is not None:
                    rec[i, :3] = g.astype(np.float32)
    return rec, cond


def restate_icp_color(src, src_rgba, tgt, nrm, rec, guess, max_corr, max_iter, eps, lam, tau=1e-12):
    """The loop of include/mm3d.h (mm3d_set_icp_color) in numpy: restate_icp_plane's loop with the two rows per correspondence.
    rec: the target's records [n][4].  Returns (T, iterations, converged, margins, singular): margins as restate_icp_plane's;
    singular = the loop ended at the degeneracy rule."""
    max_d2 = np.float32(max_corr * max_corr)
    if float(max_d2) > max_corr * max_corr:
        max_d2 = np.nextafter(max_d2, np.float32(-np.inf))
    mu = 1.0 - lam
    i_src = intensity_of(src_rgba).astype(np.float64)
    T = np.asarray(guess, dtype=np.float32).copy()
    prev_mse, iters, margins = np.finfo(np.float64).max, 0, []
    while True:
        s = _xform_f32(T, src)
        idx, d2 = _nearest(s, tgt)
        ok = d2 <= max_d2
        cnt = int(ok.sum())
        if cnt < 3:
            return T, iters, 0, margins, False
        w = idx[ok]
        sd, q, n = s[ok].astype(np.float64), tgt[w].astype(np.float64), nrm[w].astype(np.float64)
        g, it, isrc = rec[w, :3].astype(np.float64), rec[w, 3].astype(np.float64), i_src[ok]
        fin = np.isfinite(n).all(axis=1)
        sd, q, n, g, it, isrc = sd[fin], q[fin], n[fin], g[fin], it[fin], isrc[fin]
        AG = np.concatenate([np.cross(sd, n), n], axis=1)
        rG = (n * q).sum(axis=1) - (n * sd).sum(axis=1)
        if lam < 1.0:
            e = sd - q
            h = (e * n).sum(axis=1)
            m = g - (g * n).sum(axis=1)[:, None] * n
            pred = it + (g * (e - h[:, None] * n)).sum(axis=1)
            rC = isrc - pred
            AC = np.concatenate([np.cross(sd, m), m], axis=1)
            AtA, Atr = lam * (AG.T @ AG) + mu * (AC.T @ AC), lam * (AG.T @ rG) + mu * (AC.T @ rC)
        else:
            AtA, Atr = AG.T @ AG, AG.T @ rG
        floor = tau * np.trace(AtA) / 6.0
        x, pivots = _ldlt_solve(AtA, Atr, floor) if len(AG) >= 6 else (None, [])
        margins += [abs(p - floor) / max(abs(floor), 1e-300) for p in pivots]
        if x is None:
            return T, iters, 0, margins, True
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
            return T, iters, 1, margins, False
        cos_angle = 0.5 * ((float(Ti[0, 0]) + float(Ti[1, 1]) + float(Ti[2, 2])) - 1.0)
        t2 = float(Ti[0, 3]) * float(Ti[0, 3]) + float(Ti[1, 3]) * float(Ti[1, 3]) + float(Ti[2, 3]) * float(Ti[2, 3])
        margins += [abs((1.0 - cos_angle) - eps) / eps, abs(t2 - eps) / eps]
        if cos_angle >= 1.0 - eps and t2 <= eps:
            return T, iters, 1, margins, False
        mse = float(d2[ok].astype(np.float64).sum()) / cnt
        if iters > 1:                                   # (the first compares with DBL_MAX)
            margins.append(abs(abs(mse - prev_mse) - 1e-12) / 1e-12)
        if abs(mse - prev_mse) < 1e-12:
            return T, iters, 1, margins, False
        prev_mse = mse


# ---------------------------------------------------------------- scenes
def texture(xyz):
    """A smooth sinusoidal grey texture of position, quantised to 8 bits: rgba words with r = g = b."""
    p = np.asarray(xyz, dtype=np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    v = 0.5 + 0.22 * np.sin(2.0 * np.pi * x / 1.9 + 0.9 * (y + z)) + 0.18 * np.sin(2.0 * np.pi * (y - z) / 1.4 + 0.7 * x)
    g = np.clip(np.rint(v * 255.0), 0, 255).astype(np.uint32)
    return np.uint32(0xff000000) | (g << np.uint32(16)) | (g << np.uint32(8)) | g


def corridor(seed, n, size=(8.0, 2.0, 2.5)):
    """Points on the floor and the two long walls of a corridor along x -- no end walls -- with their exact normals."""
    rng = np.random.default_rng(seed)
    X, Y, Z = size
    faces = [((0, 0, 0), (X, 0, 0), (0, Y, 0), (0, 0, 1)), ((0, 0, 0), (X, 0, 0), (0, 0, Z), (0, 1, 0)),
             ((0, Y, 0), (X, 0, 0), (0, 0, Z), (0, -1, 0))]
    area = np.array([np.linalg.norm(np.cross(u, v)) for _, u, v, _ in faces])
    counts = rng.multinomial(n, area / area.sum())
    pts, nrm = [], []
    for (o, u, v, nn), k in zip(faces, counts):
        a, b = rng.random((k, 1)), rng.random((k, 1))
        pts.append(np.asarray(o) + a * np.asarray(u) + b * np.asarray(v))
        nrm.append(np.tile(np.asarray(nn, dtype=np.float64), (k, 1)))
    return np.concatenate(pts).astype(np.float32), np.concatenate(nrm).astype(np.float32)


CORRIDOR_TRUE = _pose(0.0, 0.0, 1.0, (0.25, 0.0, 0.0))     # a 0.25 m slide along the axis and a degree of yaw


def corridor_pair(n):
    """(target, its rgba, its exact normals, source, its rgba, T_true): the source is sampled independently of the target, coloured
    by the same texture where it lies in the target's frame, and moved by T_true^-1."""
    tgt, nrm = corridor(1, n)
    s_in_t, _ = corridor(2, n)
    src = (np.linalg.inv(CORRIDOR_TRUE) @ np.c_[s_in_t.astype(np.float64), np.ones(n)].T).T[:, :3].astype(np.float32)
    return tgt, texture(tgt), nrm, src, texture(s_in_t), CORRIDOR_TRUE


def _records(xyz, rgba):
    out = np.zeros(len(xyz), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")])
    out["x"], out["y"], out["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out["rgba"] = rgba
    return out


def _bits(T):
    return np.ascontiguousarray(T, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- 1. surface
@pytest.mark.gpu
def test_surface(mm):
    lib = mm.lib()
    c = mm.Context(0)
    assert mm.IcpColorOptions().as_tuple() == DEFAULTS
    assert c.getIcpColor().as_tuple() == DEFAULTS
    c.setIcpMethod(POINT_TO_PLANE)
    c.setIcpColor(enabled=1, lambda_geometric=0.5, gradient_radius=0.3, min_neighbours=6)
    assert c.getIcpColor().as_tuple() == (1, 0.5, 0.3, 6)
    assert c.getIcpMethod() == POINT_TO_PLANE             # keeps answering its own value
    assert lib.mm3d_set_icp_method(c._h, 2) == EINVAL      # and its enum stays as it is
    c.setIcpColor(enabled=0)
    assert c.getIcpColor().as_tuple() == DEFAULTS
    o = mm.IcpColorOptions()
    assert lib.mm3d_set_icp_color(None, C.byref(o)) == EINVAL and lib.mm3d_set_icp_color(c._h, None) == EINVAL
    assert lib.mm3d_get_icp_color(None, C.byref(o)) == EINVAL and lib.mm3d_get_icp_color(c._h, None) == EINVAL
    bad = [dict(enabled=2), dict(enabled=-1), dict(lambda_geometric=0.0), dict(lambda_geometric=-0.1), dict(lambda_geometric=1.5),
           dict(lambda_geometric=float("nan")), dict(gradient_radius=-0.1), dict(gradient_radius=float("inf")),
           dict(gradient_radius=float("nan")), dict(min_neighbours=3), dict(min_neighbours=0)]
    for b in bad:
        for enabled in (0, 1):
            assert lib.mm3d_set_icp_color(c._h, C.byref(mm.IcpColorOptions(**{"enabled": enabled, **b}))) == EINVAL, (enabled, b)
    assert c.getIcpColor().as_tuple() == DEFAULTS
    # the stage entry point: NULL arguments, options out of range, a radius of 0, normals of another count
    tgt, rgba, nrm, src, s_rgba, _ = corridor_pair(600)
    s_c, t_c, n_c = c.cloud(_records(src, s_rgba)), c.cloud(_records(tgt, rgba)), c.normals(_normals(nrm))
    n_short = c.normals(_normals(nrm[:-1]))
    T = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(16))
    good = mm.IcpColorOptions(gradient_radius=0.3)

    def stage(s, t, n, g, opt, out):
        return lib.mm3d_estimate_transform_icp_color(c._h, s, t, n, g, C.c_double(0.5), opt, 10, C.c_double(1e-9), out)

    assert stage(s_c._h, t_c._h, n_c._h, T, C.byref(good), T) == 0        # enabled == 0: it runs whatever that says
    for args in [(None, t_c._h, n_c._h, T, C.byref(good), T), (s_c._h, None, n_c._h, T, C.byref(good), T),
                 (s_c._h, t_c._h, None, T, C.byref(good), T), (s_c._h, t_c._h, n_c._h, None, C.byref(good), T),
                 (s_c._h, t_c._h, n_c._h, T, None, T), (s_c._h, t_c._h, n_c._h, T, C.byref(good), None),
                 (s_c._h, t_c._h, n_c._h, T, C.byref(mm.IcpColorOptions()), T),                      # gradient_radius 0
                 (s_c._h, t_c._h, n_c._h, T, C.byref(mm.IcpColorOptions(gradient_radius=0.3, min_neighbours=2)), T),
                 (s_c._h, t_c._h, n_short._h, T, C.byref(good), T)]:
        assert stage(*args) == EINVAL
    out = np.zeros((600, 4), dtype=np.float32)
    assert lib.mm3d_debug_color_gradients(c._h, t_c._h, n_short._h, C.byref(good), out.ctypes.data_as(C.c_void_p)) == EINVAL
    assert lib.mm3d_debug_color_gradients(c._h, t_c._h, n_c._h, C.byref(mm.IcpColorOptions()), out.ctypes.data_as(C.c_void_p)) == EINVAL
    # device lists and shards
    d = mm.Context(devices=[0])
    assert lib.mm3d_set_icp_color(d._h, C.byref(mm.IcpColorOptions(enabled=1))) == EUNSUPPORTED
    assert lib.mm3d_set_icp_color(d._h, C.byref(mm.IcpColorOptions(enabled=0))) == 0
    assert d.getIcpColor().as_tuple() == DEFAULTS
    d.close()
    c.setIcpColor(enabled=1)
    cloud = _records(tgt, rgba)
    with pytest.raises(mm.Mm3dError) as e:
        c.shardBegin([cloud, cloud], mm.MapMergingParams(descriptor_type=2), 0, 1)
    assert e.value.status == EUNSUPPORTED
    # rejection and colour exclude each other, in both orders
    rej = mm.IcpRejectionOptions(distance=TRIMMED, overlap_ratio=0.7)
    assert lib.mm3d_set_icp_rejection(c._h, C.byref(rej)) == EUNSUPPORTED
    assert lib.mm3d_set_icp_rejection(c._h, C.byref(mm.IcpRejectionOptions())) == 0         # (an inactive selection is fine)
    c.setIcpColor(enabled=0)
    c.setIcpRejection(rej)
    assert lib.mm3d_set_icp_color(c._h, C.byref(mm.IcpColorOptions(enabled=1))) == EUNSUPPORTED
    assert lib.mm3d_set_icp_color(c._h, C.byref(mm.IcpColorOptions(enabled=0, lambda_geometric=0.5))) == 0
    c.setIcpRejection(mm.IcpRejectionOptions())
    c.setIcpColor(enabled=1)
    assert c.getIcpColor().enabled == 1
    c.close()


# ---------------------------------------------------------------- 2. gradients
@pytest.fixture(scope="module")
def corridor6k():
    tgt, rgba, nrm, src, s_rgba, T_true = corridor_pair(6000)
    rec, cond = restate_gradients(tgt, rgba, nrm, 0.3)
    return dict(tgt=tgt, rgba=rgba, nrm=nrm, src=src, s_rgba=s_rgba, T_true=T_true, rec=rec, cond=cond)


@pytest.mark.gpu
def test_gradients_against_restatement(mm, corridor6k):
    k = corridor6k
    # 64 * 2^-53 * cond(M) bounds the double sums' reordering error: below 1e-8 relative here, under the float rounding of 6e-8
    print("largest cond(M):", k["cond"].max())
    assert k["cond"].max() < 1e6
    c = mm.Context(0)
    dev = c.debugColorGradients(c.cloud(_records(k["tgt"], k["rgba"])), c.normals(_normals(k["nrm"])), gradient_radius=0.3)
    ref = k["rec"]
    assert np.array_equal(dev[:, 3].view(np.uint32), ref[:, 3].view(np.uint32))
    err = np.abs(dev[:, :3].astype(np.float64) - ref[:, :3].astype(np.float64))
    bound = 1e-6 * np.maximum(1.0, np.abs(ref[:, :3].astype(np.float64)))
    print("largest |g_dev - g_ref| / bound:", (err / bound).max(), "largest |g|:", np.abs(ref[:, :3]).max())
    assert (err <= bound).all()
    assert np.abs(ref[:, :3]).max() > 0.1                 # (the texture does have gradients)
    c.close()


@pytest.mark.gpu
def test_gradients_of_non_finite_and_isolated_points_are_zero(mm):
    tgt, rgba, nrm, _, _, _ = corridor_pair(1500)
    tgt, nrm = tgt.copy(), nrm.copy()
    nan_n, nan_p = np.arange(0, 1500, 97), np.arange(5, 1500, 131)
    nrm[nan_n] = np.nan
    tgt[nan_p, 1] = np.nan
    far = np.array([[30.0, 0.0, 0.0], [30.0, 0.2, 0.0], [30.0, 0.0, 0.2], [-20.0, 5.0, 1.0]], dtype=np.float32)     # 3 neighbours < 4, and none
    xyz, words = np.concatenate([tgt, far]), np.concatenate([rgba, texture(far)])
    normals = np.concatenate([nrm, np.tile(np.float32([0, 0, 1]), (4, 1))])
    c = mm.Context(0)
    dev = c.debugColorGradients(c.cloud(_records(xyz, words)), c.normals(_normals(normals)), gradient_radius=0.3)
    ref, _ = restate_gradients(xyz, words, normals, 0.3)
    special = np.r_[nan_n, nan_p, 1500 + np.arange(4)]
    assert np.array_equal(dev[special, :3], np.zeros((len(special), 3), dtype=np.float32))
    assert np.array_equal(dev[:, 3].view(np.uint32), intensity_of(words).view(np.uint32))
    # and a NaN point is nobody's neighbour: everything else still follows the restatement
    assert (np.abs(dev[:, :3].astype(np.float64) - ref[:, :3]) <= 1e-6 * np.maximum(1.0, np.abs(ref[:, :3]))).all()
    c.close()


# ---------------------------------------------------------------- 3. known answer
def _corridor_run(mm, k, lam=0.968):
    c = mm.Context(0)
    T = c.estimateTransformICPColor(c.cloud(_records(k["src"], k["s_rgba"])), c.cloud(_records(k["tgt"], k["rgba"])),
                                    c.normals(_normals(k["nrm"])), np.eye(4, dtype=np.float32), 0.5, max_iterations=50,
                                    transformation_epsilon=1e-10, lambda_geometric=lam, gradient_radius=0.3)
    out = (T, c.last_icp_iterations, c.last_icp_converged)
    c.close()
    return out


@pytest.mark.gpu
def test_known_answer_textured_corridor(mm, corridor6k):
    k = corridor6k
    T, iters, conv = _corridor_run(mm, k)
    err = np.abs(T - k["T_true"]).max()
    print("coloured ICP: iterations", iters, "converged", conv, "max|T - T_true|", err)
    assert conv == 1
    assert err < 5e-3
    # point-to-plane on the same inputs: the corridor's axis is free, its degeneracy rule stops it where it started
    c = mm.Context(0)
    guess = np.eye(4, dtype=np.float32)
    Tp = c.estimateTransformICPPlane(c.cloud(_records(k["src"], k["s_rgba"])), c.cloud(_records(k["tgt"], k["rgba"])),
                                     c.normals(_normals(k["nrm"])), guess, 0.5, 50, 1e-10)
    assert c.last_icp_converged == 0
    assert np.array_equal(Tp, guess)
    c.close()


# ---------------------------------------------------------------- 4. against the restatement
def _textured_problem(seed, n=5000):
    tgt, nrm, src, T_true, guess = _problem(seed, n)
    rgba = texture(tgt)
    return tgt, nrm, src, rgba, T_true, guess          # (the source is the target moved: point for point the same colours)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_against_restatement(mm, seed):
    tgt, nrm, src, rgba, _, guess = _textured_problem(seed)
    max_corr, max_iter, eps, lam, radius = 1.0, 30, 1e-9, 0.968, 0.3
    rec, _ = restate_gradients(tgt, rgba, nrm, radius)
    T_ref, it_ref, conv_ref, margins, _ = restate_icp_color(src, rgba, tgt, nrm, rec, guess, max_corr, max_iter, eps, lam)
    assert it_ref >= 2
    assert min(margins) > 0.01, "the restatement sits within 1 % of a threshold: the comparison would be borderline"
    c = mm.Context(0)
    T = c.estimateTransformICPColor(c.cloud(_records(src, rgba)), c.cloud(_records(tgt, rgba)), c.normals(_normals(nrm)), guess, max_corr,
                                    max_iterations=max_iter, transformation_epsilon=eps, lambda_geometric=lam, gradient_radius=radius)
    print("iterations", c.last_icp_iterations, it_ref, "max|T - T_ref|", np.abs(T - T_ref).max())
    assert (c.last_icp_iterations, c.last_icp_converged) == (it_ref, conv_ref)
    assert np.abs(T - T_ref).max() < 1e-4, np.abs(T - T_ref).max()
    c.close()


# ---------------------------------------------------------------- 5. lambda == 1
@pytest.mark.gpu
def test_lambda_one_is_point_to_plane_bit_for_bit(mm):
    tgt, nrm, src, rgba, _, guess = _textured_problem(14)
    c = mm.Context(0)
    s_c, t_c, n_c = c.cloud(_records(src, rgba)), c.cloud(_records(tgt, rgba)), c.normals(_normals(nrm))
    Tp = c.estimateTransformICPPlane(s_c, t_c, n_c, guess, 1.0, 30, 1e-9)
    plane = (c.last_icp_iterations, c.last_icp_converged)
    Tc = c.estimateTransformICPColor(s_c, t_c, n_c, guess, 1.0, max_iterations=30, transformation_epsilon=1e-9, lambda_geometric=1.0,
                                     gradient_radius=0.3)
    assert plane[0] >= 2
    assert (c.last_icp_iterations, c.last_icp_converged) == plane
    assert np.array_equal(_bits(Tc), _bits(Tp))
    c.close()


# ---------------------------------------------------------------- 6. split invariance
@pytest.mark.gpu
def test_split_invariance(mm, corridor6k):
    tgt, nrm, src, rgba, _, guess = _textured_problem(15)

    def both():
        c = mm.Context(0)
        T = c.estimateTransformICPColor(c.cloud(_records(src, rgba)), c.cloud(_records(tgt, rgba)), c.normals(_normals(nrm)), guess, 1.0,
                                        max_iterations=30, transformation_epsilon=1e-9, gradient_radius=0.3)
        room = (_bits(T).copy(), c.last_icp_iterations, c.last_icp_converged)
        c.close()
        Tc, it, conv = _corridor_run(mm, corridor6k)
        return room, (_bits(Tc).copy(), it, conv)

    assert mm.icp_color_split() == 0
    try:
        assert mm.icp_color_split(1) == 1
        one = both()
        assert mm.icp_color_split(4) == 4
        four = both()
        assert mm.icp_color_split(3) == 4                    # anything but 0 / 1 / 4 changes nothing
    finally:
        assert mm.icp_color_split(0) == 0
    for a, b in zip(one, four):
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
        assert a[1] >= 2


# ---------------------------------------------------------------- 7. grey clouds
@pytest.mark.gpu
def test_grey_clouds_have_zero_gradients_and_follow_point_to_plane(mm):
    tgt, nrm, src, _, _, guess = _textured_problem(16)
    grey = np.full(len(tgt), 0xff808080, dtype=np.uint32)
    c = mm.Context(0)
    s_c, t_c, n_c = c.cloud(_records(src, grey)), c.cloud(_records(tgt, grey)), c.normals(_normals(nrm))
    rec = c.debugColorGradients(t_c, n_c, gradient_radius=0.3)
    assert np.array_equal(rec[:, :3], np.zeros((len(tgt), 3), dtype=np.float32))
    assert np.array_equal(rec[:, 3].view(np.uint32), intensity_of(grey).view(np.uint32))
    Tp = c.estimateTransformICPPlane(s_c, t_c, n_c, guess, 1.0, 30, 1e-9)
    # the systems are the same, scaled by lambda
    Tc = c.estimateTransformICPColor(s_c, t_c, n_c, guess, 1.0, max_iterations=30, transformation_epsilon=1e-9, gradient_radius=0.3)
    assert np.abs(Tc - Tp).max() < 1e-6, np.abs(Tc - Tp).max()
    c.close()


# ---------------------------------------------------------------- 8. whole-map calls
@pytest.fixture(scope="module")
def clouds(synth):
    _, maps = synth.synth_maps(7, 30000, overlap_step=0.4)
    return [synth.pack_points(x, col) for x, col, _ in maps]


def _params(mm, method=SAC_IA, **kw):
    return mm.MapMergingParams(descriptor_type=2, estimation_method=method, **kw)


def _ctx(mm, streams=1, color=1, cache=0, color_first=True):
    c = mm.Context(0)
    if color_first:
        c.setIcpColor(enabled=color)
    c.setStreams(streams)
    if not color_first:
        c.setIcpColor(enabled=color)
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


@pytest.mark.gpu
def test_drivers_and_stage_agree_bit_for_bit(mm, clouds):
    cs = clouds[:6]
    p = _params(mm)
    one = _run(_ctx(mm, 1), cs, p)
    assert one[1]["icp_iterations"].max() > 0
    _same(one, _run(_ctx(mm, 4), cs, p))
    _same(one, _run(_ctx(mm, 4, color_first=False), cs, p))       # set after mm3d_set_streams: the helpers follow
    # the stage-level entry point from each pair's pre-ICP guess (refine off), with the target map's own normals
    c = _ctx(mm, 1)
    guesses = _run(c, cs, _params(mm, refine_transform=0))[1]
    maps = [c.mapFeatures(c.cloud(x), p) for x in cs]
    normals = {}
    for g, r in zip(guesses, one[1]):
        s, t = int(r["source_idx"]), int(r["target_idx"])
        assert (int(g["source_idx"]), int(g["target_idx"])) == (s, t)
        guess = g["transform"].reshape(4, 4).T
        if t not in normals:
            normals[t] = c.computeSurfaceNormals(maps[t].points, p.normal_radius)
        T = c.estimateTransformICPColor(maps[s].points, maps[t].points, normals[t], guess, p.max_correspondence_distance,
                                        max_iterations=p.max_iterations, transformation_epsilon=p.transform_epsilon,
                                        gradient_radius=p.normal_radius)
        assert np.array_equal(T.T.reshape(16).view(np.uint32), r["transform"].view(np.uint32))
        assert c.last_icp_iterations == int(r["icp_iterations"])


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
def test_default_untouched_and_colour_never_shares_records(mm, clouds):
    cs = clouds[:6]
    p = _params(mm, MATCHING)
    fresh = _ctx(mm, 1, color=0)
    back = _ctx(mm, 1, color=1)
    back.setIcpColor(enabled=0)
    _same(_run(fresh, cs, p), _run(back, cs, p))                  # switched on and off again: the untouched reference records
    _same(_run(fresh, cs, p), _run(back, cs, p))
    color_ref = _run(_ctx(mm, 1), cs, p)
    assert not np.array_equal(color_ref[0], _run(fresh, cs, p)[0])
    c = _ctx(mm, 1, color=0, cache=64)
    plain = _run(c, cs, p)
    _same(plain, _run(fresh, cs, p))
    n_pairs = len(plain[1])
    c.mapCacheStats(reset=True)
    # the cache key: a plain record is never reused for a colour context (this call hits every map, reuses no pair)
    c.setIcpColor(enabled=1)
    _same(_run(c, cs, p), color_ref)
    st = c.mapCacheStats(reset=True)
    assert st["map_hits"] == 6 and st["pairs_reused"] == 0 and st["pairs_computed"] == n_pairs
    # ... nor a colour record for one of another lambda, nor for a plain context
    c.setIcpColor(enabled=1, lambda_geometric=0.5)
    _run(c, cs, p)
    st = c.mapCacheStats(reset=True)
    assert st["map_hits"] == 6 and st["pairs_reused"] == 0
    c.setIcpColor(enabled=0)
    _same(_run(c, cs, p), plain)
    st = c.mapCacheStats(reset=True)
    assert st["pairs_reused"] == n_pairs

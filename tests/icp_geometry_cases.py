"""Helper of test_icp_geometry_cpu.py and test_gpu_icp_geometry.py, not a test: the numpy restatement of the boundary rule and of
step 1b that include/mm3d.h states (mm3d_set_icp_geometry_rejection), on top of the restated rejection of
test_icp_rejection_cpu.py, and the scenes: the half-overlapping height field, the slanted cabinet, the lattice sheet, the disc."""
import collections
import functools

import numpy as np

from test_gpu_icp_plane import _ldlt_solve, _nearest, _problem, _xform_f32, construct_transform
from test_icp_rejection_cpu import DEFAULT, _umeyama, max_d2_of, restate_rejection

Geo = collections.namedtuple("Geo", "boundary boundary_radius boundary_angle_deg boundary_min_neighbours normals normal_angle_deg")
GEO_DEFAULT = Geo(0, 0.0, 90.0, 3, 0, 45.0)
KEPT, BOUNDARY, NORMALS, ONE_TO_ONE, DISTANCE = 0, 1, 2, 3, 4


def geo(**kw):
    return GEO_DEFAULT._replace(**kw)


def cos_deg(deg):
    """cos(theta) as the rule wants it: libm's, but exact at 90 and 180."""
    return 0.0 if deg == 90.0 else -1.0 if deg == 180.0 else float(np.cos(deg * (np.pi / 180.0)))


# ---------------------------------------------------------------- the boundary rule
def directions(p, n, q):
    """The tangent-plane directions (x, y) of the float rows q as seen from the float point p with float normal n, in double; rows
    that are no direction (q == p, or along the normal) are left out by the caller through the returned mask."""
    p, n, q = p.astype(np.float64), n.astype(np.float64), q.astype(np.float64)
    k = int(np.argmin(np.abs(n)))                 # (argmin: ties to the lowest k)
    e = np.zeros(3)
    e[k] = 1.0
    u = np.array([e[1] * n[2] - e[2] * n[1], e[2] * n[0] - e[0] * n[2], e[0] * n[1] - e[1] * n[0]])
    v = np.array([n[1] * u[2] - n[2] * u[1], n[2] * u[0] - n[0] * u[2], n[0] * u[1] - n[1] * u[0]])
    d = q - p
    x = (u[0] * d[:, 0] + u[1] * d[:, 1]) + u[2] * d[:, 2]
    y = (v[0] * d[:, 0] + v[1] * d[:, 1]) + v[2] * d[:, 2]
    return x, y, (x != 0.0) | (y != 0.0)


def wedge_unfilled(x, y, c):
    """For every direction a: does NO direction b fill its wedge (counter-clockwise of a by an angle in (0, theta])?"""
    c2 = c * c
    cross = x[:, None] * y[None, :] - y[:, None] * x[None, :]
    dot = x[:, None] * x[None, :] + y[:, None] * y[None, :]
    nn = x * x + y * y
    rhs = c2 * (nn[:, None] * nn[None, :])
    dd = dot * dot
    ccw = (cross > 0.0) | ((cross == 0.0) & (dot < 0.0))
    within = ((dot >= 0.0) & (dd >= rhs)) if c >= 0.0 else ((dot >= 0.0) | (dd <= rhs))
    return ~(ccw & within).any(axis=1)


def restate_boundary(pts, nrm, r, angle_deg=90.0, k=3, chunk=256):
    """The boundary flags of the rule, point by point.  Returns (flags bool[n], directions per point int[n])."""
    pts, nrm = np.asarray(pts, dtype=np.float32), np.asarray(nrm, dtype=np.float32)[:, :3]
    n = len(pts)
    c, r2 = cos_deg(float(angle_deg)), float(r) * float(r)
    flags, counts = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64)
    fin = np.isfinite(pts).all(axis=1)
    ok = fin & np.isfinite(nrm).all(axis=1) & (nrm != 0).any(axis=1)
    P = pts.astype(np.float64)
    cand = np.flatnonzero(fin)
    for a in range(0, n, chunk):
        rows = np.arange(a, min(a + chunk, n))
        with np.errstate(invalid="ignore"):
            d = P[cand][None, :, :] - P[rows][:, None, :]
            d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
            near = (d2 <= r2) & (d != 0.0).any(axis=2)
        for i, row in zip(rows, near):
            if not ok[i]:
                continue
            x, y, has = directions(pts[i], nrm[i], pts[cand[row]])
            x, y = x[has], y[has]
            counts[i] = len(x)
            flags[i] = len(x) >= k and bool(wedge_unfilled(x, y, c).any())
    return flags, counts


# ---------------------------------------------------------------- step 1b
def restate_step1b(T, idx, d2, g, max_d2, flags, src_nrm, tgt_nrm):
    """Reasons (0 / 1 / 2) of step 1b for the matched correspondences of one iteration at the float transform T."""
    idx = np.asarray(idx, dtype=np.int64)
    matched = (idx >= 0) & (np.asarray(d2, dtype=np.float32) <= max_d2)
    reason = np.zeros(len(idx), dtype=np.uint8)
    j = np.where(matched, idx, 0)
    if g.boundary:
        reason[matched & flags[j]] = BOUNDARY
    if g.normals:
        R = np.asarray(T, dtype=np.float32)[:3, :3]
        ns, nt = np.asarray(src_nrm, dtype=np.float32)[:, :3], np.asarray(tgt_nrm, dtype=np.float32)[j, :3]
        with np.errstate(invalid="ignore", over="ignore"):
            m = np.stack([(R[r, 0] * ns[:, 0] + R[r, 1] * ns[:, 1]) + R[r, 2] * ns[:, 2] for r in range(3)], axis=1).astype(np.float32)
            usable = np.isfinite(ns).all(axis=1) & np.isfinite(nt).all(axis=1) & np.isfinite(m).all(axis=1)
            md, td = m.astype(np.float64), nt.astype(np.float64)
            d = (md[:, 0] * td[:, 0] + md[:, 1] * td[:, 1]) + md[:, 2] * td[:, 2]
            mm = (md[:, 0] * md[:, 0] + md[:, 1] * md[:, 1]) + md[:, 2] * md[:, 2]
            tt = (td[:, 0] * td[:, 0] + td[:, 1] * td[:, 1]) + td[:, 2] * td[:, 2]
            cn = cos_deg(float(g.normal_angle_deg))
            agree = usable & (mm > 0.0) & (tt > 0.0) & (d * d >= (cn * cn) * (mm * tt))
        reason[matched & (reason == 0) & ~agree] = NORMALS
    return reason


def restate_geometry(T, idx, d2, o, g, max_d2, flags=None, src_nrm=None, tgt_nrm=None):
    """Steps 1, 1b, 2, 3 for one iteration: (kept mask, reason per source point, rejection stats, geometry stats, rank gap)."""
    idx = np.asarray(idx, dtype=np.int64)
    d2 = np.asarray(d2, dtype=np.float32)
    matched = (idx >= 0) & (d2 <= max_d2)
    dropped = restate_step1b(T, idx, d2, g, max_d2, flags, src_nrm, tgt_nrm)
    kept, st, gap = restate_rejection(np.where(dropped != 0, -1, idx), d2, o, max_d2)
    # one-to-one's losers, as restate_rejection decides them: the survivors of the rest without the distance rejector
    surv = restate_rejection(np.where(dropped != 0, -1, idx), d2, o._replace(distance=0), max_d2)[0]
    reason = np.where(kept, KEPT, np.where(~matched, DISTANCE, np.where(dropped != 0, dropped, np.where(~surv, ONE_TO_ONE, DISTANCE)))).astype(np.uint8)
    gs = dict(matched=int(matched.sum()), on_boundary=int((dropped == BOUNDARY).sum()), normal_mismatch=int((dropped == NORMALS).sum()),
              passed=int(matched.sum() - (dropped != 0).sum()), target_boundary_points=int(flags.sum()) if g.boundary else 0)
    return kept, reason, st, gs, gap


def restate_icp_geometry(src, tgt, nrm, guess, max_corr, max_iter, eps, o=DEFAULT, g=GEO_DEFAULT, flags=None, src_nrm=None, tgt_nrm=None,
                         tau=1e-12):
    """restate_icp_rejecting's loop with step 1b in its correspondence stage (nrm: the point-to-plane normals of the target, or
    None for the point-to-point estimate).  Returns (T, iterations, converged, margins, smallest rank gap, rejection stats,
    geometry stats)."""
    max_d2 = max_d2_of(max_corr)
    T = np.asarray(guess, dtype=np.float32).copy()
    fin = np.isfinite(src).all(axis=1)
    prev_mse, iters, margins, min_gap, st, gs = np.finfo(np.float64).max, 0, [], np.inf, None, None
    while True:
        s = _xform_f32(T, src)
        idx = np.full(len(src), -1, dtype=np.int64)
        d2 = np.full(len(src), np.inf, dtype=np.float32)
        idx[fin], d2[fin] = _nearest(s[fin], tgt)
        kept, _, st, gs, gap = restate_geometry(T, idx, d2, o, g, max_d2, flags, src_nrm, tgt_nrm)
        min_gap = min(min_gap, gap)
        cnt = int(kept.sum())
        if cnt < 3:
            return T, iters, 0, margins, min_gap, st, gs
        sd, d = s[kept].astype(np.float64), tgt[idx[kept]].astype(np.float64)
        if nrm is None:
            Ti = _umeyama(sd, d)
        else:
            n = nrm[idx[kept]].astype(np.float64)
            ok = np.isfinite(n).all(axis=1)
            sr, dr, n = sd[ok], d[ok], n[ok]
            sx, sy, sz = sr[:, 0], sr[:, 1], sr[:, 2]
            nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
            A = np.stack([nz * sy - ny * sz, nx * sz - nz * sx, ny * sx - nx * sy, nx, ny, nz], axis=1)
            r = (nx * dr[:, 0] + ny * dr[:, 1] + nz * dr[:, 2]) - (nx * sx + ny * sy + nz * sz)
            AtA, Atr = A.T @ A, A.T @ r
            floor = tau * np.trace(AtA) / 6.0
            x, pivots = _ldlt_solve(AtA, Atr, floor) if len(A) >= 6 else (None, [])
            margins += [abs(p - floor) / max(abs(floor), 1e-300) for p in pivots]
            if x is None:
                return T, iters, 0, margins, min_gap, st, gs
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
            return T, iters, 1, margins, min_gap, st, gs
        cos_angle = 0.5 * ((float(Ti[0, 0]) + float(Ti[1, 1]) + float(Ti[2, 2])) - 1.0)
        t2 = float(Ti[0, 3]) * float(Ti[0, 3]) + float(Ti[1, 3]) * float(Ti[1, 3]) + float(Ti[2, 3]) * float(Ti[2, 3])
        margins += [abs((1.0 - cos_angle) - eps) / eps, abs(t2 - eps) / eps]
        if cos_angle >= 1.0 - eps and t2 <= eps:
            return T, iters, 1, margins, min_gap, st, gs
        mse = float(d2[kept].astype(np.float64).sum()) / cnt
        if iters > 1:
            margins.append(abs(abs(mse - prev_mse) - 1e-12) / 1e-12)
        if abs(mse - prev_mse) < 1e-12:
            return T, iters, 1, margins, min_gap, st, gs
        prev_mse = mse


# ---------------------------------------------------------------- scenes
def _height(x, y):
    return (0.35 * np.sin(0.9 * x) * np.cos(0.8 * y) + 0.25 * np.sin(0.45 * x + 1.1 * y) + 0.15 * np.cos(1.7 * x - 0.6 * y) +
            0.2 * np.sin(2.4 * x + 0.5) * np.sin(2.2 * y))


def _height_normals(x, y):
    hx = (0.35 * 0.9 * np.cos(0.9 * x) * np.cos(0.8 * y) + 0.25 * 0.45 * np.cos(0.45 * x + 1.1 * y) - 0.15 * 1.7 * np.sin(1.7 * x - 0.6 * y) +
          0.2 * 2.4 * np.cos(2.4 * x + 0.5) * np.sin(2.2 * y))
    hy = (-0.35 * 0.8 * np.sin(0.9 * x) * np.sin(0.8 * y) + 0.25 * 1.1 * np.cos(0.45 * x + 1.1 * y) + 0.15 * 0.6 * np.sin(1.7 * x - 0.6 * y) +
          0.2 * 2.2 * np.sin(2.4 * x + 0.5) * np.cos(2.2 * y))
    n = np.stack([-hx, -hy, np.ones_like(hx)], axis=1)
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)


HF_MAX_CORR, HF_RADIUS, HF_ITER, HF_EPS = 1.0, 0.35, 80, 1e-8
HF_SEEDS = (1, 3, 4)


def height_field_sample(seed, n, x0, x1, y0=0.0, y1=6.0, noise=0.003):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)
    z = _height(x, y) + rng.normal(0.0, noise, n)
    return np.stack([x, y, z], axis=1).astype(np.float32), _height_normals(x, y)


@functools.lru_cache(maxsize=None)
def height_field_pair(seed, n=5000):
    """Two independent samples of one smooth height field, x in [0, 7] (the source) and x in [4, 11] (the target), y in [0, 6]: a
    43 % overlap, 3 mm noise.  Both are in the world frame, so the true transform is the identity; the guess is 4 degrees of yaw plus
    a shift of (0.35, -0.25, 0.02).  Returns (source, its analytic normals, target, its analytic normals, T_true, guess)."""
    src, sn = height_field_sample(seed, n, 0.0, 7.0)
    tgt, tn = height_field_sample(seed + 1000, n, 4.0, 11.0)
    guess = construct_transform(0.0, 0.0, np.radians(4.0), 0.35, -0.25, 0.02).astype(np.float32)
    return src, sn, tgt, tn, np.eye(4), guess


def frobenius(T, T_true):
    return float(np.linalg.norm(np.asarray(T, dtype=np.float64) - np.asarray(T_true, dtype=np.float64)))


def slanted_cabinet(seed, n=3000):
    """_problem(seed, n) plus 1200 source-only points on a cabinet front that leaves the wall x = 8 at 40 degrees about the vertical:
    from (7.9, 1.0) along (-sin 40, cos 40) for 4 m, z in [0, 2.5].  Returns (target, target normals, source, source normals, T_true,
    guess); the source's normals are the target's (and the front's) carried by T_true^-1."""
    tgt, nrm, src, T_true, guess = _problem(seed, n)
    rng = np.random.default_rng(seed + 500)
    a = np.radians(40.0)
    along = np.array([-np.sin(a), np.cos(a), 0.0])
    s, z = rng.uniform(0, 4, 1200), rng.uniform(0, 2.5, 1200)
    cab = np.array([7.9, 1.0, 0.0]) + s[:, None] * along + z[:, None] * np.array([0.0, 0.0, 1.0])
    cab_n = np.tile(np.array([-np.cos(a), -np.sin(a), 0.0]), (1200, 1))
    Ti = np.linalg.inv(T_true)
    cab_src = (Ti @ np.c_[cab, np.ones(len(cab))].T).T[:, :3].astype(np.float32)
    n_world = np.concatenate([nrm.astype(np.float64), cab_n])
    src_n = (Ti[:3, :3] @ n_world.T).T.astype(np.float32)
    return tgt, nrm, np.concatenate([src, cab_src]), src_n, T_true, guess


def lattice_sheet(side=40, pitch=0.25, hole=(17, 23)):
    """A side x side lattice in the plane z = 0 with the open square of lattice indices hole[0] .. hole[1] - 1 (both axes) removed,
    normals (0, 0, 1).  Returns (points, normals, lattice indices (i, j) of the rows)."""
    i, j = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    keep = ~((i >= hole[0]) & (i < hole[1]) & (j >= hole[0]) & (j < hole[1]))
    i, j = i[keep], j[keep]
    pts = np.stack([i * pitch, j * pitch, np.zeros(len(i))], axis=1).astype(np.float32)
    return pts, np.tile(np.array([0, 0, 1], dtype=np.float32), (len(pts), 1)), np.stack([i, j], axis=1)


def disc_with_sector(m, cut_deg, seed, r=0.5, centre=(3.0, -2.0, 1.0)):
    """A query point (row 0) with exactly m neighbours inside radius r in its tangent plane z = centre z, none of them in the sector
    of cut_deg degrees that starts at a seeded angle, and one on either edge of the sector: the query's largest gap is cut_deg.
    The other rows are the disc's own points, whose neighbourhoods differ.  Normals (0, 0, 1)."""
    rng = np.random.default_rng(seed)
    start = rng.uniform(0, 2 * np.pi)
    ang = start + np.radians(cut_deg) + rng.uniform(0, 2 * np.pi - np.radians(cut_deg), m)
    ang[0], ang[1] = start + np.radians(cut_deg), start + 2 * np.pi
    rad = r * np.sqrt(rng.uniform(0.01, 0.9, m))
    pts = np.asarray(centre) + np.stack([rad * np.cos(ang), rad * np.sin(ang), np.zeros(m)], axis=1)
    pts = np.concatenate([np.asarray(centre)[None, :], pts]).astype(np.float32)
    return pts, np.tile(np.array([0, 0, 1], dtype=np.float32), (len(pts), 1))

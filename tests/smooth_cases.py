"""The moving-least-squares rule of include/mm3d.h (mm3d_set_smoothing) restated in numpy, written to be read, and the clouds the
smoothing tests run it on.  The neighbour test is the rule's float d2 against r * r in double; everything behind it is double
(or, for the second formulations of test_smoothing_cpu.py, np.longdouble), the 6 x 6 system goes through an unpivoted LDLt.
O(n^2) per cloud, so every case has at most 5 000 points.  Nothing here imports the library."""
import functools

import numpy as np

INVALID, FEW, DEGENERATE, PLANE, POLYNOMIAL = 0, 1, 2, 3, 4
GAP_TAU = 1e-6                  # DEGENERATE: lambda1 - lambda0 <= GAP_TAU * trace
PIVOT_TAU = 1e-9                # order 2 is singular: a pivot <= PIVOT_TAU * trace(M) / 6
POLY_MIN = 6                    # order 2 needs as many neighbours as it has coefficients


# ---------------------------------------------------------------- the rule
def valid_rows(xyz):
    return np.isfinite(xyz).all(axis=1)


def d2_row(xyz, i):
    """The rule's d2 of every record against record i: (dx * dx + dy * dy) + dz * dz, every operation one float32 operation."""
    x = np.ascontiguousarray(xyz, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x - x[i]
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def neighbours(xyz, valid, i, r):
    """(indices, their float d2) of point i's neighbours: the valid j with (double)d2 <= r * r; i itself and duplicates count."""
    d2 = d2_row(xyz, i)
    with np.errstate(invalid="ignore"):
        nb = np.nonzero(valid & (d2.astype(np.float64) <= float(r) * float(r)))[0]
    return nb, d2[nb]


def jacobi_eigh(C):
    """Eigenvalues ascending and eigenvectors in the columns, by cyclic Jacobi in C's own dtype (np.linalg.eigh has no
    longdouble): the second formulation's solver."""
    a = np.array(C, dtype=C.dtype)
    V = np.eye(3, dtype=C.dtype)
    eps = np.finfo(C.dtype).eps
    for _ in range(60):
        off = a[0, 1] ** 2 + a[0, 2] ** 2 + a[1, 2] ** 2
        if not off > (eps * eps) * (a[0, 0] ** 2 + a[1, 1] ** 2 + a[2, 2] ** 2 + 2 * off):
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            if a[p, q] == 0:
                continue
            theta = (a[q, q] - a[p, p]) / (2 * a[p, q])
            t = (1 if theta >= 0 else -1) / (abs(theta) + np.sqrt(theta * theta + 1))
            c = 1 / np.sqrt(t * t + 1)
            s = t * c
            J = np.eye(3, dtype=C.dtype)
            J[p, p] = J[q, q] = c
            J[p, q], J[q, p] = s, -s
            a = J.T @ a @ J
            a[p, q] = a[q, p] = 0
            V = V @ J
    lam = np.array([a[0, 0], a[1, 1], a[2, 2]])
    order = np.argsort(lam, kind="stable")
    return lam[order], V[:, order]


def ldlt_solve(M, g, floor):
    """M c = g by an unpivoted LDLt in M's dtype: (c or None when a pivot is at or below floor, the smallest pivot met)."""
    n = len(g)
    L = np.eye(n, dtype=M.dtype)
    D = np.zeros(n, dtype=M.dtype)
    smallest = np.inf
    for j in range(n):
        d = M[j, j] - (L[j, :j] * L[j, :j] * D[:j]).sum()
        smallest = min(smallest, float(d))
        if not d > floor:
            return None, smallest
        D[j] = d
        for i in range(j + 1, n):
            L[i, j] = (M[i, j] - (L[i, :j] * L[j, :j] * D[:j]).sum()) / d
    y = np.zeros(n, dtype=M.dtype)
    for i in range(n):
        y[i] = g[i] - (L[i, :i] * y[:i]).sum()
    c = np.zeros(n, dtype=M.dtype)
    for i in range(n - 1, -1, -1):
        c[i] = y[i] / D[i] - (L[i + 1:, i] * c[i + 1:]).sum()
    return c, smallest


def fit_point(q, d2, r, min_neighbours, dtype=np.float64, frame=0.0):
    """Steps 2 - 5 of the rule for one valid point from its neighbours' q = (double)p_j - (double)p_i [m][3] and float d2 [m].
    Both orders at once: returns dict(state1, disp1, state2, disp2, gap, pivot) with gap = (lambda1 - lambda0) / trace (nan when
    there is none) and pivot = the smallest pivot over its floor (inf when order 2 was not tried).  frame turns u, v about n."""
    zero = np.zeros(3)
    out = dict(state1=FEW, disp1=zero, state2=FEW, disp2=zero, gap=np.nan, pivot=np.inf)
    if len(q) < min_neighbours:
        return out
    q = q.astype(dtype)
    r = dtype(r)
    w = np.exp(-d2.astype(dtype) / (r * r))
    sw = w.sum()
    mu = (w[:, None] * q).sum(axis=0) / sw
    qc = q - mu
    C = (qc.T @ (w[:, None] * qc)) / sw
    trace = C[0, 0] + C[1, 1] + C[2, 2]
    lam, V = np.linalg.eigh(C) if dtype is np.float64 else jacobi_eigh(C)
    out["state1"] = out["state2"] = DEGENERATE
    if not (np.isfinite(trace) and np.isfinite(lam).all() and np.isfinite(V).all() and trace > 0):
        return out
    out["gap"] = float((lam[1] - lam[0]) / trace)
    if lam[1] - lam[0] <= dtype(GAP_TAU) * trace:
        return out
    n = V[:, 0] / np.sqrt((V[:, 0] * V[:, 0]).sum())
    o = (mu * n).sum() * n
    out.update(state1=PLANE, disp1=o.astype(np.float64), state2=PLANE, disp2=o.astype(np.float64))
    if len(q) < POLY_MIN:
        return out
    cf, sf = dtype(np.cos(frame)), dtype(np.sin(frame))
    u, v = cf * V[:, 1] + sf * V[:, 2], cf * V[:, 2] - sf * V[:, 1]
    e = q - o
    a, b, h = (e @ u) / r, (e @ v) / r, e @ n
    Phi = np.stack([np.ones_like(a), a, b, a * a, a * b, b * b], axis=1)
    M = Phi.T @ (w[:, None] * Phi)
    g = Phi.T @ (w * h)
    floor = dtype(PIVOT_TAU) * np.trace(M) / 6
    c, smallest = ldlt_solve(M, g, floor)
    out["pivot"] = float(smallest / floor) if floor > 0 else -np.inf
    if c is None:
        return out
    d = o + c[0] * n
    if np.isfinite(d).all() and np.sqrt((d * d).sum()) <= r:
        out.update(state2=POLYNOMIAL, disp2=d.astype(np.float64))
    return out


def smooth(xyz, r, min_neighbours, queries=None, dtype=np.float64, frame=0.0, shuffle=None):
    """The rule for the records `queries` (all of them by default) of a cloud: dict of arrays in the order of `queries` --
    count, state1, disp1, state2, disp2, gap, pivot, margin (how many float32 ulps the nearest inexact d2 lies from r * r).
    shuffle: a Generator that permutes every neighbour list before anything is summed."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    valid = valid_rows(xyz)
    queries = np.arange(len(xyz)) if queries is None else np.asarray(queries)
    m = len(queries)
    res = dict(count=np.zeros(m, dtype=np.int32), state1=np.zeros(m, dtype=np.int32), state2=np.zeros(m, dtype=np.int32),
               disp1=np.zeros((m, 3)), disp2=np.zeros((m, 3)), gap=np.full(m, np.nan), pivot=np.full(m, np.inf), margin=np.full(m, np.inf))
    r2 = float(r) * float(r)
    ulp = float(np.spacing(np.float32(r2)))
    p64 = xyz.astype(np.float64)
    for k, i in enumerate(queries):
        if not valid[i]:
            continue
        d2_all = d2_row(xyz, i)
        with np.errstate(invalid="ignore"):
            off = np.abs(d2_all.astype(np.float64) - r2)
            nb = np.nonzero(valid & (d2_all.astype(np.float64) <= r2))[0]      # (neighbours(xyz, valid, i, r), on the row at hand)
        off = off[valid & (off > 0)]                           # (a d2 equal to r * r is a planted one)
        if len(off):
            res["margin"][k] = off.min() / ulp
        d2 = d2_all[nb]
        if shuffle is not None:
            perm = shuffle.permutation(len(nb))
            nb, d2 = nb[perm], d2[perm]
        f = fit_point(p64[nb] - p64[i], d2, r, min_neighbours, dtype, frame)
        res["count"][k] = len(nb)
        for key in ("state1", "state2", "disp1", "disp2", "gap", "pivot"):
            res[key][k] = f[key]
    return res


def stats_of(state, disp):
    """mm3d_smooth_stats of a whole cloud's states and displacements."""
    return dict(points=len(state), valid=int((state != INVALID).sum()), few=int((state == FEW).sum()), degenerate=int((state == DEGENERATE).sum()),
                plane=int((state == PLANE).sum()), polynomial=int((state == POLYNOMIAL).sum()),
                max_displacement=float(np.sqrt((disp * disp).sum(axis=1)).max()) if len(state) else 0.0)


def apply(xyz, disp, state):
    """Step 6: (float)((double)p + disp) per coordinate; an invalid record as it was."""
    out = np.array(xyz, dtype=np.float32)
    ok = state != INVALID
    out[ok] = (xyz[ok].astype(np.float64) + disp[ok]).astype(np.float32)
    return out


def voxel_centroids(xyz, leaf):
    """One centroid per occupied voxel of side leaf (what the library's down-sampling does to a cloud, up to its summation order)."""
    keys = np.floor(xyz.astype(np.float64) / leaf).astype(np.int64)
    _, inv = np.unique(keys, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv)
    out = np.stack([np.bincount(inv, weights=xyz[:, a].astype(np.float64)) / cnt for a in range(3)], axis=1)
    return out.astype(np.float32)


# ---------------------------------------------------------------- the clouds
LATTICE = 2.0 ** -10            # the clouds that are also translated lie on this lattice, so that the translation is exact in float32


def _snap(xyz, step=LATTICE):
    return (np.rint(np.asarray(xyz, dtype=np.float64) / step) * step).astype(np.float32)


def sphere_cap(n=750, R=2.0, sigma=0.02, centre=(5.0, -3.0, 1.0), seed=3, density=100.0, gap=0.0):
    """n points of a sphere's cap about +z at `density` points / m^2, moved along the radius by noise of deviation sigma plus gap.
    Returns (xyz float64, the sphere's centre, R): the distance to the true surface is | |p - centre| - R |."""
    rng = np.random.default_rng(seed)
    area = n / density
    cos_max = 1.0 - area / (2.0 * np.pi * R * R)
    cz = rng.uniform(cos_max, 1.0, n)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    s = np.sqrt(1.0 - cz * cz)
    d = np.stack([s * np.cos(phi), s * np.sin(phi), cz], axis=1)
    rad = R + gap + rng.normal(0.0, sigma, n)
    return np.asarray(centre)[None, :] + d * rad[:, None], np.asarray(centre, dtype=np.float64), R


SPHERE_R, SPHERE_RADIUS = 2.0, 0.3


def sphere_case():
    xyz, _, _ = sphere_cap()
    return _snap(xyz)


def plane_lattice():
    """A noise-free plane z = 1.25: 21 x 21 points 2^-4 apart.  Every displacement is zero to rounding."""
    i, j = np.meshgrid(np.arange(21), np.arange(21), indexing="ij")
    return np.stack([i.reshape(-1) / 16.0 + 2.0, j.reshape(-1) / 16.0 - 1.0, np.full(441, 1.25)], axis=1).astype(np.float32)


THRESHOLD_R = 0.5


def threshold():
    """Radius 0.5, coordinates multiples of 2^-6, so every d2 is exact.  Records come in pairs (2 k, 2 k + 1): pairs 0 - 7
    exactly 0.5 apart along x (neighbours: count 2), pairs 8 - 15 0.5 + 2^-6 apart (count 1), each family at eight offsets so
    that some pairs lie on opposite sides of a cell border whatever the cell is near 0.5 (as cluster_cases.threshold)."""
    u = 2.0 ** -6
    pts = []
    for j in range(8):
        x0 = 3.0 * j + 5 * j * u
        pts += [(x0, 0.0, 0.0), (x0 + 0.5, 0.0, 0.0)]
    for j in range(8):
        x0 = 3.0 * j + 7 * j * u
        pts += [(x0, 4.0, 0.0), (x0 + 0.5 + u, 4.0, 0.0)]
    pts += [(1.0, 8.0, 0.0), (1.0, 8.5, 0.0), (5.0, 8.0, 1.0), (5.0, 8.0, 1.5)]
    return np.array(pts, dtype=np.float32)


THRESHOLD_COUNTS = [2] * 16 + [1] * 16 + [2] * 4

COUNTS_R, COUNTS_MIN = 0.4, 4
COUNTS_SIZES = (3, 4, 5, 6, 7)


def count_boundaries():
    """Five groups ten metres apart, of min_neighbours - 1, min_neighbours, 5, 6 and 7 points, each inside a ball of diameter
    below r: every point of a group has the group's size as its count.  A group is a regular polygon of radius 0.45 r in a
    gently tilted plane, bent out of it, for 6 and 7 with its centre as well (so that no conic holds all of them)."""
    rng = np.random.default_rng(17)
    pts = []
    for g, k in enumerate(COUNTS_SIZES):
        ring = k - 1 if k >= 6 else k
        ang = 2.0 * np.pi * np.arange(ring) / ring + 0.2
        p = np.stack([0.45 * COUNTS_R * np.cos(ang), 0.45 * COUNTS_R * np.sin(ang), rng.uniform(-0.01, 0.01, ring)], axis=1)
        if k >= 6:
            p = np.concatenate([p, [[0.01, -0.02, 0.015]]])
        p[:, 2] += 0.1 * p[:, 0]
        pts.append(p + np.array([10.0 * g, 3.0, -2.0]))
    return np.concatenate(pts).astype(np.float32)


COLLINEAR_R = 0.35


def collinear():
    """Ten points 0.1 apart on a line along each axis, and one point five times over: C has exact zeros, every state is
    DEGENERATE in any arithmetic."""
    t = np.arange(10) * 0.1
    z = np.zeros(10)
    lines = [np.stack([t + 1.0, z + 2.0, z - 1.0], axis=1), np.stack([z + 6.0, t, z + 0.5], axis=1), np.stack([z - 4.0, z + 1.0, t + 3.0], axis=1)]
    return np.concatenate(lines + [np.tile([[20.0, 20.0, 20.0]], (5, 1))]).astype(np.float32)


RING_R = 0.5


def conic_ring():
    """Twelve points on a circle of radius 0.2 in a tilted plane, the radius above its diameter: the six basis functions are
    dependent on a conic, order 2 is singular and every state is PLANE."""
    ang = 2.0 * np.pi * np.arange(12) / 12.0
    p = np.stack([0.2 * np.cos(ang), 0.2 * np.sin(ang), np.zeros(12)], axis=1)
    c, s = np.cos(0.3), np.sin(0.3)
    return (p @ np.array([[1, 0, 0], [0, c, s], [0, -s, c]]) + np.array([1.0, 2.0, 3.0])).astype(np.float32)


def _sheet(n, side, seed, sigma=0.005):
    """n points of the gently curved sheet z = 0.1 sin(2 x) cos(1.5 y) over a square, with noise along z."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, side, (n, 2))
    z = 0.1 * np.sin(2.0 * xy[:, 0]) * np.cos(1.5 * xy[:, 1]) + rng.normal(0.0, sigma, n)
    return np.stack([xy[:, 0], xy[:, 1], z], axis=1)


INVALID_R = 0.3


def invalid_and_duplicates():
    """300 points of a sheet with NaN, +inf and -inf in each coordinate, the first and the last record among them, and exact
    duplicates, some of them three times."""
    xyz = _sheet(300, 1.6, 13).astype(np.float32)
    xyz[200:230] = xyz[10:40]
    xyz[230:240] = xyz[10:20]
    bad = [np.nan, np.inf, -np.inf]
    rows = [0, 299, 17, 18, 19, 101, 150, 151, 250]
    for k, r in enumerate(rows):
        xyz[r, k % 3] = bad[(k // 3) % 3]
    xyz[77] = (np.nan, np.inf, -np.inf)
    return xyz


DENSE_R = 0.4


def dense_blob():
    """5 000 points of a bent, noisy disc inside one ball of radius r / 2: everyone is everyone's neighbour."""
    rng = np.random.default_rng(11)
    rho = 0.47 * DENSE_R * np.sqrt(rng.uniform(0, 1, 5000))
    phi = rng.uniform(0, 2 * np.pi, 5000)
    x, y = rho * np.cos(phi), rho * np.sin(phi)
    z = 0.6 * x * x - 0.4 * x * y + rng.normal(0.0, 0.004, 5000)
    c, s = np.cos(0.5), np.sin(0.5)
    p = np.stack([x, y, z], axis=1) @ np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
    return (np.array([3.0, -2.0, 1.0]) + p).astype(np.float32)


ROOM_R = 0.2


def room(seed, n=4000):
    """A room-like scene: a floor of 2 x 2 m and two walls of 2 x 1 m that meet it and each other, n noisy points over the
    8 m^2, so that a ball of 0.2 m holds tens of points even at an edge."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 4, n)                                   # the floor has half the area
    a, b = rng.uniform(0, 2, n), rng.uniform(0, 1, n)
    e = rng.normal(0.0, 0.004, n)
    floor = np.stack([a, np.where(k == 0, b, b + 1.0), e], axis=1)
    wall_x = np.stack([e, a, b], axis=1)
    wall_y = np.stack([a, e, b], axis=1)
    return np.where((k <= 1)[:, None], floor, np.where((k == 2)[:, None], wall_x, wall_y))


WALL_R, WALL_LEAF, WALL_GAP = 0.15, 0.05, 0.04


def double_wall_layers(seed=5, n=2600):
    """Two noisy copies of a 3 m sphere's cap, 0.04 m apart along the normal (the second map's copy of a wall after an ICP's
    residual), noise 5 and 10 mm.  Returns (layer a, layer b, the sphere's centre, the radius of the surface between them)."""
    a, centre, R = sphere_cap(n, 3.0, 0.005, (0.0, 0.0, -3.0), seed, density=900.0, gap=-WALL_GAP / 2)
    b, _, _ = sphere_cap(n, 3.0, 0.010, (0.0, 0.0, -3.0), seed + 1, density=900.0, gap=WALL_GAP / 2)
    return a.astype(np.float32), b.astype(np.float32), centre, R


def double_wall():
    """The two layers after one voxel pass at 0.05 m: what the smoothing of the composed map sees."""
    a, b, _, _ = double_wall_layers()
    return voxel_centroids(np.concatenate([a, b]), WALL_LEAF)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (xyz float32 [n][3], radius, min_neighbours).  Made once, never written to."""
    sphere, room1 = sphere_case(), _snap(room(1))
    km1, km10 = np.array([1000.0, 1000.0, 0.0], dtype=np.float32), np.array([10000.0, 10000.0, 0.0], dtype=np.float32)
    out = {
        "a_sphere_cap": (sphere, SPHERE_RADIUS, 6),
        "b_plane_lattice": (plane_lattice(), 0.2, 6),
        "c_threshold": (threshold(), THRESHOLD_R, 3),
        "d_count_boundaries": (count_boundaries(), COUNTS_R, COUNTS_MIN),
        "e_collinear": (collinear(), COLLINEAR_R, 3),
        "f_conic_ring": (conic_ring(), RING_R, 6),
        "g_invalid_and_duplicates": (invalid_and_duplicates(), INVALID_R, 6),
        "h_dense_blob": (dense_blob(), DENSE_R, 6),
        "i_sphere_at_1km": (sphere + km1, SPHERE_RADIUS, 6),
        "j_sphere_at_10km": (sphere + km10, SPHERE_RADIUS, 6),
        "k_room_1": (room1, ROOM_R, 6),
        "l_room_1_at_1km": (room1 + km1, ROOM_R, 6),
        "m_room_1_at_10km": (room1 + km10, ROOM_R, 6),
        "n_room_2": (room(2).astype(np.float32), ROOM_R, 6),
        "o_double_wall": (double_wall(), WALL_R, 6),
        "p_empty": (np.empty((0, 3), dtype=np.float32), 0.3, 6),
        "q_one_point": (np.array([[1.0, 2.0, 3.0]], dtype=np.float32), 0.3, 6),
    }
    for name in ("i_sphere_at_1km", "j_sphere_at_10km", "l_room_1_at_1km", "m_room_1_at_10km"):      # the translations are exact
        base = out["a_sphere_cap" if "sphere" in name else "k_room_1"][0]
        off = km1 if "1km" in name else km10
        assert np.array_equal(out[name][0].astype(np.float64), base.astype(np.float64) + off.astype(np.float64))
    for xyz, _, _ in out.values():
        assert xyz.dtype == np.float32 and len(xyz) <= 5000
        xyz.setflags(write=False)
    return out


TRANSLATED = {"i_sphere_at_1km": "a_sphere_cap", "j_sphere_at_10km": "a_sphere_cap", "l_room_1_at_1km": "k_room_1", "m_room_1_at_10km": "k_room_1"}
# the cases whose degeneracy is planted: the conditions on the gap and the pivots hold for every other
PLANTED = ("e_collinear", "f_conic_ring")


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's result on a case, both orders (smooth()'s dict plus stats1, stats2): computed once, never written to."""
    xyz, r, min_nb = cases()[name]
    res = smooth(xyz, r, min_nb)
    res["stats1"] = stats_of(res["state1"], res["disp1"])
    res["stats2"] = stats_of(res["state2"], res["disp2"])
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res

"""The SPFH bins of single pairs, device against oracle, pair by pair (csrc/fpfh.hip, test hook mm3d_debug_pair_bins).

k_spfh bins a pair from pair_bins_fast -- plain f32 features plus an error bound, answering only when no feature is within its
bound of a bin edge and the two angles are clear of a tie -- and falls back to pair_features (the CPU path's floats) + the
exact binning otherwise.  A wrong bound shows only on pairs within a few u (2^-24) of a bin edge or of the angle tie; the
pipeline parity tests meet a handful of those.  Here (a) every in-radius pair of two synthetic filtered maps with the oracle's
normals and (b) pairs built to sit within a few u of each of the 30 bin edges and of the tie (kept by rejection on the ORACLE's
features), plus the degenerate geometries, go through both paths and are held against the oracle's pcl::computePairFeatures
and point_spfh binning (mo_pair_features, mo_spfh_pair_bins)."""
import ctypes as C

import numpy as np
import pytest

RES, R_DESC, R_NRM, MIN_NB = 0.1, 0.8, 0.6, 50
U = 2.0 ** -24
NB = 11
D_PI = np.float32(1.0) / (np.float32(2.0) * np.float32(np.pi))      # o_fpfh.c: 1.0f / (2.0f * (float)M_PI)
CHUNK = 1 << 22
POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")])
NORMAL = np.dtype([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("curvature", "<f4")])


def as_points(xyz):
    xyz = np.asarray(xyz, dtype=np.float32)
    p = np.zeros(len(xyz), dtype=POINT)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return p


def as_normals(v):
    v = np.asarray(v, dtype=np.float32)
    n = np.zeros(len(v), dtype=NORMAL)
    n["nx"], n["ny"], n["nz"] = v[:, 0], v[:, 1], v[:, 2]
    return n


def xyz_of(a, names=("x", "y", "z")):
    return np.stack([a[k] for k in names], 1)


def device_pair_bins(ctx, mm, p1, n1, p2, n2):
    """[n, 11] int32: f1, f2, f3 bits, branch, exact bins (3), fast ok, fast bins (3)."""
    out = np.empty((len(p1), 11), dtype=np.int32)
    for a in range(0, len(p1), CHUNK):
        b = min(a + CHUNK, len(p1))
        args = [np.ascontiguousarray(v[a:b]) for v in (p1, n1, p2, n2)]
        o = np.empty((b - a, 11), dtype=np.int32)
        ctx._ck(mm.lib().mm3d_debug_pair_bins(ctx._h, *[v.ctypes.data_as(C.c_void_p) for v in args], b - a,
                                              o.ctypes.data_as(C.c_void_p)))
        out[a:b] = o
    return out


def edge_distance(f, which):
    """Per pair: (distance of feature `which` (0: f1, 1: f2, 2: f3) to the nearest INTERIOR bin edge, in u; that edge, 1..10) --
    the edges of point_spfh's binning, evaluated as it evaluates them (double, d_pi the float)."""
    f = f.astype(np.float64)
    if which == 0:
        t = NB * ((f + np.pi) * float(D_PI))
        scale = 1.0 / (NB * float(D_PI))
    else:
        t = NB * ((f + 1.0) * 0.5)
        scale = 2.0 / NB
    k = np.rint(t)
    d = np.abs(t - k) * scale / U
    d[(k < 1) | (k > NB - 1) | ~np.isfinite(d)] = np.inf
    return d, k


def tie_distance(p1, n1, p2, n2):
    """||a1| - |a2|| in u, a_k = n_k . d / |d| in double from the float inputs."""
    d = xyz_of(p2).astype(np.float64) - xyz_of(p1).astype(np.float64)
    L = np.linalg.norm(d, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        a1 = (xyz_of(n1, ("nx", "ny", "nz")).astype(np.float64) * d).sum(1) / L
        a2 = (xyz_of(n2, ("nx", "ny", "nz")).astype(np.float64) * d).sum(1) / L
        r = np.abs(np.abs(a1) - np.abs(a2)) / U
    r[~np.isfinite(r)] = np.inf
    return r


# ---- (a) realistic pairs --------------------------------------------------------------------------------------------------
def in_radius_pairs(xyz, r):
    """Every ordered pair (i, j), i != j, with the float32 squared distance below float(r^2) (k_spfh's in-radius test)."""
    P = xyz.astype(np.float32)
    Pd = P.astype(np.float64)
    sq = (Pd * Pd).sum(1)
    r2 = np.float32(r * r)
    I, J = [], []
    for a in range(0, len(P), 2048):
        approx = sq[a:a + 2048, None] + sq[None, :] - 2.0 * Pd[a:a + 2048] @ Pd.T
        i, j = np.nonzero(approx < float(r2) * 1.01 + 1e-6)
        i = i + a
        d = P[i] - P[j]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        keep = (d2 < r2) & (i != j)
        I.append(i[keep]); J.append(j[keep])
    return np.concatenate(I), np.concatenate(J)


@pytest.fixture(scope="module")
def realistic(po, synth):
    world, maps = synth.synth_maps(2, 30000, overlap_step=0.35)
    sets = []
    for x, c, _ in maps:
        f = po.remove_outliers(po.downsample(synth.pack_points(x, c), RES), R_DESC, MIN_NB)
        n = po.normals(f, R_NRM)
        i, j = in_radius_pairs(xyz_of(f), R_DESC)
        sets.append((f[i], n[i], f[j], n[j]))
    return tuple(np.concatenate([s[k] for s in sets]) for k in range(4))


# ---- (b) near-edge and constructed pairs ----------------------------------------------------------------------------------
def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def build(rng, c, beta, f1):
    """Pairs with the unswitched features (f1, f2 = beta, f3 = c): n1 random, d = |d| (c n1 + s t) with t a unit vector normal
    to n1, n2 = alpha n1 + beta v + gamma t in the Darboux frame v = t x n1, w = t, alpha = rho cos f1, gamma = rho sin f1."""
    n = len(c)
    n1 = unit(rng.normal(size=(n, 3)))
    t = rng.normal(size=(n, 3))
    t = unit(t - (t * n1).sum(1, keepdims=True) * n1)
    v = np.cross(t, n1)
    s = np.sqrt(np.maximum(0.0, 1.0 - c * c))
    rho = np.sqrt(np.maximum(0.0, 1.0 - beta * beta))
    n2 = (rho * np.cos(f1))[:, None] * n1 + beta[:, None] * v + (rho * np.sin(f1))[:, None] * t
    L = np.exp(rng.uniform(np.log(0.05), np.log(0.8), n))
    p1 = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    p2 = (p1.astype(np.float64) + L[:, None] * (c[:, None] * n1 + s[:, None] * t)).astype(np.float32)
    n1, n2 = n1.astype(np.float32), n2.astype(np.float32)
    # a few ulps of jitter on n2 and p2 spread the features over the edge
    n2 = (n2.view(np.int32) + rng.integers(-6, 7, n2.shape).astype(np.int32)).view(np.float32)
    p2 = (p2.view(np.int32) + rng.integers(-2, 3, p2.shape).astype(np.int32)).view(np.float32)
    return as_points(p1), as_normals(n1), as_points(p2), as_normals(n2)


def near_edge_candidates(rng, per_edge=100_000):
    out = []
    f1_edges = np.arange(1, NB) / (NB * float(D_PI)) - np.pi
    f23_edges = 2.0 * np.arange(1, NB) / NB - 1.0
    for e in f23_edges:                                           # f3 = a1 at an edge
        n = per_edge
        out.append(build(rng, np.full(n, e), rng.uniform(-0.95, 0.95, n), rng.uniform(-np.pi, np.pi, n)))
    for e in f23_edges:                                           # f2 at an edge
        n = per_edge
        c = rng.uniform(0.3, 0.95, n) * rng.choice([-1.0, 1.0], n)
        out.append(build(rng, c, np.full(n, e), rng.uniform(-np.pi, np.pi, n)))
    for e in f1_edges:                                            # f1 at an edge
        n = per_edge
        c = rng.uniform(0.3, 0.95, n) * rng.choice([-1.0, 1.0], n)
        out.append(build(rng, c, rng.uniform(-0.9, 0.9, n), np.full(n, e)))
    # the tie |a1| == |a2|: rho cos(f1 - phi) = +-c with phi = atan2(s, c)
    n = 8 * per_edge
    c = rng.uniform(-0.9, 0.9, n)
    beta = rng.uniform(-1.0, 1.0, n) * np.sqrt(1.0 - c * c)
    rho = np.sqrt(1.0 - beta * beta)
    sg = rng.choice([-1.0, 1.0], n)
    phi = np.arctan2(np.sqrt(1.0 - c * c), c)
    f1 = phi + rng.choice([-1.0, 1.0], n) * np.arccos(np.clip(sg * c / rho, -1.0, 1.0))
    out.append(build(rng, c, beta, f1))
    return tuple(np.concatenate([o[k] for o in out]) for k in range(4))


def constructed_cases(rng):
    P1, N1, P2, N2 = [], [], [], []

    def add(p1, n1, p2, n2):
        m = max(len(np.atleast_2d(v)) for v in (p1, n1, p2, n2))
        for lst, v in ((P1, p1), (N1, n1), (P2, p2), (N2, n2)):
            lst.append(np.broadcast_to(np.atleast_2d(np.asarray(v, dtype=np.float32)), (m, 3)).copy())

    n = 20_000
    # |a1| == |a2| exactly and a1 == -a2: normals mirrored in the plane normal to d = (L, 0, 0)
    a = unit(rng.normal(size=(n, 3))).astype(np.float32)
    d = np.zeros((n, 3), np.float32); d[:, 0] = rng.uniform(0.05, 0.8, n)
    p1 = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    d = (p1 + d) - p1                                              # the float difference the kernels will see
    add(p1, a, p1 + d, a * np.float32([1, -1, 1]))
    add(p1, a, p1 + d, a * np.float32([-1, 1, 1]))
    add(p1, a, p1 + d, a[:, [0, 2, 1]])
    add(p1, a, p1 + d, -a)
    add(p1, a, p1 + d, a)
    # |a| at 1 - 1e-5 (both angles near +-1, the acos(|a|) > 1 edge of the fast path), kappa ~ 1000 (d nearly parallel to n1)
    for cval in (1.0 - 1e-5 * rng.uniform(0.5, 1.5, n), np.sqrt(1.0 - (1.0 / rng.uniform(900, 1100, n)) ** 2)):
        cs = cval * rng.choice([-1.0, 1.0], n)
        b = build(rng, cs, rng.uniform(-0.9, 0.9, n), rng.uniform(-np.pi, np.pi, n))
        add(xyz_of(b[0]), xyz_of(b[1], ("nx", "ny", "nz")), xyz_of(b[2]), xyz_of(b[3], ("nx", "ny", "nz")))
        # and n2 with |a2| near the same value
        n2 = xyz_of(b[1], ("nx", "ny", "nz")) * np.float32(-1)
        add(xyz_of(b[0]), xyz_of(b[1], ("nx", "ny", "nz")), xyz_of(b[2]), n2 + rng.normal(scale=1e-6, size=(n, 3)).astype(np.float32))
    # s = |d|^2 near 1e-12 and 1e12
    for s in (1e-12, 1e12):
        L = np.sqrt(s * np.exp(rng.uniform(np.log(0.5), np.log(2.0), n)))
        dd = unit(rng.normal(size=(n, 3))) * L[:, None]
        p1 = np.zeros((n, 3), np.float32) if s < 1 else rng.uniform(-1e6, 1e6, (n, 3)).astype(np.float32)
        add(p1, unit(rng.normal(size=(n, 3))), (p1 + dd).astype(np.float32), unit(rng.normal(size=(n, 3))))
    # |n|^2 at 0.98 and 1.02 (the fast path's normal-length window)
    for q in (0.98, 1.02):
        b = build(rng, rng.uniform(-0.95, 0.95, n), rng.uniform(-0.9, 0.9, n), rng.uniform(-np.pi, np.pi, n))
        sc = np.sqrt(q * (1.0 + rng.uniform(-2e-6, 2e-6, n)))[:, None]
        n1, n2 = xyz_of(b[1], ("nx", "ny", "nz")), xyz_of(b[3], ("nx", "ny", "nz"))
        add(xyz_of(b[0]), n1 * sc, xyz_of(b[2]), n2)
        add(xyz_of(b[0]), n1, xyz_of(b[2]), n2 * sc)
    # axis-aligned Darboux frames: n1 = z, d = (s, 0, c) L, so v = -y and w = x exactly
    c = rng.uniform(-0.95, 0.95, n)
    s = np.sqrt(1.0 - c * c) * rng.choice([-1.0, 1.0], n)
    p1 = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    p2 = (p1 + np.stack([s, np.zeros(n), c], 1) * rng.uniform(0.05, 0.8, n)[:, None]).astype(np.float32)
    z = np.zeros((n, 3), np.float32); z[:, 2] = 1.0
    ang = rng.uniform(-np.pi, np.pi, n)
    add(p1, z, p2, np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], 1))                  # x = n1 . n2 = 0
    al = -rng.uniform(0.05, 1.0, n)
    be = np.sqrt(1.0 - al * al) * rng.choice([-1.0, 1.0], n)
    for zero in (0.0, -0.0):                                                              # y = +-0 with x < 0: f1 at +-pi
        add(p1, z, p2, np.stack([np.full(n, zero), be, al], 1))
    # f4 == 0, NaN, infinities and zero normals
    m = 2000
    p1 = rng.uniform(-1, 1, (m, 3)).astype(np.float32)
    nn = unit(rng.normal(size=(m, 3)))
    add(p1, nn, p1, unit(rng.normal(size=(m, 3))))
    add(p1, np.zeros((m, 3)), p1 + np.float32(0.3), nn)
    add(p1, nn, p1 + np.float32(0.3), np.zeros((m, 3)))
    add(p1, np.full((m, 3), np.nan), p1 + np.float32(0.3), nn)
    add(p1, nn, p1 + np.float32([0.3, 0.0, 0.0]), np.full((m, 3), np.nan))
    add(p1, nn, np.full((m, 3), np.nan), nn)
    add(p1, nn, np.full((m, 3), np.inf), nn)
    P1, N1, P2, N2 = (np.concatenate(v) for v in (P1, N1, P2, N2))
    return as_points(P1), as_normals(N1), as_points(P2), as_normals(N2)


@pytest.fixture(scope="module")
def near_edge(po):
    rng = np.random.default_rng(2024)
    p1, n1, p2, n2 = near_edge_candidates(rng)
    f = po.pair_features(p1, n1, p2, n2)
    d = np.minimum.reduce([edge_distance(f[:, k], k)[0] for k in range(3)] + [tie_distance(p1, n1, p2, n2)])
    keep = d <= 64.0                                               # rejection on the oracle's features
    c = constructed_cases(rng)
    return tuple(np.concatenate([a[keep], b]) for a, b in zip((p1, n1, p2, n2), c)), int(keep.sum())


def same_bits(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def check_against_oracle(ctx, mm, po, pairs, label):
    p1, n1, p2, n2 = pairs
    got = device_pair_bins(ctx, mm, p1, n1, p2, n2)
    ref = po.pair_features(p1, n1, p2, n2)
    bins = po.spfh_pair_bins(p1, n1, p2, n2)
    n = len(p1)
    f = got[:, 0:3].copy().view(np.float32)
    for k, name in enumerate(("f1", "f2", "f3")):
        bad = np.flatnonzero(~same_bits(f[:, k], ref[:, k]))
        assert len(bad) == 0, f"{label}: {name} differs from the oracle on {len(bad)} of {n} pairs (first: pair {bad[0]}, " \
                              f"{f[bad[0], k]!r} vs {ref[bad[0], k]!r})"
    bad = np.flatnonzero(got[:, 3] != ref[:, 4].astype(np.int32))
    assert len(bad) == 0, f"{label}: branch code differs on {len(bad)} of {n} pairs (first: pair {bad[0]}: {got[bad[0], 3]} vs {ref[bad[0], 4]})"
    bad = np.flatnonzero((got[:, 4:7] != bins).any(1))
    assert len(bad) == 0, f"{label}: exact-path bins differ on {len(bad)} of {n} pairs (first: {got[bad[0], 4:7]} vs {bins[bad[0]]})"
    ok = got[:, 7] == 1
    bad = np.flatnonzero(ok & (got[:, 8:11] != bins).any(1))
    assert len(bad) == 0, f"{label}: pair_bins_fast answered WRONG bins on {len(bad)} of {int(ok.sum())} certified pairs " \
                          f"(first: pair {bad[0]}, {got[bad[0], 8:11]} vs {bins[bad[0]]})"
    return got, ref


@pytest.mark.gpu
def test_realistic_pairs_certified_bins_match_the_oracle(ctx, mm, po, realistic):
    """(a) every in-radius pair of two synthetic filtered maps (R = 0.8) with the oracle's normals: features, branch, exact bins
    bit-equal; the certified bins equal the oracle's wherever pair_bins_fast answers; and it declines at most 1e-3 of them."""
    got, _ = check_against_oracle(ctx, mm, po, realistic, "realistic pairs")
    declined = float(np.mean(got[:, 7] == 0))
    print(f"realistic pairs: {len(got)}, pair_bins_fast declined {declined:.3e} of them")
    assert declined <= 1e-3


@pytest.mark.gpu
def test_near_edge_pairs_certified_bins_match_the_oracle(ctx, mm, po, near_edge):
    """(b) pairs within a few u of each of the 30 bin edges and of the angle tie (the oracle's features decide), plus the
    constructed cases -- exact ties and mirrored angles, |a| at 1 - 1e-5, kappa ~ 1000, |d|^2 near 1e-12 and 1e12, |n|^2 at 0.98
    and 1.02, x = n1 . n2 = 0, y = +-0 with x < 0, f4 == 0, NaN, infinite and zero normals: every assertion of set (a), and on
    every certified pair the oracle's bins."""
    pairs, n_kept = near_edge
    got, ref = check_against_oracle(ctx, mm, po, pairs, "near-edge pairs")
    ok = got[:, 7] == 1
    print(f"near-edge pairs: {len(got)} ({n_kept} kept by rejection), certified {int(ok.sum())}")
    # coverage: pairs within 4 u of every edge and of the tie really are in the set
    short = []
    for k in range(3):
        d, e = edge_distance(ref[:, k], k)
        for edge in range(1, NB):
            cnt = int(((d <= 4.0) & (e == edge)).sum())
            if cnt < 20:
                short.append(f"f{k + 1} edge {edge}: {cnt}")
    ties = int((tie_distance(*pairs) <= 4.0).sum())
    if ties < 20:
        short.append(f"tie: {ties}")
    assert not short, f"the near-edge set lost its coverage: {short}"

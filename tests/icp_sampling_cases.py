"""ICP source sampling (mm3d_set_icp_sampling, mm3d_sample_icp_source): the rule of include/mm3d.h restated in numpy, bit for bit
-- integer arithmetic and single IEEE f32 multiplies and compares only -- and the scenes the CPU and the GPU tests share."""
import numpy as np

NONE, STRIDE, NORMAL_SPACE = 0, 1, 2
INVALID = -1


# ---------------------------------------------------------------- the rule
def restate_valid(xyz, nrm, method):
    """STRIDE: finite coordinates.  NORMAL_SPACE: also a finite normal with a non-zero component."""
    xyz = np.asarray(xyz, dtype=np.float32)
    ok = np.isfinite(xyz).all(axis=1)
    if method == NORMAL_SPACE:
        nrm = np.asarray(nrm, dtype=np.float32)
        ok &= np.isfinite(nrm).all(axis=1) & (nrm != 0).any(axis=1)
    return ok


def restate_buckets(xyz, nrm, method, bins):
    """One bucket id per point, INVALID for a point that is never sampled.  STRIDE has the one bucket 0."""
    ok = restate_valid(xyz, nrm, method)
    out = np.full(len(ok), INVALID, dtype=np.int64)
    if method == STRIDE:
        out[ok] = 0
        return out
    n = np.asarray(nrm, dtype=np.float32)[ok]
    a0, a1, a2 = np.abs(n[:, 0]), np.abs(n[:, 1]), np.abs(n[:, 2])
    face = np.zeros(len(n), dtype=np.int64)                  # the largest |component|, ties to the lowest index
    best = a0.copy()
    up = a1 > best
    face[up], best[up] = 1, a1[up]
    up = a2 > best
    face[up], best[up] = 2, a2[up]
    rows = np.arange(len(n))
    s = n[rows, face]
    r = np.abs(s)                                            # f32, > 0
    neg = s < 0                                              # antipodes fold: n and -n share a bucket
    cells = []
    for step in (1, 2):
        q = n[rows, (face + step) % 3]
        q = np.where(neg, -q, q).astype(np.float32)
        cell = np.zeros(len(n), dtype=np.int64)
        for k in range(1, bins):
            e = np.float32(-1.0 + 2.0 * k / bins)            # exact in f32 for bins 1, 2, 4, 8
            cell += q >= (e * r).astype(np.float32)          # one rounded f32 multiply
        cells.append(cell)
    out[ok] = (face * bins + cells[0]) * bins + cells[1]
    return out


def restate_budget(n_valid, fraction, max_points):
    m = min(n_valid, int(np.floor(np.float64(fraction) * np.float64(n_valid))))
    if max_points > 0:
        m = min(m, max_points)
    if n_valid > 0:
        m = max(m, 1)
    return m


def restate_waterfill(counts, m):
    """(L, take): L the largest integer in [0, max count] with sum min(c, L) <= m; take = min(c, L), and the rest of m one each
    to the buckets with c > L in ascending index."""
    c = np.asarray(counts, dtype=np.int64)
    lo, hi = 0, int(c.max()) if len(c) else 0
    while lo < hi:                                           # the largest L that still fits
        mid = (lo + hi + 1) // 2
        if int(np.minimum(c, mid).sum()) <= m:
            lo = mid
        else:
            hi = mid - 1
    L = lo
    take = np.minimum(c, L)
    rem = m - int(take.sum())
    over = np.flatnonzero(c > L)
    take[over[:rem]] += 1
    return L, take


def restate_sample(xyz, nrm, method, fraction=0.25, max_points=0, bins=4):
    """(keep flags, kept reference indices, stats) of the rule; stats as mm3d_last_icp_sampling_stats reports them."""
    n_buckets = 1 if method == STRIDE else 3 * bins * bins
    bucket = restate_buckets(xyz, nrm, method, bins)
    valid = bucket != INVALID
    counts = np.bincount(bucket[valid], minlength=n_buckets).astype(np.int64)
    n_valid = int(valid.sum())
    m = restate_budget(n_valid, fraction, max_points)
    L, take = restate_waterfill(counts, m)
    keep = np.zeros(len(bucket), dtype=bool)
    for b in np.flatnonzero(counts):
        idx = np.flatnonzero(bucket == b)                    # reference order
        r = np.arange(len(idx), dtype=np.int64)
        keep[idx] = ((r + 1) * take[b]) // counts[b] > (r * take[b]) // counts[b]
    stats = dict(points=len(bucket), valid=n_valid, sampled=m, buckets=int((counts > 0).sum()), level=L)
    return keep, np.flatnonzero(keep).astype(np.int32), stats, dict(bucket=bucket, counts=counts, take=take)


# ---------------------------------------------------------------- records
def records(xyz):
    out = np.zeros(len(xyz), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")])
    out["x"], out["y"], out["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out["rgba"] = 0xff808080
    return out


def normal_records(nrm):
    out = np.zeros(len(nrm), dtype=[("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("curvature", "<f4")])
    out["nx"], out["ny"], out["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    return out


# ---------------------------------------------------------------- normals for the exact tests
def _points(rng, n):
    return rng.uniform(-3, 3, (n, 3)).astype(np.float32)


def normals_one_bucket(rng, n):
    """(a) every normal in one bucket: ranks run across every wave and block."""
    return np.tile(np.array([0.1, -0.2, 0.97], dtype=np.float32), (n, 1))


def normals_cycling(rng, n, bins):
    """(b) the bucket changes with every point: the centre of cell (cu, cv) of face a, walking through all 3 bins^2 buckets (a
    wave of 64 points holds up to 64 distinct keys at bins 8)."""
    k = np.arange(n) * 7                                     # 7 is coprime to 3 bins^2
    face, cu, cv = (k // (bins * bins)) % 3, (k // bins) % bins, k % bins
    out = np.zeros((n, 3), dtype=np.float32)
    rows = np.arange(n)
    out[rows, face] = np.where(k % 2 == 0, 1.0, -1.0)        # both signs: folded
    sgn = out[rows, face]
    out[rows, (face + 1) % 3] = sgn * (-1.0 + (2.0 * cu + 1.0) / bins)
    out[rows, (face + 2) % 3] = sgn * (-1.0 + (2.0 * cv + 1.0) / bins)
    return out


def normals_edges(rng, n, bins):
    """(c) components exactly on the cell edges e_k r, exact |n_x| = |n_y| (= |n_z|) ties, and n beside -n."""
    r = np.array([1.0, 0.5, 3.0, 0.7, 1e-30, 1e30], dtype=np.float32)[np.arange(n) % 6]
    e = (-1.0 + 2.0 * (np.arange(n) // 6 % (bins + 1)) / bins).astype(np.float32)      # -1 ... 1: the edges and both ends
    out = np.zeros((n, 3), dtype=np.float32)
    face = (np.arange(n) // 2) % 3
    rows = np.arange(n)
    out[rows, face] = r
    out[rows, (face + 1) % 3] = (e * r).astype(np.float32)   # q == e_k r exactly (the same rounded product), and +-r ties
    out[rows, (face + 2) % 3] = (-e * r).astype(np.float32)
    third = rows % 5 == 0
    out[third] = r[third, None] * np.array([1, -1, 1], dtype=np.float32)               # |nx| = |ny| = |nz|
    out[1::2] = -out[0::2][:len(out[1::2])]                  # n against -n: the same bucket, pair by pair
    return out


def spoil(rng, xyz, nrm):
    """(d) NaN and zero normals, a negative-zero normal, an infinite component, NaN and infinite coordinates."""
    xyz, nrm = xyz.copy(), nrm.copy()
    n = len(xyz)
    if n >= 8:
        pick = rng.permutation(n)
        nrm[pick[0::8][:max(1, n // 16)]] = np.nan
        nrm[pick[1::8][:max(1, n // 16)]] = 0.0
        nrm[pick[2::8][:max(1, n // 32)]] = -0.0
        nrm[pick[3::8][:max(1, n // 32)], 1] = np.inf
        xyz[pick[4::8][:max(1, n // 16)], 2] = np.nan
        xyz[pick[5::8][:max(1, n // 32)], 0] = -np.inf
    return xyz, nrm


def skewed(rng, n, bins=8):
    """One bucket holding 90 % of the points beside buckets of one point each (water-fill: every singleton is kept): a tenth of
    the points, at most one for every other bucket of `bins`, move from the common normal to a bucket of their own."""
    nrm = normals_one_bucket(rng, n)
    singles = normals_cycling(rng, 3 * bins * bins, bins)
    zero = np.zeros((len(singles), 3), dtype=np.float32)
    big = restate_buckets(zero[:1], nrm[:1], NORMAL_SPACE, bins)[0] if n else -1
    singles = singles[restate_buckets(zero, singles, NORMAL_SPACE, bins) != big]
    few = rng.choice(n, min(n // 10, len(singles)), replace=False)
    nrm[few] = singles[:len(few)]
    return nrm


SIZES = (1, 63, 64, 65, 255, 256, 257, 4097)


# ---------------------------------------------------------------- the grooved plane
GROOVE_W, GROOVE_D = 0.08, 0.06
GROOVES_X, GROOVES_Y = (0.7, 2.1, 3.3), (1.2, 2.9)          # three grooves at fixed x (running along y), two at fixed y
SLIDE = (0.09, -0.07, 0.02)
YAW_DEG = 1.5


def _groove_profile(u, centres):
    """Depth below the plane and the slope dz/du of the V-grooves of width GROOVE_W centred at `centres`."""
    z, slope = np.zeros_like(u), np.zeros_like(u)
    for c in centres:
        d = u - c
        inside = np.abs(d) < GROOVE_W / 2
        z = np.where(inside, -(GROOVE_D - np.abs(d) * (2 * GROOVE_D / GROOVE_W)), z)
        slope = np.where(inside, np.sign(d) * (2 * GROOVE_D / GROOVE_W), slope)
    return z, slope


def grooved_plane(seed, n=10000, size=4.0, noise=0.004):
    """n points on a size x size plane with five V-grooves, their exact normals, and Gaussian noise along z."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, size, n), rng.uniform(0, size, n)
    zx, sx = _groove_profile(x, GROOVES_X)
    zy, sy = _groove_profile(y, GROOVES_Y)
    deeper_x = zx <= zy                                      # where two grooves cross, the deeper wall
    z = np.where(deeper_x, zx, zy)
    nx = np.where(deeper_x, -sx, 0.0)
    ny = np.where(deeper_x, 0.0, -sy)
    nrm = np.stack([nx, ny, np.ones(n)], axis=1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    xyz = np.stack([x, y, z + rng.normal(0, noise, n)], axis=1)
    return xyz.astype(np.float32), nrm.astype(np.float32)


def slide_pose():
    a = np.radians(YAW_DEG)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = SLIDE
    return T


def grooved_problem(seed, n=10000):
    """(source points, source normals, target points, target normals, T_true): two independent samplings of the plane, the source
    moved by T_true^-1 about the plane's centre, so that T_true registers it; the guess is the identity."""
    tgt, tn = grooved_plane(seed, n)
    src0, sn0 = grooved_plane(seed + 1000, n)
    C = np.eye(4)
    C[:3, 3] = [2.0, 2.0, 0.0]
    T_true = C @ slide_pose() @ np.linalg.inv(C)
    Ti = np.linalg.inv(T_true)
    src = (Ti @ np.c_[src0.astype(np.float64), np.ones(n)].T).T[:, :3].astype(np.float32)
    sn = (Ti[:3, :3] @ sn0.astype(np.float64).T).T.astype(np.float32)
    return src, sn, tgt, tn, T_true


def translation_error(T, T_true):
    """How far T puts the plane's centre from where T_true puts it."""
    c = np.array([2.0, 2.0, 0.0, 1.0])
    return float(np.linalg.norm((np.asarray(T, dtype=np.float64) - T_true) @ c))


if __name__ == "__main__":
    # python tests/icp_sampling_cases.py: writes tests/golden/icp_sampling_grooved.json, the restated point-to-plane ICP of the
    # full grooved-plane source (20 s of numpy; tests/test_icp_sampling_cpu.py checks the record against a fresh run)
    import json
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_icp_plane import restate_icp_plane
    from test_icp_sampling_cpu import ICP, SEEDS
    src, sn, tgt, tn, T_true = grooved_problem(SEEDS[0])
    T, it, conv, _ = restate_icp_plane(src, tgt, tn, np.eye(4, dtype=np.float32), ICP["max_corr"], ICP["max_iter"], ICP["eps"])
    rec = dict(seed=SEEDS[0], icp=ICP, iterations=int(it), converged=int(conv), T=[[float(v) for v in row] for row in T],
               error_mm=1000.0 * translation_error(T, T_true))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icp_sampling_grooved.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(path, rec["iterations"], rec["error_mm"])

"""Statistical outlier removal (mm3d_set_outlier_filter): the rule of include/mm3d.h restated in numpy, and the small clouds at
which a k-nearest search over a grid can still go wrong.  Shared by test_outliers_statistical_cpu.py, which checks the
restatement, and test_gpu_outliers_statistical.py, which holds the device against it.  Needs no GPU."""
import functools

import numpy as np

from test_gpu_icp_plane import box_room

MEAN_KS = (1, 7, 16, 50, 64)                                  # what the search is compared at
FILTER_PARAMS = ((8, 1.0), (16, 1.0), (16, 2.0), (50, 1.0))   # (mean_k, stddev_mult) the kept set is compared at
MARGIN = 1e-9                                                 # min |d_i - t| / t the kept-set comparisons rest on


# ---------------------------------------------------------------- the restatement
def _d2_rows(p, a, b):
    """d2 of points a .. b - 1 against all of p: ((dx dx + dy dy) + dz dz), every operation one float32 operation."""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = p[a:b, None, 0] - p[None, :, 0]
        dy = p[a:b, None, 1] - p[None, :, 1]
        dz = p[a:b, None, 2] - p[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    return d2


def nearest_d2(p, k, select="sort", chunk=256):
    """[len(p)][k] float32: every point's k smallest d2 to the OTHER points (a duplicate is another point), ascending.  Brute
    force; select = "sort" sorts whole rows, "partition" selects with np.partition first."""
    out = np.empty((len(p), k), dtype=np.float32)
    for a in range(0, len(p), chunk):
        b = min(a + chunk, len(p))
        d2 = _d2_rows(p, a, b)
        rows = np.arange(b - a)
        d2 = np.delete(d2.reshape(-1), rows * len(p) + a + rows).reshape(b - a, len(p) - 1)   # j != i: drop the point itself, only it
        if select == "sort":
            out[a:b] = np.sort(d2, axis=1)[:, :k]
        else:
            out[a:b] = np.sort(np.partition(d2, k - 1, axis=1)[:, :k], axis=1)
    return out


def nearest_d2_tree(p, k):
    """The same through scipy's k-d tree (double distances pick the neighbours, their float32 d2 is recomputed): equal to
    nearest_d2 where no two candidates tie within double rounding at the k-th place."""
    from scipy.spatial import cKDTree
    _, idx = cKDTree(p.astype(np.float64)).query(p.astype(np.float64), k=k + 1)
    idx = idx.reshape(len(p), k + 1)
    out = np.empty((len(p), k), dtype=np.float32)
    for i in range(len(p)):
        nb = idx[i][idx[i] != i][:k] if (idx[i] == i).any() else idx[i][:k]
        d = p[i] - p[nb]
        out[i] = np.sort((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return out


def mean_distances(xyz, mean_k, nearest=nearest_d2, near=None):
    """Step 3: (d [n] float64 with NaN where the rule has none, valid mask, k').  near: the valid points' ascending nearest d2
    when the caller has them already, at least k' columns (the k' smallest are a prefix of any longer row)."""
    x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    valid = np.isfinite(x).all(axis=1)
    d = np.full(len(x), np.nan)
    nv = int(valid.sum())
    if nv <= 1:
        return d, valid, 0
    k = min(int(mean_k), nv - 1)
    if near is None:
        near = nearest(x[valid], k)
    s = np.zeros(nv)
    with np.errstate(invalid="ignore"):
        for j in range(k):                                    # ascending order of d2, one double addition at a time
            s = s + np.sqrt(near[:, j].astype(np.float64))
    d[valid] = s / k
    return d, valid, k


def threshold(d, valid, k, stddev_mult):
    """Steps 4 and 5 on step 3's result: dict(d, keep, valid, k, mean, stddev, threshold, margin)."""
    nv = int(valid.sum())
    if nv <= 1:
        return dict(d=d, keep=valid.copy(), valid=valid, k=0, mean=0.0, stddev=0.0, threshold=0.0, margin=np.inf)
    dv = d[valid]
    with np.errstate(invalid="ignore", over="ignore"):
        S = float(np.cumsum(dv)[-1])                          # (cumsum adds one after the other; np.sum adds pairwise)
        Q = float(np.cumsum(dv * dv)[-1])
        mean = S / nv
        var = max(0.0, (Q - S * S / nv) / (nv - 1))
        std = float(np.sqrt(var))
        t = mean + float(stddev_mult) * std
        keep = valid & (d <= t)
        margin = float(np.min(np.abs(dv - t)) / t) if t > 0 else 0.0
    return dict(d=d, keep=keep, valid=valid, k=k, mean=mean, stddev=std, threshold=t, margin=margin)


def restate(xyz, mean_k, stddev_mult, nearest=nearest_d2):
    """The whole rule."""
    return threshold(*mean_distances(xyz, mean_k, nearest), stddev_mult)


# ---------------------------------------------------------------- the clouds
def room_with_planted(seed, n=4000, planted=150):
    """(a): box_room plus points planted in its free space, at least 0.45 m from every room point; shuffled.  Returns the
    cloud and the mask of the planted points."""
    from scipy.spatial import cKDTree
    room = box_room(seed, n)[0]
    rng = np.random.default_rng(1000 + seed)
    tree = cKDTree(room.astype(np.float64))
    got = np.empty((0, 3), dtype=np.float32)
    while len(got) < planted:
        c = rng.uniform([0.5, 0.5, 0.5], [7.5, 5.5, 2.5], (4 * planted, 3)).astype(np.float32)
        c = c[tree.query(c.astype(np.float64))[0] >= 0.45]
        got = np.concatenate([got, c])[:planted]
    xyz = np.concatenate([room, got])
    is_planted = np.r_[np.zeros(len(room), dtype=bool), np.ones(len(got), dtype=bool)]
    perm = rng.permutation(len(xyz))
    return xyz[perm], is_planted[perm]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (xyz float32 [n][3], compare the kept set?).  Made once, never written to."""
    rng = np.random.default_rng(77)
    out = {}
    for seed in (1, 2, 3):
        out[f"a_room_planted_{seed}"] = (room_with_planted(seed)[0], True)
    # (b) one point 40 m from a room, and one exactly on each corner of the cloud's bounding box
    far = np.concatenate([box_room(4, 2000)[0], np.array([[48.0, 3.0, 1.5]], dtype=np.float32)])
    lo, hi = far.min(axis=0), far.max(axis=0)
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float32)
    out["b_far_point_and_corners"] = (np.concatenate([far, corners]), True)
    # (c) fewer valid points than mean_k + 1, and clouds with rows that are not numbers
    out["c_twenty_points"] = (rng.uniform(0, 2, (20, 3)).astype(np.float32), True)
    out["c_empty"] = (np.empty((0, 3), dtype=np.float32), True)
    out["c_one_point"] = (np.array([[1.0, 2.0, 3.0]], dtype=np.float32), True)
    out["c_two_points"] = (np.array([[1.0, 2.0, 3.0], [1.5, 2.0, 3.0]], dtype=np.float32), True)
    bad = np.full((40, 3), np.nan, dtype=np.float32)
    bad[::3, 0] = np.inf
    bad[1::3] = [1.0, -np.inf, 2.0]
    out["c_no_valid_point"] = (bad, True)
    mixed = np.concatenate([room_with_planted(1)[0], np.full((300, 3), np.nan, dtype=np.float32)])
    mixed[-300::2, 1:] = rng.uniform(0, 5, (150, 2)).astype(np.float32)            # (one NaN coordinate is enough)
    out["c_room_with_nan_rows"] = (mixed[rng.permutation(len(mixed))], True)
    # (d) duplicates: 100 copies of one point inside a room, and a pair of identical points
    room = box_room(5, 2000)[0]
    dup = np.concatenate([room, np.tile(np.array([[4.0, 3.0, 1.5]], dtype=np.float32), (100, 1)), room[[17, 17]]])
    out["d_duplicates"] = (dup[rng.permutation(len(dup))], True)
    # (e) exact ties at the k-th place: an integer lattice (the search alone is compared)
    lat = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    out["e_integer_lattice"] = (lat[rng.permutation(len(lat))], False)
    # (f) 3 000 points within 5 cm, inside one grid cell, beside a sparse room; and a line along x
    spot = (np.array([4.0, 3.0, 1.5]) + rng.uniform(-0.025, 0.025, (3000, 3))).astype(np.float32)
    dense = np.concatenate([box_room(6, 1000)[0], spot])
    out["f_dense_spot"] = (dense[rng.permutation(len(dense))], True)
    line = np.zeros((400, 3), dtype=np.float32)
    line[:, 0] = np.sort(rng.uniform(0, 50, 400)).astype(np.float32)
    line[:, 1], line[:, 2] = 2.0, -1.0
    out["f_line_along_x"] = (line[rng.permutation(len(line))], True)
    # (g) far from the origin: coordinates with 1e-4 m to the ulp
    out["g_translated_room"] = ((room_with_planted(1)[0] + np.array([1000.0, -2000.0, 30.0], dtype=np.float32)).astype(np.float32), True)
    # (h) sizes around a wave and a block
    for n in (63, 64, 65, 255, 256, 257):
        out[f"h_random_{n}"] = (rng.uniform(0, 5, (n, 3)).astype(np.float32), True)
    for xyz, _ in out.values():
        xyz.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference_nearest(name):
    x = cases()[name][0]
    p = x[np.isfinite(x).all(axis=1)]
    return nearest_d2(p, min(max(MEAN_KS), len(p) - 1)) if len(p) > 1 else None


@functools.lru_cache(maxsize=None)
def reference_distances(name, mean_k):
    """mean_distances of a case: one brute-force search per case, shared by every mean_k and every test, never written to."""
    d, valid, k = mean_distances(cases()[name][0], mean_k, near=_reference_nearest(name))
    d.setflags(write=False)
    return d, valid, k


@functools.lru_cache(maxsize=None)
def reference_filter(name, mean_k, stddev_mult):
    return threshold(*reference_distances(name, mean_k), stddev_mult)


def first_point_per_voxel(xyz, leaf=0.1):
    """The stand-in for the voxel filter on the CPU: the first point of every occupied voxel, in input order."""
    v = np.floor(np.asarray(xyz, dtype=np.float32) * (np.float32(1.0) / np.float32(leaf))).astype(np.int64)
    _, first = np.unique(v, axis=0, return_index=True)
    return np.asarray(xyz, dtype=np.float32)[np.sort(first)]


def radius_rule_keeps(xyz, radius, min_neighbours):
    """The share the reference's radius filter keeps: points with at least min_neighbours others within the radius."""
    from scipy.spatial import cKDTree
    tree = cKDTree(xyz.astype(np.float64))
    cnt = np.array([len(v) - 1 for v in tree.query_ball_point(xyz.astype(np.float64), radius)])
    return float((cnt >= min_neighbours).mean())

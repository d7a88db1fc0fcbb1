"""Euclidean clustering (mm3d_set_cluster_filter): the rule of include/mm3d.h restated in numpy, and the small clouds at which a
union-find over a grid can still go wrong.  Shared by test_cluster_filter_cpu.py, which checks the restatement, and
test_gpu_cluster_filter.py, which holds the device against it.  Needs no GPU and nothing beyond numpy.

Every case has at most 6 000 points: the restatement is brute force, n^2 float32 distances."""
import functools

import numpy as np

OFF, MIN_SIZE, LARGEST = 0, 1, 2
TOL = 0.2                       # the tolerance of every case but the threshold one: twice the library's default resolution
SIZES_MIN = 20                  # the min_size the "sizes" case is built around


# ---------------------------------------------------------------- the restatement
def adjacency(xyz, tolerance, chunk=512):
    """(adj bool [n][n], valid bool [n]): rule 1 and 2.  d2 = (dx dx + dy dy) + dz dz, every operation one float32 operation
    (numpy rounds each elementwise operation), compared in float64 with tolerance * tolerance formed in float64."""
    x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = len(x)
    valid = np.isfinite(x).all(axis=1)
    t2 = float(tolerance) * float(tolerance)
    adj = np.zeros((n, n), dtype=bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, n, chunk):
            b = min(a + chunk, n)
            dx = x[a:b, None, 0] - x[None, :, 0]
            dy = x[a:b, None, 1] - x[None, :, 1]
            dz = x[a:b, None, 2] - x[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            adj[a:b] = d2.astype(np.float64) <= t2
    adj &= valid[:, None] & valid[None, :]
    adj[np.arange(n), np.arange(n)] = False
    return adj, valid


def labels_union_find(adj, valid):
    """Rule 3 by union-find in its quick-find form: labels[i] is always i's root, and a union renames the set of the larger
    root to the smaller.  The root of a set is its smallest member by construction."""
    n = len(valid)
    labels = np.where(valid, np.arange(n), -1).astype(np.int64)
    for i in range(n):
        if not valid[i]:
            continue
        js = np.nonzero(adj[i, i + 1:])[0]
        if len(js) == 0:
            continue
        roots = np.unique(np.append(labels[js + i + 1], labels[i]))
        for r in roots[1:]:
            labels[labels == r] = roots[0]
    return labels


def labels_min_propagation(adj, valid, chunk=512):
    """Rule 3 another way, in rounds: every point takes the smallest label among itself and its neighbours and hands it to the
    point its old label names as well (so a whole tree moves, not one point); then labels of labels are followed to their end.
    Until nothing changes.  Returns (labels, rounds)."""
    n = len(valid)
    big = np.int64(n)
    labels = np.where(valid, np.arange(n), big).astype(np.int64)
    rounds = 0
    idx = np.nonzero(valid)[0]
    while True:
        m = labels.copy()
        for a in range(0, n, chunk):
            b = min(a + chunk, n)
            m[a:b] = np.minimum(labels[a:b], np.where(adj[a:b], labels[None, :], big).min(axis=1, initial=big))
        new = m.copy()
        np.minimum.at(new, labels[idx], m[idx])
        while True:                                           # pointer jumping (a label is a valid point's index)
            nxt = np.where(new < big, new[np.minimum(new, n - 1)], big) if n else new
            if np.array_equal(nxt, new):
                break
            new = nxt
        rounds += 1
        if np.array_equal(new, labels):
            break
        labels = new
    return np.where(valid, labels, -1), rounds


def stats_of(labels, kept, kept_clusters):
    lab = labels[labels >= 0]
    sizes = np.bincount(lab, minlength=1) if len(lab) else np.zeros(1, dtype=np.int64)
    return dict(points=len(labels), valid=len(lab), kept=int(kept), clusters=int((sizes > 0).sum()) if len(lab) else 0,
                kept_clusters=int(kept_clusters), largest=int(sizes.max()) if len(lab) else 0)


def keep_mask(labels, method, min_size):
    """Rule 4: (keep bool [n], number of clusters kept)."""
    n = len(labels)
    keep = np.zeros(n, dtype=bool)
    lab = labels[labels >= 0]
    if len(lab) == 0:
        return keep, 0
    sizes = np.bincount(lab, minlength=n)
    if method == MIN_SIZE:
        keep[labels >= 0] = sizes[lab] >= min_size
        return keep, int((sizes >= min_size).sum()) if min_size >= 1 else 0
    best = int(np.argmax(sizes))                              # (argmax takes the first of equals: the smallest label)
    keep = labels == best
    return keep, 1


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(labels int32 [n], valid, stats) of a case: computed once, never written to."""
    xyz, tol = cases()[name]
    adj, valid = adjacency(xyz, tol)
    labels = labels_union_find(adj, valid)
    return dict(labels=labels.astype(np.int32), valid=valid, stats=stats_of(labels, int(valid.sum()), len(np.unique(labels[labels >= 0]))))


def reference_filter(name, method, min_size):
    labels = reference(name)["labels"]
    keep, kc = keep_mask(labels, method, min_size)
    return keep, stats_of(labels, int(keep.sum()), kc)


def partition(labels):
    """The clusters as a set of frozensets of record numbers (the invalid records apart)."""
    out = {}
    for i, l in enumerate(labels):
        if l >= 0:
            out.setdefault(int(l), []).append(i)
    return {frozenset(v) for v in out.values()}


# ---------------------------------------------------------------- the clouds
def chain():
    """3 000 points along a helix, 0.9 tolerances apart along the curve, the turns 3.5 tolerances apart, shuffled: one cluster,
    label 0, through hundreds of cells -- the longest path a cloud of this size can have."""
    n, R, pitch = 3000, 5.0, 3.5 * TOL
    b = pitch / (2.0 * np.pi)
    theta = np.arange(n) * (0.9 * TOL / np.hypot(R, b))
    xyz = np.stack([R * np.cos(theta), R * np.sin(theta), b * theta], axis=1).astype(np.float32)
    return xyz[np.random.default_rng(5).permutation(n)]


def _exact_diagonal():
    """Two floats near 0.3 and 0.4 whose float32 d2 is 0.25 exactly while a^2 + b^2 in exact arithmetic is above it: adjacent
    under the rule, not adjacent for anything that sums in double.  (Lattice values cannot do this: a^2 + b^2 = c^2 has no
    solution in dyadic rationals with c a power of two but the trivial one.)"""
    for ka in range(0, 64):
        for kb in range(0, 64):
            a = np.float32(0.3)
            b = np.float32(0.4)
            for _ in range(ka):
                a = np.nextafter(a, np.float32(1))
            for _ in range(kb):
                b = np.nextafter(b, np.float32(1))
            if np.float32(a * a) + np.float32(b * b) == np.float32(0.25) and float(a) * float(a) + float(b) * float(b) > 0.25:
                return a, b
    raise AssertionError("no such pair")


THRESHOLD_TOL = 0.5
# what test_cluster_filter_cpu.py expects of threshold(): pairs 0 - 7 and 16 - 18 are adjacent (one label per pair, the first
# record's), pairs 8 - 15 are not
THRESHOLD_LABELS = [0, 0, 2, 2, 4, 4, 6, 6, 8, 8, 10, 10, 12, 12, 14, 14,
                    16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31,
                    32, 32, 34, 34, 36, 36]


def threshold():
    """Tolerance 0.5, coordinates multiples of 2^-6, so every d2 is exact.  Records come in pairs (2 k, 2 k + 1):
    pairs 0 - 7 exactly 0.5 apart along x (adjacent), pairs 8 - 15 0.5 + 2^-6 apart (not adjacent), each family at eight
    offsets so that some pairs lie on opposite sides of a cell border whatever the cell is near 0.5; pair 16 is 0.5 apart along
    y, pair 17 along z, pair 18 is the diagonal of _exact_diagonal()."""
    u = 2.0 ** -6
    pts = []
    for j in range(8):
        x0 = 3.0 * j + 5 * j * u
        pts += [(x0, 0.0, 0.0), (x0 + 0.5, 0.0, 0.0)]
    for j in range(8):
        x0 = 3.0 * j + 7 * j * u
        pts += [(x0, 4.0, 0.0), (x0 + 0.5 + u, 4.0, 0.0)]
    pts += [(1.0, 8.0, 0.0), (1.0, 8.5, 0.0), (5.0, 8.0, 1.0), (5.0, 8.0, 1.5)]
    a, b = _exact_diagonal()                                  # (stored as they are: the pair starts at the origin of x and z)
    pts += [(0.0, 12.0, 0.0), (float(a), 12.0, float(b))]
    return np.array(pts, dtype=np.float32)


SIZES_BLOBS = (30, SIZES_MIN - 1, SIZES_MIN, SIZES_MIN + 1, 30, 1, 1, 1, 1, 1)


def sizes():
    """Blobs of 30, 19, 20, 21 and 30 points and five single points, tens of metres apart, every blob inside a ball of half a
    tolerance.  Records go round the blobs in turn, so blob b's first record is record b: its label.  Returns (xyz, blob of
    each record)."""
    rng = np.random.default_rng(9)
    centres = np.array([[40.0 * (b % 4), 35.0 * (b // 4), 3.0 * b] for b in range(len(SIZES_BLOBS))])
    members = []
    for b, m in enumerate(SIZES_BLOBS):
        d = rng.normal(size=(m, 3))
        d *= (0.45 * TOL * rng.uniform(0, 1, (m, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
        members.append(centres[b] + d)
    xyz, blob = [], []
    for r in range(max(SIZES_BLOBS)):
        for b, m in enumerate(SIZES_BLOBS):
            if r < m:
                xyz.append(members[b][r])
                blob.append(b)
    return np.array(xyz, dtype=np.float32), np.array(blob)


def dense_blob():
    """5 000 points inside a ball of radius tolerance / 2: one cell, all mutually adjacent, every hook on one root."""
    rng = np.random.default_rng(11)
    d = rng.normal(size=(5000, 3))
    d *= (0.49 * TOL * rng.uniform(0, 1, (5000, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
    return (np.array([3.0, -2.0, 1.0]) + d).astype(np.float32)


def random_cloud(seed, offset=0.0, n=4000):
    """Uniform points with 2.7 neighbours within the tolerance on average, near the percolation threshold of overlapping balls:
    many clusters of many sizes.  offset moves the cloud along x and y; the coordinates are rounded to float32 here, before
    anything looks at them."""
    side = (n * 4.0 / 3.0 * np.pi * TOL ** 3 / 2.7) ** (1.0 / 3.0)
    xyz = np.random.default_rng(seed).uniform(0.0, side, (n, 3))
    xyz[:, :2] += offset
    return xyz.astype(np.float32)


def invalid_and_duplicates():
    """300 points with NaN, +inf and -inf in each coordinate, the first and the last record among them, and exact duplicates."""
    rng = np.random.default_rng(13)
    xyz = rng.uniform(0.0, 1.6, (300, 3)).astype(np.float32)
    xyz[200:230] = xyz[10:40]                                 # duplicates, some of them three times
    xyz[230:240] = xyz[10:20]
    bad = [np.nan, np.inf, -np.inf]
    rows = [0, 299, 17, 18, 19, 101, 150, 151, 250]
    for k, r in enumerate(rows):
        xyz[r, k % 3] = bad[(k // 3) % 3]
    xyz[77] = (np.nan, np.inf, -np.inf)
    return xyz


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (xyz float32 [n][3], tolerance).  Made once, never written to."""
    out = {
        "a_chain": (chain(), TOL),
        "b_threshold": (threshold(), THRESHOLD_TOL),
        "c_sizes": (sizes()[0], TOL),
        "d_dense_blob": (dense_blob(), TOL),
        "e_invalid_and_duplicates": (invalid_and_duplicates(), TOL),
        "f_all_invalid": (np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3, [np.inf] * 3], dtype=np.float32), TOL),
        "g_empty": (np.empty((0, 3), dtype=np.float32), TOL),
        "h_one_point": (np.array([[1.0, 2.0, 3.0]], dtype=np.float32), TOL),
        "i_random_1": (random_cloud(1), TOL),
        "j_random_2": (random_cloud(2), TOL),
        "k_random_at_1km": (random_cloud(3, 1000.0), TOL),
        "l_random_at_10km": (random_cloud(4, 10000.0), TOL),
    }
    for xyz, _ in out.values():
        assert xyz.dtype == np.float32 and len(xyz) <= 6000
        xyz.setflags(write=False)
    return out


# ---------------------------------------------------------------- the room the wiring tests run through
ROOM_MIN_SIZE = 1000
BLOB_RADIUS = 0.38              # a ball of about 300 voxels of 0.1 m


def _plane(o, u, v, nu, nv, rng, pitch=0.05):
    """Points on the lattice o + (i + 1/2) pitch u + (j + 1/2) pitch v, jittered by a centimetre: four in every 0.1 m voxel the
    plane passes, when o, u, v follow the voxel lattice."""
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    p = np.asarray(o)[None, :] + ((i.reshape(-1, 1) + 0.5) * pitch) * np.asarray(u)[None, :] + ((j.reshape(-1, 1) + 0.5) * pitch) * np.asarray(v)[None, :]
    return p + rng.uniform(-0.01, 0.01, p.shape)


def room_with_blobs(seed, yaw=0.0, shift=(0.0, 0.0, 0.0)):
    """A room of 8 x 6 x 3 m without a ceiling -- the floor, four walls, one of them split in two by an opening of full height,
    and a free-standing wall of 4.4 x 3 m a metre outside (1 320 voxels: structure of its own, above ROOM_MIN_SIZE) -- sampled
    four points to the 0.1 m voxel, with three solid balls of radius 0.38 m (about 300 voxels each, eight points to the voxel)
    in its free space, at places that depend on the seed.  Textured by map_merge_amd.synth, so that the detectors find keypoints.
    Returns (xyz float32, rgb uint8, is_blob, blob boxes [(lo, hi)] in the returned frame's axes when yaw == 0)."""
    from map_merge_amd import synth
    rng = np.random.default_rng(100 + seed)
    e = 0.03                                                  # the surfaces lie 3 cm inside their voxels
    X, Y, Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    parts = [_plane((0, 0, e), X, Y, 160, 120, rng),                                  # floor
             _plane((e, 0, 0), Y, Z, 120, 60, rng), _plane((8 - e, 0, 0), Y, Z, 120, 60, rng),      # the walls x = 0 and x = 8
             _plane((0, 6 - e, 0), X, Z, 160, 60, rng),                                # the wall y = 6
             _plane((0, e, 0), X, Z, 60, 60, rng), _plane((4.2, e, 0), X, Z, 76, 60, rng),          # the wall y = 0, open from x = 3 to 4.2
             _plane((1.8, -1.0 + e, 0), X, Z, 88, 60, rng)]                            # the free-standing wall
    room = np.concatenate(parts)
    centres = np.array([[2.0, 2.0, 1.3], [5.5, 3.5, 1.5], [3.0, 4.6, 1.2]]) + rng.uniform(-0.3, 0.3, (3, 3))
    g = (np.arange(-9, 10) + 0.5) * 0.05
    ball = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    ball = ball[np.linalg.norm(ball, axis=1) <= BLOB_RADIUS]
    blobs = [np.floor(c / 0.1) * 0.1 + ball + rng.uniform(-0.01, 0.01, ball.shape) for c in centres]
    xyz = np.concatenate([room] + blobs)
    is_blob = np.r_[np.zeros(len(room), dtype=bool), np.ones(sum(len(b) for b in blobs), dtype=bool)]
    boxes = [(b.min(axis=0) - 0.05, b.max(axis=0) + 0.05) for b in blobs]
    rgb = synth._texture(xyz, np.array([150.0, 140.0, 120.0]), 40 + seed)
    c, s = np.cos(yaw), np.sin(yaw)
    xyz = xyz @ np.array([[c, s, 0], [-s, c, 0], [0, 0, 1.0]]) + np.asarray(shift)[None, :]
    perm = rng.permutation(len(xyz))
    return xyz[perm].astype(np.float32), rgb[perm], is_blob[perm], boxes

"""Inputs for the second launch of the four kernels that keep a keypoint's neighbour list in LDS up to a fixed capacity and hand a
larger neighbourhood to the same kernel with the list in global scratch: k_pfh (PFH and PFHRGB, 1024), k_shot (1024), k_sc3d (1024)
and k_harris_refine (2048).  A plain module: tests/test_overflow_cases_cpu.py shows on the CPU that the inputs hold what they
claim, tests/test_gpu_feature_scratch.py runs the device on them.

The blob cloud (the true capacities): nine blobs of exactly 40, 1023, 1024, 1025, 1500, 2047, 2048, 2049 and 2300 points, each
uniform in a ball of radius 0.45 R around its centre (R = 0.8, the search radius), the centres 4 R apart, and 300 sparse points
further than 1.6 R from every centre (so further than R from every blob point); shuffled, seeded.  That is 13 356 points.  Ten
points of the 1025 blob and ten of the 2049 blob are stored twice, inside the stated sizes, so that (d2, index) ties reach the
scratch sorts.  Normals: seeded unit normals, every 17th all-NaN.
Descriptor keypoints: each blob's centre (its neighbour count is the blob's size, and every d2 is below 0.21 R^2: nothing sits
near the d2 < R^2 boundary), one keypoint 400 m away, one with a NaN coordinate and twelve of the sparse points, interleaved so
that overflowing, fitting and pruned rows alternate.
Harris: a blob's diameter is below R, so every point of a blob has its whole blob as neighbours, and so has every position
inside the blob's ball; a corner found in the 2049 or 2300 blob overflows 2048, one in the 2047 or 2048 blob does not.  Five
corners are found in the two large blobs, and three more, found elsewhere, move into one of them while they are refined: the
replay of the refinement below counts what every search of every corner sees.

The scene case (the hook mm3d_debug_feature_lds_cap at 64, 128, 256): both maps of the two-map synth scene of
tests/test_gpu_parity.py at 6000 raw points, the oracle's filtered cloud and normals, each map's first 200 SIFT keypoints (the
maps have 160 and 129) plus a far and a non-finite one, radius 0.8: neighbourhoods from tens to 202 points, so 256 sends
nothing to scratch there.  The Harris corners (threshold 0, radius 0.8) move while they are refined: some fit a capacity at
their first search and exceed it at a later one.

The brute force forms d2 as the kernels do (device_util.hpp::dist2: float32, (dx dx + dy dy) + dz dz) and compares d2 < r2 with
r2 = float(radius * radius); every kernel sends a neighbourhood to scratch when its count m > cap (strictly)."""
import numpy as np

import feature_cases as fc

F = np.float32
POINT, NORMAL = fc.POINT, fc.NORMAL
R = 0.8
BLOB_SIZES = (40, 1023, 1024, 1025, 1500, 2047, 2048, 2049, 2300)
BLOB_RADIUS = 0.45 * R
BLOB_PITCH = 4 * R
DUPLICATED = {1025: 10, 2049: 10}                 # blob size -> points stored twice (inside the size)
N_SPARSE, SPARSE_CLEARANCE = 300, 1.6 * R
N_SPARSE_KEYPOINTS = 12
ORIGIN = np.array([20.0, -10.0, 5.0])
SEED = 7
HARRIS_THRESHOLD = 0.0
RES = 0.1

# compile-time capacities and the host's rule for the scratch pass's entries per row, given the largest overflowing count
LDS_CAP = {"pfh": 1024, "shot": 1024, "sc3d": 1024, "harris": 2048}
FAMILY = {"pfh": 0, "pfhrgb": 0, "shot": 1, "sc3d": 2, "harris": 3}      # position in mm3d_debug_feature_overflow's pairs
HOOK_CAPS = (64, 128, 256)
N_SCENE_RAW, N_SCENE_KEYPOINTS, R_SCENE_NRM, SCENE_MIN_NB = 6000, 200, 0.6, 50


def pow2_from(start, least):
    cap = start
    while cap < least:
        cap <<= 1
    return cap


def scratch_cap(family, max_m):
    """pfh.hip: max_m itself; shot.hip, sc3d.hip: the power of two from 1024 that holds it; harris.hip: from 2048, twice it."""
    if family == "pfh":
        return max_m
    if family == "harris":
        return pow2_from(LDS_CAP["harris"], 2 * max_m)
    return pow2_from(LDS_CAP[family], max_m)


def first_cap(family, hook):
    """The capacity the first launch is given: the hook's value where it is below the kernel's own."""
    return hook if 0 < hook < LDS_CAP[family] else LDS_CAP[family]


def xyz(a):
    return np.stack([a["x"], a["y"], a["z"]], axis=1).reshape(-1, 3)


def _points(p, rgba):
    out = np.zeros(len(p), dtype=POINT)
    p = np.asarray(p, F).reshape(-1, 3)
    out["x"], out["y"], out["z"], out["rgba"] = p[:, 0], p[:, 1], p[:, 2], rgba
    return out


def random_normals(rng, n):
    v = rng.normal(0, 1, (n, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    out = np.zeros(n, dtype=NORMAL)
    out["nx"], out["ny"], out["nz"] = v[:, 0], v[:, 1], v[:, 2]
    for f in NORMAL.names:
        out[f][::17] = np.nan
    return out


def neighbour_counts(q, p, radius):
    """Per row of q (m, 3): the number of rows of p with float32 d2 < float32(radius^2); a non-finite q has none."""
    r2 = F(radius * radius)
    out = np.zeros(len(q), np.int64)
    for i in range(0, len(q), 64):
        with np.errstate(invalid="ignore"):
            out[i:i + 64] = (fc.d2_matrix(q[i:i + 64], p) < r2).sum(axis=1)
    return out


def expected_overflow(counts, family, hook=0):
    """(rows sent to scratch, entries per row of the scratch pass) for a descriptor family from its keypoints' counts."""
    cap = first_cap(family, hook)
    over = counts[counts > cap]
    return (len(over), scratch_cap(family, int(over.max()))) if len(over) else (0, 0)


class BlobCloud:
    def __init__(self, seed=SEED):
        rng = np.random.default_rng(seed)
        self.centres = np.array([[BLOB_PITCH * (b % 3), BLOB_PITCH * (b // 3), 0.0] for b in range(len(BLOB_SIZES))]) + ORIGIN
        pts, label = [], []
        for b, size in enumerate(BLOB_SIZES):
            dup = DUPLICATED.get(size, 0)
            v = rng.normal(0, 1, (size - dup, 3))
            v *= (BLOB_RADIUS * 0.98 * rng.uniform(0, 1, (size - dup, 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
            p = (v + self.centres[b]).astype(F)
            pts.append(np.concatenate([p, p[:dup]]))
            label += [b] * size
        lo, hi = self.centres.min(axis=0) - [2 * R, 2 * R, R], self.centres.max(axis=0) + [2 * R, 2 * R, R]
        sparse = np.zeros((0, 3))
        while len(sparse) < N_SPARSE:
            c = rng.uniform(lo, hi, (4 * N_SPARSE, 3))
            c = c[(np.linalg.norm(c[:, None, :] - self.centres[None], axis=2) > SPARSE_CLEARANCE).all(axis=1)]
            sparse = np.concatenate([sparse, c])[:N_SPARSE]
        pts.append(sparse.astype(F))
        label += [-1] * N_SPARSE
        pts, label = np.concatenate(pts), np.array(label)
        order = rng.permutation(len(pts))
        pts, self.label = pts[order], label[order]
        self.cloud = _points(pts, 0xFF000000 | rng.integers(0, 1 << 24, len(pts)).astype(np.uint32))
        self.normals = random_normals(rng, len(pts))
        # keypoints: centres, far, non-finite and sparse points, interleaved
        centres = _points(self.centres, 0xFF000000 | rng.integers(0, 1 << 24, len(BLOB_SIZES)).astype(np.uint32))
        sparse_kp = self.cloud[np.flatnonzero(self.label < 0)[:N_SPARSE_KEYPOINTS]]
        far = sparse_kp[:1].copy()
        far["x"] += F(400.0)
        nan = sparse_kp[1:2].copy()
        nan["y"] = np.nan
        rows, kinds = [], []                       # kind: blob size, 0 far, -1 non-finite, -2 sparse
        blob_order = [3, 0, 8, 2, 6, 1, 7, 4, 5]   # 1025, 40, 2300, 1024, 2048, 1023, 2049, 1500, 2047
        extra = [(far[0], 0), (nan[0], -1)] + [(s, -2) for s in sparse_kp]
        for i, b in enumerate(blob_order):
            rows.append(centres[b]); kinds.append(BLOB_SIZES[b])
            for e in extra[i::len(blob_order)]:
                rows.append(e[0]); kinds.append(e[1])
        self.keypoints, self.kinds = np.array(rows, dtype=POINT), np.array(kinds)
        assert len(self.keypoints) == len(BLOB_SIZES) + 2 + N_SPARSE_KEYPOINTS

    def counts(self):
        return neighbour_counts(xyz(self.keypoints), xyz(self.cloud), R)


# ------------------------------------------------------------------------------------------------ the Harris refinement, replayed
def harris_replay(cloud, normals, kept, radius):
    """refineCorners (oracle/o_harris.c::refine_corner, k_harris_refine) in float32, sum by sum: per corner the neighbour count of
    every search it makes, and the refined positions (n, 3).  tests/test_overflow_cases_cpu.py holds the positions against the
    oracle's bit for bit, which is what makes the counts the ones both sides see."""
    p = xyz(cloud).astype(F)
    nrm = np.stack([normals["nx"], normals["ny"], normals["nz"]], axis=1).astype(F)
    r2 = F(np.float64(F(radius)) * np.float64(F(radius)))                          # setRadius(float(radius))
    chain = lambda t: np.add.accumulate(t, dtype=F)[-1] if len(t) else F(0)      # noqa: E731   a sequential float32 sum
    counts, out = [], np.zeros((len(kept), 3), F)
    for n, i in enumerate(kept):
        c = p[i].copy()
        seen, iterations = [], 0
        while True:
            d2 = fc.d2_matrix(c[None], p)[0]
            idx = np.flatnonzero(d2 < r2)
            seen.append(len(idx))
            idx = idx[np.lexsort((idx, d2[idx]))]
            idx = idx[np.isfinite(nrm[idx, 0])]
            nn, pp = nrm[idx], p[idx]
            N = np.zeros((3, 3), F)
            Np = np.zeros(3, F)
            for r in range(3):
                t = [nn[:, r] * nn[:, q] for q in range(3)]
                for q in range(3):
                    N[r, q] = chain(t[q])
                Np[r] = chain((t[0] * pp[:, 0] + t[1] * pp[:, 1]) + t[2] * pp[:, 2])
            a, bb, cc, d, e, f = N[0, 0], N[0, 1], N[0, 2], N[1, 1], N[1, 2], N[2, 2]
            fd_ee, ce_bf, be_cd = d * f - e * e, cc * e - bb * f, bb * e - cc * d
            det = (a * fd_ee + bb * ce_bf) + cc * be_cd
            old = c.copy()
            if det != 0:
                inv = np.array([[fd_ee, ce_bf, be_cd], [ce_bf, a * f - cc * cc, bb * cc - a * e], [be_cd, bb * cc - a * e, a * d - bb * bb]], F) / det
                c = np.array([(inv[r, 0] * Np[0] + inv[r, 1] * Np[1]) + inv[r, 2] * Np[2] for r in range(3)], F)
            dx = c - old
            diff = (dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2]
            iterations += 1
            if not (float(diff) > 1e-6 and iterations < 10):
                break
        counts.append(np.array(seen))
        out[n] = c
    return counts, out


def harris_expected_overflow(counts, hook=0):
    """(corners sent to scratch, entries per row): a corner leaves at its FIRST search with more than cap neighbours, and the
    host sizes the scratch pass by the largest such count."""
    cap = first_cap("harris", hook)
    first = [int(s[s > cap][0]) for s in counts if (s > cap).any()]
    return (len(first), scratch_cap("harris", max(first))) if first else (0, 0)


# ------------------------------------------------------------------------------------------------------------------ references
_CACHE = {}


def blob_reference(po):
    """The blob cloud with the oracle's results on it, once per process: dict name -> (kept keypoints, rows), "shot_frames",
    "harris" -> (corners xyz, kept indices), "harris_counts" -> the replay's counts."""
    if "blob" not in _CACHE:
        b = BlobCloud()
        ref = {}
        for name, fn in (("pfh", po.descriptors_pfh), ("pfhrgb", po.descriptors_pfhrgb), ("shot", po.descriptors_shot), ("sc3d", po.descriptors_sc3d)):
            ref[name] = fn(b.cloud, b.normals, b.keypoints, R)
        raw, rf = po.shot_raw(b.cloud, b.normals, b.keypoints, R)
        ref["shot_frames"] = rf[np.isfinite(raw).all(axis=1)]
        kp, idx, _ = po.keypoints_harris(b.cloud, b.normals, HARRIS_THRESHOLD, R)
        ref["harris"] = (xyz(kp), idx)
        ref["harris_counts"], ref["harris_replayed"] = harris_replay(b.cloud, b.normals, idx, R)
        _CACHE["blob"] = (b, ref)
    return _CACHE["blob"]


class SceneMap:
    """One map of the scene: cloud, normals, keypoints, their neighbour counts, and the Harris corners' counts."""

    def __init__(self, po, raw):
        self.cloud = po.remove_outliers(po.downsample(raw, RES), R, SCENE_MIN_NB)
        self.normals = po.normals(self.cloud, R_SCENE_NRM)
        kp = po.keypoints_sift(self.cloud, RES, 3, 3, 5.0)[0][:N_SCENE_KEYPOINTS].copy()
        assert len(kp) >= 125, len(kp)
        far, nan = kp[5:6].copy(), kp[6:7].copy()
        far["x"] += F(400.0)
        nan["z"] = np.nan
        self.keypoints = np.concatenate([kp[:3], far, kp[3:120], nan, kp[120:]])
        self.counts = neighbour_counts(xyz(self.keypoints), xyz(self.cloud), R)
        kp, self.harris_kept, _ = po.keypoints_harris(self.cloud, self.normals, HARRIS_THRESHOLD, R)
        self.harris = xyz(kp)
        self.harris_counts, self.harris_replayed = harris_replay(self.cloud, self.normals, self.harris_kept, R)


def scene_reference(po, synth):
    """[SceneMap] for the two maps, once per process."""
    if "scene" not in _CACHE:
        world, maps = synth.synth_maps(2, N_SCENE_RAW, overlap_step=0.35)
        _CACHE["scene"] = [SceneMap(po, synth.pack_points(x, c)) for x, c, _ in maps]
    return _CACHE["scene"]

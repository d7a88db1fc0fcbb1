"""Inputs on which neighbour distances tie exactly, for the feature kernels that rebuild radiusSearch's (d2, index) order with a
sorter of their own: normals and the Harris response (snb_lds.hpp), k_harris_refine, shot.hip and sc3d.hip (bitonic sorts),
pfh.hip (the (d2, idx) role rule) and rsd.hip (the packed min key).  A plain module: tests/test_feature_cases_cpu.py shows on the
CPU that every case holds the ties it claims and that a wrong tie order is visible through compare(); tests/test_gpu_feature_ties.py
compares the device with the oracle through the same compare().

The clouds: a dyadic lattice of pitch H = 1/8 -- a 24 x 24 plane, an 8^3 cube, three 12 x 12 faces meeting at a box corner --
shuffled, with its first 30 points stored twice (d2 = 0 between distinct indices), three isolated clusters of 1, 2 and 3 points 5 m
away, and the whole carried by OFFSET, whose components are multiples of 2^-10 below 128: every coordinate is exact in float32 and
has 15 to 17 significant bits, every coordinate difference and so every d2 is exact (ties are exact, d2 == r^2 occurs exactly at
3 H = R_NRM and 4 H = R_DESC), while the raw moment sums of the normals round and so depend on the order of tied neighbours.
Points also lie exactly on the faces of the search grid's cells (r / 2).

Normal sets: "oracle" = po.normals(cloud, R_NRM) (NaN at the clusters of 1 and 2 points), "random" = seeded unit normals with
every 17th all-NaN (order-dependent payload sums, every kernel's non-finite-normal branch), and on the plane "flat" = the oracle's
normals of the same plane BEFORE the translation: exactly (0, 0, 1) (z = 0 makes four raw moments exact zeros), so every Harris
response is 0.0f, every point is a corner and every refinement matrix diag(0, 0, n) is singular.  ("oracle" does not give that:
with 17-bit coordinates the raw moments round, and only a tenth of the plane's normals come out exactly -z; its responses still
take no more than a dozen distinct values, so equal responses among neighbours abound there too.)  "flat" goes through the Harris
stages only.
Keypoint sets: "on" = 40 cloud points, both copies of three duplicated points among them; "off" = 150 points at p + (H/2, H/2, 0),
equidistant from 2 - 8 lattice points, so that "the nearest neighbour" is decided by index ("on" is also what puts neighbours at
exactly d2 == r2 into the per-keypoint kernels: nothing lies 4 H from a point half a pitch off the lattice).  Each set also holds one keypoint 400 m
away (no neighbour) and three with exactly 1, 2 and 3 neighbours (at the clusters), spread over the set."""
import numpy as np

F = np.float32
H = 0.125
R_NRM, R_DESC = 0.375, 0.5                     # 3 H and 4 H: both squares are floats
OFFSET = np.array([100 + 37 * 2.0 ** -10, -60 + 5 * 2.0 ** -10, 20 + 11 * 2.0 ** -10])
N_DUP = 30
POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")])
NORMAL = np.dtype([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("curvature", "<f4")])
PFH, PFHRGB, FPFH, RSD, SHOT, SC3D = range(6)
DESCRIPTORS = {"pfh": PFH, "pfhrgb": PFHRGB, "fpfh": FPFH, "rsd": RSD, "shot": SHOT, "sc3d": SC3D}
NORMAL_SETS = ("oracle", "random")
KEYPOINT_SETS = ("on", "off")
CLOUDS = ("plane", "cube", "corner")
PREFIXES = (1, 4, 5, 63, 64, 65)                # keypoint counts across wave (one keypoint each) and block (k_rsd: four) edges

# lattice coordinates (units of H) of the isolated clusters, 5 m (40 H) off the lattice and 2 m from each other; and the order in which
# their six points are stored (not sorted by any coordinate)
_C1, _C2, _C3 = np.array([-40, 0, 0]), np.array([-40, 16, 0]), np.array([-40, 32, 0])
_CLUSTER_POINTS = np.array([_C3 + [1, 0, 0], _C1, _C2 + [1, 0, 0], _C3, _C2, _C3 + [0, 1, 0]])
_CLUSTER_HOMES = (_C1, _C2, _C3)                # a keypoint at home has 1, 2, 3 neighbours; so has home + (1/2, 1/2, 0)


def _lattice(name):
    if name == "plane":
        i, j = np.meshgrid(np.arange(24), np.arange(24), indexing="ij")
        return np.stack([i.ravel(), j.ravel(), np.zeros(i.size, int)], axis=1)
    if name == "cube":
        return np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3)
    if name == "corner":
        a, b = np.meshgrid(np.arange(12), np.arange(12), indexing="ij")
        a, b, o = a.ravel(), b.ravel(), np.zeros(a.size, int)
        faces = np.concatenate([np.stack([a, b, o], 1), np.stack([a, o, b], 1), np.stack([o, a, b], 1)])
        return np.unique(faces, axis=0)                                    # the shared edges once
    raise KeyError(name)


def _records(k, rgba, offset=OFFSET):
    """Lattice coordinates (units of H, halves allowed) -> POINT records at k H + offset; the translation must be exact."""
    exact = np.asarray(k, np.float64) * H + offset                         # exact in double: multiples of 2^-10 below 2^9
    got = (np.asarray(k, np.float64) * H).astype(F) + np.asarray(offset).astype(F)      # the float32 sum itself
    assert got.dtype == F and (got.astype(np.float64) == exact).all(), "the dyadic translation is not exact in float32"
    out = np.zeros(len(exact), dtype=POINT)
    out["x"], out["y"], out["z"], out["rgba"] = got[:, 0], got[:, 1], got[:, 2], rgba
    return out


def _spread(rows, specials, positions):
    """rows with specials[i] inserted so that it ends up at positions[i]."""
    rows = list(rows)
    for s, p in sorted(zip(specials, positions), key=lambda t: t[1]):
        rows.insert(p, s)
    return rows


class Case:
    """One cloud with its two keypoint sets; normals and oracle results are added by reference()."""

    def __init__(self, name, seed):
        rng = np.random.default_rng(seed)
        lat = _lattice(name)
        lat = lat[rng.permutation(len(lat))]
        self.name, self.n_lat = name, len(lat)
        k = np.concatenate([lat, lat[:N_DUP], _CLUSTER_POINTS])
        self.k = k
        self.cloud = _records(k, 0xFF000000 | rng.integers(0, 1 << 24, len(k)).astype(np.uint32))
        self.dup = [(i, self.n_lat + i) for i in range(N_DUP)]             # index pairs of coincident points
        # seeded random unit normals, every 17th all-NaN
        v = rng.normal(0, 1, (len(k), 3))
        v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
        rnd = np.zeros(len(k), dtype=NORMAL)
        rnd["nx"], rnd["ny"], rnd["nz"] = v[:, 0], v[:, 1], v[:, 2]
        for f in NORMAL.names:
            rnd[f][::17] = np.nan
        self.normals = {"random": rnd}
        # keypoints on the cloud: both copies of points 0, 1 and 7, and 34 others
        on = [0, self.n_lat, 1, self.n_lat + 1, 7, self.n_lat + 7] + list(N_DUP + rng.choice(self.n_lat - N_DUP, 34, replace=False))
        far_on = self.cloud[3:4].copy()
        far_on["x"] += F(400.0)
        homes_on = [self.cloud[np.flatnonzero((k == c).all(axis=1))[0]] for c in _CLUSTER_HOMES]
        self.special = {"on": (2, 10, 20, 30), "off": (2, 20, 62, 64)}      # where the far, 1-, 2- and 3-neighbour keypoints sit
        kp_on = _spread([self.cloud[i] for i in on], [far_on[0]] + homes_on, self.special["on"])
        # keypoints off the cloud: p + (H/2, H/2, 0)
        off = rng.choice(self.n_lat, 150, replace=False)
        half = np.array([0.5, 0.5, 0.0])
        rows = _records(np.concatenate([lat[off] + half, [lat[5] + half + [3200, 0, 0]], np.array(_CLUSTER_HOMES) + half]),
                        0xFF000000 | rng.integers(0, 1 << 24, 154).astype(np.uint32))
        kp_off = _spread(list(rows[:150]), list(rows[150:]), self.special["off"])
        self.keypoints = {"on": np.array(kp_on, dtype=POINT), "off": np.array(kp_off, dtype=POINT)}
        assert len(self.cloud) <= 650 and len(self.keypoints["on"]) == 44 and len(self.keypoints["off"]) == 154

    def xyz(self, a=None):
        a = self.cloud if a is None else a
        return np.stack([a["x"], a["y"], a["z"]], axis=1)

    def __repr__(self):
        return self.name


def make_cases():
    return [Case(name, seed) for name, seed in zip(CLOUDS, (11, 12, 13))]


# ------------------------------------------------------------------------------------------------------ float32 brute force
def d2_matrix(q, p):
    """FLANN's L2_Simple in float32: ((dx dx + dy dy) + dz dz), q (m, 3) against p (n, 3).  On these inputs every step is exact."""
    q, p = np.asarray(q, F), np.asarray(p, F)
    d = q[:, 0:1] - p[None, :, 0]
    out = d * d
    d = q[:, 1:2] - p[None, :, 1]
    out += d * d
    d = q[:, 2:3] - p[None, :, 2]
    out += d * d
    assert out.dtype == F
    return out


def tie_counts(case):
    """What the case claims, counted by brute force: dict of name -> count."""
    p = case.xyz()
    out = {"points": len(p)}
    for label, r in (("normals", R_NRM), ("descriptors", R_DESC)):
        r2 = F(r * r)
        assert float(r2) == r * r
        d2 = d2_matrix(p, p)
        inside = d2 < r2
        tied = 0
        for i in range(len(p)):
            v = d2[i, inside[i]]
            tied += len(np.unique(v)) < len(v)
        out["neighbourhoods of the %s radius with two equal d2" % label] = tied
        out["pairs at exactly d2 == r2, %s radius" % label] = int((d2 == r2).sum()) // 2
    kp = case.keypoints["off"]
    d2 = d2_matrix(case.xyz(kp), p)
    out["off-cloud keypoints whose minimum d2 is shared"] = int(((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) >= 2).sum())
    out["neighbour counts of the special keypoints, off"] = [int((d2[i] < F(R_DESC * R_DESC)).sum()) for i in case.special["off"]]
    d2 = d2_matrix(case.xyz(case.keypoints["on"]), p)
    out["neighbour counts of the special keypoints, on"] = [int((d2[i] < F(R_DESC * R_DESC)).sum()) for i in case.special["on"]]
    out["largest neighbourhood"] = int(max((d2_matrix(p, p) < F(R_DESC * R_DESC)).sum(axis=1).max(), (d2 < F(R_DESC * R_DESC)).sum(axis=1).max()))
    return out


# ------------------------------------------------------------------------------------------------------------------ compare
BIT_EQUAL = ("normals", "harris_response", "harris_keypoints", "fpfh", "pfh", "pfhrgb", "keypoints", "shot_frames")
TOLERANCE = {"shot": 2e-6, "rsd": 1e-6}            # test_shot, test_rsd
SC3D_BINS, SC3D_BIN_TOL, SC3D_MASS = 8, 1e-5, 0.05  # test_sc3d


def _words(a):
    """Rows of 32-bit words: record arrays (POINT: xyz and rgba; NORMAL), float32 matrices and vectors alike."""
    a = np.ascontiguousarray(a)
    n = len(a)
    w = a.view(np.uint32).reshape(n, -1) if n else np.zeros((0, 1), np.uint32)
    f = a.view(F).reshape(n, -1) if n else np.zeros((0, 1), F)
    return w, f


def compare(stage, got, ref):
    """Indices of the points / rows of `got` that fail the project's criterion for `stage` against `ref`.

    BIT_EQUAL stages: every 32-bit word of the row equal (a NaN matches a NaN: the sign and payload of a NaN are the host's and
    the device's own, the existing tests never compared any); "harris_keypoints" takes (n, 3) xyz, so order and count are part
    of it.  "shot" / "rsd": |got - ref| <= 2e-6 / 1e-6 in every bin (test_shot, test_rsd).  "sc3d": at most 8 bins differ by
    more than 1e-5 and the row's mass is within 5 % of the largest reference row mass (test_sc3d).  A different number of rows
    fails every row."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return np.arange(max(len(got), len(ref), 1))
    if len(ref) == 0:
        return np.zeros(0, np.int64)
    if stage in BIT_EQUAL:
        gw, gf = _words(got)
        rw, rf = _words(ref)
        same = gw == rw
        if got.dtype != POINT:                                             # (rgba words are integers, never NaNs)
            same |= np.isnan(gf) & np.isnan(rf)
        else:
            same[:, :3] |= np.isnan(gf[:, :3]) & np.isnan(rf[:, :3])
        return np.flatnonzero(~same.all(axis=1))
    if stage in TOLERANCE:
        with np.errstate(invalid="ignore"):
            ok = np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= TOLERANCE[stage]
        return np.flatnonzero(~ok.all(axis=1))
    if stage == "sc3d":
        with np.errstate(invalid="ignore"):
            bins = (~(np.abs(got - ref) <= SC3D_BIN_TOL)).sum(axis=1)
            mass = np.abs(got.sum(axis=1) - ref.sum(axis=1)) <= SC3D_MASS * ref.sum(axis=1).max()
        return np.flatnonzero((bins > SC3D_BINS) | ~mass)
    raise KeyError(stage)


def survivors(kp_in, kp_out):
    """Mask of the keypoints that pruning kept: kp_out is kp_in without some records, in order."""
    keep = np.zeros(len(kp_in), bool)
    a, b = _words(kp_in)[0], _words(kp_out)[0]
    j = 0
    for i in range(len(a)):
        if j < len(b) and (a[i] == b[j]).all():
            keep[i] = True
            j += 1
    assert j == len(b), "the pruned keypoints are not a subsequence of the input"
    return keep


# ---------------------------------------------------------------------------------------------------------------- reference
# (stage, normal set, keypoint set) that are tie-order checks, with the least number of points / rows on which compare() must
# tell a cloud from its index-reversed copy (tests/test_feature_cases_cpu.py).  SHOT's minimum is over the three clouds together.
TIE_ORDER_CHECKS = {
    ("normals", None, None): 100,
    ("harris_response", "oracle", None): 100, ("harris_response", "random", None): 100,
    ("fpfh", "random", "off"): 100,
    ("pfh", "random", "off"): 100,
    ("rsd", "random", "off"): 50,
    ("sc3d", "random", "off"): 50,
}
SHOT_TIE_ORDER_CHECKS = {("shot", "oracle", "off"): 20, ("shot", "random", "off"): 20}     # rows over the three clouds together
# Everything else the GPU test compares is "compared, not a tie-order check": PFHRGB (every ordered pair: order-free by design,
# the reversal leaves it bit-identical), the keypoints "on" (44 rows: too few for the minimums), and FPFH / PFH / RSD / SC3D with
# the oracle's normals, which on the plane are nearly all alike, so that the order of the payloads hardly shows.


HARRIS_THRESHOLDS = (-1.0, 0.0)


def oracle_all(po, cloud, normals, keypoints):
    """Every oracle stage on one cloud: dict keyed like TIE_ORDER_CHECKS.  normals: {"random": ...} ("oracle" is computed here
    when absent; a set outside NORMAL_SETS goes through the Harris stages only); keypoints: {"on": ..., "off": ...}."""
    out = {}
    nrm = dict(normals)
    out["normals", None, None] = po.normals(cloud, R_NRM)
    nrm.setdefault("oracle", out["normals", None, None])
    fn = {"pfh": po.descriptors_pfh, "pfhrgb": po.descriptors_pfhrgb, "fpfh": po.descriptors_fpfh, "rsd": po.descriptors_rsd,
          "shot": po.descriptors_shot, "sc3d": po.descriptors_sc3d}
    for ns in sorted(nrm):
        for thr in HARRIS_THRESHOLDS:
            kp, idx, resp = po.keypoints_harris(cloud, nrm[ns], thr, R_NRM)
            out["harris_keypoints", ns, thr] = np.stack([kp["x"], kp["y"], kp["z"]], axis=1).reshape(-1, 3)
            out["harris_kept", ns, thr] = idx
        out["harris_response", ns, None] = resp
        for ks in KEYPOINT_SETS if ns in NORMAL_SETS else ():
            for name in DESCRIPTORS:
                kp, rows = fn[name](cloud, nrm[ns], keypoints[ks], R_DESC)
                out[name, ns, ks] = rows
                out["keypoints", name, ns, ks] = kp
                if name == "shot":
                    raw, rf = po.shot_raw(cloud, nrm[ns], keypoints[ks], R_DESC)
                    out["shot_frames", ns, ks] = rf[np.isfinite(raw).all(axis=1)]
    return out, nrm


_REFERENCE = {}


def reference(po):
    """[(case, oracle results)] for the three clouds, computed once per process; case.normals gains the "oracle" set."""
    if "cases" not in _REFERENCE:
        cases = make_cases()
        refs = []
        for c in cases:
            if c.name == "plane":
                c.normals["flat"] = po.normals(_records(c.k, c.cloud["rgba"], offset=np.zeros(3)), R_NRM)
            ref, c.normals = oracle_all(po, c.cloud, c.normals, c.keypoints)
            refs.append(ref)
        _REFERENCE["cases"] = list(zip(cases, refs))
    return _REFERENCE["cases"]

"""Reference and aimed inputs for the ICP / score nearest-neighbour search (csrc/nn_search_body.hpp, test hook
mm3d_debug_nn_search).  A plain module: tests/test_nn_cases_cpu.py checks the inputs on the CPU, tests/test_gpu_nn_search.py
compares the device with the reference point by point.

Reference: brute force in numpy, float32, every step rounded like the device's (the library is built with -ffp-contract=off):
  p  = ((m0 x + m1 y) + m2 z) + m3         per row of the transform (device_util.hpp: xform)
  d2 = ((dx dx + dy dy) + dz dz)           (nn_search_body.hpp: d2_pair)
  winner = the least (d2 bits, original index); in range: d2 <= max_d2 as the library derives it.

Geometry (what decides which branch of the search a point takes): cell = range / 4 (0.25 m when that is not above 1 mm;
x 1.5 until the table has at most 2e8 cells), origin = the target's bounding-box minimum, d0 = max-norm distance in cells
from a query's cell to the nearest occupied cell.  All restated here in numpy, independent of the library.

A case = source, target, transform, ranges [(convention, value), ...] (0: ICP's max_correspondence_distance, 1: transformScore's
max_distance, compared with the SQUARED distance; the first one is the case's own, the one its coverage is counted at) and
a coverage function: counts taken from the reference result and the geometry, each with the minimum the case exists for.
A case that misses a minimum fails."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

F = np.float32
U32 = 2.0 ** -24          # float32 unit roundoff
DBL_MAX = np.finfo(np.float64).max
# Frobenius distance allowed between one device ICP iteration and the float64 Umeyama over the reference correspondences
# (tests/test_gpu_nn_search.py, where it is measured: 5.58e-7 at worst on an MI355X, times 4; tests/test_nn_cases_cpu.py shows that
# one wrong correspondence exceeds it)
ICP_STEP_TOLERANCE = 2.24e-6


# ---------------------------------------------------------------------------------------------------------------- reference
def xform32(T, pts):
    """pts (n, 3) float32 carried by the row-major 4x4 T, in xform()'s order, every step rounded to float32."""
    T = np.asarray(T, dtype=F)
    x, y, z = (np.ascontiguousarray(pts[:, k], dtype=F) for k in range(3))
    out = np.empty((len(pts), 3), dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):          # (non-finite source points stay non-finite)
        for r in range(3):
            out[:, r] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
    return out


def max_d2_of(convention, value):
    """The largest float32 d2 that is in range: ICP accepts (double)d2 <= max_corr_dist^2, the score (double)d2 <= max_distance."""
    lim = float(value) * float(value) if convention == 0 else float(value)
    m = F(lim)
    if float(m) > lim:
        m = np.nextafter(m, F(-np.inf))
    return F(m)


def radius_of(convention, value):
    return float(value) if convention == 0 else math.sqrt(value if value > 0 else 0.0)


def _brute_chunk(p, tgt, tfin, want_second, want_ties):
    dx = p[:, 0:1] - tgt[None, :, 0]
    d2 = dx * dx
    dx = p[:, 1:2] - tgt[None, :, 1]
    d2 += dx * dx
    dx = p[:, 2:3] - tgt[None, :, 2]
    d2 += dx * dx                                      # ((dx dx + dy dy) + dz dz), float32 throughout
    if not tfin.all():
        d2[:, ~tfin] = np.inf
    idx = np.argmin(d2, axis=1)                         # the first minimum: the lowest original index
    rows = np.arange(len(p))
    best = d2[rows, idx]
    ties = (d2 == best[:, None]).sum(axis=1) if want_ties else None
    second = second_d2 = None
    if want_second:
        d2[rows, idx] = np.inf
        second = np.argmin(d2, axis=1)
        second_d2 = d2[rows, second]
    return idx, best, ties, second, second_d2


def brute_nn(src, tgt, T, want_second=False, want_ties=False, chunk_pairs=1 << 22, threads=16):
    """Nearest target of every source point, whatever the range: dict(p, idx, d2[, ties, second, second_d2]).  Non-finite source
    points and an empty target give idx -1, d2 +inf."""
    src = np.asarray(src, dtype=F).reshape(-1, 3)
    tgt = np.asarray(tgt, dtype=F).reshape(-1, 3)
    n, m = len(src), len(tgt)
    p = xform32(T, src) if n else np.zeros((0, 3), F)
    out = dict(p=p, idx=np.full(n, -1, np.int64), d2=np.full(n, np.inf, F))
    if want_ties:
        out["ties"] = np.zeros(n, np.int64)
    if want_second:
        out["second"] = np.full(n, -1, np.int64)
        out["second_d2"] = np.full(n, np.inf, F)
    tfin = np.isfinite(tgt).all(axis=1) if m else np.zeros(0, bool)
    if n == 0 or not tfin.any():
        return out
    sfin = np.flatnonzero(np.isfinite(src).all(axis=1))
    step = max(1, chunk_pairs // m)
    jobs = [sfin[a:a + step] for a in range(0, len(sfin), step)]
    tsafe = np.where(tfin[:, None], tgt, F(0))

    def run(sel):
        with np.errstate(invalid="ignore", over="ignore"):
            return sel, _brute_chunk(p[sel], tsafe, tfin, want_second, want_ties)
    with ThreadPoolExecutor(max_workers=threads) as ex:
        for sel, (idx, best, ties, second, second_d2) in ex.map(run, jobs):
            out["idx"][sel] = idx
            out["d2"][sel] = best
            if want_ties:
                out["ties"][sel] = ties
            if want_second:
                out["second"][sel] = second
                out["second_d2"][sel] = second_d2
    return out


def in_range(nn, convention, value):
    """(idx, d2) as mm3d_debug_nn_search returns them for this range: -1 / +inf where the nearest is out of range."""
    ok = (nn["idx"] >= 0) & (nn["d2"] <= max_d2_of(convention, value))
    return np.where(ok, nn["idx"], -1).astype(np.int32), np.where(ok, nn["d2"], F(np.inf)).astype(F)


def score_of(d2):
    """fsum(d2 in range) / count in double (exactly rounded sum), and the count; DBL_MAX for none."""
    v = d2[np.isfinite(d2)].astype(np.float64)
    return (math.fsum(v) / len(v), len(v)) if len(v) else (DBL_MAX, 0)


def brute_nn64(src, tgt, T, chunk_pairs=1 << 21):
    """The same search in float64 from the float32 inputs: (idx, d2, second_d2, scale) with scale = the largest magnitude that
    entered a point's sums (what its float32 rounding is proportional to)."""
    src = np.asarray(src, np.float64).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float64).reshape(-1, 3)
    T = np.asarray(T, dtype=F).astype(np.float64)
    p = src @ T[:3, :3].T + T[:3, 3]
    mag = np.abs(src) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3])
    n, m = len(src), len(tgt)
    idx, d2, s2 = np.zeros(n, np.int64), np.zeros(n), np.zeros(n)
    step = max(1, chunk_pairs // m)
    for a in range(0, n, step):
        d = ((p[a:a + step, None, :] - tgt[None, :, :]) ** 2).sum(axis=2)
        i = np.argmin(d, axis=1)
        r = np.arange(len(i))
        idx[a:a + step], d2[a:a + step] = i, d[r, i]
        d[r, i] = np.inf
        s2[a:a + step] = d.min(axis=1) if m > 1 else np.inf
    return idx, d2, s2, np.maximum(mag.max(axis=1), np.abs(tgt).max() if m else 0.0)


def d2_rounding(d2, scale):
    """A bound of |float32 d2 - exact d2|: the transformed point is off by at most 4 roundings of its largest term per axis
    (e <= sqrt(3) 4 u scale), each difference by one more, the squares and the two sums by 3 u d2."""
    e = math.sqrt(3.0) * 5.0 * U32 * scale
    return 2.0 * np.sqrt(d2) * e + e * e + 4.0 * U32 * d2


# ----------------------------------------------------------------------------------------------------------------- geometry
def geometry(tgt, convention, value, dense_limit=3e7):
    """The target grid as nn.hip / grid.hip derive it: dict(cell, inv, origin, dims, rmax, max_ring, max_d2[, occ])."""
    tgt = np.asarray(tgt, dtype=F).reshape(-1, 3)
    tgt = tgt[np.isfinite(tgt).all(axis=1)]
    radius = radius_of(convention, value)
    cell = F(radius * 0.25)
    if not cell > F(1e-3):
        cell = F(0.25)
    nominal = cell
    bmin, bmax = tgt.min(axis=0), tgt.max(axis=0)
    while True:
        inv = 1.0 / float(cell)
        dims = [int(math.floor((float(bmax[a]) - float(bmin[a])) * inv) + 2) for a in range(3)]
        if float(dims[0]) * dims[1] * dims[2] <= 2.0e8:
            break
        cell = F(cell * F(1.5))
    rmax = F(radius * 1.0001 + 1e-5)
    g = dict(cell=cell, nominal_cell=nominal, inv=F(1.0) / cell, origin=bmin.astype(F), dims=tuple(dims), rmax=rmax,
             max_ring=int(np.ceil(rmax / cell)) + 1, max_d2=max_d2_of(convention, value))
    if float(dims[0]) * dims[1] * dims[2] <= dense_limit:
        c = np.clip(cells_of(tgt, g), 0, np.array(dims) - 1)
        occ = np.zeros(dims, dtype=bool)
        occ[c[:, 0], c[:, 1], c[:, 2]] = True
        g["occ"] = occ
    return g


def cells_of(p, g):
    """cell_floor per axis: floorf((v - min) * inv) in float32 (not clamped to the grid)."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((np.asarray(p, dtype=F) - g["origin"]) * g["inv"])
    return np.clip(np.nan_to_num(f, nan=0.0), -1048576.0, 1048576.0).astype(np.int64)


def _dilate(a):
    for ax in range(3):
        b = a.copy()
        s0 = [slice(None)] * 3
        s1 = [slice(None)] * 3
        s0[ax], s1[ax] = slice(1, None), slice(None, -1)
        b[tuple(s0)] |= a[tuple(s1)]
        b[tuple(s1)] |= a[tuple(s0)]
        a = b
    return a


def d0_of(p, g, cap=None):
    """Max-norm distance in cells from each query's cell to the nearest occupied cell (cap + 1 beyond cap); -1 outside the grid."""
    cap = g["max_ring"] + 1 if cap is None else cap
    c = cells_of(p, g)
    dims = np.array(g["dims"])
    inside = ((c >= 0) & (c < dims)).all(axis=1)
    dist = np.full(g["dims"], cap + 1, dtype=np.int16)
    reach = g["occ"]
    dist[reach] = 0
    for d in range(1, cap + 1):
        grown = _dilate(reach)
        dist[grown & ~reach] = d
        reach = grown
    out = np.full(len(c), -1, dtype=np.int64)
    ci = c[inside]
    out[inside] = dist[ci[:, 0], ci[:, 1], ci[:, 2]]
    return out


def hilbert_items(src):
    """The source's work items as grid.hip forms them: (order, items [(first, count)]) -- finite points sorted (stably) by
    (Hilbert index of the x, y column << 10 | z cell); an item starts at the first point, at every change of the 8 x 8 column
    block and at every 64th point."""
    src = np.asarray(src, dtype=F).reshape(-1, 3)
    fin = np.flatnonzero(np.isfinite(src).all(axis=1))
    pts = src[fin]
    if len(pts) == 0:
        return fin, []
    bmin, bmax = pts.min(axis=0), pts.max(axis=0)
    cell = max(F(0.25), F((bmax - bmin).max()) / F(1023.0))
    inv = F(1.0) / F(cell)
    c = np.clip(np.floor((pts - bmin) * inv), 0, 1023).astype(np.uint64)
    x, y, z = c[:, 0].copy(), c[:, 1].copy(), c[:, 2]
    d = np.zeros(len(pts), dtype=np.uint64)
    s = 512
    while s > 0:
        rx, ry = ((x & s) > 0).astype(np.uint64), ((y & s) > 0).astype(np.uint64)
        d += np.uint64(s * s) * ((np.uint64(3) * rx) ^ ry)
        flip = (ry == 0) & (rx == 1)
        x[flip], y[flip] = 1023 - x[flip], 1023 - y[flip]
        swap = ry == 0
        x[swap], y[swap] = y[swap], x[swap].copy()
        s >>= 1
    key = ((d << np.uint64(10)) | z) & np.uint64(0xFFFFFFFF)
    order = np.argsort(key, kind="stable")
    k = key[order]
    j = np.arange(len(k))
    head = (j == 0) | ((j & 63) == 0)
    head[1:] |= (k[1:] >> np.uint64(16)) != (k[:-1] >> np.uint64(16))
    starts = np.flatnonzero(head)
    counts = np.diff(np.append(starts, len(k)))
    return fin[order], list(zip(starts.tolist(), counts.tolist()))


def first_box_rows(case, g, nn):
    """Per work item: rows (ny * nz) of its first pass's box -- the union of the active lanes' own boxes, clamped to the grid."""
    order, items = hilbert_items(case.src)
    p = nn["p"]
    c = cells_of(p, g)
    d0 = d0_of(p, g)
    dims = np.array(g["dims"])
    rows = []
    for a, n in items:
        sel = order[a:a + n]
        act = (d0[sel] >= 0) & (d0[sel] <= g["max_ring"])
        if not act.any():
            rows.append(0)
            continue
        need = np.maximum(d0[sel][act], 1)
        cc = c[sel][act]
        lo = np.maximum((cc - need[:, None]).min(axis=0), 0)
        hi = np.minimum((cc + need[:, None]).max(axis=0), dims - 1)
        rows.append(int(max(hi[1] - lo[1] + 1, 0) * max(hi[2] - lo[2] + 1, 0)))
    return np.array(rows)


# -------------------------------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, name, src, tgt, ranges, T=None, coverage=None, aimed_at="", light=False):
        self.name, self.aimed_at, self.light = name, aimed_at, light     # light: a large case, no second-nearest and no tie counts
        self.src = np.ascontiguousarray(src, dtype=F).reshape(-1, 3)
        self.tgt = np.ascontiguousarray(tgt, dtype=F).reshape(-1, 3)
        self.T = np.eye(4, dtype=F) if T is None else np.asarray(T, dtype=F)
        self.ranges = list(ranges)
        self.coverage = coverage          # f(case, nn, geometry) -> {what: (count, minimum)}
        self._nn = None

    def nn(self):
        if self._nn is None:
            self._nn = brute_nn(self.src, self.tgt, self.T, want_second=not self.light, want_ties=not self.light)
        return self._nn

    def geometry(self, k=0):
        return geometry(self.tgt, *self.ranges[k])

    def check_coverage(self):
        """{what: (count, minimum)} of the case's own range; empty for a case without a condition."""
        if self.coverage is None:
            return {}
        return self.coverage(self, self.nn(), self.geometry() if len(self.tgt) else None)

    def __repr__(self):
        return self.name


def points(xyz):
    """(n, 3) float32 -> the library's POINT records (x, y, z, rgba)."""
    xyz = np.asarray(xyz, dtype=F).reshape(-1, 3)
    a = np.zeros(len(xyz), dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")]))
    a["x"], a["y"], a["z"], a["rgba"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], 0xFF808080
    return a


def rigid(angle, axis, t):
    """Rotation by `angle` about `axis`, then translation t (float64 4x4)."""
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)
    T[:3, 3] = t
    return T


def _share_in_range(nn, convention, value):
    idx, _ = in_range(nn, convention, value)
    return float((idx >= 0).mean()) if len(idx) else 0.0


def _small_rot(ax, ay, az, t):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


PARITY_RANGES = [(1, 0.25), (1, 0.0025), (1, 0.04), (1, 4.0), (1, 100.0), (0, 0.1), (0, 2.0)]


def parity_cases(po, synth):
    """The two maps of tests/test_gpu_parity.py's scene (filtered by the oracle), the three poses and five score ranges of
    test_nearest_neighbour_search_over_ranges (and its two ICP ranges).  The ordinary path."""
    _, maps = synth.synth_maps(2, 12000, overlap_step=0.35)
    filt = []
    for x, c, _T in maps:
        f = po.remove_outliers(po.downsample(synth.pack_points(x, c), 0.1), 0.8, 50)
        filt.append(np.stack([f["x"], f["y"], f["z"]], axis=1))
    gt = synth.relative_gt(maps[0][2], maps[1][2]).astype(F)
    poses = (gt, (gt @ _small_rot(0.05, -0.03, 0.2, [0.6, -0.4, 0.2])).astype(F), (gt @ _small_rot(0.0, 0.0, 0.0, [3.0, 2.0, 0.5])).astype(F))

    cases = []

    def cov(case, nn, g):
        # The middle ranges, 0.5 m and 2 m (max_distance 0.25 and 4.0).  The poses are the existing test's: the third is 3.6 m off,
        # and 16 % of its points have a neighbour within 0.5 m, so the 0.5 m share is taken over the three poses together.
        pooled = float(np.mean([_share_in_range(c.nn(), 1, 0.25) for c in cases]))
        return {"share in range at 2 m (%)": (100 * _share_in_range(nn, 1, 4.0), 30), "share in range at 0.5 m, the three poses together (%)": (100 * pooled, 30)}
    cases += [Case("parity_pose%d" % k, filt[0], filt[1], PARITY_RANGES, T, cov, "the ordinary path") for k, T in enumerate(poses)]
    return cases


def lattice_case(seed=1, n_src=1800):
    """Target: a 12^3 lattice of spacing 1/8 (coordinates are multiples of 2^-6 after the 2^-6 offset), shuffled, with 300 points
    stored twice; sources at cell centres (8 equidistant targets), face centres (4) and edge midpoints (2): every distance exact."""
    rng = np.random.default_rng(seed)
    s = 0.125
    k = np.arange(12)
    lat = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) * s + 2.0 ** -6
    tgt = np.concatenate([lat, lat[rng.choice(len(lat), 300, replace=False)]])
    tgt = tgt[rng.permutation(len(tgt))]
    base = lat[(lat < 11 * s).all(axis=1)]
    centre = base + s / 2
    face = np.concatenate([base + np.array(o) * s / 2 for o in ((1, 1, 0), (1, 0, 1), (0, 1, 1))])
    edge = np.concatenate([base + np.array(o) * s / 2 for o in ((1, 0, 0), (0, 1, 0), (0, 0, 1))])
    pick = lambda a, n: a[rng.choice(len(a), n, replace=False)]   # noqa: E731
    src = np.concatenate([pick(centre, n_src // 3), pick(face, n_src // 3), pick(edge, n_src // 3), tgt[:100]])

    def cov(case, nn, g):
        return {"minimum shared by >= 2 targets": (int((nn["ties"] >= 2).sum()), 200), "minimum shared by 8": (int((nn["ties"] >= 8).sum()), 20)}
    return Case("lattice_ties", src, tgt, [(0, 0.5), (1, 0.25), (0, 0.11)], None, cov, "tie to the lower index; early exit on equal d2")


def _offsets_hitting(want):
    """(dx, dy) float32 >= 0 with fl(fl(dx dx) + fl(dy dy)) == want, dy = 0 where one axis can do it."""
    want = F(want)
    r = F(np.sqrt(np.float64(want)))
    cand = [r]
    for _ in range(6):
        cand.append(np.nextafter(cand[-1], F(np.inf)))
        cand.insert(0, np.nextafter(cand[0], F(0)))
    for dx in cand:
        if F(dx * dx) == want:
            return F(dx), F(0)
    for e in range(-14, -4):                       # a second, small offset moves the sum by less than one step of dx
        dy = F(math.sqrt(float(want)) * 2.0 ** e)
        r = F(np.sqrt(max(np.float64(want) - np.float64(dy) ** 2, 0.0)))
        cand = [r]
        for _ in range(6):
            cand.append(np.nextafter(cand[-1], F(np.inf)))
            cand.insert(0, np.nextafter(cand[0], F(0)))
        for dx in cand:
            if F(F(dx * dx) + F(dy * dy)) == want:
                return F(dx), dy
    raise AssertionError("no offset reaches %r" % want)


def boundary_case(convention, value, pairs=72):
    """Isolated pairs 8 m apart along z: the target point at (0, 0, 8 k), its source point at the same z and an offset (exact: the
    target's x and y are 0) whose float32 d2 is EXACTLY max_d2 (in range) or the next float above it (not).  The offset runs
    along +-x or +-y: one axis where a float squares to the wanted value, else with a second, much smaller one on the other."""
    md2 = max_d2_of(convention, value)
    at, beyond = _offsets_hitting(md2), _offsets_hitting(np.nextafter(md2, F(np.inf)))
    tgt, src, kind = [], [], []
    for j in range(pairs):
        for which, (dx, dy) in enumerate((at, beyond)):
            base = np.array([0.0, 0.0, 16.0 * j + 8.0 * which], dtype=F)
            a, b = ((0, 1), (1, 0))[(j // 2) % 2]                      # the long offset along x or along y; z carries the pairs apart
            o = np.zeros(3, dtype=F)
            o[a], o[b] = dx * (1 if j % 2 else -1), dy
            tgt.append(base)
            src.append(base + o)
            kind.append(which)
    tgt, src, kind = np.array(tgt, dtype=F), np.array(src, dtype=F), np.array(kind)
    tgt = np.concatenate([tgt, [[-4, -4, -4], [4, 4, 16.0 * pairs + 4]]]).astype(F)    # the sources stay inside the grid

    def cov(case, nn, g):
        return {"exactly at max_d2": (int((nn["d2"] == md2).sum()), 50), "one ulp beyond": (int((nn["d2"] == np.nextafter(md2, F(np.inf))).sum()), 50)}
    return Case("boundary_%s_%g" % ("icp" if convention == 0 else "score", value), src, tgt, [(convention, value)], None, cov,
                "d2 == max_d2 is in range, the next float is not")


def faces_case(shift, seed=3, n=3000):
    """Range 1 m (cell 0.25): targets and sources in an 8 m box whose corner is (shift, shift, shift); a random axis (or two) of most
    points is put ON a cell face fl(min + k cell), or one float either side of it."""
    rng = np.random.default_rng(seed)
    cell, mn = F(0.25), F(shift)

    def cloud(n, corner):
        p = (mn + rng.uniform(0, 8, (n, 3))).astype(F)
        for i in range(n):
            for ax in rng.choice(3, rng.integers(0, 3), replace=False):
                f = F(mn + F(rng.integers(0, 33)) * cell)
                p[i, ax] = (np.nextafter(f, F(-np.inf)), f, np.nextafter(f, F(np.inf)))[rng.integers(0, 3)]
        if corner:
            p[0] = mn
        return np.maximum(p, mn)                  # (the target's minimum stays the corner: the faces are the grid's)
    tgt, src = cloud(n, True), cloud(n, False)

    def cov(case, nn, g):
        def near_face(p):
            k = np.round((p.astype(np.float64) - float(mn)) / 0.25)
            f = (mn + k.astype(F) * cell).astype(F)
            return (np.abs(p.astype(np.float64) - f) <= 2 * np.spacing(np.abs(f)).astype(np.float64)).any(axis=1)
        assert (case.tgt.min(axis=0) == mn).all()
        return {"sources within 2 ulp of a face": (int(near_face(case.src).sum()), 500), "targets within 2 ulp of a face": (int(near_face(case.tgt).sum()), 500),
                "share in range (%)": (100 * _share_in_range(nn, 0, 1.0), 30)}
    return Case("faces_shift_%g" % shift, src, tgt, [(0, 1.0), (1, 1.0)], None, cov, "cell_floor against guard, edge, lb_edge")


_DIRS = [np.array(v, float) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))] + \
        [np.array((a, b, c), float) / math.sqrt(3) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]


def sparse_case(seed=4, r=1.0):
    """Target: 48 tight clusters 6 m apart and a thin wall; sources approach every cluster along the six axes and the eight space
    diagonals, and the wall along its normal, at 0.5 .. 2.1 ranges from the nearest target point (2.1: the cells beyond max_ring)."""
    rng = np.random.default_rng(seed)
    cc = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3) * 6.0 + 3.0
    cc = cc + rng.uniform(-0.4, 0.4, cc.shape)
    clusters = (cc[:, None, :] + rng.uniform(-0.02, 0.02, (len(cc), 12, 3))).reshape(-1, 3)
    wy, wz = np.meshgrid(np.arange(0, 24, 0.15), np.arange(0, 18, 0.15), indexing="ij")
    wall = np.stack([np.full(wy.size, 30.0), wy.ravel(), wz.ravel()], axis=1) + rng.uniform(-0.01, 0.01, (wy.size, 3))
    tgt = np.concatenate([clusters, wall])
    grades = np.concatenate([np.linspace(0.5, 2.1, 17), np.linspace(0.95, 1.05, 8)]) * r
    src = [c + u * t + rng.uniform(-0.01, 0.01, 3) for c in cc for u in _DIRS for t in grades]
    src += [np.array([30.0 + s * t, y, z]) for s in (-1, 1) for t in grades for y, z in rng.uniform(1, 17, (25, 2))]
    src = np.array(src)

    def cov(case, nn, g):
        d0 = d0_of(nn["p"], g)
        dist = np.sqrt(nn["d2"].astype(np.float64))
        ok = nn["d2"] <= g["max_d2"]
        off = np.abs(case.tgt[nn["idx"]].astype(np.float64) - nn["p"]) / np.maximum(dist, 1e-30)[:, None]
        out = {"sources at d0 = %d" % d: (int((d0 == d).sum()), 100) for d in range(2, g["max_ring"] + 2)}
        out["in range at d0 >= 4"] = (int((ok & (d0 >= 4)).sum()), 100)
        out["within 5 % inside the limit"] = (int((ok & (dist >= 0.95 * r)).sum()), 100)
        out["within 5 % outside the limit"] = (int((~ok & (dist <= 1.05 * r)).sum()), 100)
        out["neighbour along a diagonal"] = (int((off >= 0.5).all(axis=1).sum()), 100)
        out["diagonal and in range"] = (int(((off >= 0.5).all(axis=1) & ok).sum()), 100)
        return out
    return Case("sparse_clusters_wall", src, tgt, [(0, r), (1, r * r)], None, cov, "d0 > max_ring, the lower bound, reach_cap, the corner filter")


def outside_case(seed=5, r=1.0, per=260):
    """Sources outside the target's box beyond each of its 6 sides, 12 edges and 8 corners, from touching to 2 ranges away."""
    rng = np.random.default_rng(seed)
    size = np.array([10.0, 8.0, 3.0])
    tgt = rng.uniform(0, 1, (5000, 3)) * size
    tgt[:2] = [[0, 0, 0], size]
    src, region = [], []
    signs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
    for k, sg in enumerate(signs):
        t = rng.uniform(0, 1, (per, 3)) ** 2 * 2.0 * r + 1e-4        # more of them near the box than far from it
        inner = rng.uniform(0, 1, (per, 3)) * size
        p = np.where(np.array(sg) < 0, -t, np.where(np.array(sg) > 0, size + t, inner))
        src.append(p)
        region += [k] * per
    src, region = np.concatenate(src), np.array(region)

    def cov(case, nn, g):
        c = cells_of(nn["p"], g)
        outside = ~((c >= 0) & (c < np.array(g["dims"]))).all(axis=1)
        ok = nn["d2"] <= g["max_d2"]
        out = {}
        for k, sg in enumerate(signs):
            out["%s in range" % (sg,)] = (int((ok & outside & (region == k)).sum()), 20)
            out["%s out of range" % (sg,)] = (int((~ok & outside & (region == k)).sum()), 20)
        return out
    return Case("outside_the_grid", src, tgt, [(0, r), (1, r * r)], None, cov, "the outside-the-grid branch")


def patch_case(seed=6, r=1.0):
    """Work items whose lanes need very different rings.  64 patches 4 m apart, each exactly 64 source points inside one 2 m column
    block (so each is one work item) over its own 3.4 m x 3.4 m piece of floor: even patches have 63 points ON the floor and one
    0.9 ranges above it -- over the others in every other such patch, 1.2 m to the side in the rest; odd patches are the mirror
    image, 63 points 0.9 ranges up and one on the floor."""
    rng = np.random.default_rng(seed)
    fx, fy = np.meshgrid(np.arange(-1.0, 2.4, 0.1), np.arange(-1.0, 2.4, 0.1), indexing="ij")
    floor = np.stack([fx.ravel(), fy.ravel(), np.zeros(fx.size)], axis=1)
    foot = rng.uniform(0.05, 0.45, (63, 2))
    tgt, src, far, patch = [], [], [], []
    for k in range(64):
        o = np.array([4.0 * (k % 8), 4.0 * (k // 8), 0.0])
        tgt.append(floor + o + np.append(rng.uniform(-0.005, 0.005, 2), 0.0))
        near = np.concatenate([foot, np.full((63, 1), 0.002)], axis=1)
        if k % 2 == 0:
            side = 1.2 if (k // 2) % 2 else 0.0
            one = np.array([[0.25 + side, 0.25, 0.9 * r]])
            p, f = np.concatenate([near, one]), [False] * 63 + [True]
        else:
            up = np.concatenate([rng.uniform(0.05, 1.6, (63, 2)), np.full((63, 1), 0.9 * r)], axis=1)
            p, f = np.concatenate([up, [[0.25, 0.25, 0.002]]]), [True] * 63 + [False]
        src.append(p + o)
        far += f
        patch += [k] * 64
    src, tgt, far, patch = np.concatenate(src), np.concatenate(tgt), np.array(far), np.array(patch)
    src[0, :2] = 0.0                                   # the source's corner: the column blocks start here

    def cov(case, nn, g):
        order, items = hilbert_items(case.src)
        whole = sum(1 for a, n in items if n == 64 and len(set(patch[order[a:a + n]])) == 1)
        c, tc = cells_of(nn["p"], g), cells_of(case.tgt[nn["idx"]], g)
        covered = np.zeros(len(case.src), bool)
        for k in range(64):
            nearl = (patch == k) & ~far
            lo, hi = c[nearl].min(axis=0) - 1, c[nearl].max(axis=0) + 1        # the near lanes' first box: their cells, one ring
            covered[patch == k] = ((tc[patch == k] >= lo) & (tc[patch == k] <= hi)).all(axis=1)
        ok = nn["d2"] <= g["max_d2"]
        return {"patches that are one work item": (whole, 60), "far lanes whose neighbour the near lanes' box covers": (int((far & ok & covered).sum()), 50),
                "far lanes whose neighbour lies outside it": (int((far & ok & ~covered).sum()), 50)}
    return Case("patch_mixed_rings", src, tgt, [(0, r), (1, r * r)], None, cov, "per-lane boxes, shell skipping over several passes")


def _dense_target(rng):
    bg = rng.uniform(0, 1, (2500, 3)) * np.array([12.0, 12.0, 8.0])
    bg[:2] = [[0, 0, 0], [12, 12, 8]]
    cells = {300: (10, 10, 6), 1100: (30, 12, 10), 5000: (20, 34, 16)}          # cell numbers of a 0.25 m grid at the origin
    dense = [(np.array(c) + rng.uniform(0.02, 0.98, (n, 3))) * 0.25 for n, c in cells.items()]
    return np.concatenate([bg] + dense), cells


def dense_cells_case(seed=7):
    """One cell with 300, one with 1 100 and one with 5 000 target points (tiles of 256, the padding to four); sources around them."""
    rng = np.random.default_rng(seed)
    tgt, cells = _dense_target(rng)
    src = np.concatenate([(np.array(c) + 0.5) * 0.25 + rng.uniform(-0.6, 0.6, (700, 3)) for c in cells.values()] + [rng.uniform(0, 1, (900, 3)) * [12, 12, 8]])

    def cov(case, nn, g):
        tc = cells_of(case.tgt, g)
        out = {}
        for n, c in cells.items():
            got = int((tc == np.array(c)).all(axis=1).sum())
            out["points in the cell meant to hold %d" % n] = (got if got <= n + 3 else -got, n)
        return out
    return Case("dense_cells", src, tgt, [(0, 1.0), (1, 1.0)], None, cov, "kTile tiles, the padding to four")


def wide_items_case(seed=8):
    """The same target; a sparse source of exactly 64 points per 2 m column block, spread over the block's full height, so that
    each work item's first box has more rows than one chunk of span headers holds (kRows = 256)."""
    rng = np.random.default_rng(seed)
    tgt, _ = _dense_target(rng)
    src = np.concatenate([np.array([4.0 * i, 4.0 * j, 0.0]) + rng.uniform(0.02, 1.9, (64, 3)) * [1, 1, 4.0] for i in range(3) for j in range(3)])
    src[0] = 0.0

    def cov(case, nn, g):
        rows = first_box_rows(case, g, nn)
        return {"items whose first box has > 256 rows": (int((rows > 256).sum()), 1), "share in range (%)": (100 * _share_in_range(nn, 0, 1.0), 30)}
    return Case("wide_items", src, tgt, [(0, 1.0), (1, 1.0)], None, cov, "more than kRows spans per pass")


def degenerate_cases(seed=9):
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(0, 1, (1500, 3)) * [6, 6, 2]
    src = tgt[rng.permutation(len(tgt))[:400]] + rng.normal(0, 0.2, (400, 3))
    bad = src.copy()
    bad[5, 0], bad[17, 1], bad[63, 2], bad[64] = np.nan, np.inf, -np.inf, np.nan
    flat, line = tgt.copy(), tgt.copy()
    flat[:, 2] = 1.0
    line[:, 1:] = [3.0, 1.0]
    rg = [(0, 0.5), (1, 0.25)]

    def count(what, f, least):
        return lambda case, nn, g: {what: (f(case, nn, g), least)}
    none = np.zeros((0, 3))
    return [
        Case("one_target_point", src, tgt[:1], rg, None, count("target points", lambda c, n, g: 2 - len(c.tgt), 1), "dims of 2"),
        Case("one_source_point", tgt[7:8] + 0.1, tgt, rg, None, count("in range", lambda c, n, g: int((n["d2"] <= g["max_d2"]).sum()), 1), "item edges"),
        Case("63_source_points", src[:63], tgt, rg, None, count("source points", lambda c, n, g: int(len(c.src) == 63), 1), "item edges"),
        Case("64_source_points", src[:64], tgt, rg, None, count("source points", lambda c, n, g: int(len(c.src) == 64), 1), "item edges"),
        Case("65_source_points", src[:65], tgt, rg, None, count("source points", lambda c, n, g: int(len(c.src) == 65), 1), "item edges"),
        Case("planar_target", src, flat, rg, None, count("cells in z", lambda c, n, g: int(g["dims"][2] == 2), 1), "dims of 2"),
        Case("collinear_target", src, line, rg, None, count("axes of 2 cells", lambda c, n, g: int(g["dims"][1] == 2) + int(g["dims"][2] == 2), 2), "dims of 2"),
        Case("non_finite_source_points", bad, tgt, rg, None, count("skipped points", lambda c, n, g: int((n["idx"] < 0).sum()), 4), "skipped points"),
        Case("empty_source", none, tgt, rg, None, count("source points", lambda c, n, g: 1 - len(c.src), 1), "nothing to search"),
        Case("empty_target", src, none, rg, None, count("target points", lambda c, n, g: 1 - len(c.tgt), 1), "nothing to search"),
    ]


def regime_cases(seed=10):
    """nn_cell_for and the bounded table: a range whose quarter is below 1 mm (the cell is clamped to 0.25 m), a range larger than
    the scene (a grid of a few cells), and a 4.5 mm range on a 100 m x 100 m x 3 m target (the cell grows x 1.5 until the table fits)."""
    rng = np.random.default_rng(seed)
    scene = rng.uniform(0, 1, (2500, 3)) * [20, 20, 3]
    wide = rng.uniform(0, 1, (6000, 3)) * [100, 100, 3]
    wide[:2] = [[0, 0, 0], [100, 100, 3]]

    def near(t, n, spread):
        u = rng.normal(0, 1, (n, 3))
        return t[rng.permutation(len(t))[:n]] + u / np.linalg.norm(u, axis=1)[:, None] * rng.uniform(0, spread, (n, 1))

    def regime(name, test):
        def cov(case, nn, g):
            return {name: (int(test(g)), 1), "share in range (%)": (100 * _share_in_range(nn, *case.ranges[0]), 20),
                    "share out of range (%)": (100 - 100 * _share_in_range(nn, *case.ranges[0]), 5 if name != "a grid of a few cells" else 0)}
        return cov
    return [
        Case("range_3mm_cell_clamped", near(scene, 1500, 0.006), scene, [(0, 0.003), (1, 0.003 ** 2)], None,
             regime("the cell is the clamp", lambda g: g["cell"] == F(0.25) and F(0.003 * 0.25) <= F(1e-3)), "nn_cell_for: the clamp"),
        Case("range_50m_few_cells", scene[rng.permutation(2500)[:1500]] + rng.normal(0, 3.0, (1500, 3)), scene, [(0, 50.0), (1, 2500.0)], None,
             regime("a grid of a few cells", lambda g: max(g["dims"]) <= 4 and g["cell"] == F(12.5)), "a grid of a few cells"),
        Case("range_4.5mm_cell_grown", near(wide, 3000, 0.009), wide, [(0, 0.0045), (1, 0.0045 ** 2)], None,
             regime("the cell has grown", lambda g: g["cell"] > F(1.4) * g["nominal_cell"] and g["nominal_cell"] > F(1e-3)
                    and float(np.prod(np.array(g["dims"], float))) <= 2e8), "the bounded table: the cell grows x 1.5"),
    ]


def moved(case, T=None):
    """The same search reached through a transform: 0.3 rad about a skew axis and 25 m of translation; the source is stored
    carried back by its inverse (in double, rounded once), so the transformed points land within rounding of the case's own."""
    T = rigid(0.3, (0.3, -0.5, 0.8), (20.0, -14.0, 5.0)) if T is None else T
    assert abs(np.linalg.norm(T[:3, 3]) - 25.0) < 0.3
    Ti = np.linalg.inv(T)
    src = case.src.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]
    return Case(case.name + "_moved", src, case.tgt, case.ranges, T.astype(F), None, "xform order")


def split1_case(synth):
    """A source of more than 4096 work items (the library's own choice is then SPLIT 1) against a small target."""
    _, maps = synth.synth_maps(2, 330000, overlap_step=0.35)
    src = maps[0][0].astype(F)
    tgt = maps[1][0].astype(F)
    tgt = tgt[np.random.default_rng(11).permutation(len(tgt))[:4000]]
    T = synth.relative_gt(maps[0][2], maps[1][2]).astype(F)

    def cov(case, nn, g):
        return {"source points": (len(case.src), 300000), "work items": (len(hilbert_items(case.src)[1]), 4097), "target points at most 4000": (int(len(case.tgt) <= 4000), 1),
                "share in range (%)": (100 * _share_in_range(nn, 1, 1.0), 10)}
    return Case("production_split1", src, tgt, [(1, 1.0)], T, cov, "k_nn_wave<.., 1> as the library launches it", light=True)


def aimed_cases():
    """Every case that needs neither the oracle nor a large cloud."""
    lat, sp, out = lattice_case(), sparse_case(), outside_case()
    cases = [lat]
    cases += [boundary_case(0, 0.3), boundary_case(0, 0.7), boundary_case(1, 0.1), boundary_case(1, 0.3), boundary_case(1, 0.25)]
    cases += [faces_case(0.0), faces_case(1000.0), faces_case(10000.0)]
    cases += [sp, out, patch_case(), dense_cells_case(), wide_items_case()]
    cases += degenerate_cases() + regime_cases()
    cases += [moved(lat), moved(sp), moved(out)]
    return cases


def all_cases(po, synth):
    return parity_cases(po, synth) + aimed_cases()


# ---------------------------------------------------------------------------------------------- one ICP iteration, in float64
def umeyama64(p, q):
    """Eigen's umeyama (no scaling) in float64: the rigid transform that carries p onto q in the least-squares sense."""
    mp, mq = p.mean(axis=0), q.mean(axis=0)
    sigma = (q - mq).T @ (p - mp) / len(p)
    U, S, Vt = np.linalg.svd(sigma)
    d = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        d[2] = -1.0
    T = np.eye(4)
    T[:3, :3] = U @ np.diag(d) @ Vt
    T[:3, 3] = mq - T[:3, :3] @ mp
    return T


def icp_step64(case, max_corr, swap=None):
    """One ICP iteration from the case's transform over the REFERENCE correspondences: float64 Umeyama of (transformed source,
    nearest target) for d2 <= max_d2, composed with the guess.  swap = a source index whose partner is replaced by its
    second-nearest target.  None with fewer than 3 correspondences."""
    nn = case.nn()
    ok = np.flatnonzero((nn["idx"] >= 0) & (nn["d2"] <= max_d2_of(0, max_corr)))
    if len(ok) < 3:
        return None
    partner = nn["idx"].copy()
    if swap is not None:
        partner[swap] = nn["second"][swap]
    Ti = umeyama64(nn["p"][ok].astype(np.float64), case.tgt[partner[ok]].astype(np.float64))
    return Ti @ case.T.astype(np.float64)


def swap_candidate(case, max_corr):
    """The in-range source point whose second-nearest target lies farthest from its nearest (the swap easiest to see)."""
    nn = case.nn()
    ok = np.flatnonzero((nn["idx"] >= 0) & (nn["second"] >= 0) & (nn["d2"] <= max_d2_of(0, max_corr)))
    gap = np.linalg.norm(case.tgt[nn["second"][ok]].astype(np.float64) - case.tgt[nn["idx"][ok]], axis=1)
    return int(ok[np.argmax(gap)])


def icp_clause_cases(cases):
    """Clause 4's cases: at most 2 000 source points, everything within 30 m of the origin, at least 10 correspondences at the
    case's ICP range and a target that is neither planar nor collinear (a flat moment matrix leaves the rotation to the
    SVD's rank handling, not to the search).  -> [(case, max_corr)]."""
    out = []
    for c in cases:
        icp = [v for k, v in c.ranges if k == 0]
        if not icp or len(c.src) == 0 or len(c.src) > 2000 or len(c.tgt) == 0:
            continue
        if c.name in ("planar_target", "collinear_target", "one_target_point", "non_finite_source_points"):
            continue
        nn = c.nn()
        if np.abs(nn["p"]).max() > 30 or np.abs(c.tgt).max() > 30 or np.abs(c.src).max() > 30:
            continue
        if ((nn["idx"] >= 0) & (nn["d2"] <= max_d2_of(0, icp[0]))).sum() < 10:
            continue
        out.append((c, icp[0]))
    return out

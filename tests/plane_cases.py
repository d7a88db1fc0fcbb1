"""Plane segmentation by RANSAC (mm3d_set_planes): the rule of include/mm3d.h restated in numpy, and the small clouds at which
its kernels can still go wrong.  Shared by test_planes_cpu.py, which checks the restatement, and test_gpu_planes.py, which holds
the device against it.  Needs no GPU and nothing of the library (room_with_person alone asks map_merge_amd.synth for a texture,
through cluster_cases).

Every case has at most 20 000 points and 4 096 draws; the restatement is brute force, samples x m tests in float64, where numpy
rounds every elementwise operation once and fuses nothing."""
import functools
import math

import numpy as np

OFF, REMOVE, SET_ASIDE = 0, 1, 2
NONE, INVALID = -1, -2
GAMMA = np.uint64(0x9E3779B97F4A7C15)
MARGIN = 1e-6                    # a refit case may have no valid point this close to an adopted refit plane's threshold
U = 2.0 ** -6                    # the lattice of the exact cases


def options(**kw):
    """mm3d_plane_options_default's values (the method apart), with the given ones in their place."""
    o = dict(max_planes=1, samples=1024, refit=1, seed=1, distance=0.05, min_fraction=0.05, axis=(0.0, 0.0, 1.0), max_angle_deg=10.0)
    assert set(kw) <= set(o), kw
    o.update(kw)
    return o


# ---------------------------------------------------------------- the restatement
def mix(z):
    """splitmix64's finaliser on uint64 arrays (numpy's unsigned arithmetic wraps, as the rule's mod 2^64 does)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def bounded(w, n):
    return ((w >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)


def draw_ranks(seed, p, samples, m):
    """Step 4: three distinct ranks below m for every draw h, int64 [samples] each."""
    with np.errstate(over="ignore"):
        base = np.uint64((int(seed) << 32) | (int(p) << 24)) + np.arange(samples, dtype=np.uint64)
        w = [mix(base + np.uint64(j + 1) * GAMMA) for j in range(3)]
    i0 = bounded(w[0], m).astype(np.int64)
    i1 = bounded(w[1], m - 1).astype(np.int64)
    i1 += i1 >= i0
    i2 = bounded(w[2], m - 2).astype(np.int64)
    lo, hi = np.minimum(i0, i1), np.maximum(i0, i1)
    i2 += i2 >= lo
    i2 += i2 >= hi
    return i0, i1, i2


def dot3(x, y, z, a, b, c):
    return (x * a + y * b) + z * c


def hypotheses(q, ranks, o):
    """Step 5 for the records q float64 [m][3] of R_p: (a [s][3], nrm [s][3], len2 [s], degenerate [s], off_axis [s])."""
    i0, i1, i2 = ranks
    a, b, c = q[i0], q[i1], q[i2]
    u, v = b - a, c - a
    nrm = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
    len2 = dot3(nrm[:, 0], nrm[:, 1], nrm[:, 2], nrm[:, 0], nrm[:, 1], nrm[:, 2])
    uu = dot3(u[:, 0], u[:, 1], u[:, 2], u[:, 0], u[:, 1], u[:, 2])
    vv = dot3(v[:, 0], v[:, 1], v[:, 2], v[:, 0], v[:, 1], v[:, 2])
    degenerate = ~(len2 > 1e-12 * (uu * vv))
    ax = np.asarray(o["axis"], dtype=np.float64)
    off_axis = np.zeros(len(a), dtype=bool)
    if ax.any():
        dn = dot3(nrm[:, 0], nrm[:, 1], nrm[:, 2], ax[0], ax[1], ax[2])
        off_axis = ~degenerate & ~(dn * dn >= (cos2(o) * len2) * dot3(ax[0], ax[1], ax[2], ax[0], ax[1], ax[2]))
    return a, nrm, len2, degenerate, off_axis


def cos2(o):
    c = math.cos(o["max_angle_deg"] * math.pi / 180.0)          # the host's libm, as the library takes it
    return c * c


def votes(q, a, nrm, rhs):
    """Step 6 for one hypothesis: bool [m]."""
    d = q - a[None, :]
    s = dot3(nrm[0], nrm[1], nrm[2], d[:, 0], d[:, 1], d[:, 2])
    return s * s <= rhs


def counts(q, a, nrm, rhs, chunk=96):
    """Step 6 for every hypothesis: int64 [s]; rhs = -1 marks a draw without a count (it gets 0 here and is never looked at)."""
    out = np.zeros(len(a), dtype=np.int64)
    live = np.nonzero(rhs >= 0.0)[0]
    for k in range(0, len(live), chunk):
        h = live[k:k + chunk]
        dx = q[None, :, 0] - a[h, None, 0]
        dy = q[None, :, 1] - a[h, None, 1]
        dz = q[None, :, 2] - a[h, None, 2]
        s = (nrm[h, None, 0] * dx + nrm[h, None, 1] * dy) + nrm[h, None, 2] * dz
        out[h] = (s * s <= rhs[h, None]).sum(axis=1)
    return out


def orient(n, o):
    """Step 9's sign."""
    ax = np.asarray(o["axis"], dtype=np.float64)
    if ax.any():
        flip = dot3(n[0], n[1], n[2], ax[0], ax[1], ax[2]) < 0.0
    else:
        flip = n[2] < 0.0 or (n[2] == 0.0 and (n[1] < 0.0 or (n[1] == 0.0 and n[0] < 0.0)))
    return -n if flip else n


def refit(q, a, inl, o):
    """Step 8's matrix part: (n', c, ok) from the inliers' sums about a.  The sums are numpy's (pairwise): the device's fixed
    order gives other last bits, which is what the tests' 1e-9 bounds are for."""
    d = q[inl] - a[None, :]
    N = float(len(d))
    mu = d.sum(axis=0) / N
    C = (d[:, :, None] * d[:, None, :]).sum(axis=0) / N - mu[:, None] * mu[None, :]
    w, V = np.linalg.eigh(C)
    n = orient(V[:, 0], o)
    c = a + mu
    trace = (C[0, 0] + C[1, 1]) + C[2, 2]
    ok = bool(trace > 0.0 and (w[1] - w[0]) > 1e-6 * trace and np.isfinite(n).all() and np.isfinite(c).all() and np.isfinite(w).all())
    ax = np.asarray(o["axis"], dtype=np.float64)
    if ok and ax.any():
        dn = dot3(n[0], n[1], n[2], ax[0], ax[1], ax[2])
        ok = bool(dn * dn >= cos2(o) * dot3(ax[0], ax[1], ax[2], ax[0], ax[1], ax[2]))
    return n, c, ok


def refit_distance(q, n, c):
    d = q - c[None, :]
    return np.abs(dot3(n[0], n[1], n[2], d[:, 0], d[:, 1], d[:, 2]))


def segment(xyz, o):
    """The whole rule: dict(labels int32 [n], planes [dict], stats dict, margin int, winners [(count, h)], found).  margin counts,
    over the rounds whose refit was adopted, the records of R_p within MARGIN of the refit plane's threshold; found holds, per
    plane, (the records of R_p, the winner's a, its inliers among them) for whoever wants to work a round again."""
    x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = len(x)
    valid = np.isfinite(x).all(axis=1)
    labels = np.where(valid, NONE, INVALID).astype(np.int32)
    n_valid = int(valid.sum())
    T = max(3, math.ceil(o["min_fraction"] * float(n_valid)))
    dist = float(o["distance"])
    st = dict(points=n, valid=n_valid, on_planes=0, kept=n_valid, draws=0, degenerate=0, off_axis=0, planes=0, rounds=0)
    planes, winners, found, margin = [], [], [], 0
    for p in range(o["max_planes"]):
        idx = np.nonzero(labels == NONE)[0]
        m = len(idx)
        if m < 3:
            break
        q = x[idx].astype(np.float64)
        a, nrm, len2, degenerate, off_axis = hypotheses(q, draw_ranks(o["seed"], p, o["samples"], m), o)
        st["rounds"] += 1
        st["draws"] += o["samples"]
        st["degenerate"] += int(degenerate.sum())
        st["off_axis"] += int(off_axis.sum())
        rhs = np.where(degenerate | off_axis, -1.0, (dist * dist) * len2)
        cnt = counts(q, a, nrm, rhs)
        live = rhs >= 0.0
        if not live.any():
            break
        h = int(np.argmax(np.where(live, cnt, -1)))                 # (argmax takes the first of equals: the lower h)
        winners.append((int(cnt[h]), h))
        if cnt[h] < T:
            break
        inl = votes(q, a[h], nrm[h], rhs[h])
        normal = orient(nrm[h] / math.sqrt(len2[h]), o)
        through, adopted = a[h], 0
        found.append((idx, a[h].copy(), inl.copy()))
        if o["refit"]:
            n2, c2_, ok = refit(q, a[h], inl, o)
            if ok:
                dist2 = refit_distance(q, n2, c2_)
                inl2 = dist2 <= dist
                if inl2.sum() >= inl.sum():
                    normal, through, inl, adopted = n2, c2_, inl2, 1
                    margin += int((np.abs(dist2 - dist) <= MARGIN).sum())
        labels[idx[inl]] = p
        planes.append(dict(normal=tuple(float(v) for v in normal), d=float(-dot3(normal[0], normal[1], normal[2], through[0], through[1], through[2])),
                           inliers=int(inl.sum()), draw=h, refit=adopted))
        st["planes"] += 1
        st["on_planes"] += int(inl.sum())
    st["kept"] = n_valid - st["on_planes"]
    return dict(labels=labels, planes=planes, stats=st, margin=margin, winners=winners, found=found)


# ---------------------------------------------------------------- the clouds
def _lattice_sheet(nx, ny, z, x0=0, y0=0):
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return np.stack([(x0 + i.ravel()) * U, (y0 + j.ravel()) * U, np.full(i.size, z * U)], axis=1)


def two_parallel_planes():
    """Two 32 x 32 sheets of the 2^-6 lattice one metre apart, shuffled together: every draw within one sheet counts exactly
    1 024, whichever sheet, so the lower h decides; the second round finds the other sheet."""
    xyz = np.concatenate([_lattice_sheet(32, 32, 0), _lattice_sheet(32, 32, 64)])
    return xyz[np.random.default_rng(31).permutation(len(xyz))].astype(np.float32)


THRESHOLD_DISTANCE = 2.0 ** -4


def threshold():
    """A 24 x 24 lattice sheet at z = 0, 40 records exactly 2^-4 above or below it (inliers: <= decides) and 40 one lattice step
    beyond (not inliers).  Every product of the rule is exact here."""
    rng = np.random.default_rng(32)
    sheet = _lattice_sheet(24, 24, 0)
    at = sheet[rng.choice(len(sheet), 40, replace=False)].copy()
    at[:, 2] = np.where(np.arange(40) % 2 == 0, 4, -4) * U
    beyond = sheet[rng.choice(len(sheet), 40, replace=False)].copy()
    beyond[:, 2] = np.where(np.arange(40) % 2 == 0, 5, -5) * U
    xyz = np.concatenate([sheet, at, beyond])
    kind = np.r_[np.zeros(len(sheet), dtype=int), np.ones(40, dtype=int), np.full(40, 2)]
    perm = rng.permutation(len(xyz))
    return xyz[perm].astype(np.float32), kind[perm]


def collinear():
    k = np.random.default_rng(33).permutation(500)
    return (np.stack([k, 2 * k, 3 * k], axis=1) * U).astype(np.float32)


def duplicates():
    return np.tile(np.array([[1.25, -0.5, 2.0]], dtype=np.float32), (300, 1))


def floor_and_clutter(n, seed, offset=(0.0, 0.0, 0.0)):
    """n points: 45 % on a floor z = 0.3 jittered by a centimetre, 25 % on a wall x = 0.2, the rest uniform in the 6 x 5 x 3 box."""
    rng = np.random.default_rng(seed)
    nf, nw = (45 * n) // 100, (25 * n) // 100
    floor = np.stack([rng.uniform(0, 6, nf), rng.uniform(0, 5, nf), 0.3 + rng.uniform(-0.01, 0.01, nf)], axis=1)
    wall = np.stack([0.2 + rng.uniform(-0.01, 0.01, nw), rng.uniform(0, 5, nw), rng.uniform(0, 3, nw)], axis=1)
    rest = rng.uniform(0, 1, (n - nf - nw, 3)) * np.array([6.0, 5.0, 3.0])
    xyz = np.concatenate([floor, wall, rest]) + np.asarray(offset)[None, :]
    return xyz[rng.permutation(n)].astype(np.float32)


def with_invalid_rows():
    """2 000 points of floor_and_clutter with NaN, +inf and -inf in each coordinate, the first and the last record among them."""
    xyz = floor_and_clutter(2000, 34).copy()
    bad = [np.nan, np.inf, -np.inf]
    for k, r in enumerate([0, 1999, 17, 18, 19, 101, 150, 151, 250, 1000, 1001, 1500]):
        xyz[r, k % 3] = bad[(k // 3) % 3]
    xyz[77] = (np.nan, np.inf, -np.inf)
    return xyz


ROOM_SIDES = [((0.0, 0.0, 1.0), (2.5, 2.0, 0.0)), ((0.0, 0.0, 1.0), (2.5, 2.0, 3.0)), ((1.0, 0.0, 0.0), (0.0, 2.0, 1.5)),
              ((1.0, 0.0, 0.0), (5.0, 2.0, 1.5)), ((0.0, 1.0, 0.0), (2.5, 0.0, 1.5)), ((0.0, 1.0, 0.0), (2.5, 4.0, 1.5))]   # (normal, centre) of box_room's sides
ROOM_DISTANCE = 0.02            # the room cases' distance: a centimetre of jitter and a centimetre of slack, so that a winner lies within
                                # 0.02 m and a degree of its side whatever three records made it


def which_room_side(plane, offset=(0.0, 0.0, 0.0), d_tol=0.02, deg_tol=1.0):
    """The index in ROOM_SIDES of the side of box_room(offset) that `plane` (a dict with normal and d) is: its normal within
    deg_tol degrees of the side's, and the side's centre within d_tol metres of it.  Raises when it is none of them."""
    n = np.array(plane["normal"], dtype=np.float64)
    for k, (rn, rc) in enumerate(ROOM_SIDES):
        angle = math.degrees(math.acos(min(1.0, abs(float(np.dot(n, np.array(rn)))))))
        if angle <= deg_tol and abs(float(np.dot(n, np.array(rc) + np.array(offset))) + plane["d"]) <= d_tol:
            return k
    raise AssertionError(("not a side of the room", plane))


def box_room(seed, offset=(0.0, 0.0, 0.0), clutter=0):
    """A closed room of 5 x 4 x 3 m -- floor, ceiling, four walls -- sampled on a 0.1 m lattice jittered by a centimetre in every
    direction (about 9 400 points), with `clutter` uniform points inside; offset is added before the rounding to float32."""
    rng = np.random.default_rng(seed)
    g = lambda n: (np.arange(n) + 0.5) * 0.1                                     # noqa: E731
    parts = []
    for axis, (na, nb), where in ((2, (50, 40), (0.0, 3.0)), (0, (40, 30), (0.0, 5.0)), (1, (50, 30), (0.0, 4.0))):
        others = [k for k in range(3) if k != axis]
        i, j = np.meshgrid(g(na), g(nb), indexing="ij")
        for w in where:
            p = np.zeros((i.size, 3))
            p[:, others[0]], p[:, others[1]], p[:, axis] = i.ravel(), j.ravel(), w
            parts.append(p)
    xyz = np.concatenate(parts)
    xyz = xyz + rng.uniform(-0.01, 0.01, xyz.shape)
    if clutter:
        xyz = np.concatenate([xyz, 0.3 + rng.uniform(0, 1, (clutter, 3)) * np.array([4.4, 3.4, 2.4])])
    xyz = xyz + np.asarray(offset)[None, :]
    return xyz[rng.permutation(len(xyz))].astype(np.float32)


def tilted_slab():
    """A floor of 3 000 points and a slab of 5 000 tilted by 20 degrees about x, a metre above it: the slab holds more points,
    but lies outside the 10 degrees about the axis, so the floor wins."""
    rng = np.random.default_rng(36)
    floor = np.stack([rng.uniform(0, 6, 3000), rng.uniform(0, 5, 3000), rng.uniform(-0.01, 0.01, 3000)], axis=1)
    t = np.radians(20.0)
    u, v, w = rng.uniform(0, 6, 5000), rng.uniform(0, 5, 5000), rng.uniform(-0.01, 0.01, 5000)
    slab = np.stack([u, v * np.cos(t) - w * np.sin(t), 1.0 + v * np.sin(t) + w * np.cos(t)], axis=1)
    xyz = np.concatenate([floor, slab])
    is_floor = np.r_[np.ones(3000, dtype=bool), np.zeros(5000, dtype=bool)]
    perm = rng.permutation(len(xyz))
    return xyz[perm].astype(np.float32), is_floor[perm]


AT_T_PLANE, AT_T_POINTS = 384, 1024                    # 384 / 1024 and 385 / 1024 are dyadic: min_fraction * n_valid is exact


def at_threshold():
    """384 lattice points on z = 0 and 640 scattered above them between z = 1 and z = 9, within 3 m in x and y: a plane through
    a sheet point and one of those is steeper than 13 degrees, off the axis, and the scattered ones alone gather about eight to a
    plane.  The winner counts exactly 384, which is T for min_fraction 384 / 1024 and T - 1 for 385 / 1024."""
    rng = np.random.default_rng(37)
    sheet = _lattice_sheet(24, 16, 0)
    rest = np.stack([rng.uniform(0, 3, 640), rng.uniform(0, 3, 640), rng.uniform(1, 9, 640)], axis=1)
    xyz = np.concatenate([sheet, rest])
    return xyz[rng.permutation(len(xyz))].astype(np.float32)


COLUMN_RADIUS, COLUMN_HEIGHT = 0.22, 1.7


def room_with_person(seed, yaw=0.0, shift=(0.0, 0.0, 0.0)):
    """cluster_cases.room_with_blobs plus a solid column of 0.22 m radius and 1.7 m height standing on the floor: through the
    floor it is connected to every wall, so the cluster filter alone cannot remove it.  Returns (xyz float32, rgb uint8,
    is_blob, is_column), the column's records last before the shuffle of this function."""
    import cluster_cases as cc
    from map_merge_amd import synth
    xyz, rgb, is_blob, _ = cc.room_with_blobs(seed)                      # (unrotated: the column is placed in the room's frame)
    rng = np.random.default_rng(300 + seed)
    centre = np.array([6.4, 1.6]) + rng.uniform(-0.2, 0.2, 2)
    g = (np.arange(-5, 6) + 0.5) * 0.05
    zz = (np.arange(int(COLUMN_HEIGHT / 0.05)) + 0.5) * 0.05
    col = np.stack(np.meshgrid(g, g, zz, indexing="ij"), axis=-1).reshape(-1, 3)
    col = col[np.hypot(col[:, 0], col[:, 1]) <= COLUMN_RADIUS]
    col[:, :2] += np.floor(centre / 0.1) * 0.1
    col = col + rng.uniform(-0.01, 0.01, col.shape)
    col_rgb = synth._texture(col, np.array([90.0, 110.0, 160.0]), 70 + seed)
    xyz = np.concatenate([xyz.astype(np.float64), col])
    rgb = np.concatenate([rgb, col_rgb])
    is_blob = np.r_[is_blob, np.zeros(len(col), dtype=bool)]
    is_column = np.r_[np.zeros(len(is_blob) - len(col), dtype=bool), np.ones(len(col), dtype=bool)]
    c, s = np.cos(yaw), np.sin(yaw)
    xyz = xyz @ np.array([[c, s, 0], [-s, c, 0], [0, 0, 1.0]]) + np.asarray(shift)[None, :]
    perm = rng.permutation(len(xyz))
    return xyz[perm].astype(np.float32), rgb[perm], is_blob[perm], is_column[perm]


PERSON_OPTIONS = dict(distance=0.05, samples=1024)      # the issue's setting for case (l): axis z within 10 degrees, one plane


def voxel_centroids(xyz, leaf=0.1, flags=None):
    """One centroid per occupied voxel (float64 sums, float32 result), in the voxels' sorted order: what a 0.1 m voxel pass leaves,
    near enough for the properties test_planes_cpu.py asserts (the GPU tests take the library's own pass).  With flags, also
    whether any member of the voxel carried the flag."""
    key = np.floor(xyz.astype(np.float64) / leaf).astype(np.int64)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.ravel()
    out = np.zeros((len(cnt), 3))
    np.add.at(out, inv, xyz.astype(np.float64))
    out = (out / cnt[:, None]).astype(np.float32)
    if flags is None:
        return out
    any_flag = np.zeros(len(cnt), dtype=bool)
    np.logical_or.at(any_flag, inv, flags)
    return out, any_flag


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (xyz float32 [n][3], options, refit_too): every case is checked with refit = 0, and with refit = 1 as well where
    refit_too says that no point lies within MARGIN of an adopted refit plane's threshold (test_planes_cpu.py asserts that).
    Made once, never written to."""
    none = (0.0, 0.0, 0.0)
    room = dict(axis=none, max_planes=6, samples=1024, distance=ROOM_DISTANCE)
    tri = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [0.0, 1.0, 0.5], [5.0, 5.0, 5.0]], dtype=np.float32)
    out = {
        "a_two_parallel_planes": (two_parallel_planes(), options(max_planes=2, samples=64, distance=THRESHOLD_DISTANCE), False),
        "b_threshold": (threshold()[0], options(samples=256, distance=THRESHOLD_DISTANCE), False),
        "c_collinear": (collinear(), options(samples=65, axis=none), False),
        "c_duplicates": (duplicates(), options(samples=65), False),
        "d_invalid_rows": (with_invalid_rows(), options(max_planes=2, samples=300), True),
        "e_0_points": (tri[:0], options(axis=none, samples=8), True),
        "e_1_point": (tri[:1], options(axis=none, samples=8), True),
        "e_2_points": (tri[:2], options(axis=none, samples=8), True),
        "e_3_points": (tri[:3], options(axis=none, samples=8, min_fraction=1.0), False),
        "g_room_6": (box_room(35), options(**room), True),
        "h_room_8": (box_room(38, clutter=300), options(**dict(room, max_planes=8)), True),
        "i_tilted_slab": (tilted_slab()[0], options(samples=512), True),
        "j_at_T": (at_threshold(), options(samples=512, min_fraction=AT_T_PLANE / AT_T_POINTS), False),
        "j_below_T": (at_threshold(), options(samples=512, min_fraction=(AT_T_PLANE + 1) / AT_T_POINTS), False),
        "k_room_at_1km": (box_room(35, (1000.0, 1000.0, 0.0)), options(**room), True),
        "k_room_at_10km": (box_room(35, (10000.0, -10000.0, 0.0)), options(**room), True),
    }
    for n in (4097, 16385):                                  # (f): the edges of waves, blocks and hypothesis tiles
        for samples in (1, 65, 1000, 4096):
            out["f_%d_points_%d_draws" % (n, samples)] = (floor_and_clutter(n, 40 + samples % 7), options(max_planes=2, samples=samples, seed=n + samples), True)
    for xyz, o, _ in out.values():
        assert xyz.dtype == np.float32 and len(xyz) <= 20000 and o["samples"] <= 4096
        xyz.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, refit):
    """segment() of a case with the given refit: computed once, never written to."""
    xyz, o, refit_too = cases()[name]
    assert refit == 0 or refit_too, name
    return segment(xyz, dict(o, refit=refit))


def runs():
    """Every (case, refit) the tests go through."""
    return [(name, r) for name, (_, _, refit_too) in sorted(cases().items()) for r in ((0, 1) if refit_too else (0,))]

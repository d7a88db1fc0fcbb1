"""NDT refinement (mm3d_set_refinement, mm3d_estimate_transform_ndt, mm3d_debug_ndt_voxels): the surface, the target's voxel
table voxel by voxel, a numpy restatement of the loop the header states, degenerate inputs, bit-identical results across the
drivers and through the stage-level call, the map cache's key, and the default path untouched."""
import numpy as np
import pytest

from test_gpu_icp_plane import _ldlt_solve, _problem, _records, _xform_f32, box_room, construct_transform

pytestmark = pytest.mark.gpu

ICP, NDT = 0, 1
SAC_IA, MATCHING = 1, 0
EINVAL, EUNSUPPORTED = -1, -4
DEFAULT_MULTIPLE = 10.0          # resolution = 0 means this times params.resolution (include/mm3d.h)


# ---------------------------------------------------------------- the restatement (also read by test_ndt_cpu.py)
def voxel_of(xyz, resolution):
    """(floorf(x * inv), ...) with inv = 1.0f / (float)resolution, every step one float operation."""
    inv = np.float32(1.0) / np.float32(resolution)
    return np.floor((xyz.astype(np.float32) * inv).astype(np.float32)).astype(np.int64)


def restate_table(tgt, resolution, min_points=6, kappa=0.01):
    """The voxel table of include/mm3d.h in numpy, everything in double: {(i, j, k): (count, mean, P or None)} in ascending
    (i, j, k); P = the inverse of the regularised covariance as (xx xy xz yy yz zz)."""
    fin = np.isfinite(tgt).all(axis=1)
    pts = tgt[fin].astype(np.float32)
    ijk = voxel_of(pts, resolution)
    order = np.lexsort((ijk[:, 2], ijk[:, 1], ijk[:, 0]))           # stable: ascending input index inside a voxel
    ijk, pts = ijk[order], pts[order].astype(np.float64)
    heads = np.flatnonzero(np.r_[True, (np.diff(ijk, axis=0) != 0).any(axis=1)])
    table = {}
    for a, b in zip(heads, np.r_[heads[1:], len(pts)]):
        p = pts[a:b]
        cnt = b - a
        mu = p.sum(axis=0) / cnt
        P = None
        if cnt >= min_points:
            d = p - mu
            S = (d.T @ d) / (cnt - 1)
            trace = S[0, 0] + S[1, 1] + S[2, 2]
            S = S + kappa * (trace / 3.0) * np.eye(3)
            xx, xy, xz, yy, yz, zz = S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]
            a00, a01, a02 = yy * zz - yz * yz, xz * yz - xy * zz, xy * yz - xz * yy
            a11, a12, a22 = xx * zz - xz * xz, xy * xz - xx * yz, xx * yy - xy * xy
            det = xx * a00 + xy * a01 + xz * a02
            with np.errstate(all="ignore"):
                cand = np.array([a00, a01, a02, a11, a12, a22]) / det
            if trace > 0.0 and np.isfinite(cand.astype(np.float32)).all() and np.isfinite(mu.astype(np.float32)).all():
                P = cand
        table[tuple(int(v) for v in ijk[a])] = (int(cnt), mu, P)
    return table


_OFFSETS = [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]


def restate_ndt(src, tgt, guess, resolution, neighbours=7, min_points=6, kappa=0.01, max_iter=30, eps=1e-9, tau=1e-12, table=None):
    """The loop of include/mm3d.h (mm3d_set_refinement) in numpy: float32 transforms and voxel indices, mu and P rounded to
    float once, double terms, sums and solve.  Returns (T, iterations, converged, margins, points with a term in the last
    iteration): margins = the relative distances of every convergence test from its threshold and of every pivot from the
    degeneracy floor."""
    table = restate_table(tgt, resolution, min_points, kappa) if table is None else table
    keys = [k for k, v in table.items() if v[2] is not None]
    mu = np.array([table[k][1] for k in keys]).astype(np.float32).astype(np.float64).reshape(-1, 3)
    P6 = np.array([table[k][2] for k in keys]).astype(np.float32).astype(np.float64).reshape(-1, 6)
    lookup = {k: n for n, k in enumerate(keys)}
    src = src[np.isfinite(src).all(axis=1)].astype(np.float32)
    T = np.asarray(guess, dtype=np.float32).copy()
    prev, iters, margins, n_pts = np.finfo(np.float64).max, 0, [], 0
    while True:
        s32 = _xform_f32(T, src)
        own = voxel_of(s32, resolution)
        s = s32.astype(np.float64)
        A, bq = np.zeros((len(s), 3, 3)), np.zeros((len(s), 3))
        wsum, terms = 0.0, np.zeros(len(s), dtype=np.int64)
        for off in _OFFSETS[:neighbours]:
            vid = np.array([lookup.get((i + off[0], j + off[1], k + off[2]), -1) for i, j, k in own.tolist()])
            rows = np.flatnonzero(vid >= 0)
            if not len(rows):
                continue
            p = P6[vid[rows]]
            Pm = np.stack([p[:, [0, 1, 2]], p[:, [1, 3, 4]], p[:, [2, 4, 5]]], axis=1)
            q = s[rows] - mu[vid[rows]]
            u = np.einsum("nij,nj->ni", Pm, q)
            with np.errstate(all="ignore"):
                m = np.einsum("ni,ni->n", q, u)
                ok = np.isfinite(m)
                w = np.where(ok, np.exp(-0.5 * np.where(ok, m, 0.0)), 0.0)
            A[rows] += w[:, None, None] * np.where(ok[:, None, None], Pm, 0.0)
            bq[rows] += w[:, None] * np.where(ok[:, None], u, 0.0)
            wsum += float(w.sum())
            terms[rows] += ok
        n_pts = int((terms > 0).sum())
        J = np.zeros((len(s), 3, 6))
        sx, sy, sz = s[:, 0], s[:, 1], s[:, 2]
        J[:, 1, 0], J[:, 2, 0] = -sz, sy
        J[:, 0, 1], J[:, 2, 1] = sz, -sx
        J[:, 0, 2], J[:, 1, 2] = -sy, sx
        J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
        H = np.einsum("nij,nik,nkl->jl", J, A, J)
        g = -np.einsum("nij,ni->j", J, bq)
        floor = tau * np.trace(H) / 6.0
        x, pivots = _ldlt_solve(H, g, floor) if terms.sum() >= 6 else (None, [])
        margins += [abs(p - floor) / max(abs(floor), 1e-300) for p in pivots]
        if x is None:
            return T, iters, 0, margins, n_pts
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
            return T, iters, 1, margins, n_pts
        cos_angle = 0.5 * ((float(Ti[0, 0]) + float(Ti[1, 1]) + float(Ti[2, 2])) - 1.0)
        t2 = float(Ti[0, 3]) * float(Ti[0, 3]) + float(Ti[1, 3]) * float(Ti[1, 3]) + float(Ti[2, 3]) * float(Ti[2, 3])
        margins += [abs((1.0 - cos_angle) - eps) / eps, abs(t2 - eps) / eps]
        if cos_angle >= 1.0 - eps and t2 <= eps:
            return T, iters, 1, margins, n_pts
        F = wsum / len(s)
        if iters > 1:                                   # (the first compares with DBL_MAX)
            margins.append(abs(abs(F - prev) - 1e-12) / 1e-12)
        if abs(F - prev) < 1e-12:
            return T, iters, 1, margins, n_pts
        prev = F


# ---------------------------------------------------------------- 1. surface
def test_surface(mm):
    c = mm.Context(0)
    assert c.getRefinement().as_tuple() == (ICP, 0.0, 7, 6, 0.01)
    c.setRefinement(method=NDT, resolution=0.75, neighbours=1, min_points=9, regularisation=0.5)
    assert c.getRefinement().as_tuple() == (NDT, 0.75, 1, 9, 0.5)
    assert c.getIcpMethod() == 0
    c.setIcpMethod(1)
    assert c.getIcpMethod() == 1 and c.getRefinement().method == NDT     # the two settings live side by side
    c.setIcpMethod(0)
    lib = mm.lib()
    import ctypes as C
    bad = [dict(method=-1), dict(method=2), dict(resolution=-1.0), dict(resolution=float("nan")), dict(resolution=float("inf")),
           dict(resolution=1e-45), dict(neighbours=0), dict(neighbours=6), dict(neighbours=27), dict(min_points=3), dict(min_points=-1),
           dict(regularisation=0.0), dict(regularisation=-0.1), dict(regularisation=1.5), dict(regularisation=float("nan"))]
    for kw in bad:
        for method in (ICP, NDT):                       # the values are checked whatever the method
            o = mm.RefineOptions(**{"method": method, **kw})
            assert lib.mm3d_set_refinement(c._h, C.byref(o)) == EINVAL, kw
            assert c.getRefinement().as_tuple() == (NDT, 0.75, 1, 9, 0.5)
    o = mm.RefineOptions()
    assert lib.mm3d_set_refinement(None, C.byref(o)) == EINVAL and lib.mm3d_set_refinement(c._h, None) == EINVAL
    assert lib.mm3d_get_refinement(None, C.byref(o)) == EINVAL and lib.mm3d_get_refinement(c._h, None) == EINVAL
    d = mm.Context(devices=[0])
    assert lib.mm3d_set_refinement(d._h, C.byref(mm.RefineOptions(method=NDT))) == EUNSUPPORTED
    assert d.getRefinement().method == ICP
    d.setRefinement(method=ICP, neighbours=1)           # ICP with other options is still accepted there
    d.close()
    cloud = _records(box_room(1, 2000)[0])
    with pytest.raises(mm.Mm3dError) as e:
        c.shardBegin([cloud, cloud], mm.MapMergingParams(descriptor_type=2), 0, 1)
    assert e.value.status == EUNSUPPORTED
    # the stage-level call wants a resolution of its own
    pts = c.cloud(cloud)
    T = np.zeros(16, dtype=np.float32)
    g = np.eye(4, dtype=np.float32).reshape(16)
    for res in (0.0, -1.0, float("inf")):
        o = mm.RefineOptions(method=NDT)
        o.resolution = res
        assert lib.mm3d_estimate_transform_ndt(c._h, pts._h, pts._h, g.ctypes.data_as(C.c_void_p), C.byref(o), 10, C.c_double(1e-9),
                                               T.ctypes.data_as(C.c_void_p)) == EINVAL
    c.close()


def test_index_limit_is_unsupported(mm):
    c = mm.Context(0)
    far = np.array([[0, 0, 0], [500.0, 500.0, 500.0]] * 4, dtype=np.float32)     # 501^3 > 2^26 cells at 1 m
    with pytest.raises(mm.Mm3dError) as e:
        c.ndtVoxels(c.cloud(_records(far)), method=NDT, resolution=1.0)
    assert e.value.status == EUNSUPPORTED
    c.close()


# ---------------------------------------------------------------- 2. the voxel table, voxel by voxel
def _table_scene(min_points):
    rng = np.random.default_rng(42)
    room = box_room(2, 3000)[0] - np.array([4.0, 3.0, 1.5], dtype=np.float32)      # coordinates straddle 0
    on_planes = rng.uniform(-3, 3, (40, 3)).astype(np.float32)
    on_planes[np.arange(40), np.arange(40) % 3] = rng.integers(-3, 4, 40).astype(np.float32)   # exactly on a lattice plane
    bad = rng.uniform(-3, 3, (20, 3)).astype(np.float32)
    bad[np.arange(20), np.arange(20) % 3] = np.array([np.nan, np.inf, -np.inf, np.nan] * 5, dtype=np.float32)
    few = (np.array([20.5, 20.5, 20.5]) + rng.uniform(-0.3, 0.3, (min_points - 1, 3))).astype(np.float32)
    same = np.tile(np.array([[-20.5, 7.25, -9.5]], dtype=np.float32), (min_points, 1))
    pts = np.concatenate([room, on_planes, bad, few, same])
    return pts[rng.permutation(len(pts))]


def _check_table(mm, pts, min_points, kappa):
    """The device's table of pts at 1 m against the restatement's, voxel by voxel; returns the restatement's."""
    ref = restate_table(pts, 1.0, min_points, kappa)
    c = mm.Context(0)
    got, n = c.ndtVoxels(c.cloud(_records(pts)), method=NDT, resolution=1.0, min_points=min_points, regularisation=kappa)
    c.close()
    keys = list(ref)
    assert n == len(keys) and [tuple(r) for r in got["ijk"].tolist()] == keys        # the set, and its ascending order
    assert got["count"].tolist() == [ref[k][0] for k in keys]
    assert got["valid"].tolist() == [ref[k][2] is not None for k in keys]
    for row, k in enumerate(keys):
        cnt, mu, P = ref[k]
        ulp = np.spacing(np.abs(mu.astype(np.float32)))
        assert (np.abs(got["mean"][row].astype(np.float64) - mu) <= 2.0 * ulp).all(), (k, got["mean"][row], mu)
        if P is None:
            assert not got["icov"][row].any()
        else:
            tol = 4.0 * 2.0 ** -24 * np.abs(P).max()
            assert (np.abs(got["icov"][row].astype(np.float64) - P) <= tol).all(), (k, got["icov"][row], P)
    return ref


@pytest.mark.parametrize("min_points,kappa", [(6, 0.01), (4, 1.0)])
def test_voxel_table_voxel_by_voxel(mm, min_points, kappa):
    ref = _check_table(mm, _table_scene(min_points), min_points, kappa)
    assert (20, 20, 20) in ref and ref[(20, 20, 20)][0] == min_points - 1 and ref[(20, 20, 20)][2] is None
    assert ref[(-21, 7, -10)][0] == min_points and ref[(-21, 7, -10)][2] is None     # coincident points: trace 0
    assert sum(v[2] is not None for v in ref.values()) > 100


def test_voxel_table_when_blocks_of_the_range_launch_count_nothing(mm):
    """4 100 rows make the index-range launch three blocks.  Every row below 4 096 has a coordinate that is not a number, so the
    four finite rows fall to one block and the other two count nothing; then no row is finite, no block counts anything, the
    range words keep their initial values and the table has no voxel."""
    rng = np.random.default_rng(9)
    pts = rng.uniform(-40, 40, (4100, 3)).astype(np.float32)
    pts[np.arange(4096), np.arange(4096) % 3] = np.array([np.nan, np.inf, -np.inf, np.nan] * 1024, dtype=np.float32)
    pts[4096:] = [[2.2, -2.9, 0.1], [2.7, -2.3, 0.6], [2.4, -2.5, 0.9], [2.8, -2.8, 0.3]]    # min_points of them in voxel (2, -3, 0)
    ref = _check_table(mm, pts, 4, 0.01)
    assert list(ref) == [(2, -3, 0)] and ref[(2, -3, 0)][0] == 4 and ref[(2, -3, 0)][2] is not None
    pts[4096:, 2] = np.nan
    c = mm.Context(0)
    got, n = c.ndtVoxels(c.cloud(_records(pts)), method=NDT, resolution=1.0, min_points=4)
    c.close()
    assert n == 0 and all(len(v) == 0 for v in got.values())


# ---------------------------------------------------------------- 3. against the restatement
def _against_restatement(mm, seed, neighbours, nan_rows=0, outside=False):
    tgt, _, src, _, guess = _problem(seed, 5000)
    rng = np.random.default_rng(seed + 7)
    if nan_rows:
        src = src.copy()
        src[rng.choice(len(src), nan_rows, replace=False), rng.integers(0, 3, nan_rows)] = np.nan
    if outside:                                          # a third of the source far outside the table
        src = src.copy()
        src[rng.choice(len(src), len(src) // 3, replace=False)] += np.float32(300.0)
    res, max_iter, eps = 1.0, 30, 1e-9
    T_ref, it_ref, conv_ref, margins, n_ref = restate_ndt(src, tgt, guess, res, neighbours, max_iter=max_iter, eps=eps)
    assert it_ref >= 2
    assert min(margins) > 0.01, "the restatement sits within 1 % of a threshold: the comparison would be borderline"
    c = mm.Context(0)
    T = c.estimateTransformNDT(c.cloud(_records(src)), c.cloud(_records(tgt)), guess, method=NDT, resolution=res, neighbours=neighbours,
                               max_iterations=max_iter, transformation_epsilon=eps)
    assert (c.last_icp_iterations, c.last_icp_converged) == (it_ref, conv_ref)
    assert np.abs(T - T_ref).max() < 1e-4, np.abs(T - T_ref).max()
    c.close()


@pytest.mark.parametrize("neighbours", [1, 7])
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_against_restatement(mm, seed, neighbours):
    _against_restatement(mm, seed, neighbours)


def test_non_finite_source_points_are_skipped(mm):
    _against_restatement(mm, 21, 7, nan_rows=300)


def test_source_points_outside_every_voxel_add_nothing(mm):
    _against_restatement(mm, 22, 7, outside=True)


# ---------------------------------------------------------------- 4. degenerate
def test_fewer_than_six_terms_stops_with_the_guess(mm):
    tgt, _, src, _, guess = _problem(5, 5000)
    src = (src + np.float32(500.0)).astype(np.float32)   # outside the table ...
    inside = np.linalg.inv(guess.astype(np.float64)) @ np.array([[1.5, 1.5, 0.02, 1.0], [3.5, 2.5, 0.02, 1.0], [5.5, 4.5, 0.02, 1.0]]).T
    src[:3] = inside.T[:, :3].astype(np.float32)         # ... but for three points on the floor: three terms with one voxel each
    ref = restate_ndt(src, tgt, guess, 1.0, 1)
    assert (ref[1], ref[2], ref[4]) == (0, 0, 3)
    c = mm.Context(0)
    T = c.estimateTransformNDT(c.cloud(_records(src)), c.cloud(_records(tgt)), guess, method=NDT, resolution=1.0, neighbours=1,
                               max_iterations=30, transformation_epsilon=1e-9)
    assert (c.last_icp_iterations, c.last_icp_converged) == (0, 0)
    assert np.array_equal(T.view(np.uint32), guess.view(np.uint32))
    c.close()


def test_single_plane_is_not_degenerate(mm):
    # test_gpu_icp_plane.py's scene.  The regularisation makes every P full rank, so H is too: the loop runs.
    rng = np.random.default_rng(5)
    tgt = np.c_[rng.uniform(0, 5, (4000, 2)), np.zeros(4000)].astype(np.float32)
    src = (tgt + np.array([0.05, -0.03, 0.02], dtype=np.float32)).astype(np.float32)
    guess = np.eye(4, dtype=np.float32)
    guess[:3, 3] = [0.01, 0.01, -0.01]
    _, it_ref, conv_ref, _, _ = restate_ndt(src, tgt, guess, 1.0, 7)
    assert it_ref >= 1
    c = mm.Context(0)
    T = c.estimateTransformNDT(c.cloud(_records(src)), c.cloud(_records(tgt)), guess, method=NDT, resolution=1.0,
                               max_iterations=30, transformation_epsilon=1e-9)
    assert np.isfinite(T).all()
    assert c.last_icp_converged == conv_ref
    c.close()


# ---------------------------------------------------------------- 5 - 7. drivers, cache, default path
@pytest.fixture(scope="module")
def clouds(synth):
    _, maps = synth.synth_maps(7, 30000, overlap_step=0.4)
    return [synth.pack_points(x, col) for x, col, _ in maps]


def _params(mm, method=SAC_IA, **kw):
    return mm.MapMergingParams(descriptor_type=2, estimation_method=method, **kw)


def _ctx(mm, streams=1, method=NDT, cache=0, method_first=True, **kw):
    c = mm.Context(0)
    if method_first:
        c.setRefinement(method=method, **kw)
    c.setStreams(streams)
    if not method_first:
        c.setRefinement(method=method, **kw)
    if cache:
        c.setMapCache(cache)
    return c


def _run(c, clouds, p, seed=1):
    c.srand(seed)
    T, pairs = c.estimateMapsTransforms(clouds, p, return_pairs=True)
    return np.stack(T), pairs


def _same(a, b):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8))


def test_drivers_and_stage_agree_bit_for_bit(mm, clouds):
    cs = clouds[:6]
    p = _params(mm)
    one = _run(_ctx(mm, 1), cs, p)
    assert one[1]["icp_iterations"].max() > 0 and one[1]["icp_correspondences"].max() > 0
    _same(one, _run(_ctx(mm, 4), cs, p))
    _same(one, _run(_ctx(mm, 4, method_first=False), cs, p))       # set after mm3d_set_streams: the helpers follow
    # resolution 0 is the documented multiple of params.resolution
    _same(one, _run(_ctx(mm, 1, resolution=DEFAULT_MULTIPLE * p.resolution), cs, p))
    assert not np.array_equal(one[0], _run(_ctx(mm, 1, method=ICP), cs, p)[0])
    # the stage-level entry point from each pair's pre-refinement guess (refine off) on the maps' points
    c = _ctx(mm, 1)
    guesses = _run(c, cs, _params(mm, refine_transform=0))[1]
    maps = [c.mapFeatures(c.cloud(x), p) for x in cs]
    for g, r in zip(guesses, one[1]):
        s, t = int(r["source_idx"]), int(r["target_idx"])
        assert (int(g["source_idx"]), int(g["target_idx"])) == (s, t)
        guess = g["transform"].reshape(4, 4).T
        T = c.estimateTransformNDT(maps[s].points, maps[t].points, guess, method=NDT, resolution=DEFAULT_MULTIPLE * p.resolution,
                                   max_iterations=p.max_iterations, transformation_epsilon=p.transform_epsilon)
        assert np.array_equal(T.T.reshape(16).view(np.uint32), r["transform"].view(np.uint32))
        assert c.last_icp_iterations == int(r["icp_iterations"])


@pytest.mark.parametrize("streams", [1, 4])
def test_cache_lockstep(mm, clouds, streams):
    p = _params(mm)
    cached, plain = _ctx(mm, streams, cache=64), _ctx(mm, streams)
    cs = clouds[:6]
    _same(_run(cached, cs, p), _run(plain, cs, p))
    _same(_run(cached, cs, p), _run(plain, cs, p))
    st = cached.mapCacheStats(reset=True)
    assert st["pairs_reused"] > 0 and st["device_bytes"] > 0
    changed = cs[:5] + [clouds[6]]
    _same(_run(cached, changed, p), _run(plain, changed, p))


def test_refinements_never_share_records(mm, clouds):
    cs = clouds[:6]
    p = _params(mm, MATCHING)
    ndt_ref = _run(_ctx(mm, 1), cs, p)
    wide_ref = _run(_ctx(mm, 1, resolution=2.0), cs, p)
    c = _ctx(mm, 1, ICP, cache=64)
    icp = _run(c, cs, p)
    n_pairs = len(icp[1])
    c.mapCacheStats(reset=True)
    # an ICP record is never reused for NDT (this call hits every map, reuses no pair) ...
    c.setRefinement(method=NDT)
    _same(_run(c, cs, p), ndt_ref)
    st = c.mapCacheStats(reset=True)
    assert st["map_hits"] == 6 and st["pairs_reused"] == 0 and st["pairs_computed"] == n_pairs
    # ... nor an NDT record for another resolution (the cached maps' tables are rebuilt) ...
    c.setRefinement(method=NDT, resolution=2.0)
    _same(_run(c, cs, p), wide_ref)
    st = c.mapCacheStats(reset=True)
    assert st["map_hits"] == 6 and st["pairs_reused"] == 0 and st["pairs_computed"] == n_pairs
    # ... and switching back reuses all of them
    c.setRefinement(method=NDT)
    _same(_run(c, cs, p), ndt_ref)
    assert c.mapCacheStats(reset=True)["pairs_reused"] == n_pairs
    c.setRefinement(method=ICP, resolution=2.0)          # (the ICP does not read the options: its records are shared)
    _same(_run(c, cs, p), icp)
    assert c.mapCacheStats(reset=True)["pairs_reused"] == n_pairs


@pytest.mark.parametrize("method", [MATCHING, SAC_IA])
def test_default_untouched(mm, clouds, method):
    cs = clouds[:6]
    p = _params(mm, method)
    fresh = mm.Context(0)
    back = _ctx(mm, 1, NDT)
    ndt = _run(back, cs, p)
    back.setRefinement(method=ICP)
    ref = _run(fresh, cs, p)
    _same(ref, _run(back, cs, p))
    assert not np.array_equal(ndt[0], ref[0])

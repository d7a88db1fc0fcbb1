"""Statistical outlier removal on the device (mm3d_knn_mean_distances, mm3d_remove_outliers_statistical,
mm3d_set_outlier_filter) against the numpy restatement of tests/outlier_cases.py: the surface, the search point by point, the
filter record by record, the option through the whole-map calls (features, streams, cache, shards, device lists), the cache key,
the default path untouched, and the sparse maps the option is for."""
import ctypes as C
import os

import numpy as np
import pytest

import outlier_cases as oc
import test_gpu_uniform_keypoints as ukp

pytestmark = pytest.mark.gpu

FPFH = 2
MATCHING, SAC_IA = 0, 1
RADIUS, STATISTICAL = 0, 1
EINVAL, ECAPACITY = -1, -5


def _records(mm, xyz):
    """Every record its own colour, so that a kept record names the row it came from."""
    a = np.zeros(len(xyz), dtype=mm.POINT)
    a["x"], a["y"], a["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    a["rgba"] = 0xFF000000 + np.arange(len(xyz), dtype=np.uint32) * 3
    return a


# ---------------------------------------------------------------- 1. surface
def test_surface(mm, ctx):
    L = mm.lib()
    c = mm.Context(0)
    assert c.getOutlierFilter().as_tuple() == (RADIUS, 16, 2.0)                  # a fresh context answers the defaults
    assert c.last_outlier_stats == dict(points=0, valid=0, kept=0, k=0, mean=0.0, stddev=0.0, threshold=0.0)
    c.setOutlierFilter(method=STATISTICAL, mean_k=50, stddev_mult=1.0)
    assert c.getOutlierFilter().as_tuple() == (STATISTICAL, 50, 1.0)
    for bad in (dict(method=2), dict(method=-1), dict(mean_k=0), dict(mean_k=65), dict(mean_k=-4), dict(stddev_mult=-0.5),
                dict(stddev_mult=float("nan")), dict(stddev_mult=float("inf")), dict(method=STATISTICAL, mean_k=0),
                dict(method=RADIUS, stddev_mult=-1.0)):                          # (checked whatever the method)
        assert L.mm3d_set_outlier_filter(c._h, C.byref(mm.OutlierOptions(**bad))) == EINVAL, bad
    assert c.getOutlierFilter().as_tuple() == (STATISTICAL, 50, 1.0)            # a refused call changes nothing
    assert L.mm3d_set_outlier_filter(c._h, None) == EINVAL and L.mm3d_get_outlier_filter(c._h, None) == EINVAL
    assert L.mm3d_set_outlier_filter(None, C.byref(mm.OutlierOptions())) == EINVAL
    assert L.mm3d_last_outlier_stats(c._h, None) == EINVAL and L.mm3d_last_outlier_stats(None, C.byref(mm.OutlierStats())) == EINVAL
    c.setOutlierFilter(mm.OutlierOptions())
    assert c.getOutlierFilter().as_tuple() == (RADIUS, 16, 2.0)
    cloud = c.cloud(_records(mm, oc.cases()["h_random_65"][0]))
    empty = c.cloud(np.empty(0, dtype=mm.POINT))
    out, buf = C.c_void_p(), np.zeros(80)
    ptr = buf.ctypes.data_as(C.c_void_p)
    for k in (0, 65, -1):
        assert L.mm3d_knn_mean_distances(c._h, cloud._h, k, ptr, C.c_size_t(80)) == EINVAL, k
        assert L.mm3d_remove_outliers_statistical(c._h, cloud._h, k, C.c_double(1.0), C.byref(out)) == EINVAL, k
        assert L.mm3d_remove_outliers_statistical(c._h, empty._h, k, C.c_double(1.0), C.byref(out)) == EINVAL, k
    for mult in (-1.0, float("nan"), float("inf")):
        assert L.mm3d_remove_outliers_statistical(c._h, cloud._h, 16, C.c_double(mult), C.byref(out)) == EINVAL, mult
    assert L.mm3d_knn_mean_distances(c._h, None, 16, ptr, C.c_size_t(80)) == EINVAL
    assert L.mm3d_knn_mean_distances(c._h, cloud._h, 16, None, C.c_size_t(80)) == EINVAL
    assert L.mm3d_knn_mean_distances(None, cloud._h, 16, ptr, C.c_size_t(80)) == EINVAL
    assert L.mm3d_knn_mean_distances(c._h, cloud._h, 16, ptr, C.c_size_t(64)) == ECAPACITY
    assert L.mm3d_knn_mean_distances(c._h, cloud._h, 16, ptr, C.c_size_t(65)) == 0
    assert L.mm3d_remove_outliers_statistical(c._h, None, 16, C.c_double(1.0), C.byref(out)) == EINVAL
    assert L.mm3d_remove_outliers_statistical(c._h, cloud._h, 16, C.c_double(1.0), None) == EINVAL
    assert L.mm3d_remove_outliers_statistical(None, cloud._h, 16, C.c_double(1.0), C.byref(out)) == EINVAL
    assert len(c.removeOutliersStatistical(empty, 16, 1.0)) == 0 and len(c.knnMeanDistances(empty, 16)) == 0
    assert L.mm3d_knn_mean_distances(c._h, empty._h, 16, ptr, C.c_size_t(0)) == 0
    c.close()
    d = mm.Context(devices=[0])                                                  # a device list accepts the setting
    d.setOutlierFilter(method=STATISTICAL, mean_k=8, stddev_mult=1.5)
    assert d.getOutlierFilter().as_tuple() == (STATISTICAL, 8, 1.5)
    d.close()


# ---------------------------------------------------------------- 2. the search, point by point
@pytest.fixture(scope="module")
def clouds(mm, ctx):
    """Every case's records and its device cloud, uploaded once."""
    out = {}
    for name, (xyz, _) in oc.cases().items():
        recs = _records(mm, xyz)
        out[name] = (recs, ctx.cloud(recs))
    return out


@pytest.mark.parametrize("name", sorted(oc.cases()))
def test_mean_distances_point_by_point(mm, ctx, clouds, name):
    for mean_k in oc.MEAN_KS:
        want, valid, k = oc.reference_distances(name, mean_k)
        got = ctx.knnMeanDistances(clouds[name][1], mean_k)
        assert got.shape == want.shape
        assert np.array_equal(np.isnan(got), np.isnan(want)), (name, mean_k)     # NaN exactly where the restatement has NaN
        if k == 0:
            continue
        g, w = got[valid], want[valid]
        zero = w == 0.0
        assert np.array_equal(g[zero], w[zero])                                  # exact where d_i is 0
        with np.errstate(invalid="ignore"):
            rel = np.abs(g[~zero] - w[~zero]) / w[~zero]
        worst = float(rel.max()) if rel.size else 0.0
        print(name, "mean_k", mean_k, "k'", k, "worst relative difference", worst)
        assert worst <= 4e-16 * k, (name, mean_k, worst)                         # a few double ulps: the device's sqrt is not pinned


# ---------------------------------------------------------------- 3. the filter
@pytest.mark.parametrize("name", sorted(n for n, (_, keep) in oc.cases().items() if keep))
def test_filter_keeps_the_restatements_records(mm, clouds, name):
    recs, _ = clouds[name]
    c = mm.Context(0)
    cl = c.cloud(recs)
    for mean_k, mult in oc.FILTER_PARAMS:
        r = oc.reference_filter(name, mean_k, mult)
        got = c.removeOutliersStatistical(cl, mean_k, mult).numpy()
        want = recs[r["keep"]]
        assert len(got) == len(want), (name, mean_k, mult, len(got), len(want))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, mean_k, mult)      # the cloud's order, colours included
        st = c.last_outlier_stats
        assert (st["points"], st["valid"], st["kept"], st["k"]) == (len(recs), int(r["valid"].sum()), int(r["keep"].sum()), r["k"]), st
        for key in ("mean", "stddev", "threshold"):
            assert abs(st[key] - r[key]) <= 1e-12 * abs(r[key]), (name, mean_k, mult, key, st[key], r[key])
    c.close()


def test_filter_result_is_a_cloud_like_the_radius_filters(mm, ctx, clouds):
    """The kept points' bounding box and the voxel lattice travel with the result: a grid built on it finds every point."""
    recs, _ = clouds["b_far_point_and_corners"]
    kept = ctx.removeOutliersStatistical(ctx.cloud(recs), 16, 1.0)
    again = ctx.removeOutliersStatistical(kept, 16, 1.0)                         # (its grid is built from the box it carries)
    r = oc.restate(oc.cases()["b_far_point_and_corners"][0][oc.reference_filter("b_far_point_and_corners", 16, 1.0)["keep"]], 16, 1.0)
    assert len(again) == int(r["keep"].sum())


# ---------------------------------------------------------------- 4. what it is for
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_planted_points_go_and_the_room_stays(mm, ctx, seed):
    xyz, planted = oc.room_with_planted(seed)
    recs = _records(mm, xyz)
    got = ctx.removeOutliersStatistical(ctx.cloud(recs), 16, 2.0).numpy()
    kept = np.isin(recs["rgba"], got["rgba"])
    removed, room = 1.0 - kept[planted].mean(), kept[~planted].mean()
    print("seed", seed, "planted removed", removed, "room kept", room)
    assert removed >= 0.95 and room >= 0.99


# ---------------------------------------------------------------- 5. through the pipeline
@pytest.fixture(scope="module")
def scene(synth):
    _, maps = synth.synth_maps(4, 30000, overlap_step=0.4)
    return [synth.pack_points(x, c) for x, c, _ in maps], [T for _, _, T in maps]


def test_map_features_take_the_statistical_filter(mm, scene):
    raw = scene[0][1]
    p = mm.MapMergingParams(descriptor_type=FPFH, outliers_min_neighbours=12345)                # (not read by the filter)
    c = mm.Context(0)
    c.setOutlierFilter(method=STATISTICAL, mean_k=16, stddev_mult=1.0)
    m = c.mapFeatures(c.cloud(raw), p)
    stats = c.last_outlier_stats
    want = c.removeOutliersStatistical(c.downSample(c.cloud(raw), p.resolution), 16, 1.0)
    assert 0 < len(want) and np.array_equal(m.points.numpy().view(np.uint32), want.numpy().view(np.uint32))
    assert stats == c.last_outlier_stats and stats["kept"] == len(want) and stats["k"] == 16
    kp = c.detectKeypoints(want, None, p.keypoint_type, p.keypoint_threshold, p.normal_radius, p.resolution)
    d = c.computeLocalDescriptors(want, c.computeSurfaceNormals(want, p.normal_radius), kp, FPFH, p.descriptor_radius)
    assert len(m.keypoints) > 0
    assert np.array_equal(m.keypoints.numpy().view(np.uint32), kp.numpy().view(np.uint32))
    assert np.array_equal(m.descriptors.numpy().view(np.uint32), d.numpy().view(np.uint32))
    off = mm.Context(0)                                                           # without the option: removeOutliers, as before
    q = mm.MapMergingParams(descriptor_type=FPFH)
    ref = off.mapFeatures(off.cloud(raw), q)
    rad = off.removeOutliers(off.downSample(off.cloud(raw), q.resolution), q.descriptor_radius, q.outliers_min_neighbours)
    assert np.array_equal(ref.points.numpy().view(np.uint32), rad.numpy().view(np.uint32))
    assert len(ref.points) != len(m.points)
    off.close()
    c.close()


# ---------------------------------------------------------------- 6. one answer everywhere
OPTION = dict(method=STATISTICAL, mean_k=16, stddev_mult=1.0)


def _params(mm, method):
    return mm.MapMergingParams(descriptor_type=FPFH, estimation_method=method, refine_transform=1)


def _ctx(mm, method, streams=1, cache=0, first=True, devices=None, on=True):
    c = mm.Context(devices=devices) if devices else mm.Context(0)
    if on and first:
        c.setOutlierFilter(**OPTION)
    c.setStreams(streams)
    if on and not first:
        c.setOutlierFilter(**OPTION)
    if cache:
        c.setMapCache(cache)
    return c


@pytest.mark.parametrize("method", [MATCHING, SAC_IA])
def test_bit_identical_across_streams_cache_shards_and_device_lists(mm, scene, method, monkeypatch):
    clouds = scene[0]
    p = _params(mm, method)
    one = ukp._run(_ctx(mm, method, 1), clouds, p)
    assert len(one[1]) == 6 and (one[2][0] > 0).all()
    off = ukp._run(_ctx(mm, method, 1, on=False), clouds, p)
    assert not np.array_equal(one[2][0], off[2][0])                               # other points
    ukp._same(one, ukp._run(_ctx(mm, method, 4), clouds, p))
    ukp._same(one, ukp._run(_ctx(mm, method, 4, first=False), clouds, p))         # set after mm3d_set_streams: the helpers follow
    cached = _ctx(mm, method, 4, cache=8)
    ukp._same(one, ukp._run(cached, clouds, p, close=False))                      # cold
    ukp._same(one, ukp._run(cached, clouds, p, close=False))                      # every map a hit
    st = cached.mapCacheStats()
    assert st["map_hits"] == 4 and st["map_misses"] == 4, st
    cached.close()
    monkeypatch.setattr(ukp, "_ctx", _ctx)                                        # the shard driver makes its ranks' contexts with this option
    for world in (1, 2):
        merged = ukp._run_sharded(mm, method, clouds, p, world, 3)
        assert np.array_equal(merged.view(np.uint8), one[1].view(np.uint8)), world
    ukp._same(one, ukp._run(_ctx(mm, method, 4, devices=[0]), clouds, p))
    os.environ["MM3D_DEVICES_ALLOW_DUPLICATES"] = "1"
    try:
        ukp._same(one, ukp._run(_ctx(mm, method, 4, devices=[0, 0]), clouds, p))
        ukp._same(one, ukp._run(_ctx(mm, method, 2, devices=[0, 0], first=False), clouds, p))
    finally:
        del os.environ["MM3D_DEVICES_ALLOW_DUPLICATES"]


# ---------------------------------------------------------------- 7. the cache keys it
def test_the_map_cache_keys_the_outlier_filter(mm, scene):
    clouds = scene[0][:3]
    p = _params(mm, MATCHING)
    c = mm.Context(0)
    c.setMapCache(16)
    first = ukp._run(c, clouds, p, close=False)
    assert c.mapCacheStats(reset=True)["map_misses"] == 3
    c.setOutlierFilter(**OPTION)
    on = ukp._run(c, clouds, p, close=False)
    st = c.mapCacheStats(reset=True)
    assert (st["map_hits"], st["map_misses"], st["pairs_reused"]) == (0, 3, 0), st      # not the radius filter's bundles
    assert not np.array_equal(on[2][0], first[2][0])
    for other in (dict(OPTION, mean_k=17), dict(OPTION, stddev_mult=1.25)):            # other options: other bundles
        c.setOutlierFilter(**other)
        ukp._run(c, clouds, p, close=False)
        st = c.mapCacheStats(reset=True)
        assert (st["map_hits"], st["map_misses"], st["pairs_reused"]) == (0, 3, 0), (other, st)
    c.setOutlierFilter(method=RADIUS, mean_k=17, stddev_mult=1.25)                      # (neither is read under RADIUS)
    third = ukp._run(c, clouds, p, close=False)
    st = c.mapCacheStats(reset=True)
    assert (st["map_hits"], st["map_misses"], st["pairs_reused"]) == (3, 0, 3), st
    ukp._same(first, third)
    c.setOutlierFilter(method=RADIUS, mean_k=3, stddev_mult=0.5)
    ukp._run(c, clouds, p, close=False)
    assert c.mapCacheStats(reset=True)["map_hits"] == 3
    c.close()


# ---------------------------------------------------------------- 8. default untouched
def test_a_context_set_and_reset_computes_a_fresh_ones_bytes(mm, scene):
    clouds = scene[0]
    p = _params(mm, SAC_IA)
    fresh = ukp._run(_ctx(mm, SAC_IA, 4, on=False), clouds, p)
    c = _ctx(mm, SAC_IA, 4)
    c.setOutlierFilter(mm.OutlierOptions())
    ukp._same(fresh, ukp._run(c, clouds, p))
    m0 = mm.Context(0)
    m1 = mm.Context(0)
    m1.setOutlierFilter(**OPTION)
    m1.setOutlierFilter(method=RADIUS)
    a, b = m0.mapFeatures(m0.cloud(clouds[0]), p), m1.mapFeatures(m1.cloud(clouds[0]), p)
    for x, y in ((a.points, b.points), (a.keypoints, b.keypoints), (a.descriptors, b.descriptors)):
        assert np.array_equal(x.numpy().view(np.uint32), y.numpy().view(np.uint32))
    m0.close()
    m1.close()


# ---------------------------------------------------------------- 9. sparse maps
# pairs of three within 1.0 of the truth on the sparse lattice scene, statistical filter (16, 1.0) + uniform keypoints + FPFH + SAC_IA + ICP,
# measured at srand 1, 2, 3
SPARSE_MEASURED = (1, 2, 2)


def test_sparse_maps_reach_the_pair_stage(mm, synth):
    """About 12.5 points per square metre: the radius filter at the reference's defaults leaves at most 2 % of a map, the
    statistical rule at least 75 %, and all three pair records come back finite."""
    _, maps = synth.lattice_maps(3, 20000, window=40.0, overlap_step=0.25)
    raws, Tg = [synth.pack_points(x, c) for x, c, _ in maps], [T for _, _, T in maps]
    p = _params(mm, SAC_IA)
    n_raw = np.array([len(r) for r in raws], dtype=np.float64)

    def run(on, seed):
        c = mm.Context(0)
        c.setKeypoints(source=ukp.UNIFORM)
        if on:
            c.setOutlierFilter(**OPTION)
        c.setStreams(4)
        return ukp._run(c, raws, p, seed=seed)

    off = run(False, 1)
    print("radius filter leaves", off[2][0], "of", n_raw)
    assert (off[2][0] <= 0.02 * n_raw).all()
    measured = []
    for seed in (1, 2, 3):
        on = run(True, seed)
        assert (on[2][0] >= 0.75 * n_raw).all(), on[2][0]
        assert len(on[1]) == 3 and np.isfinite(on[1]["transform"]).all() and np.isfinite(on[1]["confidence"]).all()
        good, errs = ukp._recovered(synth, on[1], Tg, 1.0)
        print("sparse: srand", seed, "statistical filter leaves", on[2][0], "recovered", good, "errors", errs)
        measured.append(good)
    print("sparse measured", tuple(measured))
    # (the measured minimum less one pair is 0 here, so this line cannot fail: the kept shares and the finite records above are
    # what this test holds; the tuple records what was measured, and the line guards a later, better measured tuple)
    assert min(measured) >= min(SPARSE_MEASURED) - 1, measured

"""The cluster filter on the device (mm3d_cluster_labels, mm3d_remove_small_clusters, mm3d_set_cluster_filter) against the numpy
restatement of tests/cluster_cases.py: labels and counts record by record, both methods byte for byte, the record order, the
stage behind the whole-map calls (features, streams, device list, cache and its key), the default untouched, and every refusal
the header names."""
import ctypes as C

import numpy as np
import pytest

import cluster_cases as cc
import test_gpu_uniform_keypoints as ukp

pytestmark = pytest.mark.gpu

FPFH = 2
MATCHING = 0
OFF, MIN_SIZE, LARGEST = cc.OFF, cc.MIN_SIZE, cc.LARGEST
EINVAL = -1
ZERO_STATS = dict(points=0, valid=0, kept=0, clusters=0, kept_clusters=0, largest=0)


def _records(mm, xyz):
    """Every record its own colour, so that a kept record names the row it came from."""
    a = np.zeros(len(xyz), dtype=mm.POINT)
    a["x"], a["y"], a["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    a["rgba"] = 0xFF000000 + np.arange(len(xyz), dtype=np.uint32) * 3
    return a


@pytest.fixture(scope="module")
def clouds(mm, ctx):
    """Every case's records and its device cloud, uploaded once."""
    out = {}
    for name, (xyz, _) in cc.cases().items():
        recs = _records(mm, xyz)
        out[name] = (recs, ctx.cloud(recs))
    return out


# ---------------------------------------------------------------- 1. labels
@pytest.mark.parametrize("name", sorted(cc.cases()))
def test_labels_and_stats_equal_the_restatement(ctx, clouds, name):
    ref = cc.reference(name)
    got, st = ctx.clusterLabels(clouds[name][1], cc.cases()[name][1], with_stats=True)
    assert got.dtype == np.int32 and got.shape == ref["labels"].shape
    differ = np.nonzero(got != ref["labels"])[0]
    print(name, "records", len(got), "stats", st, "labels that differ", len(differ))
    assert len(differ) == 0, (name, differ[:10], got[differ[:10]], ref["labels"][differ[:10]])
    assert st == ref["stats"], (st, ref["stats"])


# ---------------------------------------------------------------- 2. both methods
@pytest.mark.parametrize("name", sorted(cc.cases()))
def test_both_methods_keep_the_restatements_records(mm, ctx, clouds, name):
    recs, cloud = clouds[name]
    tol = cc.cases()[name][1]
    sizes = np.bincount(cc.reference(name)["labels"][cc.reference(name)["valid"]], minlength=1)
    top = max(int(sizes.max()), 1)                                # (min_size is at least 1)
    for method, min_size in ((MIN_SIZE, 1), (MIN_SIZE, 2), (MIN_SIZE, cc.SIZES_MIN), (MIN_SIZE, top), (MIN_SIZE, top + 1), (LARGEST, 1), (LARGEST, 7)):
        keep, want_st = cc.reference_filter(name, method, min_size)
        got = ctx.removeSmallClusters(cloud, tol, method, min_size).numpy()
        want = recs[keep]
        assert len(got) == len(want), (name, method, min_size, len(got), len(want))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, method, min_size)      # the cloud's order, colours included
        assert ctx.last_cluster_stats == want_st, (name, method, min_size, ctx.last_cluster_stats, want_st)
        if (method, min_size) == (MIN_SIZE, 1):
            assert np.array_equal(got.view(np.uint32), recs[cc.reference(name)["valid"]].view(np.uint32))   # exactly the valid records


def test_result_is_a_cloud_like_the_outlier_filters(ctx, clouds):
    """The kept points' bounding box travels with the result: a grid built on it finds every point."""
    kept = ctx.removeSmallClusters(clouds["i_random_1"][1], cc.TOL, MIN_SIZE, 10)
    again = ctx.removeSmallClusters(kept, cc.TOL, MIN_SIZE, 10)
    assert 0 < len(kept) < 4000 and np.array_equal(again.numpy().view(np.uint32), kept.numpy().view(np.uint32))
    lab = ctx.clusterLabels(kept, cc.TOL)
    assert (np.bincount(lab)[lab] >= 10).all()


# ---------------------------------------------------------------- 3. record order
@pytest.mark.parametrize("name", ["a_chain", "c_sizes", "e_invalid_and_duplicates", "i_random_1", "l_random_at_10km"])
def test_the_partition_does_not_depend_on_the_record_order(mm, ctx, name):
    xyz, tol = cc.cases()[name]
    ref = cc.reference(name)["labels"]
    perm = np.random.default_rng(21).permutation(len(xyz))        # record k of the permuted cloud is record perm[k]
    got = ctx.clusterLabels(ctx.cloud(_records(mm, xyz[perm])), tol)
    back = {frozenset(int(perm[k]) for k in s) for s in cc.partition(got)}
    assert back == cc.partition(ref)
    for s in cc.partition(got):                                   # the labels follow the new indices
        assert {int(got[k]) for k in s} == {min(s)}
    assert np.array_equal(got < 0, ref[perm] < 0)


# ---------------------------------------------------------------- 4. wiring
@pytest.fixture(scope="module")
def rooms(synth):
    """Three views of one room, each with its own blobs: (packed records, is_blob, boxes)."""
    views = ((1, 0.0, (0.0, 0.0, 0.0)), (2, 0.35, (1.5, -0.8, 0.0)), (3, -0.5, (-1.0, 1.2, 0.0)))
    out = []
    for seed, yaw, shift in views:
        xyz, rgb, is_blob, boxes = cc.room_with_blobs(seed, yaw, shift)
        out.append((synth.pack_points(xyz, rgb), is_blob, boxes))
    return out


def _inside(a, boxes):
    p = np.stack([a["x"], a["y"], a["z"]], axis=1)
    return np.any([((p >= lo) & (p <= hi)).all(axis=1) for lo, hi in boxes], axis=0)


def test_map_features_run_the_cluster_filter(mm, rooms):
    raw, is_blob, boxes = rooms[0]
    p = mm.MapMergingParams(descriptor_type=FPFH)
    c = mm.Context(0)
    down = c.downSample(c.cloud(raw), p.resolution)
    rad = c.removeOutliers(down, p.descriptor_radius, p.outliers_min_neighbours)
    stat = c.removeOutliersStatistical(down, 16, 2.0)
    for name, f in (("radius", rad), ("statistical", stat)):      # the blobs pass both outlier filters: only the cluster filter answers them
        n_in = _inside(f.numpy(), boxes).sum()
        n_down = _inside(down.numpy(), boxes).sum()
        print(name, "filter keeps", n_in, "of", n_down, "blob points")
        assert 3 * 250 <= n_down <= 3 * 450 and n_in >= 0.95 * n_down
    lab, st = c.clusterLabels(rad, 2.0 * p.resolution, with_stats=True)
    sizes = np.sort(np.bincount(lab))[::-1]
    print("clusters of the filtered room", st, sizes[sizes > 0][:8])
    c.setClusterFilter(method=MIN_SIZE, min_size=cc.ROOM_MIN_SIZE)          # tolerance 0: twice the resolution
    m = c.mapFeatures(c.cloud(raw), p)
    stats = c.last_cluster_stats
    want = c.removeSmallClusters(rad, 2.0 * p.resolution, MIN_SIZE, cc.ROOM_MIN_SIZE)
    got = m.points.numpy()
    assert 0 < len(want) < len(rad) and np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32))
    assert stats == c.last_cluster_stats and stats["kept"] == len(want) and stats["points"] == len(rad)
    assert not _inside(got, boxes).any()                                     # no point remains inside the blobs' boxes
    room = rad.numpy()[~_inside(rad.numpy(), boxes)]
    assert np.array_equal(got.view(np.uint32), room.view(np.uint32))        # and the room's own points are all kept
    assert stats["clusters"] - stats["kept_clusters"] == 3 and stats["kept_clusters"] == 2     # the room and the free-standing wall
    # the rest of the bundle is the stages' on that cloud
    kp = c.detectKeypoints(want, None, p.keypoint_type, p.keypoint_threshold, p.normal_radius, p.resolution)
    d = c.computeLocalDescriptors(want, c.computeSurfaceNormals(want, p.normal_radius), kp, FPFH, p.descriptor_radius)
    assert len(m.keypoints) > 0
    assert np.array_equal(m.keypoints.numpy().view(np.uint32), kp.numpy().view(np.uint32))
    assert np.array_equal(m.descriptors.numpy().view(np.uint32), d.numpy().view(np.uint32))
    # after the statistical filter too, and LARGEST drops the free-standing wall as well
    c.setOutlierFilter(method=1, mean_k=16, stddev_mult=2.0)
    c.setClusterFilter(method=LARGEST)
    m2 = c.mapFeatures(c.cloud(raw), p)
    want2 = c.removeSmallClusters(stat, 2.0 * p.resolution, LARGEST, 1)
    assert np.array_equal(m2.points.numpy().view(np.uint32), want2.numpy().view(np.uint32))
    assert c.last_cluster_stats["kept_clusters"] == 1 and m2.points.numpy()["y"].min() > -0.5
    c.close()


# ---------------------------------------------------------------- 5. one answer from every driver
OPTION = dict(method=MIN_SIZE, min_size=cc.ROOM_MIN_SIZE)


def _params(mm):
    return mm.MapMergingParams(descriptor_type=FPFH, estimation_method=MATCHING, refine_transform=1)


def _ctx(mm, streams=1, cache=0, first=True, devices=None, on=True):
    c = mm.Context(devices=devices) if devices else mm.Context(0)
    if on and first:
        c.setClusterFilter(**OPTION)
    c.setStreams(streams)
    if on and not first:
        c.setClusterFilter(**OPTION)
    if cache:
        c.setMapCache(cache)
    return c


@pytest.fixture(scope="module")
def one_stream(mm, rooms):
    clouds = [r[0] for r in rooms]
    return ukp._run(_ctx(mm, 1), clouds, _params(mm)), ukp._run(_ctx(mm, 1, on=False), clouds, _params(mm))


def test_bit_identical_across_streams_device_list_and_cache(mm, rooms, one_stream):
    clouds = [r[0] for r in rooms]
    p = _params(mm)
    one, off = one_stream
    print("points per map", one[2][0], "without the filter", off[2][0], "pair records", len(one[1]))
    assert len(one[1]) == 3 and (one[2][0] > 0).all() and (one[2][0] < off[2][0]).all()      # the blobs are gone from every map
    ukp._same(one, ukp._run(_ctx(mm, 4), clouds, p))
    ukp._same(one, ukp._run(_ctx(mm, 4, first=False), clouds, p))           # set after mm3d_set_streams: the helpers follow
    ukp._same(one, ukp._run(_ctx(mm, 4, devices=[0]), clouds, p))
    cached = _ctx(mm, 4, cache=8)
    ukp._same(one, ukp._run(cached, clouds, p, close=False))                # cold
    ukp._same(one, ukp._run(cached, clouds, p, close=False))                # every map a hit
    st = cached.mapCacheStats(reset=True)
    assert st["map_hits"] == 3 and st["map_misses"] == 3, st
    for other in (dict(OPTION, min_size=cc.ROOM_MIN_SIZE + 1), dict(OPTION, tolerance=0.25), dict(method=LARGEST)):   # other options: other bundles
        cached.setClusterFilter(**other)
        ukp._run(cached, clouds, p, close=False)
        st = cached.mapCacheStats(reset=True)
        assert (st["map_hits"], st["map_misses"], st["pairs_reused"]) == (0, 3, 0), (other, st)
    cached.setClusterFilter(mm.ClusterOptions(min_size=7, tolerance=0.3))  # OFF: neither field is read, and these are the plain bundles
    ukp._same(off, ukp._run(cached, clouds, p, close=False))
    cached.setClusterFilter(mm.ClusterOptions())
    ukp._same(off, ukp._run(cached, clouds, p, close=False))
    st = cached.mapCacheStats(reset=True)
    assert (st["map_hits"], st["map_misses"]) == (3, 3), st
    cached.close()


# ---------------------------------------------------------------- 6. off means off
def test_a_context_set_and_reset_computes_a_fresh_ones_bytes(mm, rooms, one_stream):
    clouds = [r[0] for r in rooms]
    p = _params(mm)
    one, off = one_stream
    c = _ctx(mm, 4)
    assert c.getClusterFilter().as_tuple() == (MIN_SIZE, cc.ROOM_MIN_SIZE, 0.0)
    ukp._same(one, ukp._run(c, clouds, p, close=False))
    assert c.getClusterFilter().as_tuple() == (MIN_SIZE, cc.ROOM_MIN_SIZE, 0.0)              # the selection stays in force across a run
    ukp._same(one, ukp._run(c, clouds, p, close=False))
    c.setClusterFilter(mm.ClusterOptions())
    assert c.getClusterFilter().as_tuple() == (OFF, 100, 0.0)
    ukp._same(off, ukp._run(c, clouds, p))
    m0, m1 = mm.Context(0), mm.Context(0)
    m1.setClusterFilter(**OPTION)
    m1.setClusterFilter(method=OFF)
    a, b = m0.mapFeatures(m0.cloud(clouds[0]), p), m1.mapFeatures(m1.cloud(clouds[0]), p)
    for x, y in ((a.points, b.points), (a.keypoints, b.keypoints), (a.descriptors, b.descriptors)):
        assert np.array_equal(x.numpy().view(np.uint32), y.numpy().view(np.uint32))
    assert m0.last_cluster_stats == ZERO_STATS and m1.last_cluster_stats == ZERO_STATS
    m0.close()
    m1.close()


# ---------------------------------------------------------------- 7. validation
def test_every_refusal_of_the_header(mm, clouds):
    L = mm.lib()
    c = mm.Context(0)
    assert c.getClusterFilter().as_tuple() == (OFF, 100, 0.0) and c.last_cluster_stats == ZERO_STATS      # a fresh context answers the defaults
    c.setClusterFilter(method=MIN_SIZE, min_size=200, tolerance=0.25)
    assert c.getClusterFilter().as_tuple() == (MIN_SIZE, 200, 0.25)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(method=3), dict(method=-1), dict(min_size=0), dict(min_size=-5), dict(tolerance=-0.1), dict(tolerance=nan),
                dict(tolerance=inf), dict(tolerance=-inf), dict(method=LARGEST, min_size=0), dict(method=OFF, tolerance=-1.0),
                dict(method=OFF, min_size=0)):                              # (checked whatever the method)
        assert L.mm3d_set_cluster_filter(c._h, C.byref(mm.ClusterOptions(**bad))) == EINVAL, bad
        assert c.getClusterFilter().as_tuple() == (MIN_SIZE, 200, 0.25)     # a refused call changes nothing
    assert L.mm3d_set_cluster_filter(c._h, None) == EINVAL and L.mm3d_get_cluster_filter(c._h, None) == EINVAL
    assert L.mm3d_set_cluster_filter(None, C.byref(mm.ClusterOptions())) == EINVAL
    assert L.mm3d_get_cluster_filter(None, C.byref(mm.ClusterOptions())) == EINVAL
    assert L.mm3d_last_cluster_stats(c._h, None) == EINVAL and L.mm3d_last_cluster_stats(None, C.byref(mm.ClusterStats())) == EINVAL
    c.setClusterFilter(method=LARGEST, tolerance=0.0)                       # zero is a value of the options
    assert c.getClusterFilter().as_tuple() == (LARGEST, 100, 0.0)
    recs = clouds["c_sizes"][0]
    cloud = c.cloud(recs)
    empty = c.cloud(np.empty(0, dtype=mm.POINT))
    n = len(recs)
    out, buf, st = C.c_void_p(), np.zeros(n + 8, dtype=np.int32), mm.ClusterStats()
    ptr = buf.ctypes.data_as(C.c_void_p)
    tol = C.c_double(cc.TOL)
    for t in (0.0, -0.2, nan, inf, -inf):                                   # the stand-alone entry points need a tolerance > 0
        assert L.mm3d_cluster_labels(c._h, cloud._h, C.c_double(t), ptr, C.c_size_t(n), C.byref(st)) == EINVAL, t
        assert L.mm3d_remove_small_clusters(c._h, cloud._h, C.c_double(t), MIN_SIZE, 10, C.byref(out)) == EINVAL, t
        assert L.mm3d_remove_small_clusters(c._h, empty._h, C.c_double(t), MIN_SIZE, 10, C.byref(out)) == EINVAL, t
    for method in (OFF, 3, -1):
        assert L.mm3d_remove_small_clusters(c._h, cloud._h, tol, method, 10, C.byref(out)) == EINVAL, method
    for method in (MIN_SIZE, LARGEST):
        for ms in (0, -1):
            assert L.mm3d_remove_small_clusters(c._h, cloud._h, tol, method, ms, C.byref(out)) == EINVAL, (method, ms)
    assert L.mm3d_remove_small_clusters(c._h, None, tol, MIN_SIZE, 10, C.byref(out)) == EINVAL
    assert L.mm3d_remove_small_clusters(c._h, cloud._h, tol, MIN_SIZE, 10, None) == EINVAL
    assert L.mm3d_remove_small_clusters(None, cloud._h, tol, MIN_SIZE, 10, C.byref(out)) == EINVAL
    assert L.mm3d_cluster_labels(c._h, None, tol, ptr, C.c_size_t(n), None) == EINVAL
    assert L.mm3d_cluster_labels(c._h, cloud._h, tol, None, C.c_size_t(n), None) == EINVAL
    assert L.mm3d_cluster_labels(None, cloud._h, tol, ptr, C.c_size_t(n), None) == EINVAL
    assert L.mm3d_cluster_labels(c._h, cloud._h, tol, ptr, C.c_size_t(n - 1), None) == EINVAL       # capacity < n
    buf[:] = -7
    assert L.mm3d_cluster_labels(c._h, cloud._h, tol, ptr, C.c_size_t(n), None) == 0                 # stats may be NULL
    assert np.array_equal(buf[:n], cc.reference("c_sizes")["labels"]) and (buf[n:] == -7).all()
    assert L.mm3d_cluster_labels(c._h, empty._h, tol, ptr, C.c_size_t(0), C.byref(st)) == 0 and st.as_dict() == ZERO_STATS
    assert len(c.removeSmallClusters(empty, cc.TOL, LARGEST, 1)) == 0 and c.last_cluster_stats == ZERO_STATS
    assert c.getClusterFilter().as_tuple() == (LARGEST, 100, 0.0)           # the stage calls do not touch the selection
    c.close()
    d = mm.Context(devices=[0])                                             # a device list accepts the setting
    d.setClusterFilter(method=MIN_SIZE, min_size=50, tolerance=0.3)
    assert d.getClusterFilter().as_tuple() == (MIN_SIZE, 50, 0.3)
    d.close()

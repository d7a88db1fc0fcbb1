"""The plane stage on the device (mm3d_segment_planes, mm3d_remove_planes, mm3d_set_planes) against the numpy restatement of
tests/plane_cases.py: labels, planes and counts record by record with and without the refit, the removed cloud byte for byte,
the record order, the stage behind the whole-map calls with the cluster filter (features, streams, device list, cache and its
key), the default untouched, and every refusal the header names."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import cluster_cases as cc
import plane_cases as pc
import test_gpu_uniform_keypoints as ukp

pytestmark = pytest.mark.gpu

FPFH = 2
MATCHING = 0
OFF, REMOVE, SET_ASIDE = pc.OFF, pc.REMOVE, pc.SET_ASIDE
EINVAL = -1
ZERO_STATS = dict(points=0, valid=0, on_planes=0, kept=0, draws=0, degenerate=0, off_axis=0, planes=0, rounds=0)


def _records(mm, xyz):
    """Every record its own colour, so that a kept record names the row it came from."""
    a = np.zeros(len(xyz), dtype=mm.POINT)
    a["x"], a["y"], a["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    a["rgba"] = 0xFF000000 + np.arange(len(xyz), dtype=np.uint32) * 3
    return a


def _xyz(a):
    return np.stack([a["x"], a["y"], a["z"]], axis=1)


@pytest.fixture(scope="module")
def clouds(mm, ctx):
    """Every case's records and its device cloud, uploaded once."""
    out = {}
    for name, (xyz, _, _) in pc.cases().items():
        recs = _records(mm, xyz)
        out[name] = (recs, ctx.cloud(recs))
    return out


def _angle(a, b):
    a, b = np.array(a), np.array(b)
    return math.atan2(np.linalg.norm(np.cross(a, b)), float(np.dot(a, b)))


# ---------------------------------------------------------------- 1. labels, planes, counts
@pytest.mark.parametrize("name,refit", pc.runs())
def test_labels_planes_and_stats_equal_the_restatement(mm, ctx, clouds, name, refit):
    ref = pc.reference(name, refit)
    o = dict(pc.cases()[name][1], refit=refit)
    labels, planes, st = ctx.segmentPlanes(clouds[name][1], **o)
    assert labels.dtype == np.int32 and labels.shape == ref["labels"].shape
    differ = np.nonzero(labels != ref["labels"])[0]
    print(name, "refit", refit, "records", len(labels), "stats", st, "labels that differ", len(differ))
    for got, want in zip(planes, ref["planes"]):
        scale = max(1.0, abs(want["d"]))
        print("  plane", got, "normal differs by", _angle(got["normal"], want["normal"]), "rad, d by", abs(got["d"] - want["d"]), "scale", scale)
    assert len(differ) == 0, (name, differ[:10], labels[differ[:10]], ref["labels"][differ[:10]])
    assert st == ref["stats"], (st, ref["stats"])
    assert len(planes) == len(ref["planes"])
    for got, want in zip(planes, ref["planes"]):
        assert (got["draw"], got["inliers"], got["refit"]) == (want["draw"], want["inliers"], want["refit"])
        if refit == 0:
            scale = max(1.0, abs(want["d"]))
            assert np.abs(np.array(got["normal"]) - np.array(want["normal"])).max() <= 1e-12 and abs(got["d"] - want["d"]) <= 1e-12 * scale
        else:
            # (a plane that kept its hypothesis is exact as above; an adopted refit sums at most 2 x 10^4 terms in another order)
            assert _angle(got["normal"], want["normal"]) <= 1e-9 and abs(got["d"] - want["d"]) <= 1e-9


# ---------------------------------------------------------------- 2. the removed cloud
@pytest.mark.parametrize("name", ["a_two_parallel_planes", "b_threshold", "c_collinear", "d_invalid_rows", "e_0_points", "e_2_points", "e_3_points",
                                  "f_4097_points_65_draws", "h_room_8", "i_tilted_slab", "k_room_at_10km"])
def test_remove_planes_keeps_the_restatements_records(mm, ctx, clouds, name):
    recs, cloud = clouds[name]
    o, refit_too = pc.cases()[name][1], pc.cases()[name][2]
    for refit in ((0, 1) if refit_too else (0,)):
        ref = pc.reference(name, refit)
        got = ctx.removePlanes(cloud, **dict(o, refit=refit)).numpy()
        want = recs[ref["labels"] == pc.NONE]
        assert len(got) == len(want), (name, refit, len(got), len(want))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, refit)          # the cloud's order, colours included
        assert ctx.last_plane_stats == ref["stats"]
        last = ctx.last_planes
        assert [(p["draw"], p["inliers"], p["refit"]) for p in last] == [(p["draw"], p["inliers"], p["refit"]) for p in ref["planes"]]


def test_result_is_a_cloud_like_the_outlier_filters(ctx, clouds):
    """The kept points' bounding box travels with the result: the stage run on it again finds what the restatement finds there,
    and the cluster filter, which builds a grid on that box, finds every point."""
    recs, cloud = clouds["f_4097_points_65_draws"]
    o = pc.cases()["f_4097_points_65_draws"][1]
    kept = ctx.removePlanes(cloud, **o)
    again = pc.segment(_xyz(kept.numpy()), o)
    labels, planes, st = ctx.segmentPlanes(kept, **o)
    assert 0 < len(kept) < len(recs) and np.array_equal(labels, again["labels"]) and st == again["stats"]
    lab = ctx.clusterLabels(kept, 0.5)
    assert (lab >= 0).all() and np.array_equal(lab, cc.labels_union_find(*cc.adjacency(_xyz(kept.numpy()), 0.5)))


# ---------------------------------------------------------------- 3. record order and seed
def test_other_records_drawn_find_the_same_room(mm, ctx):
    xyz, o, _ = pc.cases()["g_room_6"]
    perm = np.random.default_rng(21).permutation(len(xyz))
    for x, seed in ((xyz[perm], o["seed"]), (xyz, 2), (xyz[perm], 77)):
        labels, planes, st = ctx.segmentPlanes(ctx.cloud(_records(mm, x)), **dict(o, seed=seed))
        sides = [pc.which_room_side(p) for p in planes]                       # within 0.02 m and 1 degree of a side, each
        assert sorted(sides) == list(range(6)) and st["planes"] == 6 and st["kept"] == 0


# ---------------------------------------------------------------- 4. wiring
@pytest.fixture(scope="module")
def persons(synth):
    """Three views of the room with the standing column: (packed records, is_blob, is_column)."""
    views = ((1, 0.0, (0.0, 0.0, 0.0)), (2, 0.35, (1.5, -0.8, 0.0)), (3, -0.5, (-1.0, 1.2, 0.0)))
    out = []
    for seed, yaw, shift in views:
        xyz, rgb, is_blob, is_column = pc.room_with_person(seed, yaw, shift)
        out.append((synth.pack_points(xyz, rgb), is_blob, is_column, xyz))
    return out


def _column_box(xyz, is_column):
    return xyz[is_column].min(axis=0) - 0.05, xyz[is_column].max(axis=0) + 0.05


def _in_box(a, box):
    p = _xyz(a)
    return ((p >= box[0]) & (p <= box[1])).all(axis=1)


def _points(c, raw, p):
    m = c.mapFeatures(c.cloud(raw), p)                                        # (the map owns its points: it stays alive across the download)
    return m.points.numpy()


def test_map_features_compose_planes_and_clusters(mm, persons):
    raw, _, is_column, xyz = persons[0]
    box = _column_box(xyz, is_column)
    p = mm.MapMergingParams(descriptor_type=FPFH)
    c = mm.Context(0)
    rad = c.removeOutliers(c.downSample(c.cloud(raw), p.resolution), p.descriptor_radius, p.outliers_min_neighbours)
    recs = rad.numpy()
    n_col = int(_in_box(recs, box).sum())
    assert len(recs) <= 20000 and n_col >= 200
    plain = _points(c, raw, p)
    assert np.array_equal(plain.view(np.uint32), recs.view(np.uint32))
    # the cluster filter alone keeps every point of the column
    c.setClusterFilter(method=cc.MIN_SIZE, min_size=cc.ROOM_MIN_SIZE)
    alone = _points(c, raw, p)
    assert int(_in_box(alone, box).sum()) == n_col
    # SET_ASIDE + MIN_SIZE: the restatement's composition, byte for byte, in the stated order
    o = pc.options(**pc.PERSON_OPTIONS)
    seg = pc.segment(_xyz(recs), o)
    on, rest = seg["labels"] >= 0, seg["labels"] == pc.NONE
    adj, valid = cc.adjacency(_xyz(recs[rest]), 2.0 * p.resolution)
    keep, _ = cc.keep_mask(cc.labels_union_find(adj, valid), cc.MIN_SIZE, cc.ROOM_MIN_SIZE)
    want = np.concatenate([recs[on], recs[rest][keep]])
    c.setPlanes(method=SET_ASIDE, **o)
    m = c.mapFeatures(c.cloud(raw), p)
    got = m.points.numpy()
    print("filtered", len(recs), "floor", int(on.sum()), "column", n_col, "kept after SET_ASIDE + MIN_SIZE", len(got), "stats", c.last_plane_stats)
    assert len(got) == len(want) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert c.last_plane_stats == seg["stats"] and seg["stats"]["planes"] == 1
    assert [(q["draw"], q["inliers"], q["refit"]) for q in c.last_planes] == [(q["draw"], q["inliers"], q["refit"]) for q in seg["planes"]]
    assert int(_in_box(got, box).sum()) == int(_in_box(recs[on], box).sum()) <= 40          # the column is gone but for its feet on the floor
    assert c.last_cluster_stats["points"] == int(rest.sum())
    # the rest of the bundle is the stages' on that cloud
    cloud = c.cloud(want)
    kp = c.detectKeypoints(cloud, None, p.keypoint_type, p.keypoint_threshold, p.normal_radius, p.resolution)
    d = c.computeLocalDescriptors(cloud, c.computeSurfaceNormals(cloud, p.normal_radius), kp, FPFH, p.descriptor_radius)
    assert len(m.keypoints) > 0
    assert np.array_equal(m.keypoints.numpy().view(np.uint32), kp.numpy().view(np.uint32))
    assert np.array_equal(m.descriptors.numpy().view(np.uint32), d.numpy().view(np.uint32))
    # REMOVE leaves no floor point, and the cluster filter then runs on what is left
    c.setPlanes(method=REMOVE, **o)
    gone = _points(c, raw, p)
    assert np.array_equal(gone.view(np.uint32), recs[rest][keep].view(np.uint32)) and gone["z"].min() > 0.05
    c.setClusterFilter(method=cc.OFF)
    gone = _points(c, raw, p)
    assert np.array_equal(gone.view(np.uint32), recs[rest].view(np.uint32))
    # SET_ASIDE without a cluster filter: nothing runs
    c.setPlanes(method=SET_ASIDE, **o)
    before = c.last_plane_stats
    same = _points(c, raw, p)
    assert np.array_equal(same.view(np.uint32), recs.view(np.uint32)) and c.last_plane_stats == before
    # distance 0 stands for half the resolution
    c.setPlanes(method=REMOVE, **dict(o, distance=0.0))
    half = _points(c, raw, p)
    assert np.array_equal(half.view(np.uint32), recs[rest].view(np.uint32)) and p.resolution / 2 == o["distance"]
    c.close()


# ---------------------------------------------------------------- 5. one answer from every driver
OPTION = dict(method=SET_ASIDE, **pc.PERSON_OPTIONS)
CLUSTERS = dict(method=cc.MIN_SIZE, min_size=cc.ROOM_MIN_SIZE)


def _params(mm):
    return mm.MapMergingParams(descriptor_type=FPFH, estimation_method=MATCHING, refine_transform=1)


def _ctx(mm, streams=1, cache=0, first=True, devices=None, on=True, clusters=True):
    c = mm.Context(devices=devices) if devices else mm.Context(0)
    if clusters:
        c.setClusterFilter(**CLUSTERS)
    if on and first:
        c.setPlanes(**OPTION)
    c.setStreams(streams)
    if on and not first:
        c.setPlanes(**OPTION)
    if cache:
        c.setMapCache(cache)
    return c


@pytest.fixture(scope="module")
def one_stream(mm, persons):
    clouds = [r[0] for r in persons]
    return (ukp._run(_ctx(mm, 1), clouds, _params(mm)), ukp._run(_ctx(mm, 1, on=False), clouds, _params(mm)),
            ukp._run(_ctx(mm, 1, on=False, clusters=False), clouds, _params(mm)))


def test_bit_identical_across_streams_device_list_and_cache(mm, persons, one_stream):
    clouds = [r[0] for r in persons]
    p = _params(mm)
    one, off, _ = one_stream
    print("points per map", one[2][0], "with the cluster filter alone", off[2][0], "pair records", len(one[1]))
    assert len(one[1]) == 3 and (one[2][0] > 0).all() and (one[2][0] < off[2][0]).all()      # the column is gone from every map
    ukp._same(one, ukp._run(_ctx(mm, 4), clouds, p))
    ukp._same(one, ukp._run(_ctx(mm, 4, first=False), clouds, p))           # set after mm3d_set_streams: the helpers follow
    ukp._same(one, ukp._run(_ctx(mm, 4, devices=[0]), clouds, p))
    os.environ["MM3D_DEVICES_ALLOW_DUPLICATES"] = "1"
    try:
        ukp._same(one, ukp._run(_ctx(mm, 2, devices=[0, 0], first=False), clouds, p))
    finally:
        del os.environ["MM3D_DEVICES_ALLOW_DUPLICATES"]
    cached = _ctx(mm, 4, cache=8)
    ukp._same(one, ukp._run(cached, clouds, p, close=False))                # cold
    ukp._same(one, ukp._run(cached, clouds, p, close=False))                # every map a hit
    st = cached.mapCacheStats(reset=True)
    assert st["map_hits"] == 3 and st["map_misses"] == 3, st
    others = (dict(method=REMOVE), dict(max_planes=2), dict(samples=512), dict(refit=0), dict(seed=2), dict(distance=0.04), dict(min_fraction=0.1),
              dict(axis=(0.0, 0.1, 1.0)), dict(max_angle_deg=12.0))
    for other in others:                                                    # any of the nine fields: other bundles
        cached.setPlanes(**dict(OPTION, **other))
        ukp._run(cached, clouds, p, close=False)
        st = cached.mapCacheStats(reset=True)
        assert (st["map_hits"], st["map_misses"], st["pairs_reused"]) == (0, 3, 0), (other, st)
    cached.setPlanes(mm.PlaneOptions(samples=7, seed=9, distance=0.3))      # OFF: no field is read, and these are the cluster filter's bundles
    ukp._same(off, ukp._run(cached, clouds, p, close=False))
    cached.setPlanes(mm.PlaneOptions())
    ukp._same(off, ukp._run(cached, clouds, p, close=False))
    st = cached.mapCacheStats(reset=True)
    assert (st["map_hits"], st["map_misses"]) == (3, 3), st
    cached.close()


def test_the_planes_doubles_do_not_depend_on_the_context(mm, persons):
    raw = persons[1][0]
    p = _params(mm)
    seen = []
    for streams, cache in ((1, 0), (4, 0), (4, 8)):
        c = _ctx(mm, streams, cache=cache)
        c.mapFeatures(c.cloud(raw), p)
        planes, st = c.last_planes, c.last_plane_stats                      # mm3d_last_planes: the last map's
        assert len(planes) == st["planes"] == 1
        labels, again, _ = c.segmentPlanes(c.removeOutliers(c.downSample(c.cloud(raw), p.resolution), p.descriptor_radius, p.outliers_min_neighbours),
                                           **pc.options(**pc.PERSON_OPTIONS))
        seen.append(np.array([list(q["normal"]) + [q["d"]] for q in planes + again]).view(np.uint64))
        c.close()
    assert all(np.array_equal(seen[0], s) for s in seen[1:]) and np.array_equal(seen[0][0], seen[0][1])


# ---------------------------------------------------------------- 6. off means off
def test_a_context_set_and_reset_computes_a_fresh_ones_bytes(mm, persons, one_stream):
    clouds = [r[0] for r in persons]
    p = _params(mm)
    one, off, never = one_stream
    c = _ctx(mm, 4)
    want = mm.PlaneOptions(**OPTION).as_tuple()
    assert c.getPlanes().as_tuple() == want
    ukp._same(one, ukp._run(c, clouds, p, close=False))
    assert c.getPlanes().as_tuple() == want                                 # the selection stays in force across a run
    c.setPlanes(mm.PlaneOptions())
    assert c.getPlanes().as_tuple() == mm.PlaneOptions().as_tuple()
    ukp._same(off, ukp._run(c, clouds, p, close=False))
    c.setClusterFilter(method=cc.OFF)
    ukp._same(never, ukp._run(c, clouds, p))
    m0, m1 = mm.Context(0), mm.Context(0)
    m1.setPlanes(method=REMOVE, max_planes=3)
    m1.setPlanes(method=OFF)
    a, b = m0.mapFeatures(m0.cloud(clouds[0]), p), m1.mapFeatures(m1.cloud(clouds[0]), p)
    for x, y in ((a.points, b.points), (a.keypoints, b.keypoints), (a.descriptors, b.descriptors)):
        assert np.array_equal(x.numpy().view(np.uint32), y.numpy().view(np.uint32))
    assert m0.last_plane_stats == ZERO_STATS and m1.last_plane_stats == ZERO_STATS and m1.last_planes == []
    m0.close()
    m1.close()


# ---------------------------------------------------------------- 7. validation
def test_every_refusal_of_the_header(mm, clouds):
    L = mm.lib()
    c = mm.Context(0)
    default = mm.PlaneOptions().as_tuple()
    assert c.getPlanes().as_tuple() == default and c.last_plane_stats == ZERO_STATS and c.last_planes == []     # a fresh context answers the defaults
    c.setPlanes(method=REMOVE, max_planes=3, samples=500, distance=0.07)
    held = c.getPlanes().as_tuple()
    assert held == (REMOVE, 3, 500, 1, 1, 0.07, 0.05, (0.0, 0.0, 1.0), 10.0)
    nan, inf = float("nan"), float("inf")
    bads = (dict(method=3), dict(method=-1), dict(max_planes=0), dict(max_planes=9), dict(samples=0), dict(samples=65537), dict(refit=2), dict(refit=-1),
            dict(distance=-0.1), dict(distance=nan), dict(distance=inf), dict(min_fraction=-0.1), dict(min_fraction=1.1), dict(min_fraction=nan),
            dict(axis=(nan, 0, 1)), dict(axis=(0, inf, 1)), dict(axis=(0, 0, -inf)), dict(max_angle_deg=-1.0), dict(max_angle_deg=90.5),
            dict(max_angle_deg=nan), dict(method=OFF, samples=0), dict(method=OFF, distance=-1.0))      # (checked whatever the method)
    for bad in bads:
        assert L.mm3d_set_planes(c._h, C.byref(mm.PlaneOptions(**bad))) == EINVAL, bad
        assert c.getPlanes().as_tuple() == held                             # a refused call changes nothing
    n = C.c_int(0)
    arr = (mm.Plane * 8)()
    assert L.mm3d_set_planes(c._h, None) == EINVAL and L.mm3d_get_planes(c._h, None) == EINVAL
    assert L.mm3d_last_plane_stats(c._h, None) == EINVAL and L.mm3d_last_plane_stats(None, C.byref(mm.PlaneStats())) == EINVAL
    assert L.mm3d_last_planes(c._h, None, 8, C.byref(n)) == EINVAL and L.mm3d_last_planes(c._h, arr, 8, None) == EINVAL
    assert L.mm3d_last_planes(c._h, arr, -1, C.byref(n)) == EINVAL and L.mm3d_last_planes(None, arr, 8, C.byref(n)) == EINVAL
    c.setPlanes(method=SET_ASIDE, max_planes=8, samples=65536, distance=0.0, min_fraction=1.0, axis=(0, 0, 0), max_angle_deg=90.0)   # the ends of the ranges
    c.setPlanes(method=SET_ASIDE, samples=1, min_fraction=0.0, max_angle_deg=0.0)
    held = c.getPlanes().as_tuple()
    recs, _ = clouds["d_invalid_rows"]
    cloud = c.cloud(recs)
    empty = c.cloud(np.empty(0, dtype=mm.POINT))
    k = len(recs)
    out, buf, st = C.c_void_p(), np.zeros(k + 8, dtype=np.int32), mm.PlaneStats()
    ptr = buf.ctypes.data_as(C.c_void_p)
    good = dict(pc.cases()["d_invalid_rows"][1], refit=1)

    def seg(ctx_h, cloud_h, o, labels=ptr, cap=k, planes=arr, count=C.byref(n), stats=C.byref(st)):
        return L.mm3d_segment_planes(ctx_h, cloud_h, C.byref(o) if o is not None else None, labels, C.c_size_t(cap), planes, count, stats)

    for bad in bads[2:-2] + (dict(distance=0.0),):                          # the stage calls check the values too, and need a distance > 0
        o = mm.PlaneOptions(**dict(good, **bad))
        assert seg(c._h, cloud._h, o) == EINVAL, bad
        assert L.mm3d_remove_planes(c._h, cloud._h, C.byref(o), C.byref(out)) == EINVAL, bad
        assert L.mm3d_remove_planes(c._h, empty._h, C.byref(o), C.byref(out)) == EINVAL, bad
    o = mm.PlaneOptions(**good)                                             # (its method is OFF: the stage calls do not read it)
    assert seg(None, cloud._h, o) == EINVAL and seg(c._h, None, o) == EINVAL and seg(c._h, cloud._h, None) == EINVAL
    assert seg(c._h, cloud._h, o, labels=None) == EINVAL and seg(c._h, cloud._h, o, planes=None) == EINVAL and seg(c._h, cloud._h, o, count=None) == EINVAL
    assert seg(c._h, cloud._h, o, cap=k - 1) == EINVAL                      # capacity < n
    assert L.mm3d_remove_planes(None, cloud._h, C.byref(o), C.byref(out)) == EINVAL and L.mm3d_remove_planes(c._h, None, C.byref(o), C.byref(out)) == EINVAL
    assert L.mm3d_remove_planes(c._h, cloud._h, None, C.byref(out)) == EINVAL and L.mm3d_remove_planes(c._h, cloud._h, C.byref(o), None) == EINVAL
    buf[:] = -7
    assert seg(c._h, cloud._h, o, stats=None) == 0                          # stats may be NULL
    ref = pc.reference("d_invalid_rows", 1)
    assert np.array_equal(buf[:k], ref["labels"]) and (buf[k:] == -7).all() and n.value == len(ref["planes"])
    buf[:] = -7
    assert seg(c._h, cloud._h, mm.PlaneOptions(**dict(good, method=7))) == 0 and np.array_equal(buf[:k], ref["labels"])   # ... whatever it holds
    assert seg(c._h, empty._h, o, cap=0) == 0 and st.as_dict() == ZERO_STATS and n.value == 0
    assert len(c.removePlanes(empty, o)) == 0 and c.last_plane_stats == ZERO_STATS and c.last_planes == []
    assert c.getPlanes().as_tuple() == held                                 # the stage calls do not touch the selection
    c.close()
    d = mm.Context(devices=[0])                                             # a device list accepts the setting
    d.setPlanes(method=REMOVE, max_planes=2, distance=0.03)
    assert d.getPlanes().as_tuple()[:3] == (REMOVE, 2, 1024) and d.getPlanes().distance == 0.03
    d.close()

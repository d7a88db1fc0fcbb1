"""The overlap confidence on the device (mm3d_set_confidence, mm3d_transform_overlap, mm3d_debug_overlap_table) against the
numpy restatement of tests/test_confidence_cpu.py.  Every count and every table word is compared EXACTLY -- integers equal,
the double bit-equal: the rule is integer-valued up to one division, so there is no tolerance anywhere in this file.

What the restatement gives on the scene of section 3 (_problem(7, 20000) cut into two halves that share 2.5 m < x < 5.5 m),
voxel 0.1, defaults otherwise: truth 5736 / 5748 and 6169 / 6569 (confidence 0.9391), 0.3 m along x 0.9402, 5 degrees of yaw
0.6875, 90 degrees and 100 m away 0 / 0.  The truth does not reach 1.0 on the halves: the source's frame is rotated against
the target's, so the 0.8 m view cells of one map straddle the cut of the other and let points in whose twins were cut away.
On identical underlying points (the two whole clouds) hit == in and the confidence is exactly 1.0, which is asserted."""
import ctypes as C

import numpy as np
import pytest

from test_confidence_cpu import Table, restate_overlap
from test_gpu_icp_plane import _pose, _problem, _records, box_room

pytestmark = pytest.mark.gpu

REFERENCE, OVERLAP = 0, 1
SAC_IA, MATCHING = 1, 0
EINVAL, EUNSUPPORTED = -1, -4
DEFAULT_MULTIPLE = 2.0           # voxel = 0 means this times params.resolution (include/mm3d.h)
VOXEL = 0.1


@pytest.fixture(scope="module")
def c(mm):
    ctx = mm.Context(0)
    yield ctx
    ctx.close()


# ---------------------------------------------------------------- 1. surface
def test_surface(mm, c):
    lib = mm.lib()
    fresh = mm.Context(0)
    assert fresh.getConfidence().as_tuple() == (REFERENCE, 0.0, 8, 0.05, 0)
    fresh.setConfidence(method=OVERLAP, voxel=0.25, min_points=3, min_overlap=0.5, view_margin=1)
    assert fresh.getConfidence().as_tuple() == (OVERLAP, 0.25, 3, 0.5, 1)
    for kw in (dict(method=2), dict(voxel=-1.0), dict(voxel=1e-45), dict(min_points=0), dict(min_overlap=1.5), dict(view_margin=2)):
        assert lib.mm3d_set_confidence(fresh._h, C.byref(mm.ConfidenceOptions(**kw))) == EINVAL, kw
        assert fresh.getConfidence().as_tuple() == (OVERLAP, 0.25, 3, 0.5, 1)
    assert lib.mm3d_set_confidence(fresh._h, None) == EINVAL and lib.mm3d_get_confidence(fresh._h, None) == EINVAL
    assert fresh.lastConfidenceStats() == dict(points_st=0, in_st=0, hit_st=0, points_ts=0, in_ts=0, hit_ts=0, confidence=0.0)
    cloud = _records(box_room(1, 2000)[0])
    with pytest.raises(mm.Mm3dError) as e:
        fresh.shardBegin([cloud, cloud], mm.MapMergingParams(descriptor_type=2), 0, 1)
    assert e.value.status == EUNSUPPORTED
    fresh.setConfidence(method=REFERENCE)
    fresh.close()
    d = mm.Context(devices=[0])
    assert lib.mm3d_set_confidence(d._h, C.byref(mm.ConfidenceOptions(method=OVERLAP))) == EUNSUPPORTED
    assert d.getConfidence().method == REFERENCE
    d.setConfidence(method=REFERENCE, min_points=3)        # the reference with other options is still accepted there
    d.close()
    # the stage-level calls want a voxel of their own
    pts = c.cloud(cloud)
    for voxel in (0.0, -1.0, float("inf")):
        with pytest.raises(mm.Mm3dError) as e:
            c.transformOverlap(pts, pts, np.eye(4), method=OVERLAP, voxel=voxel)
        assert e.value.status == EINVAL
        with pytest.raises(mm.Mm3dError) as e:
            c.debugOverlapTable(pts, method=OVERLAP, voxel=voxel)
        assert e.value.status == EINVAL


# ---------------------------------------------------------------- 2. the table, cell by cell
def _check_table(c, pts, voxel=VOXEL, min_points=8, view_margin=0):
    ref = Table(pts, voxel, min_points, view_margin)
    got = c.debugOverlapTable(c.cloud(_records(np.asarray(pts, dtype=np.float32))), method=OVERLAP, voxel=voxel, min_points=min_points,
                              view_margin=view_margin)
    assert got["brick0"] == tuple(int(x) for x in ref.b0) and got["bricks"] == tuple(int(x) for x in ref.nb)
    assert got["view0"] == tuple(int(x) for x in ref.c0) and got["views"] == tuple(int(x) for x in ref.nc)
    words, view = ref.dense()
    bad = np.argwhere(got["words"] != words)
    assert len(bad) == 0, (len(bad), bad[:4], [hex(int(got["words"][tuple(b)])) for b in bad[:4]], [hex(int(words[tuple(b)])) for b in bad[:4]])
    assert np.array_equal(got["view"], view), np.argwhere(got["view"] != view)[:8]
    return ref, got


@pytest.mark.parametrize("brick", [(0, 0, 0), (-1, -1, -1), (3, -2, 0)])
def test_single_points_at_the_eight_corners_of_a_brick(c, brick):
    """The dilation of a corner voxel crosses three faces, three edges and one corner of its brick."""
    for corner in range(8):
        v = [4 * brick[a] + (3 if (corner >> a) & 1 else 0) for a in range(3)]
        p = np.array([[(x + 0.5) * VOXEL for x in v]], dtype=np.float32)
        ref, got = _check_table(c, p, min_points=1)
        assert ref.occ.tolist() == [v]
        assert sum(bin(int(w)).count("1") for w in got["words"].ravel()) == 27
        assert len({tuple(b) for b in (ref.near >> 2).tolist()}) == 8          # 27 voxels over 8 bricks


@pytest.mark.parametrize("view_margin", [0, 1])
def test_table_of_a_cloud_that_straddles_the_origin(c, view_margin):
    rng = np.random.default_rng(42)
    room = box_room(2, 3000)[0] - np.array([4.0, 3.0, 1.5], dtype=np.float32)      # negative indices, arithmetic shifts
    on_planes = rng.uniform(-3, 3, (60, 3)).astype(np.float32)
    on_planes[np.arange(60), np.arange(60) % 3] = (rng.integers(-30, 31, 60) * np.float32(VOXEL)).astype(np.float32)
    bad = rng.uniform(-3, 3, (20, 3)).astype(np.float32)
    bad[np.arange(20), np.arange(20) % 3] = np.array([np.nan, np.inf, -np.inf, np.nan] * 5, dtype=np.float32)
    min_points = 8
    # two far clusters, each inside one view cell (0.8 m): one point short of min_points, and exactly min_points
    few = (np.array([20.4, 20.4, 20.4]) + rng.uniform(-0.3, 0.3, (min_points - 1, 3))).astype(np.float32)
    enough = (np.array([-20.4, 7.6, -9.2]) + rng.uniform(-0.3, 0.3, (min_points, 3))).astype(np.float32)
    pts = np.concatenate([room, on_planes, bad, few, enough])
    pts = pts[rng.permutation(len(pts))]
    ref, got = _check_table(c, pts, min_points=min_points, view_margin=view_margin)
    assert ref.n_finite == len(pts) - 20
    assert ref.cnt[(25, 25, 25)] == min_points - 1 and ref.cnt[(-26, 9, -12)] == min_points
    seen = {tuple(x) for x in ref.seen.tolist()}
    assert (25, 25, 25) not in seen and (-26, 9, -12) in seen
    at = lambda cell: got["view"][tuple(np.array(cell) - np.array(got["view0"]))]      # noqa: E731
    assert at((-26, 9, -12)) == 1 and at((25, 25, 25)) == 0
    assert at((-25, 10, -11)) == view_margin                                           # a neighbour of the seen cell


def test_table_of_points_exactly_on_voxel_planes(c):
    """box_room's faces lie at 0.0, 8.0, 6.0 and 3.0: whole walls on lattice planes, at the very edge of the bounding box."""
    pts = box_room(5, 6000)[0]
    assert (pts.min(axis=0) == 0.0).all()
    _check_table(c, pts, voxel=0.25)
    _check_table(c, pts, voxel=1.0, min_points=2, view_margin=1)


@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), (1000.0, -2000.0, 30.0)])
def test_table_of_a_room_of_20000_points(c, offset):
    pts = (box_room(11, 20000)[0] + np.array(offset, dtype=np.float32)).astype(np.float32)
    ref, _ = _check_table(c, pts)
    assert len(ref.occ) > 10000 and len(ref.seen) > 100


def test_empty_and_non_finite_clouds_have_no_table(c):
    for pts in (np.zeros((0, 3), dtype=np.float32), np.full((5, 3), np.nan, dtype=np.float32)):
        got = c.debugOverlapTable(c.cloud(_records(pts)), method=OVERLAP, voxel=VOXEL)
        assert got["bricks"] == (0, 0, 0) and got["views"] == (0, 0, 0) and got["words"].size == 0


# ---------------------------------------------------------------- 3. the counts of both directions
@pytest.fixture(scope="module")
def halves():
    tgt, _, src, T_true, _ = _problem(7, 20000)
    s, t = src[tgt[:, 0] < 5.5], tgt[tgt[:, 0] > 2.5]
    return s, t, T_true, (Table(s, VOXEL), Table(t, VOXEL)), (src, tgt)


def _bits(x):
    return np.float64(x).view(np.uint64)


def _same_stats(got, ref):
    assert got == ref, (got, ref)
    assert _bits(got["confidence"]) == _bits(ref["confidence"])


POSES = dict(truth=np.eye(4), offset=_pose(0, 0, 0, [0.3, 0, 0]), yaw5=_pose(0, 0, 5, [0, 0, 0]), yaw90=_pose(0, 0, 90, [0, 0, 0]),
             disjoint=_pose(0, 0, 0, [100.0, 0, 0]))


@pytest.mark.parametrize("pose", list(POSES))
def test_counts_against_the_restatement(c, halves, pose):
    s, t, T_true, tables, _ = halves
    T = (POSES[pose] @ T_true).astype(np.float32)
    ref = restate_overlap(s, t, T, VOXEL, tables=tables)
    got = c.transformOverlap(c.cloud(_records(s)), c.cloud(_records(t)), T, method=OVERLAP, voxel=VOXEL)
    print(pose, got)
    _same_stats(got, ref)
    assert c.lastConfidenceStats() == got
    if pose in ("yaw90", "disjoint"):
        assert (got["in_st"], got["hit_st"], got["in_ts"], got["hit_ts"], got["confidence"]) == (0, 0, 0, 0, 0.0)
    else:
        assert got["in_st"] > 4000 and got["in_ts"] > 4000 and 0.5 < got["confidence"] < 1.0


@pytest.mark.parametrize("view_margin,min_points", [(1, 8), (0, 1), (0, 100)])
def test_counts_under_other_options(c, halves, view_margin, min_points):
    s, t, T_true, _, _ = halves
    T = (POSES["yaw5"] @ T_true).astype(np.float32)
    ref = restate_overlap(s, t, T, 0.2, min_points=min_points, view_margin=view_margin)
    got = c.transformOverlap(c.cloud(_records(s)), c.cloud(_records(t)), T, method=OVERLAP, voxel=0.2, min_points=min_points,
                             view_margin=view_margin)
    _same_stats(got, ref)
    assert got["in_st"] > 0 and got["in_ts"] > 0


def test_truth_on_identical_points_scores_exactly_one(c, halves):
    _, _, T_true, _, (src, tgt) = halves
    T = T_true.astype(np.float32)
    got = c.transformOverlap(c.cloud(_records(src)), c.cloud(_records(tgt)), T, method=OVERLAP, voxel=VOXEL)
    _same_stats(got, restate_overlap(src, tgt, T, VOXEL))
    assert got["in_st"] > 15000 and got["in_ts"] > 15000
    assert got["hit_st"] == got["in_st"] and got["hit_ts"] == got["in_ts"] and got["confidence"] == 1.0


def test_min_overlap_gate_flips_at_the_measured_overlap(c, halves):
    s, t, T_true, tables, _ = halves
    T = T_true.astype(np.float32)
    cs, ct = c.cloud(_records(s)), c.cloud(_records(t))
    open_ = c.transformOverlap(cs, ct, T, method=OVERLAP, voxel=VOXEL, min_overlap=0.0)
    share_st, share_ts = open_["in_st"] / open_["points_st"], open_["in_ts"] / open_["points_ts"]
    assert share_st < share_ts                                            # the source direction is the one that gates first
    below, above = (open_["in_st"] - 0.5) / open_["points_st"], (open_["in_st"] + 0.5) / open_["points_st"]
    for min_overlap, alive in ((below, True), (above, False)):
        got = c.transformOverlap(cs, ct, T, method=OVERLAP, voxel=VOXEL, min_overlap=min_overlap)
        _same_stats(got, restate_overlap(s, t, T, VOXEL, min_overlap=min_overlap, tables=tables))
        assert (got["confidence"] > 0.0) == alive and got["in_st"] == open_["in_st"]
    # the target direction gates on its own share
    got = c.transformOverlap(ct, cs, np.linalg.inv(T_true).astype(np.float32), method=OVERLAP, voxel=VOXEL, min_overlap=0.5 * (share_st + share_ts))
    assert got["confidence"] == 0.0 and got["in_st"] > 0


def test_non_finite_and_zero_transforms_score_nothing(c, halves):
    s, t, T_true, _, _ = halves
    cs, ct = c.cloud(_records(s)), c.cloud(_records(t))
    nan = T_true.astype(np.float32).copy()
    nan[1, 2] = np.nan
    inf = T_true.astype(np.float32).copy()
    inf[0, 3] = np.inf
    for T in (nan, inf, np.zeros((4, 4), dtype=np.float32)):
        got = c.transformOverlap(cs, ct, T, method=OVERLAP, voxel=VOXEL)
        assert got == dict(points_st=len(s), in_st=0, hit_st=0, points_ts=len(t), in_ts=0, hit_ts=0, confidence=0.0)
    # a finite T that throws every point beyond the index limit: nothing counts, nothing is read out of bounds
    huge = np.eye(4, dtype=np.float32)
    huge[:3, 3] = [3e8, -3e8, 3e30]
    got = c.transformOverlap(cs, ct, huge, method=OVERLAP, voxel=VOXEL)
    _same_stats(got, restate_overlap(s, t, huge, VOXEL))
    assert got["in_st"] == 0 and got["confidence"] == 0.0


def test_empty_and_one_point_clouds(c, halves):
    s, _, _, _, _ = halves
    empty = c.cloud(_records(np.zeros((0, 3), dtype=np.float32)))
    one = np.array([[0.35, -0.05, 1.25]], dtype=np.float32)
    c_one, c_s = c.cloud(_records(one)), c.cloud(_records(s))
    eye = np.eye(4, dtype=np.float32)
    for a, b, na, nb in ((empty, c_s, 0, len(s)), (c_s, empty, len(s), 0), (empty, empty, 0, 0)):
        assert c.transformOverlap(a, b, eye, method=OVERLAP, voxel=VOXEL) == dict(points_st=na, in_st=0, hit_st=0, points_ts=nb, in_ts=0,
                                                                                   hit_ts=0, confidence=0.0)
    got = c.transformOverlap(c_one, c_one, eye, method=OVERLAP, voxel=VOXEL)                    # one point is not a seen cell
    assert got == dict(points_st=1, in_st=0, hit_st=0, points_ts=1, in_ts=0, hit_ts=0, confidence=0.0)
    got = c.transformOverlap(c_one, c_one, eye, method=OVERLAP, voxel=VOXEL, min_points=1)
    assert got == dict(points_st=1, in_st=1, hit_st=1, points_ts=1, in_ts=1, hit_ts=1, confidence=1.0)
    _same_stats(got, restate_overlap(one, one, eye, VOXEL, min_points=1))
    shift = eye.copy()
    shift[0, 3] = 0.25                                       # two voxels and a half away, still inside the view cell: in, no hit
    got = c.transformOverlap(c_one, c_one, shift, method=OVERLAP, voxel=VOXEL, min_points=1)
    _same_stats(got, restate_overlap(one, one, shift, VOXEL, min_points=1))
    assert (got["in_st"], got["hit_st"]) == (1, 0) and got["confidence"] == 0.0


# ---------------------------------------------------------------- 4. limits
def test_limits_are_unsupported_and_the_context_survives(mm, c):
    far = np.array([[0.0, 0.0, 0.0], [1e5, 1e5, 1e5]], dtype=np.float32)          # 2.5e5 bricks per axis at 0.1 m
    beyond = np.array([[0.0, 0.0, 0.0], [0.0, 2e8, 0.0]], dtype=np.float32)       # voxel 2e9 >= 2^30
    ok = c.cloud(_records(box_room(1, 2000)[0]))
    for pts in (far, beyond):
        cl = c.cloud(_records(pts))
        with pytest.raises(mm.Mm3dError) as e:
            c.debugOverlapTable(cl, method=OVERLAP, voxel=VOXEL)
        assert e.value.status == EUNSUPPORTED
        for a, b in ((cl, ok), (ok, cl)):
            with pytest.raises(mm.Mm3dError) as e:
                c.transformOverlap(a, b, np.eye(4), method=OVERLAP, voxel=VOXEL)
            assert e.value.status == EUNSUPPORTED
    # at a voxel that fits, the same clouds are fine, and the context goes on working
    got = c.transformOverlap(c.cloud(_records(far)), c.cloud(_records(far)), np.eye(4), method=OVERLAP, voxel=1000.0, min_points=1)
    assert got["confidence"] == 1.0
    _check_table(c, box_room(1, 2000)[0])


# ---------------------------------------------------------------- 5 - 6. end to end, default path
@pytest.fixture(scope="module")
def scene(synth):
    _, maps = synth.synth_maps(3, 20000, overlap_step=0.4)
    return [synth.pack_points(x, col) for x, col, _ in maps], [T for _, _, T in maps]


def _params(mm, method=MATCHING, **kw):
    return mm.MapMergingParams(descriptor_type=2, estimation_method=method, **kw)


def _ctx(mm, streams=1, cache=0, method_first=True, confidence=OVERLAP, **kw):
    c = mm.Context(0)
    c.setKeypoints(source=1)                              # uniform keypoints: every map is live
    if method_first and confidence is not None:
        c.setConfidence(method=confidence, **kw)
    c.setStreams(streams)
    if not method_first and confidence is not None:
        c.setConfidence(method=confidence, **kw)
    if cache:
        c.setMapCache(cache)
    return c


def _run(c, clouds, p, seed=1):
    if seed is not None:
        c.srand(seed)
    T, pairs = c.estimateMapsTransforms(clouds, p, return_pairs=True)
    return np.stack(T), pairs


def _same(a, b):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8))


def _same_but_confidence(a, b):
    assert len(a) == len(b)
    for name in a.dtype.names:
        if name != "confidence":
            assert np.array_equal(np.ascontiguousarray(a[name]).view(np.uint8), np.ascontiguousarray(b[name]).view(np.uint8)), name


@pytest.fixture(scope="module")
def runs(mm, scene):
    clouds, _ = scene
    p = _params(mm)
    c = _ctx(mm, 1)
    ovl = _run(c, clouds, p)
    return ovl, c.lastConfidenceStats(), _run(_ctx(mm, 1, confidence=None), clouds, p)


def test_end_to_end_records(mm, synth, scene, runs):
    clouds, T_gt = scene
    (_, pairs), last, (_, ref_pairs) = runs
    p = _params(mm)
    assert len(pairs) == 3
    # every other field is what it would have been
    _same_but_confidence(pairs, ref_pairs)
    assert (ref_pairs["confidence"] > 0).all() and np.isfinite(ref_pairs["confidence"]).all()
    assert ((pairs["confidence"] >= 0.0) & (pairs["confidence"] <= 1.0)).all()
    # the confidence is the stage-level call's at the record's transform, bit for bit
    c = mm.Context(0)
    c.setKeypoints(source=1)
    maps = [c.mapFeatures(c.cloud(x), p) for x in clouds]
    for r, q in zip(pairs, ref_pairs):
        s, t = int(r["source_idx"]), int(r["target_idx"])
        T = r["transform"].reshape(4, 4).T
        st = c.transformOverlap(maps[s].points, maps[t].points, T, method=OVERLAP, voxel=DEFAULT_MULTIPLE * p.resolution)
        err = np.linalg.norm(T.astype(np.float64) - synth.relative_gt(T_gt[s], T_gt[t]))
        print(s, t, "Frobenius", err, "overlap", st, "reference", float(q["confidence"]))
        assert _bits(st["confidence"]) == _bits(r["confidence"])
        assert st["points_st"] == len(maps[s].points) and st["points_ts"] == len(maps[t].points)
    assert last == st                                      # mm3d_last_confidence_stats: the last pair's counts
    c.close()


def test_records_do_not_depend_on_streams_driver_or_cache(mm, scene, runs):
    clouds, _ = scene
    one = runs[0]
    p = _params(mm)
    _same(one, _run(_ctx(mm, 8), clouds, p))
    _same(one, _run(_ctx(mm, 8, method_first=False), clouds, p))      # set after mm3d_set_streams: the helpers follow
    _same(one, _run(_ctx(mm, 1, voxel=DEFAULT_MULTIPLE * p.resolution), clouds, p))
    # mm3d_pair_estimate against the whole call
    c = _ctx(mm, 1)
    maps = [c.mapFeatures(c.cloud(x), p) for x in clouds]
    for m in maps[:2]:
        c.mapPrepare(m, p)                                 # (the third map's table is made on first use)
    for r in one[1]:
        got = c.pairEstimate(maps[int(r["source_idx"])], maps[int(r["target_idx"])], p)
        for name in ("transform", "confidence", "icp_iterations", "n_correspondences", "n_inliers", "icp_correspondences"):
            assert np.array_equal(np.ascontiguousarray(got[name]).view(np.uint8), np.ascontiguousarray(r[name]).view(np.uint8)), name
    assert c.pairEstimate(maps[0], maps[1], p, execute=False)["confidence"] == 0.0
    c.close()


@pytest.mark.parametrize("streams", [1, 8])
def test_map_cache_keys_the_confidence(mm, scene, runs, streams):
    clouds, _ = scene
    one, _, ref = runs
    p = _params(mm)
    c = _ctx(mm, streams, cache=16)
    _same(one, _run(c, clouds, p))
    c.mapCacheStats(reset=True)
    _same(one, _run(c, clouds, p))                         # served from the cache
    st = c.mapCacheStats(reset=True)
    assert st["pairs_reused"] == 3 and st["map_hits"] == 3
    # another voxel: the maps hit, no pair record is reused, the cached maps' tables are rebuilt
    wide = _run(_ctx(mm, 1, voxel=0.4), clouds, p)
    c.setConfidence(method=OVERLAP, voxel=0.4)
    _same(wide, _run(c, clouds, p))
    st = c.mapCacheStats(reset=True)
    assert st["map_hits"] == 3 and st["pairs_reused"] == 0 and st["pairs_computed"] == 3
    _same_but_confidence(wide[1], one[1])
    assert not np.array_equal(wide[1]["confidence"], one[1]["confidence"])
    # back to the reference: 1 / score again, and no overlap record is taken for it
    c.setConfidence(method=REFERENCE)
    _same(ref, _run(c, clouds, p))
    assert c.mapCacheStats(reset=True)["pairs_reused"] == 0
    c.setConfidence(method=OVERLAP)
    _same(one, _run(c, clouds, p))
    assert c.mapCacheStats(reset=True)["pairs_reused"] == 3
    c.close()


def test_generator_ends_where_the_reference_run_ends(mm, scene):
    """SAC-IA draws from the context's rand() replay: after a call with the overlap confidence the generator stands where it
    stands after the same call with the reference's, so a second call without mm3d_srand gives the same records."""
    clouds, _ = scene
    p = _params(mm, SAC_IA)
    a, b = _ctx(mm, 1), _ctx(mm, 1, confidence=None)
    first = _run(a, clouds[:2], p, seed=5), _run(b, clouds[:2], p, seed=5)
    _same_but_confidence(first[0][1], first[1][1])
    second = _run(a, clouds[:2], p, seed=None), _run(b, clouds[:2], p, seed=None)
    _same_but_confidence(second[0][1], second[1][1])
    assert not np.array_equal(first[0][1]["transform"], second[0][1]["transform"])     # the generator did move
    a.close()
    b.close()


def test_default_path(mm, scene, runs):
    clouds, _ = scene
    p = _params(mm)
    never = runs[2]
    c = _ctx(mm, 1, confidence=REFERENCE, voxel=0.3, min_points=2)     # the reference reads none of the options
    _same(never, _run(c, clouds, p))
    c.setConfidence(method=OVERLAP)
    c.setConfidence(method=REFERENCE)
    _same(never, _run(c, clouds, p))
    c.close()

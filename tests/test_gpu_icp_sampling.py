"""ICP source sampling (mm3d_set_icp_sampling, mm3d_sample_icp_source, mm3d_estimate_transform_icp_sampled) on the device: flags,
indices and statistics equal to the numpy restatement of tests/icp_sampling_cases.py, the stage calls composed of the sample and
the plain ICP bit for bit, the pair stage's records, the cache key, the refusals, and the grooved plane."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import icp_sampling_cases as K
from test_gpu_icp_plane import restate_icp_plane
from test_icp_sampling_cpu import GOLDEN, ICP, LOST_MM, RECOVERED_MM, SEEDS

pytestmark = pytest.mark.gpu

SAC_IA, MATCHING = 1, 0
EINVAL, EUNSUPPORTED = -1, -4
NDT = 1


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _device_sample(c, xyz, nrm, **o):
    """(keep flags, indices, stats) as the device makes them; the sample cloud must be the kept records, in order."""
    pts = c.cloud(K.records(xyz))
    normals = c.normals(K.normal_records(nrm)) if nrm is not None else None
    cloud, idx = c.sampleIcpSource(pts, normals, **o)
    got = cloud.numpy()
    keep = np.zeros(len(xyz), dtype=bool)
    keep[idx] = True
    assert len(idx) == len(cloud) and (np.diff(idx) > 0).all()
    want = K.records(xyz)[idx]
    assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), "the sample is not the kept records in order"
    return keep, idx, c.lastIcpSamplingStats()


def _exact(c, xyz, nrm, method, fraction=0.25, max_points=0, bins=4):
    keep_ref, idx_ref, st_ref, _ = K.restate_sample(xyz, nrm, method, fraction, max_points, bins)
    keep, idx, st = _device_sample(c, xyz, nrm if method == K.NORMAL_SPACE else None, method=method, fraction=fraction,
                                   max_points=max_points, bins=bins)
    what = (len(xyz), method, fraction, max_points, bins)
    assert st == st_ref, (what, st, st_ref)
    assert np.array_equal(keep, keep_ref), (what, np.flatnonzero(keep != keep_ref)[:8])
    assert np.array_equal(idx, idx_ref), what
    return st


# ---------------------------------------------------------------- 1. device against restatement, exact
@pytest.mark.parametrize("n", K.SIZES)
def test_one_bucket_ranks_run_across_waves_and_blocks(ctx, n):
    rng = np.random.default_rng(100 + n)
    xyz, nrm = K._points(rng, n), K.normals_one_bucket(rng, n)
    for fraction, cap in ((0.25, 0), (1.0, 0), (0.04, 0), (0.5, 1), (0.37, 0)):
        st = _exact(ctx, xyz, nrm, K.NORMAL_SPACE, fraction, cap)
        assert st["buckets"] == 1 and st["valid"] == n
    _exact(ctx, xyz, nrm, K.STRIDE, 0.1)
    _exact(ctx, xyz, nrm, K.STRIDE, 1.0)


@pytest.mark.parametrize("bins", [1, 2, 4, 8])
@pytest.mark.parametrize("n", K.SIZES)
def test_bucket_changes_with_every_point(ctx, n, bins):
    rng = np.random.default_rng(200 + n)
    xyz, nrm = K._points(rng, n), K.normals_cycling(rng, n, bins)
    st = _exact(ctx, xyz, nrm, K.NORMAL_SPACE, 0.25, 0, bins)
    assert st["buckets"] == min(n, 3 * bins * bins)
    _exact(ctx, xyz, nrm, K.NORMAL_SPACE, 0.6, 0, bins)
    _exact(ctx, xyz, rng.normal(size=(n, 3)).astype(np.float32), K.NORMAL_SPACE, 0.3, 0, bins)


@pytest.mark.parametrize("bins", [1, 2, 4, 8])
@pytest.mark.parametrize("n", K.SIZES)
def test_edges_ties_antipodes_and_invalid_points(ctx, n, bins):
    rng = np.random.default_rng(300 + n)
    xyz, nrm = K._points(rng, n), K.normals_edges(rng, n, bins)
    _exact(ctx, xyz, nrm, K.NORMAL_SPACE, 0.5, 0, bins)
    sx, sn = K.spoil(rng, xyz, nrm)
    st = _exact(ctx, sx, sn, K.NORMAL_SPACE, 0.5, 0, bins)
    assert n < 8 or st["valid"] < n
    st = _exact(ctx, sx, sn, K.NORMAL_SPACE, 1.0, 0, bins)
    assert st["sampled"] == st["valid"]
    st = _exact(ctx, sx, sn, K.STRIDE, 0.5)                   # (a stride reads no normals: only the coordinates can spoil a point)
    assert st["valid"] == int(np.isfinite(sx).all(axis=1).sum())


def test_waterfill_cases_on_the_device(ctx):
    rng = np.random.default_rng(4)
    n = 4097
    xyz = K._points(rng, n)
    # equal counts and a remainder shared among tied buckets: bins 1 has three buckets, 300 points cycle through them
    cyc = K.normals_cycling(rng, 300, 1)
    for cap in (99, 100, 101, 2, 1):
        st = _exact(ctx, xyz[:300], cyc, K.NORMAL_SPACE, 1.0, cap, 1)
        assert (st["sampled"], st["buckets"], st["level"]) == (cap, 3, cap // 3)
    # one bucket with 90 % of the points beside singletons: every singleton is kept
    ns = 1910                                                 # 191 singletons, one for every other bucket of bins 8, and 1719 = 90 %
    skew = K.skewed(rng, ns, 8)
    st = _exact(ctx, xyz[:ns], skew, K.NORMAL_SPACE, 0.15, 0, 8)
    aux = K.restate_sample(xyz[:ns], skew, K.NORMAL_SPACE, 0.15, 0, 8)[3]
    assert (aux["counts"] == 1).sum() == 191 and aux["counts"].max() == 1719 and st["buckets"] == 192
    assert (aux["take"][aux["counts"] == 1] == 1).all() and st["level"] == aux["take"].max() == 286 - 191
    skew = K.skewed(rng, n, 4)
    # m >= n_valid: all valid points; m = 1
    st = _exact(ctx, xyz, skew, K.NORMAL_SPACE, 1.0, 0, 4)
    assert st["sampled"] == st["valid"] == n
    st = _exact(ctx, xyz, skew, K.NORMAL_SPACE, 1.0, 10 ** 9, 4)
    assert st["sampled"] == n
    st = _exact(ctx, xyz, skew, K.NORMAL_SPACE, 0.5, 1, 4)
    assert st["sampled"] == 1 and st["level"] == 0


def test_several_blocks_of_random_normals(ctx):
    rng = np.random.default_rng(5)
    n = 20011                                                 # 20 blocks of 1024 points, the last one partial
    xyz, nrm = K._points(rng, n), rng.normal(size=(n, 3)).astype(np.float32)
    sx, sn = K.spoil(rng, xyz, nrm)
    for bins in (1, 2, 4, 8):
        _exact(ctx, sx, sn, K.NORMAL_SPACE, 0.1, 0, bins)
    _exact(ctx, sx, sn, K.NORMAL_SPACE, 0.9, 5000, 8)
    _exact(ctx, sx, sn, K.STRIDE, 0.013)


# ---------------------------------------------------------------- 2. surface, refusals, empty input
def test_surface_and_refusals(mm):
    c = mm.Context(0)
    lib = mm.lib()
    assert c.getIcpSampling().as_tuple() == (K.NONE, 0.25, 0, 4)
    c.setIcpSampling(method=K.NORMAL_SPACE, fraction=0.1, bins=8, max_points=5000)
    assert c.getIcpSampling().as_tuple() == (K.NORMAL_SPACE, 0.1, 5000, 8)
    for bad in (dict(method=3), dict(method=-1), dict(fraction=0.0), dict(fraction=1.5), dict(fraction=float("nan")), dict(bins=3),
                dict(bins=0), dict(bins=16), dict(max_points=-1)):
        o = mm.IcpSamplingOptions(**bad)
        assert lib.mm3d_set_icp_sampling(c._h, C.byref(o)) == EINVAL, bad
    assert c.getIcpSampling().as_tuple() == (K.NORMAL_SPACE, 0.1, 5000, 8)
    assert lib.mm3d_set_icp_sampling(c._h, None) == EINVAL and lib.mm3d_last_icp_sampling_stats(c._h, None) == EINVAL
    # beside NDT, colour and generalized ICP: refused either way round, with the code the opt-ins use against each other
    for setter, on, off in ((c.setRefinement, dict(method=NDT), dict(method=0)), (c.setIcpColor, dict(enabled=1), dict(enabled=0)),
                            (c.setIcpGeneralized, dict(enabled=1), dict(enabled=0))):
        with pytest.raises(mm.Mm3dError) as e:
            setter(**on)
        assert e.value.status == EUNSUPPORTED
        c.setIcpSampling(method=K.NONE)
        setter(**on)
        with pytest.raises(mm.Mm3dError) as e:
            c.setIcpSampling(method=K.STRIDE)
        assert e.value.status == EUNSUPPORTED
        c.setIcpSampling(method=K.NONE, fraction=0.5)         # NONE is always accepted
        setter(**off)
        c.setIcpSampling(method=K.NORMAL_SPACE)
    # it combines with point-to-plane and with the rejection
    c.setIcpMethod(1)
    c.setIcpRejection(distance=1, overlap_ratio=0.7)
    # shards and device lists
    cloud = K.records(K._points(np.random.default_rng(1), 2000))
    with pytest.raises(mm.Mm3dError) as e:
        c.shardBegin([cloud, cloud], mm.MapMergingParams(descriptor_type=2), 0, 1)
    assert e.value.status == EUNSUPPORTED
    c.close()
    d = mm.Context(devices=[0])
    o = mm.IcpSamplingOptions(method=K.STRIDE)
    assert lib.mm3d_set_icp_sampling(d._h, C.byref(o)) == EUNSUPPORTED
    assert d.getIcpSampling().as_tuple() == (K.NONE, 0.25, 0, 4)
    d.setIcpSampling(method=K.NONE)
    d.close()


def test_stage_calls_check_their_arguments(mm):
    c = mm.Context(0)
    rng = np.random.default_rng(2)
    xyz = K._points(rng, 500)
    pts, nrm = c.cloud(K.records(xyz)), c.normals(K.normal_records(rng.normal(size=(500, 3))))
    short = c.normals(K.normal_records(rng.normal(size=(499, 3))))
    for call in (lambda: c.sampleIcpSource(pts, None, method=K.NORMAL_SPACE), lambda: c.sampleIcpSource(pts, short, method=K.NORMAL_SPACE),
                 lambda: c.sampleIcpSource(pts, nrm, method=K.NONE), lambda: c.sampleIcpSource(pts, nrm, method=K.STRIDE, fraction=2.0),
                 lambda: c.estimateTransformICPSampled(pts, None, pts, nrm, np.eye(4), 1.0, method=K.NORMAL_SPACE),
                 lambda: c.estimateTransformICPSampled(pts, short, pts, nrm, np.eye(4), 1.0, method=K.NORMAL_SPACE),
                 lambda: c.estimateTransformICPSampled(pts, nrm, pts, short, np.eye(4), 1.0, method=K.STRIDE),
                 lambda: c.estimateTransformICPSampled(pts, nrm, pts, nrm, np.eye(4), 1.0, method=K.STRIDE, bins=5)):
        with pytest.raises(mm.Mm3dError) as e:
            call()
        assert e.value.status == EINVAL
    c.close()


def test_empty_and_all_invalid_sources_return_the_guess(mm):
    c = mm.Context(0)
    rng = np.random.default_rng(3)
    tgt = K._points(rng, 3000)
    t_cloud, t_nrm = c.cloud(K.records(tgt)), c.normals(K.normal_records(rng.normal(size=(3000, 3))))
    guess = np.eye(4, dtype=np.float32)
    guess[:3, 3] = [0.25, -0.5, 0.125]
    empty = np.zeros((0, 3), dtype=np.float32)
    nan_pts = np.full((700, 3), np.nan, dtype=np.float32)
    zero_nrm = np.zeros((700, 3), dtype=np.float32)
    cases = [(empty, empty, K.STRIDE), (empty, empty, K.NORMAL_SPACE), (nan_pts, zero_nrm, K.STRIDE), (tgt[:700], zero_nrm, K.NORMAL_SPACE),
             (tgt[:700], np.full((700, 3), np.nan, dtype=np.float32), K.NORMAL_SPACE)]
    for xyz, nrm, method in cases:
        s_cloud, s_nrm = c.cloud(K.records(xyz)), c.normals(K.normal_records(nrm))
        sample, idx = c.sampleIcpSource(s_cloud, s_nrm, method=method, fraction=0.5)
        st = c.lastIcpSamplingStats()
        assert len(sample) == len(idx) == 0 and st == dict(points=len(xyz), valid=0, sampled=0, buckets=0, level=0)
        for normals in (None, t_nrm):
            T = c.estimateTransformICPSampled(s_cloud, s_nrm, t_cloud, normals, guess, 1.0, method=method, fraction=0.5, max_iterations=20)
            assert np.array_equal(_bits(T), _bits(guess)) and c.last_icp_iterations == 0
    c.close()


# ---------------------------------------------------------------- 3. the stage call is the sample followed by the plain call
@pytest.fixture(scope="module")
def room():
    """A box room sampled twice, a pose between the two and a guess near it; exact normals."""
    from test_gpu_icp_plane import _problem, box_room
    tgt, tn, src, T_true, guess = _problem(5, 6000)
    sn = (np.linalg.inv(T_true)[:3, :3] @ box_room(5, 6000)[1].astype(np.float64).T).T.astype(np.float32)
    return src, sn, tgt, tn, guess


def test_full_fraction_is_the_plain_icp_bit_for_bit(mm, room):
    src, sn, tgt, tn, guess = room
    c = mm.Context(0)
    s, t = c.cloud(K.records(src)), c.cloud(K.records(tgt))
    s_nrm, t_nrm = c.normals(K.normal_records(sn)), c.normals(K.normal_records(tn))
    plane = c.estimateTransformICPPlane(s, t, t_nrm, guess, 1.0, 30, 1e-9)
    it_plane = c.last_icp_iterations
    point = c.estimateTransformICP(s, t, guess, 1.0, 0.0, 30, 1e-9)
    it_point = c.last_icp_iterations
    assert it_plane >= 2 and it_point >= 2
    for method in (K.NORMAL_SPACE, K.STRIDE, K.NONE):
        T = c.estimateTransformICPSampled(s, s_nrm, t, t_nrm, guess, 1.0, method=method, fraction=1.0, max_iterations=30, transformation_epsilon=1e-9)
        assert np.array_equal(_bits(T), _bits(plane)) and c.last_icp_iterations == it_plane, method
        T = c.estimateTransformICPSampled(s, s_nrm, t, None, guess, 1.0, method=method, fraction=1.0, max_iterations=30, transformation_epsilon=1e-9)
        assert np.array_equal(_bits(T), _bits(point)) and c.last_icp_iterations == it_point, method
    c.close()


@pytest.mark.parametrize("o", [dict(method=K.NORMAL_SPACE, fraction=0.25), dict(method=K.NORMAL_SPACE, fraction=0.04, bins=8),
                               dict(method=K.NORMAL_SPACE, fraction=0.9, max_points=300, bins=2), dict(method=K.STRIDE, fraction=0.1)])
def test_stage_call_is_sample_then_plain_call(mm, room, o):
    src, sn, tgt, tn, guess = room
    c = mm.Context(0)
    s, t = c.cloud(K.records(src)), c.cloud(K.records(tgt))
    s_nrm, t_nrm = c.normals(K.normal_records(sn)), c.normals(K.normal_records(tn))
    sample, idx = c.sampleIcpSource(s, s_nrm, **o)
    assert np.array_equal(idx, K.restate_sample(src, sn, o["method"], o["fraction"], o.get("max_points", 0), o.get("bins", 4))[1])
    want = c.estimateTransformICPPlane(sample, t, t_nrm, guess, 1.0, 30, 1e-9)
    it = c.last_icp_iterations
    T = c.estimateTransformICPSampled(s, s_nrm, t, t_nrm, guess, 1.0, max_iterations=30, transformation_epsilon=1e-9, **o)
    assert np.array_equal(_bits(T), _bits(want)) and c.last_icp_iterations == it and it >= 1
    assert c.lastIcpSamplingStats()["sampled"] == len(sample)
    want = c.estimateTransformICP(sample, t, guess, 1.0, 0.0, 30, 1e-9)
    it = c.last_icp_iterations
    T = c.estimateTransformICPSampled(s, s_nrm, t, None, guess, 1.0, max_iterations=30, transformation_epsilon=1e-9, **o)
    assert np.array_equal(_bits(T), _bits(want)) and c.last_icp_iterations == it
    c.close()


# ---------------------------------------------------------------- 4. the pair stage
@pytest.fixture(scope="module")
def clouds(synth):
    _, maps = synth.synth_maps(4, 30000, overlap_step=0.4)
    return [synth.pack_points(x, col) for x, col, _ in maps]


NS = dict(method=K.NORMAL_SPACE, fraction=0.25)


def _params(mm, method=SAC_IA, **kw):
    return mm.MapMergingParams(descriptor_type=2, estimation_method=method, **kw)


def _ctx(mm, streams=1, o=NS, icp_method=0, cache=0, setter_first=True):
    c = mm.Context(0)
    if setter_first and o:
        c.setIcpSampling(**o)
    c.setStreams(streams)
    if not setter_first and o:
        c.setIcpSampling(**o)
    c.setIcpMethod(icp_method)
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


@pytest.mark.parametrize("icp_method", [0, 1])
def test_records_are_the_stage_calls_and_the_confidence_is_the_full_sources(mm, clouds, icp_method):
    cs = clouds[:3]
    p = _params(mm)
    c1 = _ctx(mm, 1, icp_method=icp_method)
    one = _run(c1, cs, p)
    assert len(one[1]) >= 2 and one[1]["icp_iterations"].max() > 0
    _same(one, _run(_ctx(mm, 4, icp_method=icp_method), cs, p))
    _same(one, _run(_ctx(mm, 4, icp_method=icp_method, setter_first=False), cs, p))      # set after mm3d_set_streams: the helpers follow
    # it does something, and a context set and then reset to NONE gives the bytes of a fresh one
    fresh = _run(_ctx(mm, 1, None, icp_method), cs, p)
    assert not np.array_equal(one[1].view(np.uint8), fresh[1].view(np.uint8))
    back = _ctx(mm, 1, icp_method=icp_method)
    back.setIcpSampling(method=K.NONE)
    _same(fresh, _run(back, cs, p))
    # with refine_transform 0 no ICP runs and nothing is sampled: the default's records -- which are each pair's pre-ICP guess
    guesses = _run(c1, cs, _params(mm, refine_transform=0))[1]
    assert np.array_equal(guesses.view(np.uint8), _run(_ctx(mm, 1, None, icp_method), cs, _params(mm, refine_transform=0))[1].view(np.uint8))
    maps = [c1.mapFeatures(c1.cloud(x), p) for x in cs]
    nrm = [c1.computeSurfaceNormals(m.points, p.normal_radius) for m in maps]
    for g, r in zip(guesses, one[1]):
        s, t = int(r["source_idx"]), int(r["target_idx"])
        assert (int(g["source_idx"]), int(g["target_idx"])) == (s, t)
        T = c1.estimateTransformICPSampled(maps[s].points, nrm[s], maps[t].points, nrm[t] if icp_method else None, g["transform"].reshape(4, 4).T,
                                           p.max_correspondence_distance, max_iterations=p.max_iterations,
                                           transformation_epsilon=p.transform_epsilon, **NS)
        assert np.array_equal(T.T.reshape(16).view(np.uint32), r["transform"].view(np.uint32))
        assert c1.last_icp_iterations == int(r["icp_iterations"])
        st = c1.lastIcpSamplingStats()
        assert st["points"] == len(maps[s].points) and st["sampled"] == int(0.25 * st["valid"]) < st["points"]
        assert int(r["icp_correspondences"]) <= st["sampled"]                # (they count sampled points)
        # the confidence stays 1 / transformScore over the FULL source
        score = c1.transformScore(maps[s].points, maps[t].points, r["transform"].reshape(4, 4).T, p.max_correspondence_distance)
        assert np.float64(1.0 / score).tobytes() == np.float64(r["confidence"]).tobytes()


def test_rejection_runs_on_the_sample(mm, clouds):
    cs = clouds[:3]
    p = _params(mm)
    c = _ctx(mm, 1)
    c.setIcpRejection(distance=1, overlap_ratio=0.7)
    one = _run(c, cs, p)
    st, smp = c.last_icp_rejection_stats, c.lastIcpSamplingStats()
    last = one[1][-1]
    assert st["kept"] == int(last["icp_correspondences"]) and st["iterations"] == int(last["icp_iterations"]) > 0
    assert 0 < st["kept"] <= st["matched"] <= smp["sampled"] < smp["points"]                  # the statistics count sampled points
    plain = _ctx(mm, 1, None)
    plain.setIcpRejection(distance=1, overlap_ratio=0.7)
    _run(plain, cs, p)
    assert plain.last_icp_rejection_stats["matched"] > 2 * st["matched"]                       # (the full source matches four times as many)
    four = _ctx(mm, 4)
    four.setIcpRejection(distance=1, overlap_ratio=0.7)
    _same(one, _run(four, cs, p))


def test_cache_key_and_untouched_default(mm, clouds):
    cs = clouds[:3]
    p = _params(mm, MATCHING)
    other = dict(method=K.NORMAL_SPACE, fraction=0.1)
    ref = {k: _run(_ctx(mm, 1, o), cs, p) for k, o in (("none", None), ("ns", NS), ("other", other), ("stride", dict(method=K.STRIDE)))}
    assert not np.array_equal(ref["ns"][1].view(np.uint8), ref["other"][1].view(np.uint8))
    c = _ctx(mm, 1, None, cache=64)
    _same(_run(c, cs, p), ref["none"])
    n_pairs = len(ref["none"][1])
    c.mapCacheStats(reset=True)
    for k, o in (("ns", NS), ("other", other), ("stride", dict(method=K.STRIDE))):            # every map is hit, no pair is reused
        c.setIcpSampling(**o)
        _same(_run(c, cs, p), ref[k])
        st = c.mapCacheStats(reset=True)
        assert st["map_hits"] == 3 and st["pairs_reused"] == 0 and st["pairs_computed"] == n_pairs, (k, st)
    # NONE reads none of the other values: its records are the default's, whatever they are
    c.setIcpSampling(method=K.NONE, fraction=0.5, bins=8, max_points=9)
    _same(_run(c, cs, p), ref["none"])
    assert c.mapCacheStats(reset=True)["pairs_reused"] == n_pairs
    c.setIcpSampling(**NS)
    _same(_run(c, cs, p), ref["ns"])
    st = c.mapCacheStats(reset=True)
    assert st["pairs_reused"] == n_pairs and st["device_bytes"] > 0
    # a cached context in lockstep with a plain one when a map changes
    cached, plain = _ctx(mm, 4, cache=64), _ctx(mm, 4)
    _same(_run(cached, cs, p), ref["ns"])
    changed = cs[:2] + [clouds[3]]
    _same(_run(cached, changed, p), _run(plain, changed, p))


# ---------------------------------------------------------------- 5. the grooved plane
@pytest.fixture(scope="module")
def grooved():
    return K.grooved_problem(SEEDS[0])


def _device_icp(c, grooved, **o):
    src, sn, tgt, tn, T_true = grooved
    T = c.estimateTransformICPSampled(c.cloud(K.records(src)), c.normals(K.normal_records(sn)), c.cloud(K.records(tgt)),
                                      c.normals(K.normal_records(tn)), np.eye(4, dtype=np.float32), ICP["max_corr"],
                                      max_iterations=ICP["max_iter"], transformation_epsilon=ICP["eps"], **o)
    return T, 1000.0 * K.translation_error(T, T_true)


def test_grooved_plane_device_against_restatement(mm, grooved):
    src, sn, tgt, tn, T_true = grooved
    c = mm.Context(0)
    keep = K.restate_sample(src, sn, K.NORMAL_SPACE, 0.04, 0, 4)[0]
    T_ref, it_ref, conv_ref, _ = restate_icp_plane(src[keep], tgt, tn, np.eye(4, dtype=np.float32), ICP["max_corr"], ICP["max_iter"], ICP["eps"])
    T, err = _device_icp(c, grooved, method=K.NORMAL_SPACE, fraction=0.04)
    print("normal-space: |T - T_ref| %.3g, iterations %d / %d, %.2f mm" % (np.abs(T - T_ref).max(), c.last_icp_iterations, it_ref, err))
    assert np.abs(T - T_ref).max() < 1e-4
    assert err < RECOVERED_MM
    rec = json.load(open(GOLDEN))                             # the full cloud's restatement (tests/test_icp_sampling_cpu.py keeps it honest)
    assert rec["seed"] == SEEDS[0] and rec["icp"] == ICP
    T, err = _device_icp(c, grooved, method=K.NONE)
    print("full cloud: |T - T_ref| %.3g, iterations %d / %d, %.2f mm" % (np.abs(T - np.array(rec["T"])).max(), c.last_icp_iterations,
                                                                        rec["iterations"], err))
    assert np.abs(T - np.array(rec["T"])).max() < 1e-4
    assert err < RECOVERED_MM
    c.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_grooved_plane_ordering_on_the_device(mm, seed):
    g = K.grooved_problem(seed)
    c = mm.Context(0)
    ns = _device_icp(c, g, method=K.NORMAL_SPACE, fraction=0.04)[1]
    stride = _device_icp(c, g, method=K.STRIDE, fraction=0.04)[1]
    full = _device_icp(c, g, method=K.NONE)[1]
    print("seed %d: normal-space %.2f mm, stride %.2f mm, full cloud %.2f mm" % (seed, ns, stride, full))
    assert ns < RECOVERED_MM and full < RECOVERED_MM and stride > LOST_MM
    c.close()

"""Consistency-graph estimation (mm3d_set_estimator) on the device against the numpy restatement of consistency_cases.py: the
graph, the degrees, the seeds and the consensus sets bit for bit; the hypotheses, counts and the result; the degenerate inputs;
and the stage inside the pair pipeline."""
import ctypes as C

import numpy as np
import pytest

from consistency_cases import THRESHOLD, d2_float, identity_corr, kabsch, meets_the_conditions, points, restate, scene
from test_gpu_align_prerej import rounding_band

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4
MATCHING, SAC_IA = 0, 1
CONSISTENCY = 1


def _clouds(ctx, mm, p, q):
    return ctx.cloud(points(p, mm.POINT)), ctx.cloud(points(q, mm.POINT))


def _bits(T):
    return np.ascontiguousarray(T, dtype=np.float32).view(np.uint32)


def _check_graph(ctx, mm, p, q, corr, **opts):
    """Steps 1 to 4 on the device equal the restatement's, exactly; returns (device dict, restatement)."""
    s, t = _clouds(ctx, mm, p, q)
    o = mm.EstimatorOptions(**opts)
    g = ctx.consistencyGraph(s, t, corr, THRESHOLD, o)
    r = restate(p, q, corr, THRESHOLD, tolerance=o.tolerance, seeds=o.seeds, consensus=o.consensus)
    n = len(corr)
    assert g["rows"].shape == r["rows"].shape == (n, (n + 63) // 64)
    assert np.array_equal(g["rows"], r["rows"])
    if n % 64:                                            # the bits at and beyond C in the last word of every row
        assert not (g["rows"][:, -1] >> np.uint64(n % 64)).any()
    assert np.array_equal(g["deg"], r["deg"])
    assert np.array_equal(g["seeds"], r["seeds"])
    assert g["consensus"].shape == (len(r["seeds"]), o.consensus)
    for k, K in enumerate(r["consensus"]):
        row = g["consensus"][k]
        assert np.array_equal(row[:len(K)], K) and (row[len(K):] == -1).all(), (k, row, K)
    return g, r


# ---------------------------------------------------------------- 1. the graph, exactly
@pytest.mark.parametrize("n,frac", [(3, 0.05), (63, 0.05), (64, 0.05), (65, 0.05), (1500, 0.05), (4100, 0.05), (4100, 1.0)])
def test_graph_equals_the_restatement(mm, ctx, n, frac):
    p, q, _, _, _ = scene(2, n, frac)
    g, r = _check_graph(ctx, mm, p, q, identity_corr(n, mm.CORR))
    print("C", n, "share", frac, "edges", int(r["deg"].sum()) // 2, "seeds", len(r["seeds"]), "largest degree", int(r["deg"].max()))
    if n >= 1500:
        assert len(r["seeds"]) == 64 and all(len(K) == 20 for K in r["consensus"])


def test_graph_special_cases(mm, ctx):
    n = 200
    p, q, _, _, _ = scene(3, n, 0.3)
    corr = identity_corr(n, mm.CORR)
    # tolerance 0.1 beside the default
    g_def, r_def = _check_graph(ctx, mm, p, q, corr)
    g_tol, r_tol = _check_graph(ctx, mm, p, q, corr, tolerance=0.1)
    assert r_tol["deg"].sum() < r_def["deg"].sum() and r_tol["deg"].sum() > 0
    # two correspondences sharing a target index: never compatible with each other
    shared = corr.copy()
    shared["index_match"][7] = shared["index_match"][5]
    _, r = _check_graph(ctx, mm, p, q, shared)
    assert not r["A"][5, 7] and r["A"][5].any()
    # two coincident source keypoints: da = 0 fails da > t2
    p2 = p.copy()
    p2[11] = p2[10]
    _, r = _check_graph(ctx, mm, p2, q, corr)
    assert not r["A"][10, 11]
    # one coordinate that is not a number: its row and column are empty
    p3 = p.copy()
    p3[20, 1] = np.nan
    _, r = _check_graph(ctx, mm, p3, q, corr)
    assert not r["A"][20].any() and not r["A"][:, 20].any() and r["deg"].sum() > 0
    # a short seed list and small consensus sets
    _check_graph(ctx, mm, p, q, corr, seeds=5, consensus=3)
    _check_graph(ctx, mm, p, q, corr, seeds=4096, consensus=64)


# ---------------------------------------------------------------- 2. hypotheses and counts
@pytest.mark.parametrize("frac", [0.03, 0.05])
def test_hypotheses_counts_and_winner(mm, ctx, frac):
    n = 1500
    p, q, inl, _, _ = scene(1, n, frac)
    corr = identity_corr(n, mm.CORR)
    g, r = _check_graph(ctx, mm, p, q, corr)
    s, t = _clouds(ctx, mm, p, q)
    T, inliers, st = ctx.estimateTransformConsistency(s, t, corr, THRESHOLD)
    thr2 = THRESHOLD * THRESHOLD
    band = rounding_band(p, q, THRESHOLD)
    P64, Q64 = p.astype(np.float64), q.astype(np.float64)
    excused = 0
    for k, K in enumerate(r["consensus"]):
        Th = g["hypotheses"][k]
        if len(K) < 3:
            assert g["counts"][k] == -1 and not Th.any()
            continue
        assert np.abs(Th - kabsch(p[K], q[K])).max() <= 1e-4, (k, np.abs(Th - kabsch(p[K], q[K])).max())
        T64 = Th.astype(np.float64)
        d2 = (((P64 @ T64[:3, :3].T + T64[:3, 3]) - Q64) ** 2).sum(axis=1)
        near = int((np.abs(d2 - thr2) <= band).sum())
        excused += near
        assert abs(int((d2 < thr2).sum()) - int(g["counts"][k])) <= near, (k, int((d2 < thr2).sum()), int(g["counts"][k]), near)
    print("share", frac, "counts", g["counts"].tolist(), "excused", excused, "of", len(r["seeds"]) * n, "band", band, "stats", st)
    assert excused <= 1e-3 * len(r["seeds"]) * n
    # the winner is the first maximum of the device's own counts
    assert st["winner_rank"] == int(np.argmax(g["counts"])) and st["winner_index"] == int(g["seeds"][st["winner_rank"]])
    assert st["winner_inliers"] == int(g["counts"].max())
    assert st["correspondences"] == n and st["edges"] == int(r["deg"].sum()) // 2 and st["seeds"] == len(r["seeds"])
    assert st["hypotheses"] == sum(len(K) >= 3 for K in r["consensus"])


# ---------------------------------------------------------------- 3. the result
@pytest.mark.parametrize("frac,seed", [(0.03, 1), (0.03, 2), (0.03, 3), (0.03, 4), (0.03, 5), (0.05, 1), (0.2, 1)])
def test_result(mm, ctx, po, frac, seed):
    n = 1500
    p, q, inl, R, t = scene(seed, n, frac)
    corr = identity_corr(n, mm.CORR)
    corr["distance"] = np.arange(n, dtype=np.float32)          # (carried through to the inliers)
    sc, tc = _clouds(ctx, mm, p, q)
    g = ctx.consistencyGraph(sc, tc, corr, THRESHOLD)
    T, inliers, st = ctx.estimateTransformConsistency(sc, tc, corr, THRESHOLD)
    # the correspondences within the threshold under the winner's hypothesis, as the host's float arithmetic forms them
    Tw = g["hypotheses"][st["winner_rank"]]
    want = np.flatnonzero(d2_float(Tw, p, q).astype(np.float64) < THRESHOLD * THRESHOLD)
    assert np.array_equal(inliers["index_query"], want) and np.array_equal(inliers.view(np.uint8), corr[want].view(np.uint8))
    err = np.abs(T - kabsch(p[want], q[want])).max()
    held, others = meets_the_conditions(inliers["index_query"], inl)
    print("share", frac, "seed", seed, "held", held, "of", int(inl.sum()), "others", others, "|T - Kabsch|", err,
          "|R - R_true|", np.abs(T[:3, :3] - R).max(), "|t - t_true|", np.abs(T[:3, 3] - t).max(), st)
    assert err <= 1e-4, err
    # the reference's estimator on the same scene stays the oracle's, bit for bit
    T_ref, inl_ref, _, _ = po.ransac(points(p, po.POINT), points(q, po.POINT), corr, THRESHOLD)
    T_r, inl_r = ctx.estimateTransformFromCorrespondences(sc, tc, corr, THRESHOLD)
    assert np.array_equal(inl_r["index_query"], inl_ref["index_query"]) and np.array_equal(_bits(T_r), _bits(T_ref))
    # and the call is a function of its inputs: again, on another seed of the generators
    ctx.srand(77)
    T2, inliers2, st2 = ctx.estimateTransformConsistency(sc, tc, corr, THRESHOLD)
    ctx.srand(1)
    assert np.array_equal(_bits(T), _bits(T2)) and np.array_equal(inliers.view(np.uint8), inliers2.view(np.uint8)) and st == st2


# ---------------------------------------------------------------- 4. degenerate inputs
def test_degenerate_inputs(mm, ctx):
    L = mm.lib()
    p, q, _, _, _ = scene(4, 100, 0.5)
    sc, tc = _clouds(ctx, mm, p, q)
    for n in (0, 2):
        T, inliers, st = ctx.estimateTransformConsistency(sc, tc, identity_corr(n, mm.CORR), THRESHOLD)
        assert not T.any() and len(inliers) == 0 and st["correspondences"] == n and st["winner_rank"] == -1 and st["seeds"] == 0
        g = ctx.consistencyGraph(sc, tc, identity_corr(n, mm.CORR), THRESHOLD)
        assert len(g["seeds"]) == 0
    # no compatible pair: every target the same point
    same = ctx.cloud(points(np.tile(q[:1], (100, 1)), mm.POINT))
    T, inliers, st = ctx.estimateTransformConsistency(sc, same, identity_corr(100, mm.CORR), THRESHOLD)
    assert not T.any() and len(inliers) == 0 and st["edges"] == 0 and st["seeds"] == 0 and st["winner_index"] == -1
    # one correspondence too many
    big = np.zeros(32769, dtype=mm.CORR)
    big["index_query"] = big["index_match"] = np.arange(32769) % 100
    with pytest.raises(mm.Mm3dError) as e:
        ctx.estimateTransformConsistency(sc, tc, big, THRESHOLD)
    assert e.value.status == EUNSUPPORTED
    # an index out of range
    bad = identity_corr(10, mm.CORR)
    bad["index_match"][3] = 100
    with pytest.raises(mm.Mm3dError) as e:
        ctx.estimateTransformConsistency(sc, tc, bad, THRESHOLD)
    assert e.value.status == EINVAL
    # options out of range, on the setter and on the stage call
    c = mm.Context(0)
    for wrong in (dict(method=2), dict(tolerance=-1.0), dict(tolerance=float("nan")), dict(seeds=0), dict(seeds=4097), dict(consensus=2),
                  dict(consensus=65)):
        o = mm.EstimatorOptions(**wrong)
        assert L.mm3d_set_estimator(c._h, C.byref(o)) == EINVAL, wrong
        with pytest.raises(mm.Mm3dError) as e:
            ctx.estimateTransformConsistency(sc, tc, identity_corr(100, mm.CORR), THRESHOLD, o)
        assert e.value.status == EINVAL
    assert c.getEstimator().as_tuple() == mm.EstimatorOptions().as_tuple()
    c.setEstimator(method=CONSISTENCY, tolerance=0.25, seeds=9, consensus=7)
    assert c.getEstimator().as_tuple() == (CONSISTENCY, 0.25, 9, 7)
    assert c.lastEstimatorStats() == dict(correspondences=0, edges=0, seeds=0, hypotheses=0, winner_index=-1, winner_rank=-1, winner_inliers=0)
    # the shards of the multi-process form run RANSAC
    with pytest.raises(mm.Mm3dError) as e:
        c.shardBegin([points(p, mm.POINT)], mm.MapMergingParams(descriptor_type=2), 0, 1)
    assert e.value.status == EUNSUPPORTED
    c.close()
    # so does a device list
    d = mm.Context(devices=[0])
    assert L.mm3d_set_estimator(d._h, C.byref(mm.EstimatorOptions(method=CONSISTENCY))) == EUNSUPPORTED
    assert L.mm3d_set_estimator(d._h, C.byref(mm.EstimatorOptions())) == 0
    d.close()


# ---------------------------------------------------------------- 5. plumbing
@pytest.fixture(scope="module")
def clouds(synth):
    _, maps = synth.synth_maps(3, 10000)
    return [synth.pack_points(x, col) for x, col, _ in maps]


def _params(mm, method=MATCHING, **kw):
    return mm.MapMergingParams(descriptor_type=2, estimation_method=method, **kw)


def _ctx(mm, streams=1, cache=0, on=True, first=True):
    c = mm.Context(0)
    if on and first:
        c.setEstimator(method=CONSISTENCY)
    c.setStreams(streams)
    if on and not first:
        c.setEstimator(method=CONSISTENCY)
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


def test_pair_records_are_the_stage_calls(mm, clouds):
    """With refine_transform = 0 a pair record's transform, n_correspondences and n_inliers are mm3d_find_correspondences followed
    by mm3d_estimate_transform_consistency on the maps' parts, bit for bit; and mm3d_pair_estimate is the same pair."""
    p = _params(mm, refine_transform=0)
    c = _ctx(mm, 1)
    one = _run(c, clouds, p)
    assert len(one[1]) == 3
    maps = [c.mapFeatures(c.cloud(x), p) for x in clouds]
    for m in maps:
        c.mapPrepare(m, p)
    live = 0
    for r in one[1]:
        s, t = maps[int(r["source_idx"])], maps[int(r["target_idx"])]
        corr = c.findFeatureCorrespondences(s.descriptors, t.descriptors, int(p.matching_k))
        T, inliers, st = c.estimateTransformConsistency(s.keypoints, t.keypoints, corr, p.inlier_threshold, c.getEstimator())
        assert np.array_equal(_bits(T.T.reshape(16)), r["transform"].view(np.uint32))
        assert (int(r["n_correspondences"]), int(r["n_inliers"])) == (len(corr), len(inliers))
        rec = c.pairEstimate(s, t, p)
        assert c.lastEstimatorStats() == st
        for k in ("transform", "confidence", "icp_iterations", "n_correspondences", "n_inliers", "icp_correspondences"):
            assert np.atleast_1d(rec[k]).tobytes() == np.atleast_1d(r[k]).tobytes(), k
        live += len(inliers) >= 3
        print("pair", int(r["source_idx"]), int(r["target_idx"]), "correspondences", len(corr), "inliers", len(inliers), st)
    assert live >= 1
    c.close()


def test_bit_identical_across_streams_batches_cache_and_seeds(mm, clouds):
    p = _params(mm)
    one = _run(_ctx(mm, 1), clouds, p)
    assert len(one[1]) == 3
    for s in (2, 4):
        _same(one, _run(_ctx(mm, s), clouds, p))                       # the stream driver: batches of several pairs
    _same(one, _run(_ctx(mm, 4, first=False), clouds, p))             # set after mm3d_set_streams: the helpers follow
    _same(one, _run(_ctx(mm, 4), clouds, p, seed=9))                  # nothing is drawn
    for s in (1, 4):
        cached = _ctx(mm, s, cache=8)
        _same(one, _run(cached, clouds, p))
        _same(one, _run(cached, clouds, p, seed=5))                    # served from the cache
        assert cached.mapCacheStats()["pairs_reused"] == 3
    # a pair estimated alone = the same pair inside the call
    c = _ctx(mm, 1)
    maps = [c.mapFeatures(c.cloud(x), p) for x in clouds]
    for m in maps:
        c.mapPrepare(m, p)
    for r in one[1]:
        rec = c.pairEstimate(maps[int(r["source_idx"])], maps[int(r["target_idx"])], p)
        assert np.array_equal(np.asarray(rec["transform"]).view(np.uint32), r["transform"].view(np.uint32))
        assert float(rec["confidence"]) == float(r["confidence"])
    c.close()


def test_default_untouched_and_estimators_never_share_records(mm, clouds):
    cs = clouds[:2]
    for method in (MATCHING, SAC_IA):
        p = _params(mm, method)
        fresh = _run(_ctx(mm, 1, on=False), cs, p)
        back = _ctx(mm, 1)
        back.setEstimator(method=0)                                    # selected, then back to the reference's
        _same(fresh, _run(back, cs, p))
        _same(fresh, _run(_ctx(mm, 4, on=False), cs, p))
    p = _params(mm, SAC_IA)                                            # SAC_IA does not read the setting
    _same(_run(_ctx(mm, 1, on=False), cs, p), _run(_ctx(mm, 1), cs, p))
    # one cache, the two estimators in turn: neither is served the other's record
    p = _params(mm)
    c = _ctx(mm, 1, cache=8, on=False)
    ransac = _run(c, cs, p)
    c.setEstimator(method=CONSISTENCY)
    cons = _run(c, cs, p)
    assert c.mapCacheStats()["pairs_reused"] == 0 and c.mapCacheStats()["map_hits"] == 2
    _same(cons, _run(_ctx(mm, 1), cs, p))
    c.setEstimator(method=CONSISTENCY, seeds=32)                       # other options: another record
    _run(c, cs, p)
    assert c.mapCacheStats()["pairs_reused"] == 0
    c.setEstimator(method=0, seeds=32)                                 # RANSAC does not read them: its record is shared
    _same(ransac, _run(c, cs, p))
    assert c.mapCacheStats()["pairs_reused"] == 1
    c.setEstimator(method=CONSISTENCY)
    _same(cons, _run(c, cs, p))
    assert c.mapCacheStats()["pairs_reused"] == 2
    c.close()

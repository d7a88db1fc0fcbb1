"""mm3d_set_map_cache: estimateMapsTransforms with the feature / pair cache on gives the bits of a plain context, call after
call, whatever changed between the calls -- and skips the work of what did not.  Every case runs a caching context and a
plain one in lock-step from the same mm3d_srand and compares the transforms, the pair records (as bytes) and the map sizes
bit for bit after every call, then the cache's exact counters."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MATCHING, SAC_IA = 0, 1


@pytest.fixture(scope="module")
def all_clouds(synth):
    _, maps = synth.synth_maps(7, 30000, overlap_step=0.4)
    return [synth.pack_points(x, c) for x, c, _ in maps]


@pytest.fixture(scope="module")
def clouds(all_clouds):
    return all_clouds[:6]


def _pair(mm, streams, cache=64):
    a, b = mm.Context(0), mm.Context(0)
    for c in (a, b):
        c.setStreams(streams)
        c.srand(1)
    a.setMapCache(cache)
    assert a.getMapCache() == cache and b.getMapCache() == 0
    return a, b


def _call(c, clouds, params):
    T, pairs = c.estimateMapsTransforms(clouds, params, return_pairs=True)
    pts, kps = c.lastRunMapSizes()
    return np.stack(T), pairs, pts, kps


def _lockstep(cached, plain, clouds, params, seed=None):
    """One call on both contexts; the bits must agree.  Returns the number of pair records and the cache's counters of the call."""
    if seed is not None:
        cached.srand(seed)
        plain.srand(seed)
    a = _call(cached, clouds, params)
    b = _call(plain, clouds, params)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8))
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    return len(b[1]), cached.mapCacheStats(reset=True)


def _stats(hits, misses, reused, computed):
    return {"map_hits": hits, "map_misses": misses, "pairs_reused": reused, "pairs_computed": computed}


def _check(st, **want):
    got = {k: st[k] for k in ("map_hits", "map_misses", "pairs_reused", "pairs_computed")}
    assert got == _stats(**want), got


def _params(mm, method, **kw):
    return mm.MapMergingParams(descriptor_type=2, estimation_method=method, **kw)


@pytest.mark.parametrize("streams", [1, 4])
@pytest.mark.parametrize("method", [MATCHING, SAC_IA])
def test_repeat_hits_everything(mm, clouds, method, streams):
    a, b = _pair(mm, streams)
    try:
        p = _params(mm, method)
        P, st = _lockstep(a, b, clouds, p)
        _check(st, hits=0, misses=6, reused=0, computed=P)
        assert st["maps_held"] == 6 and st["device_bytes"] >= 6 * 30000 * 16
        P, st = _lockstep(a, b, clouds, p)
        # SAC_IA without mm3d_srand: the generator has moved on, so only the features are reused
        _check(st, hits=6, misses=0, reused=P if method == MATCHING else 0, computed=0 if method == MATCHING else P)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("streams", [1, 4])
@pytest.mark.parametrize("method", [MATCHING, SAC_IA])
def test_changed_maps_miss(mm, clouds, method, streams):
    a, b = _pair(mm, streams)
    try:
        p = _params(mm, method)
        _lockstep(a, b, clouds, p)
        changed = [c.copy() for c in clouds]
        changed[2]["x"][17] = np.nextafter(changed[2]["x"][17], np.float32(np.inf))     # one ulp
        changed[3]["rgba"][5] ^= 1                                                      # one colour bit
        P, st = _lockstep(a, b, changed, p)
        same = sum(1 for i in range(6) for j in range(i + 1, 6) if i not in (2, 3) and j not in (2, 3))
        _check(st, hits=4, misses=2, reused=same if method == MATCHING else 0, computed=P - same if method == MATCHING else P)
        # and back: the original maps 2 and 3 are still cached (capacity 64), their new versions too
        P, st = _lockstep(a, b, clouds, p)
        _check(st, hits=6, misses=0, reused=P if method == MATCHING else 0, computed=0 if method == MATCHING else P)
        assert st["maps_held"] == 8
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("streams", [1, 4])
@pytest.mark.parametrize("method", [MATCHING, SAC_IA])
def test_reorder_and_append(mm, all_clouds, method, streams):
    a, b = _pair(mm, streams)
    try:
        p = _params(mm, method)
        _lockstep(a, b, all_clouds[:6], p)
        order = [0, 2, 1, 5, 3, 4, 6]           # maps moved, a new robot at the end
        P, st = _lockstep(a, b, [all_clouds[k] for k in order], p)
        # a pair is reused when its two maps were a pair in the same source -> target order before
        same = sum(1 for i in range(7) for j in range(i + 1, 7) if order[i] < 6 and order[j] < 6 and order[i] < order[j])
        _check(st, hits=6, misses=1, reused=same if method == MATCHING else 0, computed=P - same if method == MATCHING else P)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("streams", [1, 4])
@pytest.mark.parametrize("method", [MATCHING, SAC_IA])
def test_parameters_in_the_keys(mm, clouds, method, streams):
    a, b = _pair(mm, streams)
    try:
        _lockstep(a, b, clouds, _params(mm, method))
        reuse = method == MATCHING
        # confidence_threshold is the pose graph's alone
        P, st = _lockstep(a, b, clouds, _params(mm, method, confidence_threshold=0.5))
        _check(st, hits=6, misses=0, reused=P if reuse else 0, computed=0 if reuse else P)
        # max_iterations is the pair stage's
        P, st = _lockstep(a, b, clouds, _params(mm, method, max_iterations=300))
        _check(st, hits=6, misses=0, reused=0, computed=P)
        # descriptor_radius is the features'
        P, st = _lockstep(a, b, clouds, _params(mm, method, descriptor_radius=0.7))
        _check(st, hits=0, misses=6, reused=0, computed=P)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("streams", [1, 4])
def test_sac_ia_with_srand_reuses_pairs(mm, clouds, streams):
    a, b = _pair(mm, streams)
    try:
        p = _params(mm, SAC_IA)
        P, st = _lockstep(a, b, clouds, p, seed=7)
        _check(st, hits=0, misses=6, reused=0, computed=P)
        P, st = _lockstep(a, b, clouds, p, seed=7)
        _check(st, hits=6, misses=0, reused=P, computed=0)
        # the generator state the reused pairs leave behind is the plain one's: an uncached continuation agrees
        P, st = _lockstep(a, b, clouds[:3], p)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("streams", [1, 4])
def test_stride_32_padding_does_not_count(mm, clouds, streams):
    def wide(c, pad):
        v = np.ascontiguousarray(c).view(np.uint32).reshape(-1, 4)
        w = np.zeros((len(c), 8), dtype=np.uint32)
        w[:, :3] = v[:, :3]
        w[:, 4] = v[:, 3]
        w[:, 3] = pad
        w[:, 5:] = pad + 1
        return w

    a, b = _pair(mm, streams)
    try:
        p = _params(mm, MATCHING)
        first = [wide(c, 0) for c in clouds]
        _lockstep(a, b, [(w.ctypes.data, len(w), 32, 16) for w in first], p)
        second = [wide(c, 0xdeadbeef) for c in clouds]
        P, st = _lockstep(a, b, [(w.ctypes.data, len(w), 32, 16) for w in second], p)
        _check(st, hits=6, misses=0, reused=P, computed=0)
        # and the packed form of the same points is the same map
        P, st = _lockstep(a, b, clouds, p)
        _check(st, hits=6, misses=0, reused=P, computed=0)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("streams", [1, 4])
@pytest.mark.parametrize("method", [MATCHING, SAC_IA])
def test_small_capacity_stays_exact(mm, clouds, method, streams):
    a, b = _pair(mm, streams, cache=3)
    try:
        p = _params(mm, method)
        for _ in range(3):
            P, st = _lockstep(a, b, clouds, p)
            assert st["maps_held"] <= 3
        # the last three maps of the call stay: they hit, their 3 pairs are reused (MATCHING)
        _check(st, hits=3, misses=3, reused=3 if method == MATCHING else 0, computed=P - 3 if method == MATCHING else P)
        a.setMapCache(2)
        assert a.getMapCache() == 2 and a.mapCacheStats()["maps_held"] == 2
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("streams", [1, 2])
def test_failed_call_leaves_the_cache_as_it_was(mm, clouds, streams):
    rng = np.random.default_rng(5)
    blob = np.zeros(20000, dtype=mm.POINT)
    xyz = rng.uniform(0.0, 0.5, size=(20000, 3)).astype(np.float32)
    blob["x"], blob["y"], blob["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    blob["rgba"] = rng.integers(0, 1 << 24, size=20000, dtype=np.uint32)
    dense = mm.MapMergingParams(descriptor_type=2, estimation_method=1, resolution=0.01, descriptor_radius=0.08,
                                outliers_min_neighbours=1, normal_radius=0.6)
    a, b = _pair(mm, streams)
    try:
        p = _params(mm, MATCHING)
        _lockstep(a, b, clouds[:4], p)
        before = a.mapCacheStats()
        box = {}

        def failing():
            try:
                a.estimateMapsTransforms([blob, blob.copy(), clouds[0]], dense)
            except mm.Mm3dError as e:
                box["status"] = e.status

        t = threading.Thread(target=failing, daemon=True)
        t.start()
        t.join(timeout=300)
        assert not t.is_alive(), "the failing call did not come back"
        assert box.get("status") == -4
        after = a.mapCacheStats()
        assert after == before, (before, after)
        P, st = _lockstep(a, b, clouds[:4], p, seed=1)
        _check(st, hits=4, misses=0, reused=P, computed=0)
        fresh = mm.Context(0)
        try:
            fresh.setStreams(streams)
            T1, pairs1 = fresh.estimateMapsTransforms(clouds[:4], p, return_pairs=True)
            T, pairs = a.estimateMapsTransforms(clouds[:4], p, return_pairs=True)
        finally:
            fresh.close()
        assert np.array_equal(np.stack(T).view(np.uint32), np.stack(T1).view(np.uint32))
        assert np.array_equal(pairs.view(np.uint8), pairs1.view(np.uint8))
    finally:
        a.close(); b.close()


def test_a_hit_runs_no_feature_or_pair_kernel(mm, clouds):
    a, b = _pair(mm, 1)
    try:
        p = _params(mm, MATCHING)
        _lockstep(a, b, clouds, p)
        a.profile(True)
        a.profile_reset()
        T, pairs = a.estimateMapsTransforms(clouds, p, return_pairs=True)
        ran = {k: v["launches"] for k, v in a.profile_entries().items() if v["launches"] > 0}
        a.profile(False)
        assert ran == {"cloud_digest_compare": 6}, ran
        st = a.mapCacheStats()
        assert st["map_hits"] == 6 and st["pairs_reused"] == len(pairs) and st["pairs_computed"] == 0
    finally:
        a.close(); b.close()


def test_device_list_context_has_no_cache(mm):
    c = mm.Context(devices=[0])
    try:
        with pytest.raises(mm.Mm3dError) as e:
            c.setMapCache(4)
        assert e.value.status == -4
        assert c.getMapCache() == 0
    finally:
        c.close()

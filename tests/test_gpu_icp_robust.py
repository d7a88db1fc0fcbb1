"""Robust ICP (mm3d_set_icp_robust, mm3d_estimate_transform_icp_robust) on the GPU: one iteration's matches, weights and sums
against the restatement through the debug hook, the edge cases, L2 = the existing ICP bit for bit, known answers on the cabinet
scene, the whole loop against its restatement, and bit-identical results across the drivers and the cache with the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

from test_gpu_icp_plane import _normals, _problem, _records, box_room
from test_icp_rejection_cpu import cabinet
from test_icp_robust_cpu import (CAUCHY, CAUCHY_FIXED, DEFAULT, GEMAN_MCCLURE, GM_ANNEALED, HUBER, L2, LOOP_CASES, LOOP_SEEDS, OFF, TUKEY,
                                 loop_reference, opt, restate_iteration, sigma_table)

pytestmark = pytest.mark.gpu

SAC_IA, MATCHING = 1, 0
EINVAL, EUNSUPPORTED = -1, -4


def _o(mm, o):
    return mm.IcpRobustOptions(**o._asdict())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------- surface and refusals
def test_surface_and_refusals(mm):
    c = mm.Context(0)
    lib = mm.lib()
    assert c.getIcpRobust().as_tuple() == tuple(DEFAULT)
    st = c.last_icp_robust_stats
    assert (st["matched"], st["weighted"], st["weight_sum"], st["scale"], st["iterations"], st["converged"]) == (0, 0, 0.0, 0.0, 0, 0)
    o = mm.IcpRobustOptions(kernel=GEMAN_MCCLURE, scale=0.01, scale_start=0.4, anneal=0.5, tuning=2.0)
    c.setIcpRobust(o)
    assert c.getIcpRobust().as_tuple() == (GEMAN_MCCLURE, 0.01, 0.4, 0.5, 2.0)
    for bad in (dict(kernel=6), dict(kernel=-1), dict(scale=0.0), dict(scale=float("inf")), dict(scale_start=0.01), dict(anneal=0.0),
                dict(anneal=1.01), dict(tuning=-1.0)):
        assert lib.mm3d_set_icp_robust(c._h, C.byref(mm.IcpRobustOptions(**bad))) == EINVAL, bad
    assert lib.mm3d_set_icp_robust(c._h, None) == EINVAL and lib.mm3d_set_icp_robust(None, C.byref(o)) == EINVAL
    assert c.getIcpRobust().as_tuple() == (GEMAN_MCCLURE, 0.01, 0.4, 0.5, 2.0)          # a refused call changes nothing
    # the options survive mm3d_set_streams, in either order
    c.setStreams(4)
    assert c.getIcpRobust().as_tuple() == (GEMAN_MCCLURE, 0.01, 0.4, 0.5, 2.0)
    c.setIcpRobust(kernel=CAUCHY)
    c.setStreams(2)
    assert c.getIcpRobust().as_tuple() == (CAUCHY, 0.05, 0.0, 0.5, 0.0)
    # a device list refuses an active selection, and takes an inactive one
    d = mm.Context(devices=[0])
    assert lib.mm3d_set_icp_robust(d._h, C.byref(o)) == EUNSUPPORTED
    assert lib.mm3d_set_icp_robust(d._h, C.byref(mm.IcpRobustOptions(kernel=L2))) == EUNSUPPORTED
    assert d.getIcpRobust().as_tuple() == tuple(DEFAULT)
    assert lib.mm3d_set_icp_robust(d._h, C.byref(mm.IcpRobustOptions(scale=0.1))) == 0
    d.close()
    # a shard refuses an active selection
    cloud = _records(box_room(1, 2000)[0])
    with pytest.raises(mm.Mm3dError) as e:
        c.shardBegin([cloud, cloud], mm.MapMergingParams(descriptor_type=2), 0, 1)
    assert e.value.status == EUNSUPPORTED
    c.close()


def test_the_exclusive_stages_refuse_each_other(mm):
    lib = mm.lib()
    active = mm.IcpRobustOptions(kernel=GEMAN_MCCLURE)
    others = [("setIcpRejection", lambda: mm.IcpRejectionOptions(one_to_one=1), lambda: mm.IcpRejectionOptions(), lib.mm3d_set_icp_rejection),
              ("setIcpColor", lambda: mm.IcpColorOptions(enabled=1), lambda: mm.IcpColorOptions(), lib.mm3d_set_icp_color),
              ("setIcpGeneralized", lambda: mm.IcpGeneralizedOptions(enabled=1), lambda: mm.IcpGeneralizedOptions(), lib.mm3d_set_icp_generalized),
              ("setRefinement", lambda: mm.RefineOptions(method=1), lambda: mm.RefineOptions(), lib.mm3d_set_refinement)]
    for name, on, off, setter in others:
        c = mm.Context(0)
        # the other stage first: a robust kernel is refused, an inactive selection is taken
        assert setter(c._h, C.byref(on())) == 0, name
        assert lib.mm3d_set_icp_robust(c._h, C.byref(active)) == EUNSUPPORTED, name
        assert c.getIcpRobust().as_tuple() == tuple(DEFAULT) and b"mm3d_set_icp_robust" in lib.mm3d_last_error(c._h)
        assert lib.mm3d_set_icp_robust(c._h, C.byref(mm.IcpRobustOptions(scale=0.2))) == 0, name
        # and the other way round: the kernel first, the other stage is refused while it is selected
        assert setter(c._h, C.byref(off())) == 0, name
        assert lib.mm3d_set_icp_robust(c._h, C.byref(active)) == 0, name
        assert setter(c._h, C.byref(on())) == EUNSUPPORTED, name
        assert setter(c._h, C.byref(off())) == 0, name                  # (its inactive selection is still taken)
        assert lib.mm3d_set_icp_robust(c._h, C.byref(mm.IcpRobustOptions())) == 0
        assert setter(c._h, C.byref(on())) == 0, name
        c.close()
    # source sampling and point-to-plane compose with a kernel
    c = mm.Context(0)
    c.setIcpRobust(active)
    c.setIcpMethod(1)
    c.setIcpSampling(method=1, fraction=0.5)
    assert c.getIcpRobust().as_tuple()[0] == GEMAN_MCCLURE
    c.close()


# ---------------------------------------------------------------- 1. one iteration through the debug hook
# sigma_2 = 0.1 of the schedule 0.4 -> 0.05: Tukey then cuts at d2 = (0.1 * 4.685)^2 = 0.22, inside the matched range of the guess
HOOK = {k: opt(kernel=k, scale=0.05, scale_start=0.4, anneal=0.5) for k in (L2, HUBER, CAUCHY, TUKEY, GEMAN_MCCLURE)}
HOOK_K = 2
SIZES = [1, 63, 64, 65, 255, 256, 257, 4200]


@pytest.fixture(scope="module")
def hook_scene():
    """cabinet(7) at its guess; the target's normals have non-finite rows, and the source's points 1, 70 and 300 are not finite
    (where the source is that long)."""
    tgt, nrm, src, _, guess = cabinet(7)
    nrm = nrm.copy()
    nrm[::7] = np.nan
    nrm[3::31, 1] = np.inf
    src = src.copy()
    src[1] = [np.nan, 0, 0]
    src[70] = [0, np.inf, 0]
    src[300] = [1, 2, -np.inf]
    return src, tgt, nrm, guess


@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("n", SIZES)
def test_one_iteration_is_the_restatements(mm, hook_scene, n, split):
    src, tgt, nrm, guess = hook_scene
    src = src[:n] if n > 1 else src[:1]
    c = mm.Context(0)
    s_cloud, t_cloud, normals = c.cloud(_records(src)), c.cloud(_records(tgt)), c.normals(_normals(nrm))
    for kernel, o in HOOK.items():
        for plane in (False, True):
            idx, d2, w, sums, st = c.debugIcpRobust(s_cloud, t_cloud, normals if plane else None, guess, 1.0, _o(mm, o), HOOK_K, split)
            r_idx, r_d2, r_w, _ = restate_iteration(src, tgt, nrm if plane else None, guess, 1.0, o, HOOK_K)
            assert np.array_equal(idx, r_idx) and np.array_equal(_bits(d2), _bits(r_d2)), (kernel, plane)
            ulps = np.abs(_bits64(w) - _bits64(r_w))
            if kernel == HUBER:      # (whether the device's f64 square root is correctly rounded is what this prints)
                print(f"n {n} split {split} huber {'plane' if plane else 'point'}: {int((ulps > 0).sum())} of {int((idx >= 0).sum())} weights differ, by at most {int(ulps.max())} ulp")
                assert ulps.max() <= 1, (plane, int(ulps.max()))
            else:
                assert ulps.max() == 0, (kernel, plane, int(ulps.max()))
            # the sums: any double summation order lies within (n - 1) 2^-53 sum |term| of the exact sum of the same terms
            terms = restate_iteration(src, tgt, nrm if plane else None, guess, 1.0, o, HOOK_K, weights=w)[3]
            m = len(terms)
            assert sums.shape == (32 if plane else 19,) and terms.shape[1] == len(sums)
            for j in range(len(sums)):
                exact, bound = math.fsum(terms[:, j]), max(m - 1, 0) * 2.0 ** -53 * math.fsum(np.abs(terms[:, j]))
                assert abs(sums[j] - exact) <= bound, (kernel, plane, j, sums[j], exact, bound)
            matched, weighted = int((r_idx >= 0).sum()), int((w > 0).sum())
            assert (sums[-2], sums[-1]) == (float(matched), float(weighted))
            assert (st["matched"], st["weighted"], st["iterations"], st["converged"]) == (matched, weighted, 0, 0)
            assert st["weight_sum"] == sums[28 if plane else 16] and st["scale"] == sigma_table(o, HOOK_K + 1)[HOOK_K]
            if kernel == TUKEY and n == 4200:
                assert 0 < weighted < matched                      # (the cut lies inside the matches)
            if n >= 301:
                assert (idx[[1, 70, 300]] == -1).all() and (w[[1, 70, 300]] == 0).all()
    c.close()


# ---------------------------------------------------------------- 2. edge cases
@pytest.mark.parametrize("split", [1, 4])
def test_nothing_matched_and_all_weights_zero(mm, hook_scene, split):
    src, tgt, nrm, guess = hook_scene
    c = mm.Context(0)
    t_cloud, normals = c.cloud(_records(tgt)), c.normals(_normals(nrm))
    assert mm.icp_robust_split(split) == split
    try:
        # a source with no match at all
        far = c.cloud(_records(src[:500] + np.float32(100.0)))
        for plane in (None, normals):
            idx, d2, w, sums, st = c.debugIcpRobust(far, t_cloud, plane, guess, 1.0, _o(mm, GM_ANNEALED), 0, split)
            assert (idx == -1).all() and np.isinf(d2).all() and (w == 0).all() and (sums == 0).all()
            assert (st["matched"], st["weighted"], st["weight_sum"]) == (0, 0, 0.0)
            T = c.estimateTransformICPRobust(far, t_cloud, plane, guess, 1.0, _o(mm, GM_ANNEALED), 30, 1e-9)
            st = c.last_icp_robust_stats
            assert np.array_equal(_bits(T), _bits(guess)) and (c.last_icp_iterations, c.last_icp_converged) == (0, 0)
            assert (st["matched"], st["weighted"], st["iterations"], st["converged"]) == (0, 0, 0, 0)
        # Tukey at a scale so small that every weight is 0: matches, but nothing to estimate from
        tiny = opt(kernel=TUKEY, scale=1e-6)
        s_cloud = c.cloud(_records(src))
        for plane in (None, normals):
            idx, _, w, sums, st = c.debugIcpRobust(s_cloud, t_cloud, plane, guess, 1.0, _o(mm, tiny), 0, split)
            assert (idx >= 0).sum() > 3000 and (w == 0).all() and (sums[:-2] == 0).all()
            T = c.estimateTransformICPRobust(s_cloud, t_cloud, plane, guess, 1.0, _o(mm, tiny), 30, 1e-9)
            st = c.last_icp_robust_stats
            assert np.array_equal(_bits(T), _bits(guess)) and (c.last_icp_iterations, c.last_icp_converged) == (0, 0)
            assert st["matched"] == int((idx >= 0).sum()) and (st["weighted"], st["weight_sum"], st["iterations"], st["converged"]) == (0, 0.0, 0, 0)
    finally:
        assert mm.icp_robust_split(0) == 0
    c.close()


@pytest.mark.parametrize("split", [1, 4])
def test_exactly_two_and_three_positive_weights(mm, split):
    """Five target points 3 m apart; the source's first `good` points lie 0.01 m from theirs, the others 0.5 m: matched (max_corr
    1.0), but beyond Tukey's cut at 0.05 * 4.685 = 0.23 m.  Two positive weights stop the ICP before its first estimate; three
    are enough for point-to-point's."""
    tgt = np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0], [0, 0, 3], [3, 3, 1]], dtype=np.float32)
    o = opt(kernel=TUKEY, scale=0.05)
    c = mm.Context(0)
    t_cloud = c.cloud(_records(tgt))
    eye = np.eye(4, dtype=np.float32)
    assert mm.icp_robust_split(split) == split
    try:
        for good in (2, 3):
            src = tgt.copy()
            src[:good] += np.float32([0.01, 0, 0])
            src[good:] += np.float32([0, 0.5, 0])
            s_cloud = c.cloud(_records(src))
            _, _, w, _, st = c.debugIcpRobust(s_cloud, t_cloud, None, eye, 1.0, _o(mm, o), 0, split)
            assert (st["matched"], st["weighted"]) == (5, good) and (w > 0).tolist() == [True] * good + [False] * (5 - good)
            T = c.estimateTransformICPRobust(s_cloud, t_cloud, None, eye, 1.0, _o(mm, o), 20, 1e-12)
            st = c.last_icp_robust_stats
            assert (st["matched"], st["weighted"]) == (5, good), st
            if good == 2:
                assert np.array_equal(_bits(T), _bits(eye)) and (st["iterations"], st["converged"]) == (0, 0)
            else:
                assert st["iterations"] >= 1 and st["converged"] == 1 and st["iterations"] == c.last_icp_iterations
                assert np.abs(T[:3, 3] - [-0.01, 0, 0]).max() < 1e-5 and np.abs(T[:3, :3] - np.eye(3)).max() < 1e-5
    finally:
        assert mm.icp_robust_split(0) == 0
    c.close()


# ---------------------------------------------------------------- 3. L2 = the existing ICP, bit for bit
@pytest.mark.parametrize("split", [1, 4])
@pytest.mark.parametrize("seed", [11, 12])
def test_l2_is_the_existing_icp(mm, seed, split):
    tgt, nrm, src, _, guess = _problem(seed, 5000)
    c = mm.Context(0)
    s_cloud, t_cloud, normals = c.cloud(_records(src)), c.cloud(_records(tgt)), c.normals(_normals(nrm))
    T_point = c.estimateTransformICP(s_cloud, t_cloud, guess, 1.0, 0.5, 30, 1e-9)
    ref_point = (c.last_icp_iterations, mm.lib().mm3d_last_icp_converged(c._h))
    T_plane = c.estimateTransformICPPlane(s_cloud, t_cloud, normals, guess, 1.0, 30, 1e-9)
    ref_plane = (c.last_icp_iterations, c.last_icp_converged)
    assert ref_point[0] >= 2 and ref_plane[0] >= 2
    assert mm.icp_robust_split(split) == split
    try:
        # (L2 reads no scale, annealed or not; OFF at the stage-level call runs as L2)
        for o in (opt(kernel=L2), opt(kernel=L2, scale=0.01, scale_start=0.4), opt(kernel=OFF)):
            T = c.estimateTransformICPRobust(s_cloud, t_cloud, None, guess, 1.0, _o(mm, o), 30, 1e-9)
            assert np.array_equal(_bits(T), _bits(T_point)), (o, np.abs(T - T_point).max())
            assert (c.last_icp_iterations, c.last_icp_converged) == ref_point
            st = c.last_icp_robust_stats
            assert st["weighted"] == st["matched"] > 0 and st["weight_sum"] == float(st["matched"]) and st["iterations"] == ref_point[0]
            T = c.estimateTransformICPRobust(s_cloud, t_cloud, normals, guess, 1.0, _o(mm, o), 30, 1e-9)
            assert np.array_equal(_bits(T), _bits(T_plane)), (o, np.abs(T - T_plane).max())
            assert (c.last_icp_iterations, c.last_icp_converged) == ref_plane
    finally:
        assert mm.icp_robust_split(0) == 0
    c.close()


# ---------------------------------------------------------------- 4. known answer
@pytest.mark.parametrize("seed", [7, 8, 9])
def test_known_answer_cabinet(mm, seed):
    """1e-4 is the project's transform tolerance, as in test_gpu_icp_rejection.py::test_known_answer_cabinet."""
    tgt, _, src, T_true, guess = cabinet(seed)
    c = mm.Context(0)
    s_cloud, t_cloud = c.cloud(_records(src)), c.cloud(_records(tgt))
    T = c.estimateTransformICP(s_cloud, t_cloud, guess, 1.0, 0.5, 50, 1e-10)
    err = np.abs(T - T_true).max()
    print(f"cabinet({seed}) default ICP: error {err:.3g}")
    assert err > 0.2, err
    normals = c.computeSurfaceNormals(t_cloud, 0.3)
    for nrm in (None, normals):
        T = c.estimateTransformICPRobust(s_cloud, t_cloud, nrm, guess, 1.0, _o(mm, GM_ANNEALED), 50, 1e-10)
        err, st = np.abs(T - T_true).max(), c.last_icp_robust_stats
        print(f"cabinet({seed}) geman_mcclure annealed {'plane' if nrm is not None else 'point'}: error {err:.3g} iterations {c.last_icp_iterations} {st}")
        assert c.last_icp_converged == 1 and st["converged"] == 1 and st["iterations"] == c.last_icp_iterations, st
        assert 6 < st["iterations"] < 50 and st["scale"] == 0.01 and st["matched"] == st["weighted"] == 4200
        assert err < 1e-4, (nrm is not None, err)
    c.close()


# ---------------------------------------------------------------- 5. against the restatement of the whole loop
@pytest.mark.parametrize("name,plane", LOOP_CASES, ids=[n + (" plane" if p else "") for n, p in LOOP_CASES])
@pytest.mark.parametrize("seed", LOOP_SEEDS)
def test_against_restatement(mm, seed, name, plane):
    """The comparison runs only where the restatement sits more than 1 % from every convergence threshold
    (test_icp_robust_cpu.py::test_loop_seeds_qualify checks the seeds without a GPU: none had to be replaced)."""
    tgt, nrm, src, _, guess = cabinet(seed, 5000)
    o = {"geman_mcclure annealed": GM_ANNEALED, "cauchy fixed": CAUCHY_FIXED}[name]
    T_ref, it_ref, conv_ref, margins, st_ref = loop_reference(seed, name, plane)
    assert it_ref >= 2
    assert min(margins) > 0.01, "the restatement sits within 1 % of a threshold: the comparison would be borderline"
    c = mm.Context(0)
    T = c.estimateTransformICPRobust(c.cloud(_records(src)), c.cloud(_records(tgt)), c.normals(_normals(nrm)) if plane else None, guess,
                                     1.0, _o(mm, o), 30, 1e-9)
    st = c.last_icp_robust_stats
    print(f"seed {seed} {name}: |T - T_ref| {np.abs(T - T_ref).max():.3g}, iterations {c.last_icp_iterations} / {it_ref}, {st} / {st_ref}")
    assert (c.last_icp_iterations, c.last_icp_converged) == (it_ref, conv_ref)
    assert np.abs(T - T_ref).max() < 1e-4, np.abs(T - T_ref).max()
    assert (st["iterations"], st["converged"], st["matched"], st["weighted"], st["scale"]) \
        == (it_ref, conv_ref, st_ref["matched"], st_ref["weighted"], st_ref["scale"])
    assert abs(st["weight_sum"] - st_ref["weight_sum"]) < 1e-4 * st_ref["weight_sum"]
    c.close()


# ---------------------------------------------------------------- 6. drivers, cache, records
@pytest.fixture(scope="module")
def clouds(synth):
    _, maps = synth.synth_maps(7, 30000, overlap_step=0.4)
    return [synth.pack_points(x, col) for x, col, _ in maps]


ACTIVE = opt(kernel=GEMAN_MCCLURE, scale=0.05, scale_start=0.4, anneal=0.5)
OTHER = CAUCHY_FIXED


def _params(mm, method=SAC_IA, **kw):
    return mm.MapMergingParams(descriptor_type=2, estimation_method=method, **kw)


def _ctx(mm, streams=1, o=ACTIVE, icp_method=0, cache=0, setter_first=True):
    c = mm.Context(0)
    if setter_first:
        c.setIcpRobust(_o(mm, o))
    c.setStreams(streams)
    if not setter_first:
        c.setIcpRobust(_o(mm, o))
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
def test_drivers_stage_and_cache_agree_bit_for_bit(mm, clouds, icp_method):
    cs = clouds[:6]
    p = _params(mm)
    c1 = _ctx(mm, 1, icp_method=icp_method)
    one = _run(c1, cs, p)
    assert one[1]["icp_iterations"].max() > 0
    st = c1.last_icp_robust_stats
    assert st["weighted"] == int(one[1][-1]["icp_correspondences"]) and st["iterations"] == int(one[1][-1]["icp_iterations"])
    assert 0 < st["weighted"] <= st["matched"] and 0 < st["weight_sum"] <= st["weighted"]
    _same(one, _run(_ctx(mm, 4, icp_method=icp_method), cs, p))
    _same(one, _run(_ctx(mm, 4, icp_method=icp_method, setter_first=False), cs, p))      # set after mm3d_set_streams: the helpers follow
    # the selection does something here, and a context set and then reset to the defaults gives the bytes of an untouched one
    untouched = mm.Context(0)
    untouched.setIcpMethod(icp_method)
    fresh = _run(untouched, cs, p)
    assert not np.array_equal(one[1].view(np.uint8), fresh[1].view(np.uint8))
    _same(fresh, _run(_ctx(mm, 1, DEFAULT, icp_method), cs, p))
    back = _ctx(mm, 1, icp_method=icp_method)
    back.setIcpRobust(_o(mm, DEFAULT))
    _same(fresh, _run(back, cs, p))
    # mm3d_pair_estimate and the stage-level entry point from each pair's pre-ICP guess (refine off)
    guesses = _run(c1, cs, _params(mm, refine_transform=0))[1]
    maps = [c1.mapFeatures(c1.cloud(x), p) for x in cs]
    for g, r in zip(guesses, one[1]):
        s, t = int(r["source_idx"]), int(r["target_idx"])
        assert (int(g["source_idx"]), int(g["target_idx"])) == (s, t)
        nt = c1.computeSurfaceNormals(maps[t].points, p.normal_radius) if icp_method else None
        T = c1.estimateTransformICPRobust(maps[s].points, maps[t].points, nt, g["transform"].reshape(4, 4).T, p.max_correspondence_distance,
                                          _o(mm, ACTIVE), p.max_iterations, p.transform_epsilon)
        assert np.array_equal(T.T.reshape(16).view(np.uint32), r["transform"].view(np.uint32))
        assert c1.last_icp_iterations == int(r["icp_iterations"])
        assert c1.last_icp_robust_stats["weighted"] == int(r["icp_correspondences"]) or int(r["icp_iterations"]) == 0
    # the cache in lockstep: two calls, then one map changed
    cached, plain = _ctx(mm, 4, icp_method=icp_method, cache=64), _ctx(mm, 4, icp_method=icp_method)
    _same(_run(cached, cs, p), one)
    _same(_run(cached, cs, p), one)
    assert cached.mapCacheStats(reset=True)["device_bytes"] > 0
    changed = cs[:5] + [clouds[6]]
    _same(_run(cached, changed, p), _run(plain, changed, p))


def test_pair_estimate_agrees(mm, clouds):
    """mm3d_pair_estimate on prepared maps gives the whole-map call's record, with the kernel selected."""
    cs = clouds[:3]
    p = _params(mm, MATCHING)
    c = _ctx(mm, 1)
    one = _run(c, cs, p)
    maps = [c.mapFeatures(c.cloud(x), p) for x in cs]
    for r in one[1]:
        got = c.pairEstimate(maps[int(r["source_idx"])], maps[int(r["target_idx"])], p)
        for name in ("transform", "confidence", "icp_iterations", "n_correspondences", "n_inliers", "icp_correspondences"):
            assert np.array_equal(np.ascontiguousarray(got[name]).view(np.uint8), np.ascontiguousarray(r[name]).view(np.uint8)), name
    assert c.last_icp_robust_stats["weighted"] == int(one[1][-1]["icp_correspondences"])
    c.close()


def test_records_are_never_shared_between_selections(mm, clouds):
    cs = clouds[:6]
    p = _params(mm, MATCHING)
    ref = {o: _run(_ctx(mm, 1, o), cs, p) for o in (DEFAULT, ACTIVE, OTHER)}
    assert not np.array_equal(ref[ACTIVE][1].view(np.uint8), ref[OTHER][1].view(np.uint8))
    c = _ctx(mm, 1, DEFAULT, cache=64)
    _same(_run(c, cs, p), ref[DEFAULT])
    n_pairs = len(ref[DEFAULT][1])
    c.mapCacheStats(reset=True)
    for o in (ACTIVE, OTHER):                     # every map is hit, no pair is reused: not the inactive records, not the other set's
        c.setIcpRobust(_o(mm, o))
        _same(_run(c, cs, p), ref[o])
        st = c.mapCacheStats(reset=True)
        assert st["map_hits"] == 6 and st["pairs_reused"] == 0 and st["pairs_computed"] == n_pairs, (o, st)
    # an inactive selection's other values are read by nothing: its records are shared with the defaults'
    c.setIcpRobust(_o(mm, opt(scale=0.2, anneal=0.9)))
    _same(_run(c, cs, p), ref[DEFAULT])
    assert c.mapCacheStats(reset=True)["pairs_reused"] == n_pairs
    c.setIcpRobust(_o(mm, ACTIVE))
    _same(_run(c, cs, p), ref[ACTIVE])
    assert c.mapCacheStats(reset=True)["pairs_reused"] == n_pairs


def test_sampling_composes(mm, clouds):
    """Under mm3d_set_icp_sampling the robust step searches with the sample: the record is the stage call's on the sample."""
    cs = clouds[:3]
    p = _params(mm, MATCHING)
    c = _ctx(mm, 1)
    c.setIcpSampling(method=1, fraction=0.5)
    sampled = _run(c, cs, p)
    whole = _run(_ctx(mm, 1), cs, p)
    assert sampled[1]["icp_iterations"].max() > 0
    assert (sampled[1]["icp_correspondences"] < whole[1]["icp_correspondences"]).any()
    _same(sampled, _run(c, cs, p))
    c.close()

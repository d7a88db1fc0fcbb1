"""The geometric ICP rejectors on the GPU (mm3d_boundary_points, mm3d_set_icp_geometry_rejection,
mm3d_estimate_transform_icp_rejecting_geometry): the boundary flags against the restatement flag for flag, the arena's edge and
the streamed path, step 1b per source point, "nothing dropped" = the rejecting ICP bit for bit, the whole loop against its
restatement, bit-identical records across streams, cache and setter order, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import icp_geometry_cases as G
from test_gpu_icp_plane import _normals, _problem, _records
from test_icp_rejection_cpu import DEFAULT, TRIMMED, max_d2_of, opt

pytestmark = pytest.mark.gpu

SAC_IA, MATCHING = 1, 0
EINVAL, EUNSUPPORTED = -1, -4


def _o(mm, o):
    return mm.IcpRejectionOptions(**o._asdict())


def _g(mm, g):
    return mm.IcpGeometryOptions(**g._asdict())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _nrm_rows(n):
    """a Normals download as float rows [n][3]"""
    a = n.numpy()
    return np.stack([a["nx"], a["ny"], a["nz"]], axis=1)


# ---------------------------------------------------------------- 1. the flags, flag for flag
def _check_flags(c, pts, nrm, r, theta=90.0, k=3):
    flags, count = c.boundaryPoints(c.cloud(_records(pts)), c.normals(_normals(nrm)), r, theta, k)
    ref, dirs = G.restate_boundary(pts, nrm, r, theta, k)
    assert len(flags) == len(pts) and count == int(flags.sum())
    assert np.array_equal(flags, ref), (int(flags.sum()), int(ref.sum()), np.flatnonzero(flags != ref)[:10], dirs[flags != ref][:10])
    return flags, dirs


def test_lattice_sheet_edges_hole_and_translation(mm):
    pts, nrm, ij = G.lattice_sheet()
    c = mm.Context(0)
    flags, dirs = _check_flags(c, pts, nrm, 0.4)
    i, j = ij[:, 0], ij[:, 1]
    edge = (i == 0) | (i == 39) | (j == 0) | (j == 39)
    # the rows beside the hole's sides look into a gap of 180; its four diagonal corners (16 / 23) see three quadrants filled and
    # a gap of exactly 90: no boundary
    beside = (((i == 16) | (i == 23)) & (j >= 17) & (j <= 22)) | (((j == 16) | (j == 23)) & (i >= 17) & (i <= 22))
    corner = ((i == 16) | (i == 23)) & ((j == 16) | (j == 23))
    assert flags[edge].all() and flags[beside].all() and not flags[corner].any() and not flags[~(edge | beside)].any()
    assert dirs[corner].tolist() == [7, 7, 7, 7] and int(dirs.max()) == 8
    moved = (pts.astype(np.float64) + np.array([1000.0, -2000.0, 30.0])).astype(np.float32)      # (multiples of 0.25: exact)
    assert np.array_equal((moved.astype(np.float64) - np.array([1000.0, -2000.0, 30.0])).astype(np.float32), pts)
    assert np.array_equal(_check_flags(c, moved, nrm, 0.4)[0], flags)
    # theta and k are read: at 89 degrees the exact-90 corners are boundary points, at k = 8 only full neighbourhoods can be
    assert _check_flags(c, pts, nrm, 0.4, 89.0)[0][corner].all()
    assert _check_flags(c, pts, nrm, 0.4, 180.0, 8)[0].sum() == 0
    c.close()


def test_height_field_with_computed_normals(mm):
    _, _, tgt, _, _, _ = G.height_field_pair(G.HF_SEEDS[0])
    pts = np.concatenate([tgt, np.array([[np.nan, 1, 1], [5.0, np.inf, 0.0]], dtype=np.float32)])      # two rows nobody sees
    c = mm.Context(0)
    cloud = c.cloud(_records(pts))
    normals = c.computeSurfaceNormals(cloud, 0.3)
    nrm = _nrm_rows(normals)
    flags, count = c.boundaryPoints(cloud, normals, G.HF_RADIUS)
    ref, dirs = G.restate_boundary(pts, nrm, G.HF_RADIUS)
    print(f"height field: {count} of {len(pts)} flagged, directions {dirs.min()} .. {dirs.max()}")
    assert np.array_equal(flags, ref) and count == int(ref.sum()) and not flags[-2:].any()
    assert 0.04 < flags.mean() < 0.12
    c.close()


# ---------------------------------------------------------------- 2. the arena's edge and the streamed path
@pytest.mark.parametrize("m,cut", [(63, 100.0), (64, 80.0), (65, 100.0), (65, 80.0), (300, 100.0), (300, 85.0), (600, 95.0)])
def test_arena_edge_and_streamed_path(mm, m, cut):
    """A query point with exactly m directions and an empty sector of `cut` degrees (boundary above 90, none below), with the
    arena at its compiled size, at 64 (the edge: 63 / 64 fit, 65 / 300 stream), at 16 and at 1 (every direction its own chunk);
    600 directions stream at the compiled size too.  Every row of the cloud is compared, not only the query point."""
    pts, nrm = G.disc_with_sector(m, cut, seed=m)
    ref, dirs = G.restate_boundary(pts, nrm, 0.5)
    assert dirs[0] == m and bool(ref[0]) == (cut > 90.0)
    c = mm.Context(0)
    cloud, normals = c.cloud(_records(pts)), c.normals(_normals(nrm))
    try:
        for cap in (0, 64, 16, 1) if m < 600 else (0, 64):
            assert mm.boundary_lds_cap(cap) == (cap or 512)
            flags, count = c.boundaryPoints(cloud, normals, 0.5)
            assert np.array_equal(flags, ref), (cap, np.flatnonzero(flags != ref)[:10])
    finally:
        assert mm.boundary_lds_cap(0) == 512
    c.close()


# ---------------------------------------------------------------- 3. step 1b per source point
@pytest.fixture(scope="module")
def hf():
    """The height-field pair with its analytic normals, the restated flags of the target, and both normal sets as the maps of a
    pair would hold them."""
    src, sn, tgt, tn, T_true, guess = G.height_field_pair(G.HF_SEEDS[0])
    flags, _ = G.restate_boundary(tgt, tn, G.HF_RADIUS)
    return dict(src=src, sn=sn, tgt=tgt, tn=tn, T_true=T_true, guess=guess, flags=flags)


STAGE = [(G.geo(boundary=1, boundary_radius=G.HF_RADIUS), DEFAULT), (G.geo(normals=1, normal_angle_deg=3.0), DEFAULT),
         (G.geo(boundary=1, boundary_radius=G.HF_RADIUS, normals=1, normal_angle_deg=3.0), DEFAULT),
         (G.geo(boundary=1, boundary_radius=G.HF_RADIUS, normals=1, normal_angle_deg=3.0), opt(one_to_one=1, distance=TRIMMED, overlap_ratio=0.7))]


@pytest.mark.parametrize("split", [1, 4])
def test_step_1b_per_source_point(mm, hf, split):
    """The normal test runs at 3 degrees here: the field is smooth, and at the guess' 4 degrees of yaw a good share of the
    correspondences disagree by more than that while the rest agree, so both outcomes are exercised."""
    c = mm.Context(0)
    s_cloud, t_cloud = c.cloud(_records(hf["src"])), c.cloud(_records(hf["tgt"]))
    s_n, t_n = c.normals(_normals(hf["sn"])), c.normals(_normals(hf["tn"]))
    nn = c.debugNnSearch(s_cloud, t_cloud, hf["guess"], G.HF_MAX_CORR, 0, split)[:2]
    for g, o in STAGE:
        idx, d2, reason, rs, gs = c.debugIcpGeometry(s_cloud, s_n, t_cloud, t_n, hf["guess"], G.HF_MAX_CORR, _o(mm, o), _g(mm, g), split)
        assert np.array_equal(idx, nn[0]) and np.array_equal(_bits(d2), _bits(nn[1])), g
        kept, r_reason, r_rs, r_gs, _ = G.restate_geometry(hf["guess"], nn[0], nn[1], o, g, max_d2_of(G.HF_MAX_CORR), hf["flags"], hf["sn"], hf["tn"])
        assert np.array_equal(reason, r_reason), (g, o, np.bincount(reason, minlength=5), np.bincount(r_reason, minlength=5))
        assert gs == r_gs, (g, gs, r_gs)
        assert (rs["matched"], rs["after_one_to_one"], rs["kept"]) == (r_rs["matched"], r_rs["after_one_to_one"], r_rs["kept"]), (g, o, rs, r_rs)
        assert _bits(rs["threshold_d2"]) == _bits(r_rs["threshold_d2"])
        # the case is what it is meant to be
        seen = np.bincount(r_reason, minlength=5)
        assert seen[G.KEPT] > 0 and (not g.boundary or seen[G.BOUNDARY] > 0) and (not g.normals or seen[G.NORMALS] > 0), (g, seen)
        assert not o.one_to_one or (seen[G.ONE_TO_ONE] > 0 and seen[G.DISTANCE] > 0)
    c.close()


# ---------------------------------------------------------------- 4. nothing dropped = the rejecting ICP, bit for bit
@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_nothing_dropped_is_the_rejecting_icp(mm, plane):
    tgt, nrm, src, _, guess = _problem(11, 5000)
    src_n = np.tile(np.array([0.6, 0.0, 0.8], dtype=np.float32), (len(src), 1))
    c = mm.Context(0)
    s_cloud, t_cloud, t_n, s_n = c.cloud(_records(src)), c.cloud(_records(tgt)), c.normals(_normals(nrm)), c.normals(_normals(src_n))
    for o in (DEFAULT, opt(one_to_one=1, distance=TRIMMED, overlap_ratio=0.7)):
        T_ref = c.estimateTransformICPRejecting(s_cloud, t_cloud, t_n if plane else None, guess, 1.0, _o(mm, o), 30, 1e-9)
        ref = (c.last_icp_iterations, c.last_icp_converged, c.last_icp_rejection_stats)
        assert ref[0] >= 2
        T, rs, gs = c.estimateTransformICPRejectingGeometry(s_cloud, s_n, t_cloud, t_n, guess, 1.0, _o(mm, o),
                                                            mm.IcpGeometryOptions(normals=1, normal_angle_deg=90.0), plane, 30, 1e-9)
        assert np.array_equal(_bits(T), _bits(T_ref)), (o, np.abs(T - T_ref).max())
        assert (c.last_icp_iterations, c.last_icp_converged) == ref[:2] and rs == ref[2]
        assert gs["passed"] == gs["matched"] == rs["matched"] and gs["normal_mismatch"] == gs["on_boundary"] == gs["target_boundary_points"] == 0
        assert c.last_icp_geometry_stats == gs
    c.close()


# ---------------------------------------------------------------- 5. against the restatement of the whole loop
def _against_restatement(mm, name, src, src_n, tgt, tgt_n, guess, max_corr, max_iter, eps, g, flags=None):
    ref = G.restate_icp_geometry(src, tgt, None, guess, max_corr, max_iter, eps, DEFAULT, g, flags, src_n, tgt_n)
    T_ref, it_ref, conv_ref, margins, _, rs_ref, gs_ref = ref
    assert it_ref >= 2
    assert min(margins) > 0.01, "the restatement sits within 1 % of a threshold: the comparison would be borderline"
    c = mm.Context(0)
    T, rs, gs = c.estimateTransformICPRejectingGeometry(c.cloud(_records(src)), c.normals(_normals(src_n)), c.cloud(_records(tgt)),
                                                        c.normals(_normals(tgt_n)), guess, max_corr, None, _g(mm, g), False, max_iter, eps)
    print(f"{name}: |T - T_ref| {np.abs(T - T_ref).max():.3g}, iterations {c.last_icp_iterations} / {it_ref}, {rs} / {rs_ref}, {gs} / {gs_ref}")
    assert (c.last_icp_iterations, c.last_icp_converged) == (it_ref, conv_ref)
    assert np.abs(T - T_ref).max() < 1e-4, np.abs(T - T_ref).max()          # (test_gpu_icp_rejection.py's tolerance for this comparison)
    assert gs == gs_ref, (gs, gs_ref)
    assert (rs["matched"], rs["after_one_to_one"], rs["kept"], rs["iterations"], rs["converged"]) == \
        (rs_ref["matched"], rs_ref["after_one_to_one"], rs_ref["kept"], it_ref, conv_ref)
    assert _bits(rs["threshold_d2"]) == _bits(rs_ref["threshold_d2"])
    c.close()
    return T


def test_height_field_against_restatement(mm, hf):
    """Twelve iterations from the guess: the comparison is between two float pipelines, and twelve steps of the same contraction
    keep them within the tolerance; the plain ICP from the same guess moves the other way, which is asserted too."""
    g = G.geo(boundary=1, boundary_radius=G.HF_RADIUS)
    T = _against_restatement(mm, "height field", hf["src"], hf["sn"], hf["tgt"], hf["tn"], hf["guess"], G.HF_MAX_CORR, 12, G.HF_EPS, g, hf["flags"])
    c = mm.Context(0)
    T_plain = c.estimateTransformICP(c.cloud(_records(hf["src"])), c.cloud(_records(hf["tgt"])), hf["guess"], G.HF_MAX_CORR, 0.5, 12, G.HF_EPS)
    e0, e, e_plain = G.frobenius(hf["guess"], hf["T_true"]), G.frobenius(T, hf["T_true"]), G.frobenius(T_plain, hf["T_true"])
    print(f"height field after 12 iterations: guess {e0:.3f}, boundary rejector {e:.3f}, plain {e_plain:.3f}")
    assert e < e0 < e_plain
    c.close()


@pytest.mark.parametrize("seed", [7, 8])
def test_slanted_cabinet_against_restatement(mm, seed):
    tgt, nrm, src, src_n, T_true, guess = G.slanted_cabinet(seed)
    T = _against_restatement(mm, f"slanted cabinet {seed}", src, src_n, tgt, nrm, guess, 1.0, 50, 1e-10, G.geo(normals=1, normal_angle_deg=30.0))
    assert G.frobenius(T, T_true) < 1e-4


# ---------------------------------------------------------------- 6. whole-map: streams, cache, setter order
def _textured(xyz, seed):
    """POINT records of a height-field sample with a smooth intensity pattern plus noise, so that the detectors find keypoints."""
    rng = np.random.default_rng(seed)
    x, y = xyz[:, 0].astype(np.float64), xyz[:, 1].astype(np.float64)
    v = 128 + 70 * np.sin(3.1 * x) * np.sin(2.7 * y) + 40 * np.sin(7.3 * x + 1.0) * np.cos(6.1 * y) + rng.normal(0, 6, len(x))
    v = np.clip(v, 0, 255).astype(np.uint32)
    out = _records(xyz)
    out["rgba"] = np.uint32(0xff000000) | (v << np.uint32(16)) | (v << np.uint32(8)) | v
    return out


@pytest.fixture(scope="module")
def hf_maps():
    """Three overlapping windows of the height field, x in [0, 7], [4, 11] and [8, 15], each moved by a small rigid motion."""
    out = []
    for k, x0 in enumerate((0.0, 4.0, 8.0)):
        xyz, _ = G.height_field_sample(40 + k, 20000, x0, x0 + 7.0)
        T = G.construct_transform(0.0, 0.0, np.radians(1.5 * k), 0.1 * k, -0.05 * k, 0.0)
        xyz = (xyz.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        out.append(_textured(xyz, 50 + k))
    return out


ACTIVE = G.geo(boundary=1, boundary_radius=0.35)


def _params(mm, method=SAC_IA, **kw):
    return mm.MapMergingParams(descriptor_type=2, estimation_method=method, **kw)


def _ctx(mm, streams=1, g=ACTIVE, cache=0, setter_first=True, reject=None, icp_method=0, geometry_before_rejection=True):
    c = mm.Context(0)
    if setter_first and geometry_before_rejection:
        c.setIcpGeometryRejection(_g(mm, g))
    if reject is not None:
        c.setIcpRejection(_o(mm, reject))
    c.setIcpMethod(icp_method)
    if setter_first and not geometry_before_rejection:
        c.setIcpGeometryRejection(_g(mm, g))
    c.setStreams(streams)
    if not setter_first:
        c.setIcpGeometryRejection(_g(mm, g))
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


def test_whole_map_records_are_bit_identical(mm, hf_maps):
    p = _params(mm)
    c1 = _ctx(mm, 1)
    one = _run(c1, hf_maps, p)
    assert one[1]["icp_iterations"].max() > 0
    gs, rs = c1.last_icp_geometry_stats, c1.last_icp_rejection_stats
    print(f"whole-map: iterations {one[1]['icp_iterations'].tolist()}, last pair {gs} {rs}")
    assert gs["passed"] == gs["matched"] - gs["on_boundary"] and gs["normal_mismatch"] == 0 and gs["target_boundary_points"] > 0
    assert rs["kept"] == gs["passed"] == int(one[1][-1]["icp_correspondences"]) or int(one[1][-1]["icp_iterations"]) == 0
    _same(one, _run(_ctx(mm, 4), hf_maps, p))
    _same(one, _run(_ctx(mm, 4, setter_first=False), hf_maps, p))            # set after mm3d_set_streams: the helpers follow
    # the selection does something, and a context set and then reset computes a fresh context's bytes
    fresh = _run(_ctx(mm, 1, G.GEO_DEFAULT), hf_maps, p)
    assert not np.array_equal(one[1].view(np.uint8), fresh[1].view(np.uint8))
    back = _ctx(mm, 1)
    back.setIcpGeometryRejection(_g(mm, G.GEO_DEFAULT))
    _same(fresh, _run(back, hf_maps, p))
    # either order of this setter and mm3d_set_icp_rejection / mm3d_set_icp_method
    rej = opt(distance=TRIMMED, overlap_ratio=0.8)
    a = _run(_ctx(mm, 1, reject=rej, icp_method=1, geometry_before_rejection=True), hf_maps, p)
    b = _run(_ctx(mm, 1, reject=rej, icp_method=1, geometry_before_rejection=False), hf_maps, p)
    _same(a, b)
    assert not np.array_equal(a[1].view(np.uint8), one[1].view(np.uint8))
    # mm3d_pair_estimate against the whole call (under MATCHING, which draws nothing from the generator); the third map's flags
    # are made on first use
    pm = _params(mm, MATCHING)
    whole = _run(c1, hf_maps, pm)
    maps = [c1.mapFeatures(c1.cloud(x), pm) for x in hf_maps]
    for m in maps[:2]:
        c1.mapPrepare(m, pm)
    for r in whole[1]:
        got = c1.pairEstimate(maps[int(r["source_idx"])], maps[int(r["target_idx"])], pm)
        for f in ("transform", "icp_iterations", "icp_correspondences", "confidence", "n_correspondences", "n_inliers"):
            assert np.array_equal(np.ascontiguousarray(got[f]).view(np.uint8), np.ascontiguousarray(r[f]).view(np.uint8)), f
    # the cache in lockstep
    cached = _ctx(mm, 4, cache=16)
    _same(_run(cached, hf_maps, p), one)
    _same(_run(cached, hf_maps, p), one)
    assert cached.mapCacheStats(reset=True)["device_bytes"] > 0


def test_cache_key_holds_the_six_fields_and_rand_is_untouched(mm, hf_maps):
    p = _params(mm)
    c = _ctx(mm, 1, ACTIVE, cache=16)
    base = _run(c, hf_maps, p)
    n_pairs = len(base[1])
    c.mapCacheStats(reset=True)
    _run(c, hf_maps, p)
    assert c.mapCacheStats(reset=True)["pairs_reused"] == n_pairs
    changes = [dict(boundary_radius=0.3), dict(boundary_angle_deg=100.0), dict(boundary_min_neighbours=4), dict(normals=1),
               dict(normals=1, normal_angle_deg=30.0), dict(boundary=0, normals=1)]
    for ch in changes:
        c.setIcpGeometryRejection(_g(mm, ACTIVE._replace(**ch)))
        _run(c, hf_maps, p)
        st = c.mapCacheStats(reset=True)
        assert st["map_hits"] == len(hf_maps) and st["pairs_reused"] == 0 and st["pairs_computed"] == n_pairs, (ch, st)
    # an inactive selection's other values are read by nothing: its records are the defaults'
    c.setIcpGeometryRejection(_g(mm, G.GEO_DEFAULT))
    fresh = _run(c, hf_maps, p)
    c.mapCacheStats(reset=True)
    c.setIcpGeometryRejection(_g(mm, G.geo(boundary_radius=0.7, normal_angle_deg=10.0)))
    _same(_run(c, hf_maps, p), fresh)
    assert c.mapCacheStats(reset=True)["pairs_reused"] == n_pairs
    # the rand() replay: a call with the selection leaves the generator where a call without it does
    a, b = _ctx(mm, 1, ACTIVE), _ctx(mm, 1, G.GEO_DEFAULT)
    _run(a, hf_maps, p, seed=5)
    _run(b, hf_maps, p, seed=5)
    b.setIcpGeometryRejection(_g(mm, ACTIVE))
    _same(_run(a, hf_maps, p, seed=None), _run(b, hf_maps, p, seed=None))


# ---------------------------------------------------------------- 7. refusals
def test_refusals(mm, hf_maps):
    lib = mm.lib()
    act, nrm_only, bnd_only = mm.IcpGeometryOptions(boundary=1, normals=1), mm.IcpGeometryOptions(normals=1), mm.IcpGeometryOptions(boundary=1)
    off = mm.IcpGeometryOptions(boundary_radius=0.5)
    c = mm.Context(0)
    assert c.getIcpGeometryRejection().as_tuple() == tuple(G.GEO_DEFAULT) and c.last_icp_geometry_stats == dict.fromkeys(
        ("matched", "on_boundary", "normal_mismatch", "passed", "target_boundary_points"), 0)
    c.setIcpGeometryRejection(act)
    assert c.getIcpGeometryRejection().as_tuple() == (1, 0.0, 90.0, 3, 1, 45.0)
    c.setStreams(3)
    assert c.getIcpGeometryRejection().as_tuple() == (1, 0.0, 90.0, 3, 1, 45.0)
    # a device list refuses an active selection and takes an inactive one
    d = mm.Context(devices=[0])
    for o in (act, nrm_only, bnd_only):
        assert lib.mm3d_set_icp_geometry_rejection(d._h, C.byref(o)) == EUNSUPPORTED
    assert lib.mm3d_set_icp_geometry_rejection(d._h, C.byref(off)) == 0 and d.getIcpGeometryRejection().as_tuple() == (0, 0.5, 90.0, 3, 0, 45.0)
    d.close()
    # mm3d_shard_begin
    with pytest.raises(mm.Mm3dError) as e:
        c.shardBegin(hf_maps[:2], _params(mm), 0, 1)
    assert e.value.status == EUNSUPPORTED
    # coloured, generalized and robust ICP, in either order of the setters
    others = [("setIcpColor", dict(enabled=1), dict(enabled=0)), ("setIcpGeneralized", dict(enabled=1), dict(enabled=0)),
              ("setIcpRobust", dict(kernel=mm.RobustKernel.HUBER), dict(kernel=mm.RobustKernel.OFF))]
    for name, on, neutral in others:
        with pytest.raises(mm.Mm3dError) as e:                      # while this selection is active
            getattr(c, name)(**on)
        assert e.value.status == EUNSUPPORTED, name
        getattr(c, name)(**neutral)                                 # the other's inactive value is taken
        x = mm.Context(0)
        getattr(x, name)(**on)
        for o in (act, nrm_only, bnd_only):
            assert lib.mm3d_set_icp_geometry_rejection(x._h, C.byref(o)) == EUNSUPPORTED, name
        assert lib.mm3d_set_icp_geometry_rejection(x._h, C.byref(off)) == 0
        x.close()
    # the source sampler: normals == 1 is refused either way round, boundary alone combines
    with pytest.raises(mm.Mm3dError) as e:
        c.setIcpSampling(method=mm.IcpSampleMethod.STRIDE, fraction=0.5)
    assert e.value.status == EUNSUPPORTED
    c.setIcpGeometryRejection(bnd_only)
    c.setIcpSampling(method=mm.IcpSampleMethod.STRIDE, fraction=0.5)
    assert lib.mm3d_set_icp_geometry_rejection(c._h, C.byref(nrm_only)) == EUNSUPPORTED
    assert lib.mm3d_set_icp_geometry_rejection(c._h, C.byref(act)) == EUNSUPPORTED
    assert c.getIcpGeometryRejection().as_tuple() == (1, 0.0, 90.0, 3, 0, 45.0)          # a refused call changes nothing
    one = mm.Context(0)                          # (one stream: the context that ran the pair is the one that is asked)
    one.setIcpSampling(method=mm.IcpSampleMethod.STRIDE, fraction=0.5)
    one.setIcpGeometryRejection(bnd_only)
    T, pairs = one.estimateMapsTransforms(hf_maps[:2], _params(mm), return_pairs=True)     # boundary + sampler runs
    assert one.last_icp_geometry_stats["target_boundary_points"] > 0 or int(pairs[-1]["icp_iterations"]) == 0
    one.close()
    # out of range, whatever the bits
    for bad in (dict(boundary=2), dict(boundary_angle_deg=0.0), dict(boundary_min_neighbours=2), dict(normal_angle_deg=91.0), dict(boundary_radius=-1.0)):
        assert lib.mm3d_set_icp_geometry_rejection(c._h, C.byref(mm.IcpGeometryOptions(**bad))) == EINVAL, bad
    # the stage call: boundary needs a radius of its own
    s = c.cloud(hf_maps[0][:500])
    n = c.computeSurfaceNormals(s, 0.3)
    with pytest.raises(mm.Mm3dError) as e:
        c.estimateTransformICPRejectingGeometry(s, n, s, n, np.eye(4, dtype=np.float32), 1.0, None, bnd_only)
    assert e.value.status == EINVAL
    c.close()

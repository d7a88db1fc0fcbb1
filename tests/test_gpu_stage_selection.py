"""The opt-in stages selected TOGETHER (mm3d_set_icp_method, mm3d_set_alignment, mm3d_set_keypoints, mm3d_set_refinement,
mm3d_set_coarse_alignment, mm3d_set_confidence).  Each stage's own file (test_gpu_icp_plane.py ... test_gpu_confidence.py)
checks it alone; here a context holds several selections at once, and whatever the order of the setters and mm3d_set_streams
-- helpers made before, after, or destroyed and remade -- every context must hold the same selection and compute the same
bits.  Then what every ICP selection shares, the pair batch: pairs of unequal size in one batch against the stage-level entry
points, and the entry points with nothing to search.  Every comparison is exact: the library promises bit-identical records
for every stream count.  Last, which of the seventeen selections may stand together at all, on one device, on a device list and
in a shard: every ordered pair of setters against the policy written out here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FPFH = 2
MATCHING, SAC_IA = 0, 1

# (setter, getter, options class, what the case sets); mm3d_set_icp_method takes and answers a bare int
SEVERAL = dict(
    Keypoints=dict(source=1, leaf=0.4),
    CoarseAlignment=dict(method=1, cell=1.0, yaw_steps=360),
    Refinement=dict(method=1, resolution=2.0, min_points=5),
    Confidence=dict(method=1, voxel=0.25, min_points=3),
)
PLANE_PREREJECTIVE = dict(
    IcpMethod=1,
    Alignment=dict(method=1, k=8, inlier_fraction=0.2),
)
OPTIONS = dict(Alignment="AlignmentOptions", Keypoints="KeypointOptions", Refinement="RefineOptions", CoarseAlignment="CoarseOptions",
               Confidence="ConfidenceOptions")


@pytest.fixture(scope="module")
def clouds(synth):
    _, maps = synth.synth_maps(3, 30000, overlap_step=0.4)
    return [synth.pack_points(x, col) for x, col, _ in maps]


def _params(mm, method):
    return mm.MapMergingParams(descriptor_type=FPFH, estimation_method=method)


def _fields(o):
    return tuple(getattr(o, k) for k, _ in o._fields_)


def _select(mm, c, selection):
    for name, what in selection.items():
        if name == "IcpMethod":
            c.setIcpMethod(what)
        else:
            getattr(c, "set" + name)(**what)


def _holds(mm, c, selection):
    """every getter answers what `selection` set, and the defaults for what it did not name"""
    assert int(c.getIcpMethod()) == selection.get("IcpMethod", 0)
    for name, cls in OPTIONS.items():
        want = getattr(mm, cls)(**selection.get(name, {}))
        assert _fields(getattr(c, "get" + name)()) == _fields(want), name


def _reset(mm, c):
    """every option back to its mm3d_*_options_default"""
    c.setIcpMethod(0)
    for name, cls in OPTIONS.items():
        getattr(c, "set" + name)(getattr(mm, cls)())


def _contexts(mm, selection):
    """(a) one stream; (b) setters, then streams; (c) streams, then setters; (d) helpers destroyed and remade after the setters"""
    a = mm.Context(0)
    _select(mm, a, selection)
    b = mm.Context(0)
    _select(mm, b, selection)
    b.setStreams(4)
    c = mm.Context(0)
    c.setStreams(4)
    _select(mm, c, selection)
    d = mm.Context(0)
    d.setStreams(4)
    _select(mm, d, selection)
    d.setStreams(2)
    d.setStreams(4)
    return [a, b, c, d]


def _run(c, clouds, p, seed=1):
    c.srand(seed)
    T, pairs = c.estimateMapsTransforms(clouds, p, return_pairs=True)
    return np.stack(T), pairs


def _same(a, b):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8))


@pytest.fixture(scope="module")
def untouched(mm, clouds):
    """the reference stages on four streams, per estimation method: computed once, read by the cases below"""
    out = {}
    for method in (MATCHING, SAC_IA):
        c = mm.Context(0)
        c.setStreams(4)
        out[method] = _run(c, clouds, _params(mm, method))
        c.close()
    return out


@pytest.mark.parametrize("selection,method", [(SEVERAL, MATCHING), (SEVERAL, SAC_IA), (PLANE_PREREJECTIVE, SAC_IA)],
                         ids=["several-matching", "several-sac_ia", "plane_prerejective-sac_ia"])
def test_selections_together_in_every_order_of_the_calls(mm, clouds, untouched, selection, method):
    p = _params(mm, method)
    cs = _contexts(mm, selection)
    for c in cs:
        _holds(mm, c, selection)
    runs = [_run(c, clouds, p) for c in cs]
    assert len(runs[0][1]) == 3                                   # three maps, three pair records
    for r in runs[1:]:
        _same(runs[0], r)
    assert not np.array_equal(runs[0][1].view(np.uint8), untouched[method][1].view(np.uint8))      # the selection was in force
    for c in cs:
        _holds(mm, c, selection)                                  # (a run changes no selection)
    # back to the reference: a four-stream context that ran with the selection, every option reset to its default
    back = cs[2]
    _reset(mm, back)
    _holds(mm, back, {})
    _same(_run(back, clouds, p), untouched[method])
    for c in cs:
        c.close()


# ---------------------------------------------------------------- the ICP variants' side of a pair batch
# what a context selects, and the stage-level entry point that runs the same ICP on one pair (nt: the target's normals)
TRIM_ONE_TO_ONE = dict(one_to_one=1, distance=1, overlap_ratio=0.7)
NDT_RESOLUTION = 2.0
ICP_VARIANTS = {
    "default": ({}, lambda c, s, t, nt, g, p: c.estimateTransformICP(s, t, g, p.max_correspondence_distance, 0.0, p.max_iterations,
                                                                        p.transform_epsilon)),
    "plane": (dict(IcpMethod=1), lambda c, s, t, nt, g, p: c.estimateTransformICPPlane(s, t, nt, g, p.max_correspondence_distance,
                                                                                        p.max_iterations, p.transform_epsilon)),
    "ndt": (dict(Refinement=dict(method=1, resolution=NDT_RESOLUTION)),
            lambda c, s, t, nt, g, p: c.estimateTransformNDT(s, t, g, method=1, resolution=NDT_RESOLUTION, max_iterations=p.max_iterations,
                                                             transformation_epsilon=p.transform_epsilon)),
    "rejecting": (dict(IcpRejection=TRIM_ONE_TO_ONE),
                  lambda c, s, t, nt, g, p: c.estimateTransformICPRejecting(s, t, None, g, p.max_correspondence_distance,
                                                                            max_iterations=p.max_iterations,
                                                                            transformation_epsilon=p.transform_epsilon, **TRIM_ONE_TO_ONE)),
    "rejecting-plane": (dict(IcpRejection=TRIM_ONE_TO_ONE, IcpMethod=1),
                        lambda c, s, t, nt, g, p: c.estimateTransformICPRejecting(s, t, nt, g, p.max_correspondence_distance,
                                                                                  max_iterations=p.max_iterations,
                                                                                  transformation_epsilon=p.transform_epsilon, **TRIM_ONE_TO_ONE)),
    "coloured": (dict(IcpColor=dict(enabled=1)),      # (gradient_radius 0: the normal radius)
                 lambda c, s, t, nt, g, p: c.estimateTransformICPColor(s, t, nt, g, p.max_correspondence_distance,
                                                                       max_iterations=p.max_iterations,
                                                                       transformation_epsilon=p.transform_epsilon, gradient_radius=p.normal_radius)),
}
NEEDS_NORMALS = ("plane", "rejecting-plane", "coloured")
THINNING = (1, 2, 3, 4)      # every k-th point of the fixture's maps: four maps of clearly different size


@pytest.fixture(scope="module")
def unequal_clouds(synth):
    _, maps = synth.synth_maps(4, 30000, overlap_step=0.4)
    return [synth.pack_points(x, col)[::k].copy() for (x, col, _), k in zip(maps, THINNING)]


@pytest.mark.parametrize("variant", list(ICP_VARIANTS))
def test_unequal_sources_in_one_batch(mm, unequal_clouds, variant):
    """Pairs of different source and target sizes in one batch (every per-pair offset into the batch's arrays differs from its
    neighbours'): one and four streams give the same bytes, and every pair is the stage-level entry point's result from the
    pair's pre-ICP guess, bit for bit."""
    selection, stage = ICP_VARIANTS[variant]
    p = _params(mm, SAC_IA)
    c = mm.Context(0)
    _select(mm, c, selection)
    four = mm.Context(0)
    _select(mm, four, selection)
    four.setStreams(4)
    one = _run(c, unequal_clouds, p)
    _same(one, _run(four, unequal_clouds, p))
    hook = dict(rejecting=mm.icp_rejection_split, coloured=mm.icp_color_split).get(variant.split("-")[0])
    if hook:          # the launches with four work items per block, over the same unequal jobs: the same bytes
        hook(1)
        try:
            _same(one, _run(c, unequal_clouds, p))
        finally:
            hook(0)
    p_off = _params(mm, SAC_IA)
    p_off.refine_transform = 0
    guesses = _run(c, unequal_clouds, p_off)[1]
    maps = [c.mapFeatures(c.cloud(x), p) for x in unequal_clouds]
    normals = [c.computeSurfaceNormals(m.points, p.normal_radius) if variant in NEEDS_NORMALS else None for m in maps]
    iterated = set()
    for g, r in zip(guesses, one[1]):
        s, t = int(r["source_idx"]), int(r["target_idx"])
        assert (int(g["source_idx"]), int(g["target_idx"])) == (s, t)
        T = stage(c, maps[s].points, maps[t].points, normals[t], g["transform"].reshape(4, 4).T, p)
        assert np.array_equal(T.T.reshape(16).view(np.uint32), r["transform"].view(np.uint32))
        assert c.last_icp_iterations == int(r["icp_iterations"])
        if int(r["icp_iterations"]) > 0:
            iterated.add(len(maps[s].points))
    assert len(iterated) >= 3          # at least three pairs that iterate, their sources of pairwise different size
    c.close()
    four.close()


@pytest.mark.parametrize("empty", ["source", "target"])
@pytest.mark.parametrize("variant", list(ICP_VARIANTS))
def test_nothing_to_search(mm, variant, empty):
    """An empty source, or an empty target: every stage-level entry point answers MM3D_OK, the guess bit for bit and no iteration."""
    _, stage = ICP_VARIANTS[variant]
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-2.0, 2.0, (300, 3)).astype(np.float32)
    full = np.zeros(300, dtype=mm.POINT)
    full["x"], full["y"], full["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    c = mm.Context(0)
    clouds = dict(source=c.cloud(full), target=c.cloud(full))
    clouds[empty] = c.cloud(full[:0])
    nt = c.computeSurfaceNormals(clouds["target"], 0.5) if variant in NEEDS_NORMALS else None
    guess = np.eye(4, dtype=np.float32)
    guess[:3, :3] = [[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]]
    guess[:3, 3] = [0.1, -0.2, 0.3]
    T = stage(c, clouds["source"], clouds["target"], nt, guess, _params(mm, SAC_IA))
    assert np.array_equal(np.asarray(T, dtype=np.float32).view(np.uint32), guess.view(np.uint32))
    assert c.last_icp_iterations == 0
    c.close()


def test_defaults_exist_once(mm):
    """a fresh context's options are the mm3d_*_options_default ones, field for field (the Python classes' constructors call them)"""
    c = mm.Context(0)
    _holds(mm, c, {})
    c.setStreams(3)
    _holds(mm, c, {})
    c.close()


# ---------------------------------------------------------------- which selections may stand together (csrc/stage_rules.cpp)
# The policy written out, not read from the table it checks: the seventeen setters with a value that makes each active (the
# geometric rejectors twice: they conflict differently), the fourteen unordered pairs that refuse each other, and the five
# stages whose data travels in the bundles of a device list and a shard.
EUNSUPPORTED = -4
STAGES = [      # (Context.set<name> / get<name>, the C setter a message names, the options class, an active value)
    ("IcpMethod", "mm3d_set_icp_method", None, 1),
    ("Alignment", "mm3d_set_alignment", "AlignmentOptions", dict(method=1)),
    ("Keypoints", "mm3d_set_keypoints", "KeypointOptions", dict(source=1)),
    ("Refinement", "mm3d_set_refinement", "RefineOptions", dict(method=1)),
    ("CoarseAlignment", "mm3d_set_coarse_alignment", "CoarseOptions", dict(method=1)),
    ("Confidence", "mm3d_set_confidence", "ConfidenceOptions", dict(method=1)),
    ("IcpRejection", "mm3d_set_icp_rejection", "IcpRejectionOptions", dict(distance=1)),
    ("IcpGeometryRejection", "mm3d_set_icp_geometry_rejection", "IcpGeometryOptions", dict(normals=1)),
    ("IcpGeometryRejection", "mm3d_set_icp_geometry_rejection", "IcpGeometryOptions", dict(boundary=1)),
    ("IcpRobust", "mm3d_set_icp_robust", "IcpRobustOptions", dict(kernel=2)),
    ("IcpColor", "mm3d_set_icp_color", "IcpColorOptions", dict(enabled=1)),
    ("IcpGeneralized", "mm3d_set_icp_generalized", "IcpGeneralizedOptions", dict(enabled=1)),
    ("Estimator", "mm3d_set_estimator", "EstimatorOptions", dict(method=1)),
    ("IcpSampling", "mm3d_set_icp_sampling", "IcpSamplingOptions", dict(method=1)),
    ("OutlierFilter", "mm3d_set_outlier_filter", "OutlierOptions", dict(method=1)),
    ("ClusterFilter", "mm3d_set_cluster_filter", "ClusterOptions", dict(method=2)),
    ("Smoothing", "mm3d_set_smoothing", "SmoothOptions", dict(method=1)),
    ("Planes", "mm3d_set_planes", "PlaneOptions", dict(method=1)),
]
CONFLICTS = [
    ("IcpRejection", "IcpColor"), ("IcpRejection", "IcpGeneralized"), ("IcpRejection", "IcpRobust"),
    ("IcpGeometryRejection", "IcpColor"), ("IcpGeometryRejection", "IcpGeneralized"), ("IcpGeometryRejection", "IcpRobust"),
    ("IcpGeometryRejection", "IcpSampling"),          # only while the normal rejector is set: the boundary rejector composes with a sampler
    ("IcpSampling", "Refinement"), ("IcpSampling", "IcpColor"), ("IcpSampling", "IcpGeneralized"),
    ("IcpColor", "IcpGeneralized"), ("IcpColor", "IcpRobust"), ("IcpGeneralized", "IcpRobust"),
    ("IcpRobust", "Refinement"),
]
TRAVELLING = ("Keypoints", "OutlierFilter", "ClusterFilter", "Smoothing", "Planes")


def _conflicting(a, b):
    if (a[0], b[0]) not in CONFLICTS and (b[0], a[0]) not in CONFLICTS:
        return False
    if {a[0], b[0]} == {"IcpGeometryRejection", "IcpSampling"}:
        return bool((a if a[0] == "IcpGeometryRejection" else b)[3].get("normals"))
    return True


def _set_stage(mm, c, stage, active):
    """(status, message) of the stage's setter with its active value, or with its default"""
    name, _, cls, what = stage
    try:
        if cls is None:
            c.setIcpMethod(what if active else 0)
        else:
            getattr(c, "set" + name)(getattr(mm, cls)(**(what if active else {})))
    except mm.Mm3dError as e:
        return e.status, str(e)
    return 0, ""


def _record(c):
    """what every getter answers, field for field"""
    out = [int(c.getIcpMethod())]
    for name, _, cls, _ in STAGES:
        if cls is not None:
            o = getattr(c, "get" + name)()
            out.append(tuple(tuple(v) if hasattr(v, "__len__") else v for v in _fields(o)))
    return out


def test_every_ordered_pair_of_stages(mm):
    """A active, then B: refused exactly when {A, B} is a listed pair, whichever came first; a refusal names both calls and changes
    nothing; B's default is always accepted."""
    c = mm.Context(0)
    fresh = _record(c)
    refusals = 0
    for a in STAGES:
        for b in STAGES:
            if a[0] == b[0]:
                continue
            for s in STAGES:                                   # back to the defaults
                assert _set_stage(mm, c, s, False) == (0, "")
            assert _record(c) == fresh
            assert _set_stage(mm, c, a, True) == (0, ""), (a[0], b[0])
            before = _record(c)
            assert before != fresh
            st, msg = _set_stage(mm, c, b, True)
            if _conflicting(a, b):
                refusals += 1
                assert st == EUNSUPPORTED and b[1] + ":" in msg and "(" + a[1] + ")" in msg, (a[0], b[0], st, msg)
                assert _record(c) == before, (a[0], b[0])
            else:
                assert st == 0 and _record(c) != before, (a[0], b[0], msg)
                assert _set_stage(mm, c, a, True) == (0, ""), (a[0], b[0])      # and A again beside B
            assert _set_stage(mm, c, b, False) == (0, ""), (a[0], b[0])
            assert _record(c) == before
    assert refusals == 2 * 17      # fourteen pairs, geometry's four twice (two rejectors), less boundary - sampling; both orders
    c.close()


def test_device_list_and_shard_carry_five_stages(mm):
    """A device-list context and a shard refuse the twelve stages whose data stays on its device while one is active, and
    accept its default; the five that travel are accepted."""
    from test_gpu_icp_plane import _records, box_room
    d = mm.Context(devices=[0])
    c = mm.Context(0)
    cloud = _records(box_room(1, 2000)[0])
    p = mm.MapMergingParams(descriptor_type=FPFH)
    for s in STAGES:
        before = _record(d)
        st, msg = _set_stage(mm, d, s, True)
        if s[0] in TRAVELLING:
            assert st == 0 and _record(d) != before, (s[0], msg)
        else:
            assert st == EUNSUPPORTED and s[1] + ":" in msg and _record(d) == before, (s[0], st, msg)
        # the default is accepted -- but for mm3d_set_icp_method, which a device list refuses whatever the method
        assert _set_stage(mm, d, s, False)[0] == (EUNSUPPORTED if s[0] == "IcpMethod" else 0), s[0]
        assert _record(d) == before
        if s[0] in TRAVELLING:
            continue                                           # (a shard with the stage: the stage's own file)
        assert _set_stage(mm, c, s, True) == (0, "")
        with pytest.raises(mm.Mm3dError) as e:
            c.shardBegin([cloud, cloud], p, 0, 1)
        assert e.value.status == EUNSUPPORTED and "mm3d_shard_begin:" in str(e.value), s[0]
        assert _set_stage(mm, c, s, False) == (0, "")
    d.close()
    c.close()

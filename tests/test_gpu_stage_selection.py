"""The opt-in stages selected TOGETHER (mm3d_set_icp_method, mm3d_set_alignment, mm3d_set_keypoints, mm3d_set_refinement,
mm3d_set_coarse_alignment, mm3d_set_confidence).  Each stage's own file (test_gpu_icp_plane.py ... test_gpu_confidence.py)
checks it alone; here a context holds several selections at once, and whatever the order of the setters and mm3d_set_streams
-- helpers made before, after, or destroyed and remade -- every context must hold the same selection and compute the same
bits.  Every comparison is exact: the library promises bit-identical records for every stream count."""
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


def test_defaults_exist_once(mm):
    """a fresh context's options are the mm3d_*_options_default ones, field for field (the Python classes' constructors call them)"""
    c = mm.Context(0)
    _holds(mm, c, {})
    c.setStreams(3)
    _holds(mm, c, {})
    c.close()

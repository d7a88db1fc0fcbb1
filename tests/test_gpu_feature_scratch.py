"""The second launch of k_pfh (PFH, PFHRGB), k_shot, k_sc3d and k_harris_refine: a neighbourhood beyond the kernel's LDS capacity is
handed to the same kernel with its list in global scratch -- through the overflow list, rows[blockIdx.x], a run-time stride, a
sort over a run-time padded length, SC3D's per-keypoint random directions read out of order, and a compaction over rows that two
launches wrote.  tests/overflow_cases.py holds the inputs; tests/test_overflow_cases_cpu.py shows that they reach what is tested.

(a) the scene case with mm3d_debug_feature_lds_cap at 64, 128, 256 against the run at 0: device against device, so every bit.
(b) the blob cloud at the true capacities against the oracle, by the acceptance of the LDS-path tests of test_gpu_parity.py.
(c) SC3D's random directions stay the keypoint's own when its row is computed by the second launch.
(d) a call that took the scratch route leaves nothing behind for the next.
Everywhere the counters of mm3d_debug_feature_overflow must show the route the CPU brute force predicts."""
import numpy as np
import pytest

import feature_cases as fc
import overflow_cases as oc

pytestmark = pytest.mark.gpu

DESC = ("pfh", "pfhrgb", "shot", "sc3d")


@pytest.fixture(scope="module")
def blob(po):
    return oc.blob_reference(po)


@pytest.fixture(scope="module")
def scene(po, synth):
    return oc.scene_reference(po, synth)


@pytest.fixture(scope="module")
def blob_dev(ctx, blob):
    b, _ = blob
    return ctx.cloud(b.cloud), ctx.normals(b.normals)


@pytest.fixture(scope="module")
def scene_dev(ctx, scene):
    return [(ctx.cloud(s.cloud), ctx.normals(s.normals)) for s in scene]


@pytest.fixture()
def hook(mm):
    """The hook at 0 and the counters cleared before the test, and the hook back at 0 after it whatever happens."""
    mm.feature_lds_cap(0)
    mm.feature_overflow(reset=True)
    try:
        yield mm
    finally:
        mm.feature_lds_cap(0)


def describe(ctx, dev, keypoints, name):
    """(rows, keypoints after pruning, frames or None) of one descriptor on the device."""
    k = ctx.cloud(keypoints)
    d = ctx.computeLocalDescriptors(dev[0], dev[1], k, fc.DESCRIPTORS[name], oc.R)
    out = d.numpy(), k.numpy(), d.frames() if name == "shot" else None
    d.free()
    k.free()
    return out


def corners(ctx, dev):
    k = ctx.detectKeypoints(dev[0], dev[1], 1, oc.HARRIS_THRESHOLD, oc.R, oc.RES)
    out = k.numpy()
    k.free()
    return out


def route(mm, name):
    """(rows sent to scratch, largest capacity) of one family since the last call, every other family's counters being zero."""
    c = mm.feature_overflow(reset=True)
    at = 2 * oc.FAMILY[name]
    assert not any(c[:at] + c[at + 2:]), c
    return c[at], c[at + 1]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def first_difference(a, b):
    if a.shape != b.shape:
        return "shapes %s and %s" % (a.shape, b.shape)
    rows = np.flatnonzero([x.tobytes() != y.tobytes() for x, y in zip(a, b)])
    return "%d of %d rows differ, first %d" % (len(rows), len(a), rows[0]) if len(rows) else "equal"


# ------------------------------------------------------------------------------------------------ (a) scratch against LDS
@pytest.mark.parametrize("name", DESC)
def test_descriptor_scratch_rows_are_the_lds_rows_bit_for_bit(ctx, hook, scene, scene_dev, name):
    fam = "pfh" if name == "pfhrgb" else name
    for n_map, (s, dev) in enumerate(zip(scene, scene_dev)):
        assert hook.feature_lds_cap(0) == 0
        base = describe(ctx, dev, s.keypoints, name)
        assert route(hook, name) == (0, 0)
        assert len(base[0]) >= 100 and np.isfinite(base[0]).all()
        for cap in oc.HOOK_CAPS:
            hook.feature_lds_cap(cap)
            got = describe(ctx, dev, s.keypoints, name)
            assert hook.feature_lds_cap(0) == cap
            sent = route(hook, name)
            want = oc.expected_overflow(s.counts, fam, cap)
            print("%s, map %d, capacity %d: %d of %d keypoints through scratch, %d entries per row" % (name, n_map, cap, sent[0], len(s.keypoints), sent[1]))
            assert sent == want, (name, n_map, cap, sent, want)
            assert same_bits(got[1], base[1]), (name, n_map, cap, "kept keypoints", first_difference(got[1], base[1]))
            assert same_bits(got[0], base[0]), (name, n_map, cap, "rows", first_difference(got[0], base[0]))
            if name == "shot":
                assert same_bits(got[2], base[2]), (name, n_map, cap, "frames", first_difference(got[2], base[2]))


def test_harris_scratch_corners_are_the_lds_corners_bit_for_bit(ctx, hook, scene, scene_dev):
    for n_map, (s, dev) in enumerate(zip(scene, scene_dev)):
        base = corners(ctx, dev)
        assert route(hook, "harris") == (0, 0)
        # the oracle's corners: the CPU replay's neighbour counts are those of this trajectory
        assert len(fc.compare("harris_keypoints", oc.xyz(base), s.harris)) == 0
        for cap in oc.HOOK_CAPS:
            hook.feature_lds_cap(cap)
            got = corners(ctx, dev)
            assert hook.feature_lds_cap(0) == cap
            sent = route(hook, "harris")
            want = oc.harris_expected_overflow(s.harris_counts, cap)
            print("harris, map %d, capacity %d: %d of %d corners through scratch, %d entries per row" % (n_map, cap, sent[0], len(base), sent[1]))
            assert sent == want, (n_map, cap, sent, want)
            assert same_bits(got, base), (n_map, cap, first_difference(got, base))


def test_the_hook_takes_what_it_documents(hook):
    for bad in (-1, 1, 32, 63, 65, 96, 1000, 4096, 1 << 20):
        assert hook.feature_lds_cap(bad) == 0
    assert hook.feature_lds_cap(2048) == 0 and hook.feature_lds_cap(3) == 2048 and hook.feature_lds_cap(64) == 2048
    assert hook.feature_lds_cap(0) == 64 and hook.feature_lds_cap(0) == 0


# ------------------------------------------------------------------------------- (b) the true capacities against the oracle
def _worst(err, rows):
    return float(err[rows].max()) if rows.any() else 0.0


@pytest.mark.parametrize("name", DESC)
def test_descriptors_at_the_true_capacities(ctx, hook, blob, blob_dev, name):
    """Nine keypoints with exactly 40 .. 2300 neighbours among far, non-finite and sparse ones: 1023 and 1024 stay in LDS, 1025 and
    above leave, and every row -- whichever launch wrote it -- meets the acceptance of the descriptor's LDS-path test
    (test_pfh, test_pfhrgb: the oracle's bits; test_shot: 2e-6 per bin, frames bit-exact; test_sc3d: at most 8 bins beyond 1e-5
    and the mass bound).  The overflow rows are no further from the oracle than the fitting rows of the same call."""
    b, ref = blob
    fam = "pfh" if name == "pfhrgb" else name
    counts = b.counts()
    rows, kept, frames = describe(ctx, blob_dev, b.keypoints, name)
    sent = route(hook, name)
    print("%s, blob cloud: %d keypoints through scratch, %d entries per row" % (name, sent[0], sent[1]))
    assert sent == oc.expected_overflow(counts, fam) and sent[0] == (counts > oc.LDS_CAP[fam]).sum() == 6
    kp_ref, rows_ref = ref[name]
    assert len(fc.compare("keypoints", kept, kp_ref)) == 0                       # the oracle's pruning, in order, every bit
    assert rows.shape == rows_ref.shape
    keep = fc.survivors(b.keypoints, kp_ref)
    over = (counts > oc.LDS_CAP[fam])[keep]
    assert over.sum() == 6 and (~over).sum() >= 7
    with np.errstate(invalid="ignore"):
        delta = np.abs(rows.astype(np.float64) - rows_ref.astype(np.float64))
    if name in ("pfh", "pfhrgb"):
        err, bound = (rows.view(np.uint32) != rows_ref.view(np.uint32)).sum(axis=1).astype(np.float64), 0.0     # words that differ
    elif name == "shot":
        err, bound = delta.max(axis=1), fc.TOLERANCE["shot"]
        assert len(fc.compare("shot_frames", frames, ref["shot_frames"])) == 0
    else:
        err, bound = (~(delta <= fc.SC3D_BIN_TOL)).sum(axis=1).astype(np.float64), float(fc.SC3D_BINS)
    print("%s: worst overflow row %g, worst fitting row %g, bound %g" % (name, _worst(err, over), _worst(err, ~over), bound))
    assert len(fc.compare(name, rows, rows_ref)) == 0, (name, fc.compare(name, rows, rows_ref), err)
    assert _worst(err, over) <= max(_worst(err, ~over), bound)


def test_harris_at_the_true_capacity(ctx, hook, blob, blob_dev):
    """Corners of the 2047 and 2048 blobs are refined in LDS, those of the 2049 and 2300 blobs -- and the sparse corners that jump
    into one -- in scratch; positions are the oracle's bit for bit (test_harris_keypoints)."""
    b, ref = blob
    got = corners(ctx, blob_dev)
    sent = route(hook, "harris")
    print("harris, blob cloud: %d of %d corners through scratch, %d entries per row" % (sent[0], len(got), sent[1]))
    assert sent == oc.harris_expected_overflow(ref["harris_counts"]) and sent[0] >= 5
    assert len(fc.compare("harris_keypoints", oc.xyz(got), ref["harris"][0])) == 0
    assert (got["rgba"] == 0).all()


# ------------------------------------------------------------------------------------------- (c) SC3D's random directions
def test_sc3d_scratch_rows_take_their_own_random_directions(ctx, hook, blob, blob_dev):
    """The mt19937 replay is per kept keypoint in keypoint order, whichever launch computes the row: the row of an overflowing
    keypoint in a call that holds only it and its predecessors is its row in the full call."""
    b, ref = blob
    counts = b.counts()
    full, kept, _ = describe(ctx, blob_dev, b.keypoints, "sc3d")
    assert route(hook, "sc3d")[0] == 6
    keep = fc.survivors(b.keypoints, kept)
    pos = np.cumsum(keep) - 1
    for i in np.flatnonzero(counts > oc.LDS_CAP["sc3d"]):
        rows, _, _ = describe(ctx, blob_dev, b.keypoints[:i + 1], "sc3d")
        sent = route(hook, "sc3d")
        assert sent[0] == (counts[:i + 1] > oc.LDS_CAP["sc3d"]).sum()
        assert len(rows) == pos[i] + 1
        assert same_bits(rows, full[:pos[i] + 1]), (i, first_difference(rows, full[:pos[i] + 1]))
    # and the draws differ from keypoint to keypoint: with its predecessors gone, the first overflowing blob's row changes
    i = int(np.flatnonzero((counts > oc.LDS_CAP["sc3d"]) & (np.arange(len(counts)) > 2))[0])
    alone, _, _ = describe(ctx, blob_dev, b.keypoints[i:i + 1], "sc3d")
    assert route(hook, "sc3d")[0] == 1 and len(alone) == 1 and not same_bits(alone[0], full[pos[i]])


# --------------------------------------------------------------------------------------------- (d) no state is left behind
def test_route_changes_leave_no_state(ctx, hook, blob, blob_dev, scene, scene_dev):
    b, _ = blob
    first = describe(ctx, blob_dev, b.keypoints, "pfh")
    c1 = hook.feature_overflow()
    hook.feature_lds_cap(128)
    between = describe(ctx, scene_dev[0], scene[0].keypoints, "pfh")
    assert hook.feature_lds_cap(0) == 128
    c2 = hook.feature_overflow()
    second = describe(ctx, blob_dev, b.keypoints, "pfh")
    c3 = hook.feature_overflow(reset=True)
    again = describe(ctx, scene_dev[0], scene[0].keypoints, "pfh")
    assert route(hook, "pfh") == (0, 0)
    assert same_bits(first[0], second[0]) and same_bits(first[1], second[1])
    assert same_bits(between[0], again[0]) and same_bits(between[1], again[1])
    blob_sent = oc.expected_overflow(b.counts(), "pfh")
    scene_sent = oc.expected_overflow(scene[0].counts, "pfh", 128)
    assert c1[:2] == list(blob_sent)
    assert c2[:2] == [blob_sent[0] + scene_sent[0], max(blob_sent[1], scene_sent[1])]
    assert c3[:2] == [2 * blob_sent[0] + scene_sent[0], max(blob_sent[1], scene_sent[1])]
    assert not any(c3[2:])

"""The feature kernels where neighbour distances tie exactly: normals, the Harris response and corners, and the six descriptors
against the oracle on the lattice clouds of tests/feature_cases.py, through compare() -- the project's criteria, stage by stage --
with ZERO failing points or rows wanted everywhere.  Each kernel rebuilds radiusSearch's (d2, index) order with a sorter of its
own; on these clouds nearly every neighbourhood holds equal d2, pairs sit exactly at d2 == r2 (the ball is open), points are
stored twice, and "the nearest neighbour" of the off-cloud keypoints is decided by index alone.

tests/test_feature_cases_cpu.py shows on the CPU that the clouds hold those ties and that a wrong tie order fails compare() on
hundreds of points or rows for the cases of feature_cases.TIE_ORDER_CHECKS; the rest (PFHRGB, the on-cloud keypoints, FPFH / PFH /
RSD / SC3D with the oracle's normals) is compared all the same, but is no tie-order check.  Everything stays below the kernels'
LDS capacities (largest neighbourhood < 300 points): the main kernels only."""
import datetime
import os

import numpy as np
import pytest

import feature_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(po):
    return fc.reference(po)


@pytest.fixture(scope="module")
def device(ctx, cases):
    """Per cloud: the device cloud and every normal set on the device."""
    return [dict(cloud=ctx.cloud(c.cloud), normals={ns: ctx.normals(v) for ns, v in c.normals.items()}) for c, _ in cases]


def xyz(a):
    return np.stack([a["x"], a["y"], a["z"]], axis=1).reshape(-1, 3)


def describe(ctx, dev, case, name, ns, keypoints):
    """(rows, keypoints after pruning, frames or None) of one descriptor on the device."""
    k = ctx.cloud(keypoints)
    d = ctx.computeLocalDescriptors(dev["cloud"], dev["normals"][ns], k, fc.DESCRIPTORS[name], fc.R_DESC)
    return d.numpy(), k.numpy(), d.frames() if name == "shot" else None


def report(wrong, case, what, bad, got, ref):
    if len(bad):
        i = int(bad[0])
        wrong.append("%s %s: %d of %d fail; first: %d, device %s, oracle %s"
                     % (case.name, what, len(bad), max(len(got), len(ref)), i, got[i] if i < len(got) else None, ref[i] if i < len(ref) else None))


def test_normals(ctx, cases, device):
    wrong = []
    for (c, ref), dev in zip(cases, device):
        got = ctx.computeSurfaceNormals(dev["cloud"], fc.R_NRM).numpy()
        report(wrong, c, "normals", fc.compare("normals", got, ref["normals", None, None]), got, ref["normals", None, None])
    assert not wrong, "\n".join(wrong)


def test_harris_response(ctx, cases, device):
    """Both normal sets, and on the plane the exactly vertical normals: every response 0.0f."""
    wrong = []
    for (c, ref), dev in zip(cases, device):
        for ns in sorted(c.normals):
            got = ctx.harrisResponse(dev["cloud"], dev["normals"][ns], fc.R_NRM)
            report(wrong, c, "response, normals %s" % ns, fc.compare("harris_response", got, ref["harris_response", ns, None]), got, ref["harris_response", ns, None])
    assert not wrong, "\n".join(wrong)


def test_harris_keypoints(ctx, cases, device):
    """Thresholds -1.0 and 0.0: equal responses keep each other (every point of the plane is a corner under vertical normals, and
    its singular refinement leaves it in place), corners that move on `corner`, NaN normals in the sums.  xyz bits, in order."""
    wrong = []
    for (c, ref), dev in zip(cases, device):
        for ns in sorted(c.normals):
            for thr in fc.HARRIS_THRESHOLDS:
                kp = ctx.detectKeypoints(dev["cloud"], dev["normals"][ns], 1, thr, fc.R_NRM, fc.H).numpy()
                want = ref["harris_keypoints", ns, thr]
                report(wrong, c, "corners, normals %s, threshold %g" % (ns, thr), fc.compare("harris_keypoints", xyz(kp), want), xyz(kp), want)
                assert (kp["rgba"] == 0).all()
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("name", list(fc.DESCRIPTORS))
def test_descriptor(ctx, cases, device, name):
    """Rows, the keypoints after pruning and (SHOT) the frames, both normal sets, both keypoint sets, radius 0.5."""
    wrong = []
    for (c, ref), dev in zip(cases, device):
        for ns in fc.NORMAL_SETS:
            for ks in fc.KEYPOINT_SETS:
                rows, kept, frames = describe(ctx, dev, c, name, ns, c.keypoints[ks])
                what = "%s, normals %s, keypoints %s" % (name, ns, ks)
                report(wrong, c, what + " (pruning)", fc.compare("keypoints", kept, ref["keypoints", name, ns, ks]), kept, ref["keypoints", name, ns, ks])
                report(wrong, c, what, fc.compare(name, rows, ref[name, ns, ks]), rows, ref[name, ns, ks])
                if frames is not None:
                    report(wrong, c, what + " (frames)", fc.compare("shot_frames", frames, ref["shot_frames", ns, ks]), frames, ref["shot_frames", ns, ks])
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("name", ["rsd", "shot", "sc3d", "pfh"])
def test_keypoint_counts_across_wave_and_block_edges(ctx, po, cases, device, name):
    """RSD, SHOT, SC3D (one wave per keypoint; k_rsd has four per block) and PFH (one block per keypoint) on the first 1, 4, 5, 63,
    64 and 65 off-cloud keypoints: the corresponding prefix of the full run's oracle rows (the far keypoint sits third, the
    1- and 2-neighbour ones 21st and 63rd, the 3-neighbour one 65th).  SC3D's mt19937 draws run in keypoint order, so its
    reference is the oracle on the same prefix."""
    wrong = []
    for (c, ref), dev in zip(cases, device):
        kp = c.keypoints["off"]
        keep = fc.survivors(kp, ref["keypoints", name, "random", "off"])
        for n in fc.PREFIXES:
            rows, kept, _ = describe(ctx, dev, c, name, "random", kp[:n])
            want = ref[name, "random", "off"][:keep[:n].sum()]
            if name == "sc3d":
                want = po.descriptors_sc3d(c.cloud, c.normals["random"], kp[:n], fc.R_DESC)[1]
            report(wrong, c, "%s, first %d keypoints (pruning)" % (name, n), fc.compare("keypoints", kept, kp[:n][keep[:n]]), kept, kp[:n][keep[:n]])
            report(wrong, c, "%s, first %d keypoints" % (name, n), fc.compare(name, rows, want), rows, want)
    assert not wrong, "\n".join(wrong)


def test_bit_equal_shares_on_lattice_inputs(ctx, cases, device):
    """SHOT, RSD and SC3D carry a tolerance because a double acos / atan2 (SHOT, RSD) or an atan2f / acosf ulp at a bin edge (SC3D)
    may differ between the two libms.  How many rows are bit-equal on these inputs is printed, with the exact counts a fix would
    move, and no minimum is asserted: the absolute criteria of compare() are the assertions (test_descriptor).  With
    MM3D_FEATURE_TIES_OUT set the figures are also written to that file (profiles/feature_ties.txt is such a run)."""
    lines = ["bit-equal rows of SHOT, RSD and SC3D against the oracle on the lattice clouds of tests/feature_cases.py",
             "run of %s; radius %g; rows = keypoints after pruning" % (datetime.date.today().isoformat(), fc.R_DESC), "",
             "%-7s %-5s %-7s %-4s %5s %9s %8s  %s" % ("cloud", "desc", "normals", "kp", "rows", "bit-equal", "share", "what differs")]
    for (c, ref), dev in zip(cases, device):
        for name in ("shot", "rsd", "sc3d"):
            for ns in fc.NORMAL_SETS:
                for ks in fc.KEYPOINT_SETS:
                    rows, _, _ = describe(ctx, dev, c, name, ns, c.keypoints[ks])
                    want = ref[name, ns, ks]
                    if rows.shape != want.shape:
                        lines.append("%-7s %-5s %-7s %-4s shapes differ: %s against %s" % (c.name, name, ns, ks, rows.shape, want.shape))
                        continue
                    diff = rows.view(np.uint32) != want.view(np.uint32)
                    same = ~diff.any(axis=1)
                    with np.errstate(invalid="ignore"):
                        delta = np.abs(rows.astype(np.float64) - want.astype(np.float64))
                    detail = "-"
                    if diff.any():
                        detail = "%d rows, %d values differ in bits, largest |delta| %.3g" % ((~same).sum(), diff.sum(), np.nanmax(delta))
                        if name == "sc3d":
                            moved = (delta > fc.SC3D_BIN_TOL).sum(axis=1)
                            detail += "; rows with a moved vote %d, most bins moved in a row %d" % ((moved > 0).sum(), moved.max())
                        if name == "rsd":
                            detail += "; rows beyond 1e-7: %d" % (delta > 1e-7).any(axis=1).sum()
                    lines.append("%-7s %-5s %-7s %-4s %5d %9d %7.2f%%  %s" % (c.name, name, ns, ks, len(want), same.sum(), 100.0 * same.mean() if len(want) else 100.0, detail))
    text = "\n".join(lines) + "\n"
    print(text)
    out = os.environ.get("MM3D_FEATURE_TIES_OUT")
    if out:
        with open(out, "w") as f:
            f.write(text)

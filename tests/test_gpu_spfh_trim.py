"""FPFH rows of small clouds, device against oracle, bit for bit, through computeLocalDescriptors with every point a keypoint: the
cases that exercise the bookkeeping around k_spfh's pair features (csrc/fpfh.hip) -- the per-candidate hit masks, the
candidate-major pool and its chunks, the pairs shared inside a block, the tile boundaries, and the epilogue's chain replay
(csrc/spfh_replay.hpp) at its shortest and longest chains.  The pair features themselves are held against the oracle on the same
pairs through mm3d_debug_pair_bins, as tests/test_gpu_spfh_pairs.py does."""
import numpy as np
import pytest

from test_gpu_spfh_pairs import as_normals, as_points, check_against_oracle, in_radius_pairs, xyz_of

R = 0.8


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def random_normals(rng, n):
    return unit(rng.normal(size=(n, 3))).astype(np.float32)


def ball(rng, n, radius, centre=(0.0, 0.0, 0.0)):
    v = unit(rng.normal(size=(n, 3))) * (radius * rng.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0))
    return (v + np.asarray(centre)).astype(np.float32)


def rows_equal_the_oracle(ctx, po, xyz, nrm, radius=R, label=""):
    pts, n = as_points(xyz), as_normals(nrm)
    ref_kp, ref = po.descriptors_fpfh(pts, n, pts, radius)
    kp = ctx.cloud(pts)
    got = ctx.computeLocalDescriptors(ctx.cloud(pts), ctx.normals(n), kp, 2, radius).numpy()
    got_kp = kp.numpy()
    assert len(got) == len(ref) and len(got_kp) == len(ref_kp), f"{label}: {len(got)} rows, the oracle keeps {len(ref)}"
    assert all(np.array_equal(got_kp[c], ref_kp[c]) for c in ("x", "y", "z")), f"{label}: other keypoints survive the pruning"
    bad = np.flatnonzero((got.view(np.uint32) != ref.view(np.uint32)).any(1))
    assert len(bad) == 0, f"{label}: {len(bad)} of {len(ref)} FPFH rows differ from the oracle (first: row {bad[0]})"
    return len(ref)


@pytest.mark.gpu
def test_planar_lattice_longest_chains(ctx, po):
    """(a) 20 x 20 lattice at 0.1 m in a plane, normals along z, radius 0.8: every hit of a point lands in one bin per feature."""
    g = np.arange(20, dtype=np.float32) * np.float32(0.1)
    xyz = np.stack([np.repeat(g, 20), np.tile(g, 20), np.zeros(400, np.float32)], 1)
    nrm = np.zeros((400, 3), np.float32); nrm[:, 2] = 1.0
    assert rows_equal_the_oracle(ctx, po, xyz, nrm, label="lattice") == 400


@pytest.mark.gpu
def test_one_two_and_three_neighbours(ctx, po):
    """(b) an isolated point, a pair and a triple, far from each other: |N| - 1 = 0 (100 / 0), 1 and 2."""
    rng = np.random.default_rng(5)
    xyz = np.float32([[0, 0, 0], [10, 0, 0], [10.3, 0.1, 0.05], [20, 0, 0], [20.2, 0.3, 0.1], [19.9, -0.2, 0.3]])
    rows_equal_the_oracle(ctx, po, xyz, random_normals(rng, len(xyz)), label="1, 2, 3 neighbours")
    for k in (1, 2, 3):                                   # and each group as a cloud of its own
        sub = xyz[{1: slice(0, 1), 2: slice(1, 3), 3: slice(3, 6)}[k]]
        rows_equal_the_oracle(ctx, po, sub, random_normals(rng, len(sub)), label=f"{k} points")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [300, 520])
def test_compact_blob(ctx, po, n):
    """(c) more than one block, pairs inside a block and across blocks, items of fewer than 64 points."""
    rng = np.random.default_rng(n)
    assert rows_equal_the_oracle(ctx, po, ball(rng, n, 1.2), random_normals(rng, n), label=f"blob {n}") == n


@pytest.mark.gpu
@pytest.mark.parametrize("dense", [64, 150])
def test_a_tile_with_more_hits_than_the_pool(ctx, po, dense):
    """(d) `dense` points inside a ball of radius r / 2 (every one within r of every other) plus 200 spread points: one tile's hits
    exceed kSpfhPool, so the pool is filled and emptied in chunks."""
    rng = np.random.default_rng(dense)
    xyz = np.concatenate([ball(rng, dense, 0.5 * R - 0.01), ball(rng, 200, 3.0)])
    rows_equal_the_oracle(ctx, po, xyz, random_normals(rng, len(xyz)), label=f"dense {dense} + 200")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 65, 128])
def test_tile_boundaries(ctx, po, n):
    """(e) n points within r / 2 of each other: every wave stages exactly n candidates (one full tile, one more, two full)."""
    rng = np.random.default_rng(1000 + n)
    assert rows_equal_the_oracle(ctx, po, ball(rng, n, 0.25 * R), random_normals(rng, n), label=f"{n} candidates") == n


@pytest.mark.gpu
def test_exact_tie_inside_one_block(ctx, po):
    """(f) two points with parallel normals perpendicular to their difference vector: both angles are 0, an exact tie, so the pair
    is evaluated the second way for the candidate's histogram -- with a few more points around them."""
    rng = np.random.default_rng(6)
    xyz = np.concatenate([np.float32([[0, 0, 0], [0.5, 0, 0]]), ball(rng, 20, 0.6, (0.25, 0, 0))])
    nrm = np.concatenate([np.float32([[0, 0, 1], [0, 0, 1]]), random_normals(rng, 20)])
    rows_equal_the_oracle(ctx, po, xyz, nrm, label="tie + 20")
    rows_equal_the_oracle(ctx, po, xyz[:2], nrm[:2], label="tie alone")


@pytest.mark.gpu
def test_translated_cloud_and_its_pair_features(ctx, mm, po):
    """(g) a blob translated by (1000, -2000, 30) m; and the certified pair path, unchanged, on that cloud's in-radius pairs."""
    rng = np.random.default_rng(7)
    xyz = (ball(rng, 300, 1.2).astype(np.float64) + np.float64([1000.0, -2000.0, 30.0])).astype(np.float32)
    nrm = random_normals(rng, 300)
    assert rows_equal_the_oracle(ctx, po, xyz, nrm, label="translated blob") == 300
    i, j = in_radius_pairs(xyz, R)
    assert len(i) > 10_000
    pts, n = as_points(xyz), as_normals(nrm)
    check_against_oracle(ctx, mm, po, (pts[i], n[i], pts[j], n[j]), "translated blob's pairs")
    assert np.array_equal(xyz_of(pts), xyz)

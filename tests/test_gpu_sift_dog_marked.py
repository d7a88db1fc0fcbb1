"""The exact DoG of single marked points (csrc/sift.hip::k_sift_dog_marked, test hook mm3d_debug_sift_dog_marked): step 4 of
the certified SIFT octave gives the few points its certificate leaves open the CPU path's float sums, one block per point --
the ball's members as (d2, index) keys, sorted, summed in list order; lists longer than the sort buffer in distance bands.
Every comparison here is bit for bit against the `dog` rows of the oracle's scale space of the same octave cloud.
Run with `-m gpu` on the MI355X box; all calls go through the C ABI."""
import numpy as np
import pytest

from test_gpu_sift_cert import RES, R_DESC, MIN_NB, random_scene

pytestmark = pytest.mark.gpu

EUNSUPPORTED = -4        # include/mm3d.h: a size outside what the kernels are built for
SMALL_K = 128            # the sort buffer of the small_capacity instantiation (csrc/sift.hip::kMarkedCapSmall)
GRID_BLOCKS = 256        # the launch's fixed grid: more ids than this and a block strides over the list


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def seeded_ids(n, count, seed):
    """`count` distinct ids of range(n), the first and the last point among them."""
    rng = np.random.default_rng(seed)
    ids = rng.choice(n, size=min(count, n), replace=False).astype(np.int32)
    ids[0], ids[-1] = 0, n - 1
    return np.unique(ids)


@pytest.fixture(scope="module")
def big_scene(po, synth):
    """The scene of tests/test_gpu_sift_cert.py: three populated octaves (about 50 k filtered points)."""
    world, maps = synth.synth_maps(2, 70000, overlap_step=0.35)
    x, c, _ = maps[0]
    raw = synth.pack_points(x, c)
    return po.remove_outliers(po.downsample(raw, RES), R_DESC, MIN_NB)


@pytest.fixture(scope="module")
def big_reference(po, big_scene):
    """The oracle's float DoG of the three octaves, computed once: {octave: dog[n, 5]}."""
    ref = {}
    for octv in range(3):
        r = po.sift_octave_debug(big_scene, RES, octv)
        assert r is not None
        ref[octv] = r[1]
    return ref


@pytest.fixture(scope="module")
def lattice(po):
    """The 61 x 61 lattice at 0.1 spacing of test_ties_everywhere...: many equal distances, index order decides."""
    gx, gy = np.meshgrid(np.arange(-30, 31) * 0.1, np.arange(-30, 31) * 0.1)
    pts = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], 1).astype(np.float32)
    c = np.zeros(len(pts), dtype=po.POINT)
    c["x"], c["y"], c["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    c["rgba"] = np.where(c["x"] < 0.0, 0xFF404040, 0xFF808080).astype(np.uint32)
    r = po.sift_octave_debug(c, 0.1, 0)
    assert r is not None and len(r[0]) == 3721
    return c, r[1]


@pytest.mark.parametrize("octave", range(3))
def test_ordinary_lists_and_their_bands(ctx, big_scene, big_reference, octave):
    """300 seeded ids per octave, the first and the last point among them: the oracle's bits with the product's buffer (one
    band) and with the small one (every list several bands)."""
    dog = big_reference[octave]
    ids = seeded_ids(len(dog), 300, 10 + octave)
    cloud = ctx.cloud(big_scene)
    one = ctx.siftDogMarked(cloud, RES, octave, ids)
    assert np.array_equal(bits(one), bits(dog[ids]))
    banded = ctx.siftDogMarked(cloud, RES, octave, ids, small_capacity=True)
    assert np.array_equal(bits(banded), bits(one))
    assert np.array_equal(bits(banded), bits(dog[ids]))


@pytest.mark.parametrize("small", (False, True))
def test_ties_and_band_edges_inside_runs_of_equal_distances(ctx, lattice, small):
    """Every point of the lattice (3 721 ids: far more than the grid has blocks, so the blocks stride over the list)."""
    c, dog = lattice
    ids = np.arange(len(dog), dtype=np.int32)
    assert len(ids) > GRID_BLOCKS
    got = ctx.siftDogMarked(ctx.cloud(c), 0.1, 0, ids, small_capacity=small)
    assert np.array_equal(bits(got), bits(dog))


def test_duplicated_points(ctx, po):
    """The jittered lattice with a tenth of its points duplicated -- after the octave's voxel grid the copies are gone, the
    near-coincident centroids stay: lists that begin with several entries at d2 = 0 or next to it."""
    cloud, res, _ = random_scene(po, 3)
    r = po.sift_octave_debug(cloud, res, 0)
    assert r is not None
    dog = r[1]
    ids = seeded_ids(len(dog), 500, 3)
    for small in (False, True):
        got = ctx.siftDogMarked(ctx.cloud(cloud), res, 0, ids, small_capacity=small)
        assert np.array_equal(bits(got), bits(dog[ids])), small


@pytest.mark.parametrize("seed", (2, 6))
def test_sparse_border(ctx, po, seed):
    """The sparse scatter in a slab, 200 ids: at resolution 0.2 (seed 2) lists of 56 to 140 entries, at 0.1 (seed 6) of 9 to 50
    -- a handful at the slab's border.  (Lists of the query alone and of two or three entries: the far points of
    test_overflow_is_reported_not_miscounted.)"""
    cloud, res, _ = random_scene(po, seed)
    r = po.sift_octave_debug(cloud, res, 0)
    assert r is not None
    oc, dog, resp, cnt, knn = r
    ids = seeded_ids(len(dog), 200, seed)
    print(f"seed {seed}: lists of {cnt[ids, 5].min()} to {cnt[ids, 5].max()} entries, median {np.median(cnt[ids, 5])}")
    for small in (False, True):
        got = ctx.siftDogMarked(ctx.cloud(cloud), res, 0, ids, small_capacity=small)
        assert np.array_equal(bits(got), bits(dog[ids])), small


def test_counts(ctx, lattice):
    """No id: nothing is touched.  One id works.  (More ids than blocks: the lattice test above.)"""
    c, dog = lattice
    cloud = ctx.cloud(c)
    none = ctx.siftDogMarked(cloud, 0.1, 0, np.zeros(0, dtype=np.int32))
    assert none.shape == (0, 5)
    one = ctx.siftDogMarked(cloud, 0.1, 0, np.array([1860], dtype=np.int32))
    assert np.array_equal(bits(one), bits(dog[[1860]]))
    with pytest.raises(Exception) as e:
        ctx.siftDogMarked(cloud, 0.1, 0, np.array([len(dog)], dtype=np.int32))
    assert getattr(e.value, "status", None) == -1


def sphere_scene(po):
    """300 points on ONE sphere around the origin whose float squared distances to it are all equal, and three points far
    away.  The float coordinates nearest to an arbitrary sphere would not give equal float distances, so the points are the
    integer triples of squared norm 2141 (936 of them) scaled by 2^-6: every product and sum of ((dx dx + dy dy) + dz dz) is
    exact, d2 = 2141 / 4096 = 0.5227 for all of them (radius 0.723: inside octave 0's 3 sigma_max ball of 0.756).  One point
    per 0.1 voxel is taken, so that the octave's voxel grid returns every point as it is."""
    n2, scale = 2141, 2.0 ** -6
    m = int(np.sqrt(n2))
    a, b = np.meshgrid(np.arange(-m, m + 1), np.arange(-m, m + 1), indexing="ij")
    c2 = n2 - a * a - b * b
    c = np.rint(np.sqrt(np.maximum(c2, 0))).astype(np.int64)
    ok = (c2 >= 0) & (c * c == c2)
    a, b, c = a[ok], b[ok], c[ok]
    v = np.concatenate([np.stack([a, b, c], 1), np.stack([a, b, -c], 1)[c > 0]])
    p = (v * scale).astype(np.float32)
    _, first = np.unique(np.floor(p * np.float32(10.0)).astype(np.int64), axis=0, return_index=True)
    sphere = p[np.sort(first)[:300]]
    assert len(sphere) == 300
    far = np.array([[5.05, 0.05, 0.05], [5.05, 0.35, 0.05], [5.35, 0.05, 0.05]], dtype=np.float32)
    p = np.concatenate([np.zeros((1, 3), dtype=np.float32), sphere, far])
    cl = np.zeros(len(p), dtype=po.POINT)
    cl["x"], cl["y"], cl["z"] = p[:, 0], p[:, 1], p[:, 2]
    cl["rgba"] = (0xFF000000 | (np.arange(len(p)) * 7919 % 256 * 0x010101)).astype(np.uint32)
    return cl


def test_overflow_is_reported_not_miscounted(ctx, po):
    """With the small buffer the sphere's centre has more list entries at ONE squared distance than the buffer holds, which no
    band can split: the hook must say "does not fit" -- and still give a point outside the sphere's reach its bits."""
    c = sphere_scene(po)
    r = po.sift_octave_debug(c, 0.1, 0)
    assert r is not None
    oc, dog, resp, cnt, knn = r
    x = np.stack([oc["x"], oc["y"], oc["z"]], 1)
    d0 = np.linalg.norm(x.astype(np.float64), axis=1)
    centre_id, far_id = int(np.argmin(d0)), int(np.argmax(d0))
    # the float squared distances as the search computes them: ((dx dx + dy dy) + dz dz) in float32
    d = (x - x[centre_id]).astype(np.float32)
    d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float32) + d[:, 2] * d[:, 2]).astype(np.float32)
    most = int(np.unique(d2.view(np.uint32), return_counts=True)[1].max())
    print(f"sphere: octave cloud of {len(oc)} points, {most} at the most common squared distance from the centre")
    if most <= SMALL_K:
        pytest.skip(f"only {most} points share the most common squared distance: not above the small buffer's {SMALL_K}")
    cloud = ctx.cloud(c)
    with pytest.raises(Exception) as e:
        ctx.siftDogMarked(cloud, 0.1, 0, np.array([centre_id], dtype=np.int32), small_capacity=True)
    assert getattr(e.value, "status", None) == EUNSUPPORTED
    got = ctx.siftDogMarked(cloud, 0.1, 0, np.array([far_id], dtype=np.int32), small_capacity=True)
    assert np.array_equal(bits(got), bits(dog[[far_id]]))
    # the three far points: lists of the query alone and of two or three entries, at both capacities
    far_ids = np.sort(np.argsort(d0)[-3:]).astype(np.int32)
    assert cnt[far_ids, 0].min() == 1 and cnt[far_ids, 5].max() <= 3
    for small in (False, True):
        got = ctx.siftDogMarked(cloud, 0.1, 0, far_ids, small_capacity=small)
        assert np.array_equal(bits(got), bits(dog[far_ids])), small
    # the product's buffer holds the centre's list: the oracle's bits
    got = ctx.siftDogMarked(cloud, 0.1, 0, np.array([centre_id], dtype=np.int32))
    assert np.array_equal(bits(got), bits(dog[[centre_id]]))

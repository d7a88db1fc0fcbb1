"""SAC-IA's error kernel (csrc/registration.hip::k_sacia_err) gives a thread K source keypoints of its hypothesis: a tile is
256 K consecutive queries, the last tile of a pair is ragged, and the shorter pairs of a batch leave whole tiles out.  Through
the entry the parity tests use (estimateTransformFromDescriptorsSets) against the CPU oracle, the transform bit for bit, with
source keypoint counts on either side of one tile and of two, few and many hypotheses, K forced on (small launches would
otherwise keep one query per thread) and left to the launch's size; and one batch of pairs whose sources differ in size
through estimateMapsTransforms without the ICP refinement, whose pair transforms are then SAC-IA's own."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NT = 300


def _keypoints(mm, rng, n, shift):
    a = np.zeros(n, dtype=mm.POINT)
    a["x"] = rng.uniform(-6, 6, n) + shift
    a["y"] = rng.uniform(-6, 6, n) - 0.5 * shift
    a["z"] = rng.uniform(0, 2, n)
    a["rgba"] = 0xFF808080
    return a


@pytest.fixture(scope="module")
def clouds(mm):
    """One target and the largest source; the smaller sources are its prefixes."""
    k = mm.sacia_queries_per_thread()
    rng = np.random.default_rng(21)
    n_max = 2 * 256 * k + 3
    tgt = _keypoints(mm, rng, NT, 0.0)
    src = _keypoints(mm, rng, n_max, 0.7)
    # descriptors: a few clusters, so that the ten nearest features of a source row are not arbitrary
    centres = rng.uniform(0, 100, (12, 33)).astype(np.float32)
    td = (centres[rng.integers(0, 12, NT)] + rng.normal(0, 3, (NT, 33))).astype(np.float32)
    sd = (centres[rng.integers(0, 12, n_max)] + rng.normal(0, 3, (n_max, 33))).astype(np.float32)
    return k, src, sd, tgt, td


@pytest.fixture(scope="module")
def forced(mm):
    def force(k):
        mm.sacia_queries_per_thread(k)
    yield force
    mm.sacia_queries_per_thread(0)


def _counts(k):
    return [1, 255, 256 * k - 1, 256 * k + 1, 2 * 256 * k + 3]


@pytest.mark.parametrize("hyp", [7, 513])
@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("force_k", [True, False])
def test_sac_ia_tiles_against_the_oracle(ctx, po, clouds, forced, which, hyp, force_k):
    k, src, sd, tgt, td = clouds
    ns = _counts(k)[which]
    forced(k if force_k else 0)
    po.srand(100 + which)
    T_ref, best_it, _ = po.sac_ia(src[:ns], sd[:ns], tgt, td, 0.5, 1.0, hyp)
    ctx.srand(100 + which)
    T = ctx.estimateTransformFromDescriptorsSets(ctx.cloud(src[:ns]), ctx.descriptors(sd[:ns]), ctx.cloud(tgt), ctx.descriptors(td), 0.5, 1.0, hyp)
    assert np.array_equal(T.view(np.uint32), T_ref.view(np.uint32)), (ns, hyp, k, best_it)
    if ns >= 3:
        assert best_it >= 0


@pytest.mark.parametrize("force_k", [1, 2, 4, 8])
def test_every_tile_width_gives_the_same_transform(ctx, po, clouds, forced, force_k):
    """The other widths the kernel is compiled for, on the count that leaves their last tile ragged and one lane short."""
    _, src, sd, tgt, td = clouds
    ns = min(len(src), 256 * force_k + 63)
    forced(force_k)
    po.srand(7)
    T_ref, _, _ = po.sac_ia(src[:ns], sd[:ns], tgt, td, 0.5, 1.0, 64)
    ctx.srand(7)
    T = ctx.estimateTransformFromDescriptorsSets(ctx.cloud(src[:ns]), ctx.descriptors(sd[:ns]), ctx.cloud(tgt), ctx.descriptors(td), 0.5, 1.0, 64)
    assert np.array_equal(T.view(np.uint32), T_ref.view(np.uint32)), (ns, force_k)


def test_a_batch_of_pairs_whose_sources_differ_in_size(ctx, po, mm, synth, forced):
    """Three maps of different sizes, every pair scored by SAC-IA, no refinement: the pairs of one batch share a launch as
    wide as the largest of them, and the smaller ones' blocks past their last tile leave at once."""
    _, maps = synth.synth_maps(3, 9000, overlap_step=0.35)
    raws = [synth.pack_points(x, c) for x, c, _ in maps]
    raws = [raws[0], raws[1][:6500], raws[2][:4500]]
    params = mm.MapMergingParams(descriptor_type=2, estimation_method=1, refine_transform=0)
    op = po.params_default(); op.descriptor_type = 2; op.estimation_method = 1; op.refine_transform = 0
    forced(mm.sacia_queries_per_thread())
    po.srand(4); ctx.srand(4)
    _, ref_pairs = po.estimate_maps_transforms(raws, op)
    _, pairs = ctx.estimateMapsTransforms(raws, params, return_pairs=True)
    assert len(pairs) == len(ref_pairs) == 3
    sizes = set()
    for r in raws:
        f = ctx.mapFeatures(ctx.cloud(r), params)
        sizes.add(len(f.keypoints.numpy()))
        f.free()
    assert len(sizes) == 3, sizes                       # the sources do differ
    for p, r in zip(pairs, ref_pairs):
        assert (p["source_idx"], p["target_idx"]) == (r["source_idx"], r["target_idx"])
        assert np.array_equal(p["transform"].view(np.uint32), r["transform"].view(np.uint32)), (p["source_idx"], p["target_idx"])

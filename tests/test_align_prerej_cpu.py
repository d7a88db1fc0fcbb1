"""Prerejective alignment without a GPU: the header and the library carry the surface, the option defaults are the stated ones,
the NULL paths return MM3D_EINVAL, the numpy generator of tests/test_gpu_align_prerej.py reproduces literal vectors (the same
ones pin the device's generator there), and the shim reads MM3D_ALIGN (the shim itself compiles in test_shim_cpu.py)."""
import ctypes as C
import os
import re

import numpy as np

from test_gpu_align_prerej import GENERATOR_VECTORS, bounded, draws, rigid_fit, survivors, words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


def test_header_declares_the_alignment():
    h = _read("include", "mm3d.h")
    assert re.search(r"MM3D_ALIGN_SAC_IA\s*=\s*0\s*,\s*MM3D_ALIGN_PREREJECTIVE\s*=\s*1", h)
    for decl in (r"void mm3d_alignment_options_default\(mm3d_alignment_options \*o\);",
                 r"int mm3d_set_alignment\(mm3d_ctx \*ctx, const mm3d_alignment_options \*options\);",
                 r"int mm3d_get_alignment\(const mm3d_ctx \*ctx, mm3d_alignment_options \*options\);",
                 r"int mm3d_last_alignment_stats\(const mm3d_ctx \*ctx, mm3d_alignment_stats \*stats\);",
                 r"int mm3d_estimate_transform_prerejective\(mm3d_ctx \*ctx, const mm3d_cloud \*source_keypoints, "
                 r"const mm3d_desc \*source_descriptors,\s*const mm3d_cloud \*target_keypoints, const mm3d_desc \*target_descriptors,\s*"
                 r"double inlier_distance, const mm3d_alignment_options \*options, float T\[16\],\s*mm3d_alignment_stats \*stats\);"):
        assert re.search(decl, h), decl
    # mm3d_params and mm3d_pair_result carry nothing of it
    for struct in ("mm3d_params", "mm3d_pair_result"):
        body = h[:h.index("} " + struct + ";")]
        assert "align" not in body[body.rindex("typedef struct"):]


def test_library_exports_and_defaults(mm):
    L = mm.lib()
    for name in ("mm3d_alignment_options_default", "mm3d_set_alignment", "mm3d_get_alignment", "mm3d_last_alignment_stats",
                 "mm3d_estimate_transform_prerejective", "mm3d_debug_prerejective_survivors"):
        assert hasattr(L, name), name
    o = mm.AlignmentOptions()
    assert C.sizeof(o) == 32 and C.sizeof(mm.AlignmentStats) == 40
    assert (o.method, o.k, o.similarity, o.inlier_fraction) == (mm.AlignMethod.SAC_IA, 10, 0.9, 0.25)
    assert 1 <= o.samples <= 1 << 30 and o.samples & (o.samples - 1) == 0
    L.mm3d_alignment_options_default(None)                      # a NULL is ignored


def test_null_arguments_are_einval(mm):
    L = mm.lib()
    o, st = mm.AlignmentOptions(), mm.AlignmentStats()
    T = (C.c_float * 16)()
    n = C.c_size_t()
    assert L.mm3d_set_alignment(None, C.byref(o)) == EINVAL
    assert L.mm3d_get_alignment(None, C.byref(o)) == EINVAL
    assert L.mm3d_last_alignment_stats(None, C.byref(st)) == EINVAL
    assert L.mm3d_estimate_transform_prerejective(None, None, None, None, None, C.c_double(1.0), C.byref(o), T, C.byref(st)) == EINVAL
    assert L.mm3d_debug_prerejective_survivors(None, None, None, None, None, C.c_double(1.0), C.byref(o), None, None, C.c_size_t(0),
                                               C.byref(n)) == EINVAL


def test_generator_reproduces_the_literal_vectors():
    for seed, h, ns, kk, idx, pick in GENERATOR_VECTORS:
        i, p = draws(seed, [h], ns, kk)
        assert tuple(int(v) for v in i[0]) == idx, (seed, h)
        assert tuple(int(v) for v in p[0]) == pick, (seed, h)
    # word 0 of (seed 1, h 0), written out with Python integers
    M = (1 << 64) - 1
    z = (((1 << 32) | 0) + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z ^= z >> 31
    assert int(words(1, [0])[0, 0]) == z and int(bounded(np.array([z], dtype=np.uint64), 1000)[0]) == ((z >> 32) * 1000) >> 32


def test_draws_are_distinct_uniform_and_a_function_of_seed_and_h():
    idx, pick = draws(5, np.arange(200000), 7, 3)
    assert ((idx >= 0) & (idx < 7)).all() and ((pick >= 0) & (pick < 3)).all()
    assert (idx[:, 0] != idx[:, 1]).all() and (idx[:, 0] != idx[:, 2]).all() and (idx[:, 1] != idx[:, 2]).all()
    for col in range(3):                                        # each of the 7 keypoints about one time in seven
        f = np.bincount(idx[:, col], minlength=7) / len(idx)
        assert np.abs(f - 1 / 7).max() < 0.01
    again, _ = draws(5, np.arange(1000, 2000), 7, 3)            # any slice of the stream is the same stream
    assert np.array_equal(again, idx[1000:2000])
    assert not np.array_equal(draws(6, np.arange(1000), 7, 3)[0], idx[:1000])


def test_restated_survivors_keep_congruent_triangles_only():
    rng = np.random.default_rng(0)
    src = rng.uniform(-5, 5, (60, 3)).astype(np.float32)
    T = rigid_fit(src[:3], src[:3] + np.float32(1.0))
    assert np.allclose(T[:3, :3], np.eye(3), atol=1e-6) and np.allclose(T[:3, 3], 1.0, atol=1e-6)
    tgt = (src + np.float32(2.0)).astype(np.float32)
    nn = np.stack([np.arange(60), (np.arange(60) + 1) % 60], axis=1)          # the true match, then a wrong one
    rows = survivors(src, tgt, nn, 1, 4000, 0.999)
    assert len(rows) > 100 and (np.diff(rows[:, 0]) > 0).all()
    assert (rows[:, 1:4] == rows[:, 4:7]).mean() > 0.99          # nearly every survivor took the three true matches
    loose = survivors(src, tgt, nn, 1, 4000, 0.0)               # similarity 0 rejects only a repeated target
    assert 3800 < len(loose) < 4000 and all(len(set(r[4:7])) == 3 for r in loose.tolist())


def test_shim_selects_the_alignment_from_the_environment():
    s = _read("include", "map_merge_3d_shim.hpp")
    assert 'std::getenv("MM3D_ALIGN")' in s and 'std::getenv("MM3D_ALIGN_SAMPLES")' in s
    assert "o.method = MM3D_ALIGN_PREREJECTIVE" in s and "mm3d_set_alignment(e, &o)" in s
    assert re.search(r'align == "prerejective" && std::getenv\("MM3D_DEVICES"\)', s)

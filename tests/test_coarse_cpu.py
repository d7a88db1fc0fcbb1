"""The correlative coarse alignment without a GPU: the header declares it, the library exports it and the ctypes mirror binds
it, the defaults, the NULL and range handling of the entry points that touch no device, the shim's MM3D_COARSE, and the numpy
restatement of tests/test_gpu_coarse.py: it reproduces the literal vectors committed there, recovers the planted poses of the
yard within the margin the GPU test asserts, and its plane error on the tilted scene is below the figure that test doubles."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import test_gpu_coarse as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _read(*p):
    return open(os.path.join(ROOT, *p)).read()


def test_header_declares_the_surface():
    h = _read("include", "mm3d.h")
    assert re.search(r"typedef enum \{ MM3D_COARSE_NONE = 0, MM3D_COARSE_CORRELATIVE = 1 \} mm3d_coarse_method;", h)
    assert re.search(r"typedef struct mm3d_coarse_options \{\s*int method;[^}]*double cell;[^}]*int cell_factor;[^}]*int yaw_steps;"
                     r"[^}]*int yaw_factor;[^}]*int candidates;[^}]*double wall_nz;[^}]*double ground_nz;[^}]*int min_points;"
                     r"[^}]*double accept_fraction;[^}]*\} mm3d_coarse_options;", h)
    assert re.search(r"typedef struct mm3d_coarse_stats \{\s*int source_cells, target_cells;[^}]*int coarse_votes;[^}]*int candidates;"
                     r"[^}]*int score;[^}]*int yaw_index;[^}]*int ground_pairs;[^}]*int converged;\s*\} mm3d_coarse_stats;", h)
    for decl in (r"void mm3d_coarse_options_default\(mm3d_coarse_options \*o\);",
                 r"int mm3d_set_coarse_alignment\(mm3d_ctx \*ctx, const mm3d_coarse_options \*options\);",
                 r"int mm3d_get_coarse_alignment\(const mm3d_ctx \*ctx, mm3d_coarse_options \*options\);",
                 r"int mm3d_last_coarse_stats\(const mm3d_ctx \*ctx, mm3d_coarse_stats \*stats\);",
                 r"int mm3d_estimate_transform_correlative\(mm3d_ctx \*ctx, const mm3d_cloud \*source, const mm3d_normals \*source_normals,",
                 r"int mm3d_debug_correlative_signature\(", r"int mm3d_debug_correlative_votes\("):
        assert re.search(decl, h), decl
    # the alignment's enum did not grow: the correlative search is not a third value of it
    assert re.search(r"MM3D_ALIGN_SAC_IA = 0, MM3D_ALIGN_PREREJECTIVE = 1 \}", h)
    assert "2^24" in h and "2^24" in _read("INTEGRATION.md")          # the size limits are stated in both


def test_library_exports_and_mirror_binds(mm):
    lib = mm.lib()
    for name in ("mm3d_coarse_options_default", "mm3d_set_coarse_alignment", "mm3d_get_coarse_alignment", "mm3d_last_coarse_stats",
                 "mm3d_estimate_transform_correlative", "mm3d_debug_correlative_signature", "mm3d_debug_correlative_votes"):
        assert getattr(lib, name)
    for name in ("setCoarseAlignment", "getCoarseAlignment", "lastCoarseStats", "estimateTransformCorrelative", "correlativeSignature",
                 "correlativeVotes"):
        assert callable(getattr(mm.Context, name))
    assert (mm.CoarseMethod.NONE, mm.CoarseMethod.CORRELATIVE) == (0, 1)
    assert C.sizeof(mm.CoarseStats) == 32


def test_defaults_and_null_handling(mm):
    o = mm.CoarseOptions()
    assert o.as_tuple() == (0, 0.0, 4, 720, 6, 32, 0.5, 0.9, 3, 0.25)
    lib = mm.lib()
    lib.mm3d_coarse_options_default(None)                 # a no-op, not a crash
    st = mm.CoarseStats()
    T = (C.c_float * 16)()
    n = (C.c_size_t * 3)()
    frame = (C.c_int * 5)()
    assert lib.mm3d_set_coarse_alignment(None, C.byref(o)) == EINVAL
    assert lib.mm3d_get_coarse_alignment(None, C.byref(o)) == EINVAL
    assert lib.mm3d_last_coarse_stats(None, C.byref(st)) == EINVAL
    assert lib.mm3d_estimate_transform_correlative(None, None, None, None, None, C.byref(o), T, C.byref(st)) == EINVAL
    assert lib.mm3d_debug_correlative_signature(None, None, None, C.byref(o), None, None, None, None, C.c_size_t(0), n) == EINVAL
    assert lib.mm3d_debug_correlative_votes(None, None, None, None, None, C.byref(o), 0, frame, None, C.c_size_t(0), None, None,
                                            C.c_size_t(0), C.byref(C.c_size_t())) == EINVAL


BAD = [dict(method=2), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=1e-45), dict(cell_factor=0), dict(cell_factor=17),
       dict(yaw_steps=7), dict(yaw_steps=7201), dict(yaw_factor=0), dict(yaw_steps=720, yaw_factor=7), dict(candidates=0),
       dict(candidates=1025), dict(wall_nz=-0.1), dict(wall_nz=1.5, ground_nz=1.0), dict(wall_nz=0.9, ground_nz=0.9), dict(ground_nz=1.1),
       dict(ground_nz=float("nan")), dict(min_points=0), dict(accept_fraction=-0.1), dict(accept_fraction=float("nan"))]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
@pytest.mark.parametrize("method", [0, 1])
def test_out_of_range_options_are_refused_whatever_the_method(mm, bad, method):
    """The check comes before anything touches a device or the handle: a context that is never dereferenced shows it."""
    o = mm.CoarseOptions(**{"method": method, **bad})
    fake = C.create_string_buffer(1 << 16)                 # never read: the options are checked first
    assert mm.lib().mm3d_set_coarse_alignment(C.cast(fake, C.c_void_p), C.byref(o)) == EINVAL


def test_shim_reads_the_environment():
    s = _read("include", "map_merge_3d_shim.hpp")
    assert 'std::getenv("MM3D_COARSE")' in s
    assert "mm3d_set_coarse_alignment(e, &coarse)" in s
    assert re.search(r"correlative.*MM3D_DEVICES", s)


def test_cells_on_lattice_lines():
    p = np.array([[0.0, -0.0], [-1.0, -1e-7], [2.5, -2.5], [0.49999997, 0.5]], dtype=np.float32)
    assert G.cells_of(p, 0.5).tolist() == [[0, 0], [-2, -1], [5, -5], [0, 1]]


def test_restatement_reproduces_the_ten_point_cells():
    sig = G.restate_signature(G.TEN_POINTS, G.TEN_NORMALS, 0.5, F=2, min_points=2)
    assert sig["structure"].tolist() == G.TEN_STRUCTURE
    assert sig["ground"].tolist() == G.TEN_GROUND
    assert sig["coarse"].tolist() == G.TEN_COARSE
    assert sig["ground_height"].tolist() == [float(np.float32(0.5 * (float(np.float32(0.5)) + float(np.float32(0.7)))))]
    assert abs(sig["ground_height"][0] - G.TEN_HEIGHT[0]) < 1e-7


def test_restatement_reproduces_the_three_by_three_votes():
    acc, u0, v0 = G.restate_votes(np.array(G.PAIR_SRC), np.array(G.PAIR_TGT), 1.0, 1, 2, 8)
    assert acc.shape[0] == 4
    for q, want in G.PAIR_VOTES.items():
        got = {(int(u) + u0, int(v) + v0): int(acc[q, u, v]) for u, v in zip(*np.nonzero(acc[q]))}
        assert got == want, q
    assert acc.sum(axis=(1, 2)).tolist() == [6, 6, 6, 6]
    # the identity's double vote is the best candidate, and nothing next to it survives
    cands = G.restate_candidates(acc, u0, v0, 8)
    assert cands[0].tolist() == [0, 0, 1, 2]
    assert all(max(abs(int(c[1]) - 0), abs(int(c[2]) - 1)) > 1 or c[0] == 2 for c in cands[1:])


@pytest.fixture(scope="module")
def yard_signature():
    xyz, nrm = G.yard()
    return G.restate_signature(xyz.astype(np.float32), nrm.astype(np.float32), G.CELL)


@pytest.mark.parametrize("yaw_deg,shift", [(35.0, (3.0, -2.0)), (-110.0, (-1.5, 4.0)), (180.0, (0.5, 0.5))])
def test_restatement_recovers_a_lattice_pose(yard_signature, yaw_deg, shift):
    src, _ = G._planted_pair(G.pose(yaw_deg, shift))
    r = G.restate_align(G.restate_signature(*src, G.CELL), yard_signature, G.CELL, 4, 2, 72, 32)
    print(r["stats"], r["T"][:3, 3])
    assert r["stats"]["converged"] == 1
    G._check_lattice(r["stats"]["yaw_index"], r["T"], yaw_deg, shift, 72)
    assert abs(r["T"][2, 3]) < 0.02 and abs(r["T"][2, 0]) < 2e-3 and abs(r["T"][2, 1]) < 2e-3


def test_restatement_plane_error_on_the_tilted_scene(yard_signature):
    src, _ = G._planted_pair(G.pose(**G.TILTED))
    r = G.restate_align(G.restate_signature(*src, G.CELL), yard_signature, G.CELL, 4, 2, 72, 32)
    want = G.planted_plane(**G.TILTED)
    err = [abs(g - w) for g, w in zip(r["plane"], want)]
    print(r["stats"], "fitted", r["plane"], "planted", want, "error", err)
    assert r["stats"]["converged"] == 1 and r["stats"]["ground_pairs"] >= 1000
    G._check_lattice(r["stats"]["yaw_index"], r["T"], G.TILTED["yaw_deg"], G.TILTED["shift"], 72)
    assert all(e <= b for e, b in zip(err, G.PLANE_ERROR)), (err, G.PLANE_ERROR)
    back = G.plane_of(r["T"], *(t[r["stats"]["yaw_index"]] for t in G.yaw_table(72)))
    assert np.allclose(back, r["plane"], rtol=0, atol=1e-6)

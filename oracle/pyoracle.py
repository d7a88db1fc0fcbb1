"""ctypes binding of the CPU oracle (liboracle_mm3d.so).  TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module
(see oracle/mm3d_oracle.h).  The product package never does.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")])
NORMAL = np.dtype([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("curvature", "<f4")])
CORR = np.dtype([("index_query", "<i4"), ("index_match", "<i4"), ("distance", "<f4")])
ESTIMATE = np.dtype([("source_idx", "<u8"), ("target_idx", "<u8"), ("transform", "<f4", (16,)),
                     ("confidence", "<f8")])


class Params(C.Structure):
    _fields_ = [("resolution", C.c_double), ("descriptor_radius", C.c_double),
                ("outliers_min_neighbours", C.c_int), ("normal_radius", C.c_double),
                ("keypoint_type", C.c_int), ("keypoint_threshold", C.c_double),
                ("descriptor_type", C.c_int), ("estimation_method", C.c_int),
                ("refine_transform", C.c_int), ("inlier_threshold", C.c_double),
                ("max_correspondence_distance", C.c_double), ("max_iterations", C.c_int),
                ("matching_k", C.c_uint64), ("transform_epsilon", C.c_double),
                ("confidence_threshold", C.c_double), ("output_resolution", C.c_double)]


def build(force: bool = False) -> str:
    so = os.path.join(_HERE, "liboracle_mm3d.so")
    if force or not os.path.exists(so):
        subprocess.check_call(["make", "-C", _HERE, "-s"])
    return so


def lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        L = _LIB
        L.mo_transform_score.restype = C.c_double
        L.mo_mt19937_next.restype = C.c_uint32
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _pts(a):
    a = np.ascontiguousarray(a, dtype=POINT)
    return a


def params_default() -> Params:
    p = Params()
    lib().mo_params_default(C.byref(p))
    return p


def downsample(pts, resolution):
    pts = _pts(pts)
    out = np.empty(len(pts), dtype=POINT)
    n = lib().mo_downsample(_p(pts), len(pts), C.c_double(resolution), _p(out))
    return out[:n].copy()


def remove_outliers(pts, radius, min_neighbors):
    pts = _pts(pts)
    out = np.empty(len(pts), dtype=POINT)
    n = lib().mo_remove_outliers(_p(pts), len(pts), C.c_double(radius), int(min_neighbors), _p(out))
    return out[:n].copy()


def normals(pts, radius):
    pts = _pts(pts)
    out = np.empty(len(pts), dtype=NORMAL)
    lib().mo_normals(_p(pts), len(pts), C.c_double(radius), _p(out))
    return out


def keypoints_sift(pts, min_scale, nr_octaves=3, nr_scales=3, min_contrast=5.0):
    pts = _pts(pts)
    outp = C.c_void_p()
    outs = C.c_void_p()
    n = lib().mo_keypoints_sift(_p(pts), len(pts), C.c_double(min_scale), nr_octaves, nr_scales,
                                C.c_double(min_contrast), C.byref(outp), C.byref(outs))
    if n > 0:
        kp = np.frombuffer((C.c_char * (16 * n)).from_address(outp.value), dtype=POINT).copy()
        sc = np.frombuffer((C.c_char * (4 * n)).from_address(outs.value), dtype=np.float32).copy()
    else:
        kp = np.empty(0, dtype=POINT)
        sc = np.empty(0, dtype=np.float32)
    lib().mo_free(outp)
    lib().mo_free(outs)
    return kp, sc


def sift_octave_debug(pts, min_scale, octave, nr_scales=3):
    """One octave's scale space laid open (mo_sift_octave_debug): (cloud, dog[n,5] f32, resp[n,6] f64, cnt[n,6], knn[n,25]),
    or None when the octave does not exist."""
    pts = _pts(pts)
    pc, pd, pr, pn, pk = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    n = C.c_int(0)
    rc = lib().mo_sift_octave_debug(_p(pts), len(pts), C.c_double(min_scale), int(octave), int(nr_scales), C.byref(pc), C.byref(n),
                                    C.byref(pd), C.byref(pr), C.byref(pn), C.byref(pk))
    if rc != 0:
        return None
    n = n.value
    ns = nr_scales + 3
    cloud = np.frombuffer((C.c_char * (16 * n)).from_address(pc.value), dtype=POINT).copy()
    dog = np.frombuffer((C.c_char * (4 * n * (ns - 1))).from_address(pd.value), dtype=np.float32).reshape(n, ns - 1).copy()
    resp = np.frombuffer((C.c_char * (8 * n * ns)).from_address(pr.value), dtype=np.float64).reshape(n, ns).copy()
    cnt = np.frombuffer((C.c_char * (4 * n * ns)).from_address(pn.value), dtype=np.int32).reshape(n, ns).copy()
    knn = np.frombuffer((C.c_char * (4 * n * 25)).from_address(pk.value), dtype=np.int32).reshape(n, 25).copy()
    for p in (pc, pd, pr, pn, pk):
        lib().mo_free(p)
    return cloud, dog, resp, cnt, knn


def keypoints_harris(pts, nrm, threshold, radius):
    """detectKeypoints(HARRIS): (keypoints, source indices, response of every point)."""
    pts = _pts(pts)
    nrm = np.ascontiguousarray(nrm, dtype=NORMAL)
    outp, outi = C.c_void_p(), C.c_void_p()
    resp = np.empty(max(len(pts), 1), dtype=np.float32)
    n = lib().mo_keypoints_harris(_p(pts), _p(nrm), len(pts), C.c_double(threshold), C.c_double(radius),
                                  C.byref(outp), C.byref(outi), _p(resp))
    if n > 0:
        kp = np.frombuffer((C.c_char * (16 * n)).from_address(outp.value), dtype=POINT).copy()
        idx = np.frombuffer((C.c_char * (4 * n)).from_address(outi.value), dtype=np.int32).copy()
    else:
        kp, idx = np.empty(0, dtype=POINT), np.empty(0, dtype=np.int32)
    lib().mo_free(outp)
    lib().mo_free(outi)
    return kp, idx, resp[:len(pts)].copy()


def fpfh_raw(surface, nrm, keypoints, radius):
    surface = _pts(surface)
    nrm = np.ascontiguousarray(nrm, dtype=NORMAL)
    keypoints = _pts(keypoints)
    desc = np.empty((len(keypoints), 33), dtype=np.float32)
    support = np.empty(len(surface), dtype=np.int32)
    spfh = np.empty((len(surface), 33), dtype=np.float32)
    ns = lib().mo_fpfh_raw(_p(surface), _p(nrm), len(surface), _p(keypoints), len(keypoints),
                           C.c_double(radius), _p(desc), _p(support), _p(spfh))
    return desc, support[:ns].copy(), spfh[:ns].copy()


def pair_features(p1, n1, p2, n2):
    """pcl::computePairFeatures on n pairs (test hook): rows {f1, f2, f3, f4, branch} with branch = 1 when the call switched
    p1 and p2, 0 when not, 2 on the coincident-points exit."""
    p1, p2 = _pts(p1), _pts(p2)
    n1 = np.ascontiguousarray(n1, dtype=NORMAL)
    n2 = np.ascontiguousarray(n2, dtype=NORMAL)
    out = np.empty((len(p1), 5), dtype=np.float32)
    lib().mo_pair_features(_p(p1), _p(n1), _p(p2), _p(n2), len(p1), _p(out))
    return out


def spfh_pair_bins(p1, n1, p2, n2):
    """The three SPFH bins computePointSPFHSignature gives each pair (test hook): rows {f1 bin, f2 bin, f3 bin}."""
    p1, p2 = _pts(p1), _pts(p2)
    n1 = np.ascontiguousarray(n1, dtype=NORMAL)
    n2 = np.ascontiguousarray(n2, dtype=NORMAL)
    out = np.empty((len(p1), 3), dtype=np.int32)
    lib().mo_spfh_pair_bins(_p(p1), _p(n1), _p(p2), _p(n2), len(p1), _p(out))
    return out


def descriptors_pfh(surface, nrm, keypoints, radius):
    """computeLocalDescriptors(PFH): returns (pruned keypoints, desc[n, 125])."""
    surface = _pts(surface)
    nrm = np.ascontiguousarray(nrm, dtype=NORMAL)
    kp = _pts(keypoints).copy()
    desc = np.empty((max(len(kp), 1), 125), dtype=np.float32)
    n = lib().mo_descriptors_pfh(_p(surface), _p(nrm), len(surface), _p(kp), len(kp), C.c_double(radius), _p(desc))
    return kp[:n].copy(), desc[:n].copy()


def pfh_raw(surface, nrm, keypoints, radius):
    """Un-pruned PFH rows (NaN where a keypoint has no neighbour)."""
    surface = _pts(surface)
    nrm = np.ascontiguousarray(nrm, dtype=NORMAL)
    keypoints = _pts(keypoints)
    desc = np.empty((max(len(keypoints), 1), 125), dtype=np.float32)
    lib().mo_pfh_raw(_p(surface), _p(nrm), len(surface), _p(keypoints), len(keypoints), C.c_double(radius), _p(desc))
    return desc[:len(keypoints)].copy()


def sc3d_tables(radius):
    """ShapeContext3DEstimation::initCompute: (radii[16], theta_div[12], phi_div[13], volume_lut[1980])."""
    r, t, ph, lut = (np.empty(n, dtype=np.float32) for n in (16, 12, 13, 1980))
    lib().mo_sc3d_tables(C.c_double(radius), _p(r), _p(t), _p(ph), _p(lut))
    return r, t, ph, lut


def descriptors_sc3d(surface, nrm, keypoints, radius):
    """computeLocalDescriptors(SC3D): returns (pruned keypoints, desc[n, 1980])."""
    surface = _pts(surface)
    nrm = np.ascontiguousarray(nrm, dtype=NORMAL)
    kp = _pts(keypoints).copy()
    desc = np.empty((max(len(kp), 1), 1980), dtype=np.float32)
    n = lib().mo_descriptors_sc3d(_p(surface), _p(nrm), len(surface), _p(kp), len(kp), C.c_double(radius), _p(desc))
    return kp[:n].copy(), desc[:n].copy()


def descriptors_rsd(surface, nrm, keypoints, radius):
    """computeLocalDescriptors(RSD): returns (pruned keypoints, desc[n, 2] = r_min, r_max)."""
    surface = _pts(surface)
    nrm = np.ascontiguousarray(nrm, dtype=NORMAL)
    kp = _pts(keypoints).copy()
    desc = np.empty((max(len(kp), 1), 2), dtype=np.float32)
    n = lib().mo_descriptors_rsd(_p(surface), _p(nrm), len(surface), _p(kp), len(kp), C.c_double(radius), _p(desc))
    return kp[:n].copy(), desc[:n].copy()


def descriptors_pfhrgb(surface, nrm, keypoints, radius):
    """computeLocalDescriptors(PFHRGB): returns (pruned keypoints, desc[n, 250])."""
    surface = _pts(surface)
    nrm = np.ascontiguousarray(nrm, dtype=NORMAL)
    kp = _pts(keypoints).copy()
    desc = np.empty((max(len(kp), 1), 250), dtype=np.float32)
    n = lib().mo_descriptors_pfhrgb(_p(surface), _p(nrm), len(surface), _p(kp), len(kp), C.c_double(radius), _p(desc))
    return kp[:n].copy(), desc[:n].copy()


def descriptors_shot(surface, nrm, keypoints, radius):
    """computeLocalDescriptors(SHOT) = SHOTColorEstimation/SHOT1344: (pruned keypoints, desc[n, 1344])."""
    surface = _pts(surface)
    nrm = np.ascontiguousarray(nrm, dtype=NORMAL)
    kp = _pts(keypoints).copy()
    desc = np.empty((max(len(kp), 1), 1344), dtype=np.float32)
    n = lib().mo_descriptors_shot(_p(surface), _p(nrm), len(surface), _p(kp), len(kp), C.c_double(radius), _p(desc))
    return kp[:n].copy(), desc[:n].copy()


def shot_raw(surface, nrm, keypoints, radius):
    """Un-pruned SHOT1344 rows (NaN where PCL gives up) and the local reference frames [n, 9]."""
    surface = _pts(surface)
    nrm = np.ascontiguousarray(nrm, dtype=NORMAL)
    keypoints = _pts(keypoints)
    desc = np.empty((max(len(keypoints), 1), 1344), dtype=np.float32)
    rf = np.empty((max(len(keypoints), 1), 9), dtype=np.float32)
    lib().mo_shot_raw(_p(surface), _p(nrm), len(surface), _p(keypoints), len(keypoints), C.c_double(radius),
                      _p(desc), _p(rf))
    return desc[:len(keypoints)].copy(), rf[:len(keypoints)].copy()


def shot_rgb2lab(r, g, b):
    out = (C.c_float * 3)()
    lib().mo_shot_rgb2lab(C.c_ubyte(r), C.c_ubyte(g), C.c_ubyte(b), out)
    return np.array(out[:], dtype=np.float32)


def descriptors_fpfh(surface, nrm, keypoints, radius):
    """Returns (pruned keypoints, descriptors) like computeLocalDescriptors (which mutates keypoints)."""
    surface = _pts(surface)
    nrm = np.ascontiguousarray(nrm, dtype=NORMAL)
    kp = _pts(keypoints).copy()
    desc = np.empty((max(len(kp), 1), 33), dtype=np.float32)
    n = lib().mo_descriptors_fpfh(_p(surface), _p(nrm), len(surface), _p(kp), len(kp),
                                  C.c_double(radius), _p(desc))
    return kp[:n].copy(), desc[:n].copy()


def desc_knn(a, b, k):
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    idx = np.empty((len(a), k), dtype=np.int32)
    d2 = np.empty((len(a), k), dtype=np.float32)
    lib().mo_desc_knn(_p(a), len(a), _p(b), len(b), a.shape[1], k, _p(idx), _p(d2))
    return idx, d2


def find_correspondences(ds, dt, k=5):
    ds = np.ascontiguousarray(ds, dtype=np.float32)
    dt = np.ascontiguousarray(dt, dtype=np.float32)
    out = np.empty(max(len(ds), 1), dtype=CORR)
    n = lib().mo_find_correspondences(_p(ds), len(ds), _p(dt), len(dt), ds.shape[1] if ds.ndim == 2 else 33,
                                      C.c_size_t(k), _p(out))
    return out[:n].copy()


def ransac(src_kp, tgt_kp, corr, inlier_threshold):
    src_kp, tgt_kp = _pts(src_kp), _pts(tgt_kp)
    corr = np.ascontiguousarray(corr, dtype=CORR)
    T = np.zeros(16, dtype=np.float32)
    inl = np.empty(max(len(corr), 1), dtype=CORR)
    iters, best = C.c_int(), C.c_int()
    n = lib().mo_ransac(_p(src_kp), len(src_kp), _p(tgt_kp), len(tgt_kp), _p(corr), len(corr),
                        C.c_double(inlier_threshold), _p(T), _p(inl), C.byref(iters), C.byref(best))
    return T.reshape(4, 4).T.copy(), inl[:n].copy(), iters.value, best.value


def srand(seed):
    lib().mo_srand(C.c_uint(seed))


def set_threads(n):
    """Baseline B2: OpenMP threads for the loops over points / keypoints (results do not depend on it)."""
    lib().mo_set_threads(int(n))


def get_threads():
    return int(lib().mo_get_threads())


def rand():
    return lib().mo_rand()


def sac_ia(src_kp, src_desc, tgt_kp, tgt_desc, min_sample_distance, max_corr_dist, max_iterations):
    src_kp, tgt_kp = _pts(src_kp), _pts(tgt_kp)
    sd = np.ascontiguousarray(src_desc, dtype=np.float32)
    td = np.ascontiguousarray(tgt_desc, dtype=np.float32)
    T = np.zeros(16, dtype=np.float32)
    bi, be = C.c_int(), C.c_float()
    lib().mo_sac_ia(_p(src_kp), _p(sd), len(src_kp), _p(tgt_kp), _p(td), len(tgt_kp), sd.shape[1],
                    C.c_double(min_sample_distance), C.c_double(max_corr_dist), int(max_iterations),
                    _p(T), C.byref(bi), C.byref(be))
    return T.reshape(4, 4).T.copy(), bi.value, be.value


def sac_ia_errors(src_kp, src_desc, tgt_kp, tgt_desc, min_sample_distance, max_corr_dist, max_iterations):
    """sac_ia + every hypothesis' error sum: the CPU path's float chain and the same terms summed in double (study hook)."""
    ef = np.zeros(int(max_iterations), dtype=np.float32)
    ed = np.zeros(int(max_iterations), dtype=np.float64)
    lib().mo_sac_ia_error_sink(_p(ef), _p(ed), int(max_iterations))
    try:
        T, bi, be = sac_ia(src_kp, src_desc, tgt_kp, tgt_desc, min_sample_distance, max_corr_dist, max_iterations)
    finally:
        lib().mo_sac_ia_error_sink(None, None, 0)
    return T, bi, be, ef, ed


def icp(src, tgt, guess, max_corr_dist, outlier_thr, max_iterations, eps):
    src, tgt = _pts(src), _pts(tgt)
    g = np.ascontiguousarray(np.asarray(guess, dtype=np.float32).T.reshape(16))
    T = np.zeros(16, dtype=np.float32)
    it = C.c_int()
    lib().mo_icp(_p(src), len(src), _p(tgt), len(tgt), _p(g), C.c_double(max_corr_dist),
                 C.c_double(outlier_thr), int(max_iterations), C.c_double(eps), _p(T), C.byref(it))
    return T.reshape(4, 4).T.copy(), it.value


def icp_double_sums(src, tgt, guess, max_corr_dist, max_iterations, eps):
    """ICP with double sums over the original points: exact-arithmetic yardstick, not the reference's arithmetic."""
    src, tgt = _pts(src), _pts(tgt)
    g = np.ascontiguousarray(np.asarray(guess, dtype=np.float32).T.reshape(16))
    T = np.zeros(16, dtype=np.float32)
    it = C.c_int()
    lib().mo_icp_double_sums(_p(src), len(src), _p(tgt), len(tgt), _p(g), C.c_double(max_corr_dist), int(max_iterations),
                             C.c_double(eps), _p(T), C.byref(it))
    return T.reshape(4, 4).T.copy(), it.value


def transform_score(src, tgt, T, max_distance):
    src, tgt = _pts(src), _pts(tgt)
    t = np.ascontiguousarray(np.asarray(T, dtype=np.float32).T.reshape(16))
    return lib().mo_transform_score(_p(src), len(src), _p(tgt), len(tgt), _p(t), C.c_double(max_distance))


def umeyama_f32(src, dst):
    src = np.ascontiguousarray(src, dtype=np.float32)
    dst = np.ascontiguousarray(dst, dtype=np.float32)
    T = np.zeros(16, dtype=np.float32)
    lib().mo_umeyama_f32(_p(src), _p(dst), len(src), _p(T))
    return T.reshape(4, 4).T.copy()


def mat4_inverse(A):
    a = np.ascontiguousarray(np.asarray(A, dtype=np.float32).T.reshape(16))
    o = np.zeros(16, dtype=np.float32)
    lib().mo_mat4_inverse(_p(a), _p(o))
    return o.reshape(4, 4).T.copy()


def make_estimates(pairs):
    """pairs: iterable of (src, tgt, T 4x4 row/col numpy, confidence)."""
    est = np.zeros(len(pairs), dtype=ESTIMATE)
    for i, (s, t, T, c) in enumerate(pairs):
        est[i]["source_idx"], est[i]["target_idx"], est[i]["confidence"] = s, t, c
        est[i]["transform"] = np.asarray(T, dtype=np.float32).T.reshape(16)
    return est


def global_transforms(est, confidence_threshold, cap_nodes=None):
    est = np.ascontiguousarray(est, dtype=ESTIMATE)
    cap = cap_nodes or (int(max(est["source_idx"].max(initial=0), est["target_idx"].max(initial=0))) + 1
                        if len(est) else 1)
    out = np.zeros((cap, 16), dtype=np.float32)
    n = lib().mo_global_transforms(_p(est), len(est), C.c_double(confidence_threshold), _p(out), cap)
    return [out[i].reshape(4, 4).T.copy() for i in range(max(n, 0))]


def largest_component(est, thr):
    est = np.ascontiguousarray(est, dtype=ESTIMATE)
    kept = np.zeros(max(len(est), 1), dtype=np.int32)
    lib().mo_largest_component(_p(est), len(est), C.c_double(thr), _p(kept))
    return kept[:len(est)].astype(bool)


def spanning_tree_centers(est):
    est = np.ascontiguousarray(est, dtype=ESTIMATE)
    c = (C.c_size_t * 2)()
    n = lib().mo_max_spanning_tree_centers(_p(est), len(est), c)
    return [int(c[i]) for i in range(min(n, 2))], n


def estimate_maps_transforms(clouds, params: Params):
    clouds = [_pts(c) for c in clouds]
    n = len(clouds)
    ptrs = (C.c_void_p * max(n, 1))(*[c.ctypes.data for c in clouds])
    sizes = (C.c_int * max(n, 1))(*[len(c) for c in clouds])
    out = np.zeros((max(n, 1), 16), dtype=np.float32)
    pairs = np.zeros(max(n * (n - 1) // 2, 1), dtype=ESTIMATE)
    npairs = C.c_int()
    m = lib().mo_estimate_maps_transforms(ptrs, sizes, n, C.byref(params), _p(out), _p(pairs), C.byref(npairs))
    if m < 0:
        raise RuntimeError(f"oracle estimate_maps_transforms failed: {m}")
    return [out[i].reshape(4, 4).T.copy() for i in range(m)], pairs[:npairs.value].copy()


def libm_eval(fn, x, y=None):
    """The host libm's expf (0), atanf (1), sinf (2), cosf (3) of x or atan2f(y, x) (4), element by element; fn 5: the pair
    features' switch acos(fabs(x)) > acos(fabs(y)) in double, as 1.0 / 0.0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y if y is not None else x, dtype=np.float32)
    out = np.empty_like(x)
    lib().mo_libm_eval(int(fn), _p(x), _p(y), len(x), _p(out))
    return out


TRACE = np.dtype([("n_correspondences", "<i4"), ("n_inliers", "<i4"), ("icp_iterations", "<i4"), ("icp_correspondences", "<i4")])


def last_run_traces():
    """Per-pair integer observables of the most recent estimate_maps_transforms (cross-match / inlier counts of
    R/src/registration_visualisation.cpp:129-130, ICP iterations and last-iteration correspondences), in pair order."""
    n = lib().mo_last_run_traces(None, 0)
    out = np.zeros(max(n, 1), dtype=TRACE)
    lib().mo_last_run_traces(_p(out), n)
    return out[:n].copy()


# ---- THE stated ICP / pair-transform tolerance (BASELINE.md "Reported metrics") -----------------
# Both clauses must hold for a pair; tests/ and bench.py's parity_check assert exactly these.
#   exact:  || T_dev - T_exact ||_F <= TOL_T_EXACT with equal ICP iteration counts, T_exact = the same ICP from the same
#           initial estimate with its sums in double (icp_double_sums: what exact arithmetic gives);
#   oracle: || T_dev - T_oracle ||_F <= transform_tolerance(n_src) with equal ICP iteration counts.  T_oracle's float
#           sums carry the CPU path's own summation noise, which grows with the number of summed points (measured
#           || T_oracle - T_exact ||_F / n_src <= 5.4e-9 over every BASELINE configuration): 1e-3 up to 1e5 points,
#           1e-8 per point beyond -- and, since the pair's OWN noise is measured (both yardsticks run), never more than
#           that noise plus TOL_T_EXACT: a device regression of a few 1e-3 on a large cloud whose CPU noise is 1e-3
#           fails, where the blanket per-point bound of 1e-2 would have let it through.
TOL_T_EXACT = 1e-4


def transform_tolerance(n_src, cpu_noise=None):
    """Bound of the oracle clause.  cpu_noise = || T_oracle - T_exact ||_F of the SAME pair (None where the yardstick was
    not run): the bound is then the smaller of the blanket per-point figure and noise + TOL_T_EXACT."""
    blanket = 1e-3 * max(1.0, float(n_src) / 1e5)
    if cpu_noise is None:
        return blanket
    return min(blanket, float(cpu_noise) + TOL_T_EXACT)


def set_exact_yardstick(on):
    """estimate_maps_transforms also runs the double-sum ICP from every pair's initial estimate (test yardstick)."""
    lib().mo_set_exact_yardstick(int(bool(on)))


def last_run_exact():
    """(T[n][4][4] column-major records as stored, iterations[n], last-iteration correspondences[n]) of the yardstick."""
    n = lib().mo_last_run_exact(None, None, None, 0)
    T = np.zeros((max(n, 1), 16), dtype=np.float32)
    it = np.zeros(max(n, 1), dtype=np.int32)
    corr = np.zeros(max(n, 1), dtype=np.int32)
    lib().mo_last_run_exact(_p(T), _p(it), _p(corr), n)
    return T[:n].copy(), it[:n].copy(), corr[:n].copy()


def last_pair_trace():
    out = np.zeros(1, dtype=TRACE)
    lib().mo_last_pair_trace(_p(out))
    return out[0]


def compose_maps(clouds, transforms, resolution):
    clouds = [_pts(c) for c in clouds]
    n = len(clouds)
    ptrs = (C.c_void_p * max(n, 1))(*[c.ctypes.data for c in clouds])
    sizes = (C.c_int * max(n, 1))(*[len(c) for c in clouds])
    tr = np.ascontiguousarray(np.stack([np.asarray(T, dtype=np.float32).T.reshape(16) for T in transforms])
                              if len(transforms) else np.zeros((0, 16), np.float32))
    outp = C.c_void_p()
    m = lib().mo_compose_maps(ptrs, sizes, n, _p(tr) if len(tr) else None, len(transforms),
                              C.c_double(resolution), C.byref(outp))
    if m == -1:
        return None
    if m == -2:
        raise RuntimeError("composeMaps: clouds and transforms size must be the same.")
    res = np.frombuffer((C.c_char * (16 * m)).from_address(outp.value), dtype=POINT).copy() if m > 0 \
        else np.empty(0, dtype=POINT)
    lib().mo_free(outp)
    return res

"""map_merge_3d on MI355X: Python host mirror of the reference's C++ API over libmm3d.so.

The product is the C-ABI library (include/mm3d.h).  This module is the thin host side used by the
tests and bench.py; it mirrors the names and argument meaning of the reference's free functions
(R/include/map_merge_3d/features.h:34-98, matching.h:26-152, map_merging.h:28-101) so the parity
tests read like the reference's own harnesses.  There is NO CPU fallback: if libmm3d.so is missing
or no GPU is visible, calls raise.

The directory is named `map-merge_amd`; import it as `map_merge_amd` through `load()` in
__graft_entry__.py / tests/conftest.py (a hyphen is not importable).
"""
from __future__ import annotations

import ctypes as C
import enum
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MM3D_LIB: an instrumentation build of the same library (scripts/nn_stats.py, scripts/sn_stats.py)
LIB_PATH = os.environ.get("MM3D_LIB") or os.path.join(_HERE, "libmm3d.so")

POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")])
NORMAL = np.dtype([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("curvature", "<f4")])
CORR = np.dtype([("index_query", "<i4"), ("index_match", "<i4"), ("distance", "<f4")])
PAIR = np.dtype([("source_idx", "<u8"), ("target_idx", "<u8"), ("transform", "<f4", (16,)),
                 ("confidence", "<f8"), ("icp_iterations", "<i4"), ("n_correspondences", "<i4"),
                 ("n_inliers", "<i4"), ("icp_correspondences", "<i4")])


class Mm3dError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"mm3d status {status}: {msg}")
        self.status = status


class Descriptor(enum.IntEnum):      # features.h:20-24
    PFH = 0
    PFHRGB = 1
    FPFH = 2
    RSD = 3
    SHOT = 4
    SC3D = 5


class Keypoint(enum.IntEnum):        # features.h:49
    SIFT = 0
    HARRIS = 1


class EstimationMethod(enum.IntEnum):  # matching.h:103
    MATCHING = 0
    SAC_IA = 1


class IcpMethod(enum.IntEnum):      # mm3d_icp_method (not a reference enum)
    POINT_TO_POINT = 0
    POINT_TO_PLANE = 1


class AlignMethod(enum.IntEnum):    # mm3d_align_method (not a reference enum)
    SAC_IA = 0
    PREREJECTIVE = 1


class AlignmentOptions(C.Structure):
    """mm3d_alignment_options (mm3d_set_alignment); the defaults are mm3d_alignment_options_default's."""
    _fields_ = [("method", C.c_int), ("samples", C.c_int), ("k", C.c_int), ("similarity", C.c_double),
                ("inlier_fraction", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().mm3d_alignment_options_default(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("unknown alignment option " + k)
            setattr(self, k, int(v) if k in ("method", "samples", "k") else float(v))


class KeypointSource(enum.IntEnum):  # mm3d_keypoint_source (not a reference enum)
    REFERENCE = 0
    UNIFORM = 1


class KeypointOptions(C.Structure):
    """mm3d_keypoint_options (mm3d_set_keypoints); the defaults are mm3d_keypoint_options_default's."""
    _fields_ = [("source", C.c_int), ("leaf", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().mm3d_keypoint_options_default(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("unknown keypoint option " + k)
            setattr(self, k, int(v) if k == "source" else float(v))


class OutlierMethod(enum.IntEnum):  # mm3d_outlier_method (not a reference enum)
    RADIUS = 0
    STATISTICAL = 1


class OutlierOptions(C.Structure):
    """mm3d_outlier_options (mm3d_set_outlier_filter); the defaults are mm3d_outlier_options_default's."""
    _fields_ = [("method", C.c_int), ("mean_k", C.c_int), ("stddev_mult", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().mm3d_outlier_options_default(C.byref(self))
        kinds = dict(self._fields_)
        for k, v in kw.items():
            if k not in kinds:
                raise TypeError("unknown outlier option " + k)
            setattr(self, k, int(v) if kinds[k] is C.c_int else float(v))

    def as_tuple(self):
        return (int(self.method), int(self.mean_k), float(self.stddev_mult))


class OutlierStats(C.Structure):
    """mm3d_outlier_stats"""
    _fields_ = [("points", C.c_longlong), ("valid", C.c_longlong), ("kept", C.c_longlong), ("k", C.c_int), ("mean", C.c_double),
                ("stddev", C.c_double), ("threshold", C.c_double)]

    def as_dict(self):
        return {k: (float if t is C.c_double else int)(getattr(self, k)) for k, t in self._fields_}


class ClusterMethod(enum.IntEnum):  # mm3d_cluster_method (not a reference enum)
    OFF = 0
    MIN_SIZE = 1
    LARGEST = 2


class ClusterOptions(C.Structure):
    """mm3d_cluster_options (mm3d_set_cluster_filter); the defaults are mm3d_cluster_options_default's."""
    _fields_ = [("method", C.c_int), ("min_size", C.c_int), ("tolerance", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().mm3d_cluster_options_default(C.byref(self))
        kinds = dict(self._fields_)
        for k, v in kw.items():
            if k not in kinds:
                raise TypeError("unknown cluster option " + k)
            setattr(self, k, int(v) if kinds[k] is C.c_int else float(v))

    def as_tuple(self):
        return (int(self.method), int(self.min_size), float(self.tolerance))


class ClusterStats(C.Structure):
    """mm3d_cluster_stats"""
    _fields_ = [("points", C.c_longlong), ("valid", C.c_longlong), ("kept", C.c_longlong), ("clusters", C.c_longlong),
                ("kept_clusters", C.c_longlong), ("largest", C.c_longlong)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class PlaneMethod(enum.IntEnum):    # mm3d_plane_method (not a reference enum)
    OFF = 0
    REMOVE = 1
    SET_ASIDE = 2


PLANE_NONE, PLANE_INVALID = -1, -2      # MM3D_PLANE_NONE, MM3D_PLANE_INVALID: labels that name no plane


class PlaneOptions(C.Structure):
    """mm3d_plane_options (mm3d_set_planes); the defaults are mm3d_plane_options_default's."""
    _fields_ = [("method", C.c_int), ("max_planes", C.c_int), ("samples", C.c_int), ("refit", C.c_int), ("seed", C.c_uint),
                ("distance", C.c_double), ("min_fraction", C.c_double), ("axis", C.c_double * 3), ("max_angle_deg", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().mm3d_plane_options_default(C.byref(self))
        kinds = dict(self._fields_)
        for k, v in kw.items():
            if k not in kinds:
                raise TypeError("unknown plane option " + k)
            if k == "axis":
                self.axis = (C.c_double * 3)(*[float(x) for x in v])
            else:
                setattr(self, k, float(v) if kinds[k] is C.c_double else int(v))

    def as_tuple(self):
        return (int(self.method), int(self.max_planes), int(self.samples), int(self.refit), int(self.seed), float(self.distance),
                float(self.min_fraction), tuple(float(x) for x in self.axis), float(self.max_angle_deg))


class Plane(C.Structure):
    """mm3d_plane: normal . x + d = 0, the inliers, the winning draw, whether the refit was adopted"""
    _fields_ = [("normal", C.c_double * 3), ("d", C.c_double), ("inliers", C.c_longlong), ("draw", C.c_int), ("refit", C.c_int)]

    def as_dict(self):
        return dict(normal=tuple(float(x) for x in self.normal), d=float(self.d), inliers=int(self.inliers), draw=int(self.draw), refit=int(self.refit))


class PlaneStats(C.Structure):
    """mm3d_plane_stats"""
    _fields_ = [("points", C.c_longlong), ("valid", C.c_longlong), ("on_planes", C.c_longlong), ("kept", C.c_longlong),
                ("draws", C.c_longlong), ("degenerate", C.c_longlong), ("off_axis", C.c_longlong), ("planes", C.c_int), ("rounds", C.c_int)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class SmoothMethod(enum.IntEnum):   # mm3d_smooth_method (not a reference enum)
    OFF = 0
    MLS = 1


class SmoothWhere(enum.IntFlag):    # the bits of mm3d_smooth_options.where
    MAPS = 1
    COMPOSED = 2


class SmoothState(enum.IntEnum):    # MM3D_SMOOTH_INVALID .. MM3D_SMOOTH_POLYNOMIAL: a record's state under the rule
    INVALID = 0
    FEW = 1
    DEGENERATE = 2
    PLANE = 3
    POLYNOMIAL = 4


class SmoothOptions(C.Structure):
    """mm3d_smooth_options (mm3d_set_smoothing); the defaults are mm3d_smooth_options_default's."""
    _fields_ = [("method", C.c_int), ("order", C.c_int), ("min_neighbours", C.c_int), ("where", C.c_int), ("radius", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().mm3d_smooth_options_default(C.byref(self))
        kinds = dict(self._fields_)
        for k, v in kw.items():
            if k not in kinds:
                raise TypeError("unknown smoothing option " + k)
            setattr(self, k, int(v) if kinds[k] is C.c_int else float(v))

    def as_tuple(self):
        return (int(self.method), int(self.order), int(self.min_neighbours), int(self.where), float(self.radius))


class SmoothStats(C.Structure):
    """mm3d_smooth_stats"""
    _fields_ = [("points", C.c_longlong), ("valid", C.c_longlong), ("few", C.c_longlong), ("degenerate", C.c_longlong),
                ("plane", C.c_longlong), ("polynomial", C.c_longlong), ("max_displacement", C.c_double)]

    def as_dict(self):
        return {k: (float if t is C.c_double else int)(getattr(self, k)) for k, t in self._fields_}


class RefineMethod(enum.IntEnum):   # mm3d_refine_method (not a reference enum)
    ICP = 0
    NDT = 1


class RefineOptions(C.Structure):
    """mm3d_refine_options (mm3d_set_refinement); the defaults are mm3d_refine_options_default's."""
    _fields_ = [("method", C.c_int), ("resolution", C.c_double), ("neighbours", C.c_int), ("min_points", C.c_int),
                ("regularisation", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().mm3d_refine_options_default(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("unknown refinement option " + k)
            setattr(self, k, int(v) if k in ("method", "neighbours", "min_points") else float(v))

    def as_tuple(self):
        return (int(self.method), float(self.resolution), int(self.neighbours), int(self.min_points), float(self.regularisation))


class CoarseMethod(enum.IntEnum):   # mm3d_coarse_method (not a reference enum)
    NONE = 0
    CORRELATIVE = 1


class CoarseOptions(C.Structure):
    """mm3d_coarse_options (mm3d_set_coarse_alignment); the defaults are mm3d_coarse_options_default's."""
    _fields_ = [("method", C.c_int), ("cell", C.c_double), ("cell_factor", C.c_int), ("yaw_steps", C.c_int), ("yaw_factor", C.c_int),
                ("candidates", C.c_int), ("wall_nz", C.c_double), ("ground_nz", C.c_double), ("min_points", C.c_int),
                ("accept_fraction", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().mm3d_coarse_options_default(C.byref(self))
        kinds = dict(self._fields_)
        for k, v in kw.items():
            if k not in kinds:
                raise TypeError("unknown coarse alignment option " + k)
            setattr(self, k, int(v) if kinds[k] is C.c_int else float(v))

    def as_tuple(self):
        return tuple(int(getattr(self, k)) if t is C.c_int else float(getattr(self, k)) for k, t in self._fields_)


class CoarseStats(C.Structure):
    """mm3d_coarse_stats"""
    _fields_ = [("source_cells", C.c_int), ("target_cells", C.c_int), ("coarse_votes", C.c_int), ("candidates", C.c_int),
                ("score", C.c_int), ("yaw_index", C.c_int), ("ground_pairs", C.c_int), ("converged", C.c_int)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class ConfidenceMethod(enum.IntEnum):   # mm3d_confidence_method (not a reference enum)
    REFERENCE = 0
    OVERLAP = 1


class ConfidenceOptions(C.Structure):
    """mm3d_confidence_options (mm3d_set_confidence); the defaults are mm3d_confidence_options_default's."""
    _fields_ = [("method", C.c_int), ("voxel", C.c_double), ("min_points", C.c_int), ("min_overlap", C.c_double),
                ("view_margin", C.c_int)]

    def __init__(self, **kw):
        super().__init__()
        lib().mm3d_confidence_options_default(C.byref(self))
        kinds = dict(self._fields_)
        for k, v in kw.items():
            if k not in kinds:
                raise TypeError("unknown confidence option " + k)
            setattr(self, k, int(v) if kinds[k] is C.c_int else float(v))

    def as_tuple(self):
        return tuple(int(getattr(self, k)) if t is C.c_int else float(getattr(self, k)) for k, t in self._fields_)


class RejectDistance(enum.IntEnum):   # mm3d_reject_distance (not a reference enum)
    NONE = 0
    TRIMMED = 1
    MEDIAN = 2


class IcpRejectionOptions(C.Structure):
    """mm3d_icp_rejection_options (mm3d_set_icp_rejection); the defaults are mm3d_icp_rejection_options_default's."""
    _fields_ = [("one_to_one", C.c_int), ("distance", C.c_int), ("overlap_ratio", C.c_double), ("min_correspondences", C.c_int),
                ("median_factor", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().mm3d_icp_rejection_options_default(C.byref(self))
        kinds = dict(self._fields_)
        for k, v in kw.items():
            if k not in kinds:
                raise TypeError("unknown ICP rejection option " + k)
            setattr(self, k, int(v) if kinds[k] is C.c_int else float(v))

    def as_tuple(self):
        return tuple(int(getattr(self, k)) if t is C.c_int else float(getattr(self, k)) for k, t in self._fields_)


class IcpGeometryOptions(C.Structure):
    """mm3d_icp_geometry_options (mm3d_set_icp_geometry_rejection); the defaults are mm3d_icp_geometry_options_default's."""
    _fields_ = [("boundary", C.c_int), ("boundary_radius", C.c_double), ("boundary_angle_deg", C.c_double),
                ("boundary_min_neighbours", C.c_int), ("normals", C.c_int), ("normal_angle_deg", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().mm3d_icp_geometry_options_default(C.byref(self))
        kinds = dict(self._fields_)
        for k, v in kw.items():
            if k not in kinds:
                raise TypeError("unknown ICP geometry option " + k)
            setattr(self, k, int(v) if kinds[k] is C.c_int else float(v))

    def as_tuple(self):
        return tuple(int(getattr(self, k)) if t is C.c_int else float(getattr(self, k)) for k, t in self._fields_)


class RobustKernel(enum.IntEnum):   # mm3d_robust_kernel (not a reference enum)
    OFF = 0
    L2 = 1
    HUBER = 2
    CAUCHY = 3
    TUKEY = 4
    GEMAN_MCCLURE = 5


class IcpRobustOptions(C.Structure):
    """mm3d_icp_robust_options (mm3d_set_icp_robust); the defaults are mm3d_icp_robust_options_default's."""
    _fields_ = [("kernel", C.c_int), ("scale", C.c_double), ("scale_start", C.c_double), ("anneal", C.c_double), ("tuning", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().mm3d_icp_robust_options_default(C.byref(self))
        kinds = dict(self._fields_)
        for k, v in kw.items():
            if k not in kinds:
                raise TypeError("unknown robust ICP option " + k)
            setattr(self, k, int(v) if kinds[k] is C.c_int else float(v))

    def as_tuple(self):
        return tuple(int(getattr(self, k)) if t is C.c_int else float(getattr(self, k)) for k, t in self._fields_)


class IcpColorOptions(C.Structure):
    """mm3d_icp_color_options (mm3d_set_icp_color); the defaults are mm3d_icp_color_options_default's."""
    _fields_ = [("enabled", C.c_int), ("lambda_geometric", C.c_double), ("gradient_radius", C.c_double), ("min_neighbours", C.c_int)]

    def __init__(self, **kw):
        super().__init__()
        lib().mm3d_icp_color_options_default(C.byref(self))
        kinds = dict(self._fields_)
        for k, v in kw.items():
            if k not in kinds:
                raise TypeError("unknown coloured ICP option " + k)
            setattr(self, k, int(v) if kinds[k] is C.c_int else float(v))

    def as_tuple(self):
        return tuple(int(getattr(self, k)) if t is C.c_int else float(getattr(self, k)) for k, t in self._fields_)


class IcpGeneralizedOptions(C.Structure):
    """mm3d_icp_generalized_options (mm3d_set_icp_generalized); the defaults are mm3d_icp_generalized_options_default's."""
    _fields_ = [("enabled", C.c_int), ("epsilon", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().mm3d_icp_generalized_options_default(C.byref(self))
        kinds = dict(self._fields_)
        for k, v in kw.items():
            if k not in kinds:
                raise TypeError("unknown generalized ICP option " + k)
            setattr(self, k, int(v) if kinds[k] is C.c_int else float(v))

    def as_tuple(self):
        return tuple(int(getattr(self, k)) if t is C.c_int else float(getattr(self, k)) for k, t in self._fields_)


class EstimatorMethod(enum.IntEnum):   # mm3d_estimator_method (not a reference enum)
    RANSAC = 0
    CONSISTENCY = 1


class EstimatorOptions(C.Structure):
    """mm3d_estimator_options (mm3d_set_estimator); the defaults are mm3d_estimator_options_default's."""
    _fields_ = [("method", C.c_int), ("tolerance", C.c_double), ("seeds", C.c_int), ("consensus", C.c_int)]

    def __init__(self, **kw):
        super().__init__()
        lib().mm3d_estimator_options_default(C.byref(self))
        kinds = dict(self._fields_)
        for k, v in kw.items():
            if k not in kinds:
                raise TypeError("unknown estimator option " + k)
            setattr(self, k, int(v) if kinds[k] is C.c_int else float(v))

    def as_tuple(self):
        return tuple(int(getattr(self, k)) if t is C.c_int else float(getattr(self, k)) for k, t in self._fields_)


class IcpSampleMethod(enum.IntEnum):   # mm3d_icp_sample_method (not a reference enum)
    NONE = 0
    STRIDE = 1
    NORMAL_SPACE = 2


class IcpSamplingOptions(C.Structure):
    """mm3d_icp_sampling_options (mm3d_set_icp_sampling); the defaults are mm3d_icp_sampling_options_default's."""
    _fields_ = [("method", C.c_int), ("fraction", C.c_double), ("max_points", C.c_int), ("bins", C.c_int)]

    def __init__(self, **kw):
        super().__init__()
        lib().mm3d_icp_sampling_options_default(C.byref(self))
        kinds = dict(self._fields_)
        for k, v in kw.items():
            if k not in kinds:
                raise TypeError("unknown ICP sampling option " + k)
            setattr(self, k, int(v) if kinds[k] is C.c_int else float(v))

    def as_tuple(self):
        return tuple(int(getattr(self, k)) if t is C.c_int else float(getattr(self, k)) for k, t in self._fields_)


class IcpSamplingStats(C.Structure):
    """mm3d_icp_sampling_stats"""
    _fields_ = [("points", C.c_longlong), ("valid", C.c_longlong), ("sampled", C.c_longlong), ("buckets", C.c_int), ("level", C.c_int)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class EstimatorStats(C.Structure):
    """mm3d_estimator_stats"""
    _fields_ = [("correspondences", C.c_longlong), ("edges", C.c_longlong), ("seeds", C.c_longlong), ("hypotheses", C.c_longlong),
                ("winner_index", C.c_int), ("winner_rank", C.c_int), ("winner_inliers", C.c_int)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class IcpRejectionStats(C.Structure):
    """mm3d_icp_rejection_stats"""
    _fields_ = [("matched", C.c_longlong), ("after_one_to_one", C.c_longlong), ("kept", C.c_longlong), ("threshold_d2", C.c_float),
                ("iterations", C.c_int), ("converged", C.c_int)]

    def as_dict(self):
        return {k: (float if t is C.c_float else int)(getattr(self, k)) for k, t in self._fields_}


class IcpGeometryStats(C.Structure):
    """mm3d_icp_geometry_stats"""
    _fields_ = [("matched", C.c_longlong), ("on_boundary", C.c_longlong), ("normal_mismatch", C.c_longlong), ("passed", C.c_longlong),
                ("target_boundary_points", C.c_longlong)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class IcpRobustStats(C.Structure):
    """mm3d_icp_robust_stats"""
    _fields_ = [("matched", C.c_longlong), ("weighted", C.c_longlong), ("weight_sum", C.c_double), ("scale", C.c_double),
                ("iterations", C.c_int), ("converged", C.c_int)]

    def as_dict(self):
        return {k: (float if t is C.c_double else int)(getattr(self, k)) for k, t in self._fields_}


class OverlapStats(C.Structure):
    """mm3d_overlap_stats"""
    _fields_ = [("points_st", C.c_longlong), ("in_st", C.c_longlong), ("hit_st", C.c_longlong), ("points_ts", C.c_longlong),
                ("in_ts", C.c_longlong), ("hit_ts", C.c_longlong), ("confidence", C.c_double)]

    def as_dict(self):
        return {k: (float if t is C.c_double else int)(getattr(self, k)) for k, t in self._fields_}


class AlignmentStats(C.Structure):
    """mm3d_alignment_stats"""
    _fields_ = [("draws", C.c_longlong), ("survivors", C.c_longlong), ("hypotheses_scored", C.c_longlong),
                ("winner_h", C.c_longlong), ("winner_inliers", C.c_int), ("converged", C.c_int)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class MapMergingParams(C.Structure):
    """R/include/map_merge_3d/map_merging.h:28-44, field for field."""
    _fields_ = [("resolution", C.c_double), ("descriptor_radius", C.c_double),
                ("outliers_min_neighbours", C.c_int), ("normal_radius", C.c_double),
                ("keypoint_type", C.c_int), ("keypoint_threshold", C.c_double),
                ("descriptor_type", C.c_int), ("estimation_method", C.c_int),
                ("refine_transform", C.c_int), ("inlier_threshold", C.c_double),
                ("max_correspondence_distance", C.c_double), ("max_iterations", C.c_int),
                ("matching_k", C.c_uint64), ("transform_epsilon", C.c_double),
                ("confidence_threshold", C.c_double), ("output_resolution", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().mm3d_params_default(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, int(v) if isinstance(v, enum.IntEnum) else v)

    @staticmethod
    def fromCommandLine(argv):
        """MapMergingParams::fromCommandLine (R/src/map_merging.cpp:10-54); argv[0] is the program."""
        p = MapMergingParams()
        arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
        st = lib().mm3d_params_from_command_line(len(argv), arr, C.byref(p))
        if st != 0:
            # enums::from_string throws std::runtime_error on a bad value (enum.h:58-60)
            raise RuntimeError("from_string: invalid value for enum")
        return p

    def __str__(self):
        n = lib().mm3d_params_to_string(C.byref(self), None, 0)
        buf = C.create_string_buffer(n)
        lib().mm3d_params_to_string(C.byref(self), buf, n)
        return buf.value.decode()


class _View(C.Structure):
    _fields_ = [("points", C.c_void_p), ("n", C.c_size_t), ("stride", C.c_size_t), ("rgba_offset", C.c_size_t)]


class NnSearchInfo(C.Structure):
    """mm3d_nn_search_info: what mm3d_debug_nn_search derived from its range and the target."""
    _fields_ = [("max_d2", C.c_float), ("rmax", C.c_float), ("cell", C.c_float), ("origin", C.c_float * 3),
                ("dims", C.c_int * 3), ("max_ring", C.c_int), ("n_items", C.c_int)]

    def as_dict(self):
        return dict(max_d2=np.float32(self.max_d2), rmax=np.float32(self.rmax), cell=np.float32(self.cell),
                    origin=np.array(self.origin[:], dtype=np.float32), dims=tuple(self.dims[:]), max_ring=int(self.max_ring),
                    n_items=int(self.n_items))


_LIB = None


def build(force: bool = False) -> str:
    """Compile libmm3d.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call([os.path.join(_HERE, "build.sh")])
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise Mm3dError(-2, f"{LIB_PATH} is missing: run map-merge_amd/build.sh (no CPU fallback exists)")
        L = C.CDLL(LIB_PATH)
        L.mm3d_last_error.restype = C.c_char_p
        for f in ("mm3d_cloud_size", "mm3d_normals_size", "mm3d_desc_size", "mm3d_params_to_string"):
            getattr(L, f).restype = C.c_size_t
        for f in ("mm3d_descriptor_name", "mm3d_descriptor_field_name", "mm3d_keypoint_name",
                  "mm3d_estimation_method_name"):
            getattr(L, f).restype = C.c_char_p
        for f in ("mm3d_map_points", "mm3d_map_keypoints", "mm3d_map_descriptors"):
            getattr(L, f).restype = C.c_void_p
        _LIB = L
    return _LIB


def _T(T):
    """4x4 (row-major numpy) -> column-major float[16] as the ABI takes it."""
    return np.ascontiguousarray(np.asarray(T, dtype=np.float32).reshape(4, 4).T.reshape(16))


def _Tout(a):
    return np.asarray(a, dtype=np.float32).reshape(4, 4).T.copy()


def sift_cert_stats(reset=False):
    """Process-wide counters of the certified SIFT decision (mm3d_debug_sift_cert_stats): octaves, points, exact-path points,
    open points, octaves sent back, bound violations, still-open points, unstaged items."""
    out = (C.c_longlong * 8)()
    lib().mm3d_debug_sift_cert_stats(out, 1 if reset else 0)
    return list(out)


def knn_paths(ctx):
    """mm3d_debug_knn_paths: the routes the descriptor k-NN took on this context while mm3d_set_debug was on, one bit per route
    (1 small brute force, 2 lists, 4 filter, 8 lists of 125-wide rows, 16 wide bf16, 32 wide f32, 64 any k); read and cleared."""
    f = lib().mm3d_debug_knn_paths
    f.restype = C.c_uint
    return int(f(ctx._h))


def sacia_stats(reset=False, collect=-1):
    """Process-wide counters of SAC-IA's certified pick (mm3d_debug_sacia_stats): pairs scored, pairs decided without a float
    chain, candidate hypotheses the intervals left, chains run.  collect = 1 / 0 switches the collection on / off."""
    out = (C.c_longlong * 4)()
    lib().mm3d_debug_sacia_stats(out, 1 if reset else 0, int(collect))
    return list(out)


def sacia_queries_per_thread(k=-1):
    """mm3d_debug_sacia_queries_per_thread: force SAC-IA's error kernel to k source keypoints per thread (1, 2, 4, 8; 0: by
    the launch's size again; negative: leave as it is).  Returns the count large launches use."""
    return int(lib().mm3d_debug_sacia_queries_per_thread(int(k)))


def icp_rejection_split(split=-1):
    """mm3d_debug_icp_rejection_split: force every rejecting launch to one work item per wave (1) or per block (4); 0: chosen by
    size again; negative: leave as it is.  Returns the value in force."""
    return int(lib().mm3d_debug_icp_rejection_split(int(split)))


def icp_robust_split(split=-1):
    """mm3d_debug_icp_robust_split: force every robust launch to one work item per wave (1) or per block (4); 0: chosen by size
    again; negative: leave as it is.  Returns the value in force."""
    return int(lib().mm3d_debug_icp_robust_split(int(split)))


def boundary_lds_cap(cap=-1):
    """mm3d_debug_boundary_lds_cap: the directions a wave of the boundary kernel keeps in LDS (1 .. 512; 0 restores the compiled
    value; negative asks).  Returns the value in force."""
    return int(lib().mm3d_debug_boundary_lds_cap(int(cap)))


def feature_lds_cap(cap):
    """mm3d_debug_feature_lds_cap: the neighbour capacity the first launch of PFH / PFHRGB, SHOT, SC3D and the Harris refinement
    is given (a power of two from 64 to 2048; 0: the compile-time capacities again); larger neighbourhoods take the scratch pass.
    Returns the previous value; anything else changes nothing."""
    return int(lib().mm3d_debug_feature_lds_cap(int(cap)))


def feature_overflow(reset=False):
    """Process-wide counters of the scratch passes (mm3d_debug_feature_overflow): (rows sent to scratch, largest capacity per row
    chosen) for PFH / PFHRGB, SHOT, SC3D and the Harris refinement, in that order."""
    out = (C.c_longlong * 8)()
    lib().mm3d_debug_feature_overflow(out, 1 if reset else 0)
    return list(out)


def icp_color_split(split=-1):
    """mm3d_debug_icp_color_split: force every coloured ICP launch to one work item per wave (1) or per block (4); 0: chosen by
    size again; negative: leave as it is.  Returns the value in force."""
    return int(lib().mm3d_debug_icp_color_split(int(split)))


def icp_generalized_split(split=-1):
    """mm3d_debug_icp_generalized_split: force every generalized ICP launch to one work item per wave (1) or per block (4); 0:
    chosen by size again; negative: leave as it is.  Returns the value in force."""
    return int(lib().mm3d_debug_icp_generalized_split(int(split)))


class Context:
    """One registration engine on one GPU (mm3d_ctx) -- or, with `devices`, on a list of GPUs of this one process
    (mm3d_create_devices): estimateMapsTransforms then shards over them inside the library and gathers the pair
    records through RCCL; every other call works on the first device of the list."""

    def __init__(self, device: int = 0, devices=None):
        self._h = C.c_void_p()
        if devices is not None:
            devices = [int(d) for d in devices]
            arr = (C.c_int * max(len(devices), 1))(*devices)
            st = lib().mm3d_create_devices(arr, len(devices), C.byref(self._h))
            if st != 0:
                why = (lib().mm3d_last_error(None) or b"").decode()
                raise Mm3dError(st, f"mm3d_create_devices({devices}) failed: {why or 'bad list, a device twice, no such device, or RCCL could not create its communicators'} "
                                    "(there is no CPU path)")
            device = devices[0]
        else:
            st = lib().mm3d_create(int(device), C.byref(self._h))
            if st != 0:
                raise Mm3dError(st, "mm3d_create failed: no usable MI355X/HIP device (there is no CPU path)")
        self.device = device

    @property
    def devices(self):
        return [lib().mm3d_device_at(self._h, i) for i in range(lib().mm3d_device_count(self._h))]

    @property
    def uses_rccl(self) -> bool:
        return bool(lib().mm3d_devices_use_rccl(self._h))

    def lastRunDeviceSeconds(self):
        """(exchange_s, pairs_s, gather_s) of the most recent estimateMapsTransforms on a device list."""
        a, b, g = C.c_double(), C.c_double(), C.c_double()
        self._ck(lib().mm3d_last_run_device_seconds(self._h, C.byref(a), C.byref(b), C.byref(g)))
        return a.value, b.value, g.value

    def close(self):
        if self._h:
            lib().mm3d_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st):
        if st != 0:
            raise Mm3dError(st, (lib().mm3d_last_error(self._h) or b"").decode())

    def srand(self, seed: int):
        lib().mm3d_srand(self._h, C.c_uint(seed))

    def setStreams(self, n: int):
        """mm3d_set_streams: HIP streams estimateMapsTransforms deals its two loops to (results are
        bit-identical for every setting)."""
        self._ck(lib().mm3d_set_streams(self._h, int(n)))

    def lastRunMapSizes(self):
        """mm3d_last_run_map_sizes: (points after filtering, keypoints after pruning) per cloud of the last estimateMapsTransforms."""
        f = lib().mm3d_last_run_map_sizes
        f.restype = C.c_size_t
        n = f(self._h, None, None, C.c_size_t(0))
        pts, kps = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
        f(self._h, pts.ctypes.data_as(C.c_void_p), kps.ctypes.data_as(C.c_void_p), C.c_size_t(n))
        return pts[:n], kps[:n]

    def setMapCache(self, max_maps: int):
        """mm3d_set_map_cache: estimateMapsTransforms keeps the features of up to max_maps distinct clouds and the pair
        records among them, and reuses them while clouds and parameters are unchanged (bit-identical results); 0 = off."""
        self._ck(lib().mm3d_set_map_cache(self._h, int(max_maps)))

    def getMapCache(self) -> int:
        return lib().mm3d_get_map_cache(self._h)

    def clearMapCache(self):
        lib().mm3d_map_cache_clear(self._h)

    def mapCacheStats(self, reset: bool = False) -> dict:
        """mm3d_map_cache_stats: counters since the last reset, and what the cache holds now."""
        out = (C.c_longlong * 6)()
        self._ck(lib().mm3d_map_cache_stats(self._h, out, 1 if reset else 0))
        keys = ("map_hits", "map_misses", "pairs_reused", "pairs_computed", "maps_held", "device_bytes")
        return dict(zip(keys, (int(v) for v in out)))

    def setIcpMethod(self, method):
        """mm3d_set_icp_method: the pair stage's ICP, IcpMethod.POINT_TO_POINT (the reference's, the default) or POINT_TO_PLANE."""
        self._ck(lib().mm3d_set_icp_method(self._h, int(method)))

    def getIcpMethod(self) -> "IcpMethod":
        return IcpMethod(lib().mm3d_get_icp_method(self._h))

    def setAlignment(self, options=None, **kw):
        """mm3d_set_alignment: the pair stage's initial alignment under SAC_IA.  An AlignmentOptions, or its fields as keywords
        (method=AlignMethod.PREREJECTIVE, samples=..., k=..., similarity=..., inlier_fraction=...)."""
        o = options if options is not None else AlignmentOptions(**kw)
        self._ck(lib().mm3d_set_alignment(self._h, C.byref(o)))

    def getAlignment(self) -> "AlignmentOptions":
        o = AlignmentOptions()
        self._ck(lib().mm3d_get_alignment(self._h, C.byref(o)))
        return o

    def lastAlignmentStats(self) -> dict:
        st = AlignmentStats()
        self._ck(lib().mm3d_last_alignment_stats(self._h, C.byref(st)))
        return st.as_dict()

    def setEstimator(self, options=None, **kw):
        """mm3d_set_estimator: what estimates a pair from its correspondences under MATCHING.  An EstimatorOptions, or its fields
        as keywords (method=EstimatorMethod.CONSISTENCY, tolerance=..., seeds=..., consensus=...)."""
        o = options if options is not None else EstimatorOptions(**kw)
        self._ck(lib().mm3d_set_estimator(self._h, C.byref(o)))

    def getEstimator(self) -> "EstimatorOptions":
        o = EstimatorOptions()
        self._ck(lib().mm3d_get_estimator(self._h, C.byref(o)))
        return o

    def lastEstimatorStats(self) -> dict:
        st = EstimatorStats()
        self._ck(lib().mm3d_last_estimator_stats(self._h, C.byref(st)))
        return st.as_dict()

    def setKeypoints(self, options=None, **kw):
        """mm3d_set_keypoints: where the whole-map calls take a map's keypoints from.  A KeypointOptions, or its fields as
        keywords (source=KeypointSource.UNIFORM, leaf=... in metres; 0 = the default fraction of descriptor_radius)."""
        o = options if options is not None else KeypointOptions(**kw)
        self._ck(lib().mm3d_set_keypoints(self._h, C.byref(o)))

    def getKeypoints(self) -> "KeypointOptions":
        o = KeypointOptions()
        self._ck(lib().mm3d_get_keypoints(self._h, C.byref(o)))
        return o

    def setOutlierFilter(self, options=None, **kw):
        """mm3d_set_outlier_filter: what filters a down-sampled map behind the whole-map calls.  An OutlierOptions, or its fields
        as keywords (method=OutlierMethod.STATISTICAL, mean_k=1 .. 64, stddev_mult=...)."""
        o = options if options is not None else OutlierOptions(**kw)
        self._ck(lib().mm3d_set_outlier_filter(self._h, C.byref(o)))

    def getOutlierFilter(self) -> "OutlierOptions":
        o = OutlierOptions()
        self._ck(lib().mm3d_get_outlier_filter(self._h, C.byref(o)))
        return o

    @property
    def last_outlier_stats(self) -> dict:
        """mm3d_last_outlier_stats: the statistical filter's last run on this context."""
        st = OutlierStats()
        self._ck(lib().mm3d_last_outlier_stats(self._h, C.byref(st)))
        return st.as_dict()

    def setClusterFilter(self, options=None, **kw):
        """mm3d_set_cluster_filter: what drops the small connected components of a filtered map behind the whole-map calls.  A
        ClusterOptions, or its fields as keywords (method=ClusterMethod.MIN_SIZE or LARGEST, min_size >= 1, tolerance=... in metres;
        0 = twice params.resolution)."""
        o = options if options is not None else ClusterOptions(**kw)
        self._ck(lib().mm3d_set_cluster_filter(self._h, C.byref(o)))

    def getClusterFilter(self) -> "ClusterOptions":
        o = ClusterOptions()
        self._ck(lib().mm3d_get_cluster_filter(self._h, C.byref(o)))
        return o

    @property
    def last_cluster_stats(self) -> dict:
        """mm3d_last_cluster_stats: the cluster filter's last run on this context."""
        st = ClusterStats()
        self._ck(lib().mm3d_last_cluster_stats(self._h, C.byref(st)))
        return st.as_dict()

    def setPlanes(self, options=None, **kw):
        """mm3d_set_planes: what takes the dominant planes out of a filtered map behind the whole-map calls, before the cluster
        filter.  A PlaneOptions, or its fields as keywords (method=PlaneMethod.REMOVE or SET_ASIDE, max_planes 1 .. 8, samples,
        refit, seed, distance=... in metres; 0 = half of params.resolution, min_fraction, axis=(x, y, z), max_angle_deg)."""
        o = options if options is not None else PlaneOptions(**kw)
        self._ck(lib().mm3d_set_planes(self._h, C.byref(o)))

    def getPlanes(self) -> "PlaneOptions":
        o = PlaneOptions()
        self._ck(lib().mm3d_get_planes(self._h, C.byref(o)))
        return o

    @property
    def last_plane_stats(self) -> dict:
        """mm3d_last_plane_stats: the plane stage's last run on this context."""
        st = PlaneStats()
        self._ck(lib().mm3d_last_plane_stats(self._h, C.byref(st)))
        return st.as_dict()

    @property
    def last_planes(self) -> list:
        """mm3d_last_planes: the planes of the plane stage's last run on this context, as dicts."""
        arr = (Plane * 8)()
        n = C.c_int(0)
        self._ck(lib().mm3d_last_planes(self._h, arr, 8, C.byref(n)))
        return [arr[i].as_dict() for i in range(min(n.value, 8))]

    def setSmoothing(self, options=None, **kw):
        """mm3d_set_smoothing: moving-least-squares smoothing of a map's filtered points before its normals (where & MAPS) and of
        the composed map between two voxel passes (where & COMPOSED).  A SmoothOptions, or its fields as keywords
        (method=SmoothMethod.MLS, order=1 or 2, min_neighbours >= 3, where=SmoothWhere.MAPS | SmoothWhere.COMPOSED, radius=... in
        metres; 0 = three times the resolution in force)."""
        o = options if options is not None else SmoothOptions(**kw)
        self._ck(lib().mm3d_set_smoothing(self._h, C.byref(o)))

    def getSmoothing(self) -> "SmoothOptions":
        o = SmoothOptions()
        self._ck(lib().mm3d_get_smoothing(self._h, C.byref(o)))
        return o

    @property
    def last_smooth_stats(self) -> dict:
        """mm3d_last_smooth_stats: the smoothing's last run on this context."""
        st = SmoothStats()
        self._ck(lib().mm3d_last_smooth_stats(self._h, C.byref(st)))
        return st.as_dict()

    def setRefinement(self, options=None, **kw):
        """mm3d_set_refinement: what refines a pair's initial estimate.  A RefineOptions, or its fields as keywords
        (method=RefineMethod.NDT, resolution=... in metres; 0 = the default multiple of params.resolution, neighbours=1 or 7,
        min_points=..., regularisation=...)."""
        o = options if options is not None else RefineOptions(**kw)
        self._ck(lib().mm3d_set_refinement(self._h, C.byref(o)))

    def getRefinement(self) -> "RefineOptions":
        o = RefineOptions()
        self._ck(lib().mm3d_get_refinement(self._h, C.byref(o)))
        return o

    def setCoarseAlignment(self, options=None, **kw):
        """mm3d_set_coarse_alignment: what replaces a pair's initial estimate.  A CoarseOptions, or its fields as keywords
        (method=CoarseMethod.CORRELATIVE, cell=... in metres; 0 = the default multiple of params.resolution, ...)."""
        o = options if options is not None else CoarseOptions(**kw)
        self._ck(lib().mm3d_set_coarse_alignment(self._h, C.byref(o)))

    def getCoarseAlignment(self) -> "CoarseOptions":
        o = CoarseOptions()
        self._ck(lib().mm3d_get_coarse_alignment(self._h, C.byref(o)))
        return o

    def lastCoarseStats(self) -> dict:
        st = CoarseStats()
        self._ck(lib().mm3d_last_coarse_stats(self._h, C.byref(st)))
        return st.as_dict()

    def setConfidence(self, options=None, **kw):
        """mm3d_set_confidence: what a pair record's confidence is.  A ConfidenceOptions, or its fields as keywords
        (method=ConfidenceMethod.OVERLAP, voxel=... in metres; 0 = the default multiple of params.resolution, min_points=...,
        min_overlap=..., view_margin=0 or 1).  Under OVERLAP the confidence lives in [0, 1]."""
        o = options if options is not None else ConfidenceOptions(**kw)
        self._ck(lib().mm3d_set_confidence(self._h, C.byref(o)))

    def getConfidence(self) -> "ConfidenceOptions":
        o = ConfidenceOptions()
        self._ck(lib().mm3d_get_confidence(self._h, C.byref(o)))
        return o

    def setIcpRejection(self, options=None, **kw):
        """mm3d_set_icp_rejection: which correspondences the pair stage's ICP ignores.  An IcpRejectionOptions, or its fields as
        keywords (one_to_one=0 / 1, distance=RejectDistance.TRIMMED / MEDIAN, overlap_ratio=..., min_correspondences=...,
        median_factor=...)."""
        o = options if options is not None else IcpRejectionOptions(**kw)
        self._ck(lib().mm3d_set_icp_rejection(self._h, C.byref(o)))

    def getIcpRejection(self) -> "IcpRejectionOptions":
        o = IcpRejectionOptions()
        self._ck(lib().mm3d_get_icp_rejection(self._h, C.byref(o)))
        return o

    def setIcpGeometryRejection(self, options=None, **kw):
        """mm3d_set_icp_geometry_rejection: the geometric rejectors of the pair stage's ICP.  An IcpGeometryOptions, or its fields as
        keywords (boundary=0 / 1, boundary_radius=..., boundary_angle_deg=..., boundary_min_neighbours=..., normals=0 / 1,
        normal_angle_deg=...)."""
        o = options if options is not None else IcpGeometryOptions(**kw)
        self._ck(lib().mm3d_set_icp_geometry_rejection(self._h, C.byref(o)))

    def getIcpGeometryRejection(self) -> "IcpGeometryOptions":
        o = IcpGeometryOptions()
        self._ck(lib().mm3d_get_icp_geometry_rejection(self._h, C.byref(o)))
        return o

    def setIcpRobust(self, options=None, **kw):
        """mm3d_set_icp_robust: the robust kernel that weights the correspondences of the pair stage's ICP.  An IcpRobustOptions, or
        its fields as keywords (kernel=RobustKernel.GEMAN_MCCLURE ..., scale=..., scale_start=..., anneal=..., tuning=...)."""
        o = options if options is not None else IcpRobustOptions(**kw)
        self._ck(lib().mm3d_set_icp_robust(self._h, C.byref(o)))

    def getIcpRobust(self) -> "IcpRobustOptions":
        o = IcpRobustOptions()
        self._ck(lib().mm3d_get_icp_robust(self._h, C.byref(o)))
        return o

    @property
    def last_icp_robust_stats(self) -> dict:
        """mm3d_last_icp_robust_stats: the last iteration of the most recent robust ICP this context ran."""
        st = IcpRobustStats()
        self._ck(lib().mm3d_last_icp_robust_stats(self._h, C.byref(st)))
        return st.as_dict()

    def setIcpColor(self, options=None, **kw):
        """mm3d_set_icp_color: coloured ICP in the pair stage.  An IcpColorOptions, or its fields as keywords (enabled=0 / 1,
        lambda_geometric=..., gradient_radius=..., min_neighbours=...)."""
        o = options if options is not None else IcpColorOptions(**kw)
        self._ck(lib().mm3d_set_icp_color(self._h, C.byref(o)))

    def getIcpColor(self) -> "IcpColorOptions":
        o = IcpColorOptions()
        self._ck(lib().mm3d_get_icp_color(self._h, C.byref(o)))
        return o

    def setIcpGeneralized(self, options=None, **kw):
        """mm3d_set_icp_generalized: generalized (plane-to-plane) ICP in the pair stage.  An IcpGeneralizedOptions, or its fields
        as keywords (enabled=0 / 1, epsilon=...)."""
        o = options if options is not None else IcpGeneralizedOptions(**kw)
        self._ck(lib().mm3d_set_icp_generalized(self._h, C.byref(o)))

    def getIcpGeneralized(self) -> "IcpGeneralizedOptions":
        o = IcpGeneralizedOptions()
        self._ck(lib().mm3d_get_icp_generalized(self._h, C.byref(o)))
        return o

    def setIcpSampling(self, options=None, **kw):
        """mm3d_set_icp_sampling: the pair stage's ICP searches with a sample of the source map.  An IcpSamplingOptions, or its
        fields as keywords (method=IcpSampleMethod.STRIDE / NORMAL_SPACE, fraction=..., max_points=..., bins=...)."""
        o = options if options is not None else IcpSamplingOptions(**kw)
        self._ck(lib().mm3d_set_icp_sampling(self._h, C.byref(o)))

    def getIcpSampling(self) -> "IcpSamplingOptions":
        o = IcpSamplingOptions()
        self._ck(lib().mm3d_get_icp_sampling(self._h, C.byref(o)))
        return o

    def lastIcpSamplingStats(self) -> dict:
        """mm3d_last_icp_sampling_stats: the most recent sample this context made or fetched from a map."""
        st = IcpSamplingStats()
        self._ck(lib().mm3d_last_icp_sampling_stats(self._h, C.byref(st)))
        return st.as_dict()

    @property
    def last_icp_rejection_stats(self) -> dict:
        """mm3d_last_icp_rejection_stats: the last iteration of the most recent rejecting ICP this context ran."""
        st = IcpRejectionStats()
        self._ck(lib().mm3d_last_icp_rejection_stats(self._h, C.byref(st)))
        return st.as_dict()

    @property
    def last_icp_geometry_stats(self) -> dict:
        """mm3d_last_icp_geometry_stats: step 1b's counts in the last iteration of the most recent such ICP this context ran."""
        st = IcpGeometryStats()
        self._ck(lib().mm3d_last_icp_geometry_stats(self._h, C.byref(st)))
        return st.as_dict()

    def lastConfidenceStats(self) -> dict:
        st = OverlapStats()
        self._ck(lib().mm3d_last_confidence_stats(self._h, C.byref(st)))
        return st.as_dict()

    def synchronize(self):
        self._ck(lib().mm3d_synchronize(self._h))

    # ---- objects -------------------------------------------------------------------------
    def cloud(self, pts) -> "Cloud":
        """Host numpy records (POINT dtype) -> device cloud."""
        pts = np.ascontiguousarray(pts, dtype=POINT)
        h = C.c_void_p()
        self._ck(lib().mm3d_cloud_create(self._h, pts.ctypes.data_as(C.c_void_p), C.c_size_t(len(pts)),
                                         C.c_size_t(16), C.c_size_t(12), C.byref(h)))
        return Cloud(self, h)

    def cloud_from_ptr(self, ptr: int, n: int, stride: int = 16, rgba_offset: int = 12) -> "Cloud":
        """Host or device (HBM) address, e.g. a torch tensor's data_ptr()."""
        h = C.c_void_p()
        self._ck(lib().mm3d_cloud_create(self._h, C.c_void_p(ptr), C.c_size_t(n), C.c_size_t(stride),
                                         C.c_size_t(rgba_offset), C.byref(h)))
        return Cloud(self, h)

    def normals(self, nrm) -> "Normals":
        nrm = np.ascontiguousarray(nrm, dtype=NORMAL)
        h = C.c_void_p()
        self._ck(lib().mm3d_normals_create(self._h, nrm.ctypes.data_as(C.c_void_p), C.c_size_t(len(nrm)),
                                           C.c_size_t(16), C.byref(h)))
        return Normals(self, h)

    def descriptors(self, data, descriptor=Descriptor.FPFH) -> "Descriptors":
        data = np.ascontiguousarray(data, dtype=np.float32)
        h = C.c_void_p()
        self._ck(lib().mm3d_desc_create(self._h, data.ctypes.data_as(C.c_void_p), C.c_size_t(len(data)),
                                        int(descriptor), C.byref(h)))
        return Descriptors(self, h)

    # ---- features.h ------------------------------------------------------------------------
    def downSample(self, cloud: "Cloud", resolution: float) -> "Cloud":
        h = C.c_void_p()
        self._ck(lib().mm3d_downsample(self._h, cloud._h, C.c_double(resolution), C.byref(h)))
        return Cloud(self, h)

    def removeOutliers(self, cloud: "Cloud", radius: float, min_neighbours: int) -> "Cloud":
        h = C.c_void_p()
        self._ck(lib().mm3d_remove_outliers(self._h, cloud._h, C.c_double(radius), int(min_neighbours), C.byref(h)))
        return Cloud(self, h)

    def computeSurfaceNormals(self, cloud: "Cloud", radius: float) -> "Normals":
        h = C.c_void_p()
        self._ck(lib().mm3d_compute_normals(self._h, cloud._h, C.c_double(radius), C.byref(h)))
        return Normals(self, h)

    def detectKeypoints(self, points: "Cloud", normals, type, threshold: float, radius: float,
                        resolution: float) -> "Cloud":
        h = C.c_void_p()
        self._ck(lib().mm3d_detect_keypoints(self._h, points._h, normals._h if normals is not None else None,
                                             int(type), C.c_double(threshold), C.c_double(radius),
                                             C.c_double(resolution), C.byref(h)))
        return Cloud(self, h)

    def uniformKeypoints(self, points: "Cloud", leaf: float) -> "Cloud":
        """mm3d_uniform_keypoints: of every occupied voxel of the global lattice of side leaf, the point nearest its centre."""
        h = C.c_void_p()
        self._ck(lib().mm3d_uniform_keypoints(self._h, points._h, C.c_double(leaf), C.byref(h)))
        return Cloud(self, h)

    def knnMeanDistances(self, points: "Cloud", mean_k: int) -> np.ndarray:
        """mm3d_knn_mean_distances: every point's mean distance to its min(mean_k, valid points - 1) nearest neighbours, float64 in
        the cloud's order; NaN for a non-finite point."""
        out = np.empty(len(points), dtype=np.float64)
        self._ck(lib().mm3d_knn_mean_distances(self._h, points._h, int(mean_k), out.ctypes.data_as(C.c_void_p), C.c_size_t(len(out))))
        return out

    def removeOutliersStatistical(self, cloud: "Cloud", mean_k: int = 16, stddev_mult: float = 2.0) -> "Cloud":
        """mm3d_remove_outliers_statistical: the points whose mean distance to their mean_k nearest neighbours is at most the
        cloud's mean of it plus stddev_mult standard deviations."""
        h = C.c_void_p()
        self._ck(lib().mm3d_remove_outliers_statistical(self._h, cloud._h, int(mean_k), C.c_double(stddev_mult), C.byref(h)))
        return Cloud(self, h)

    def clusterLabels(self, points: "Cloud", tolerance: float, with_stats: bool = False):
        """mm3d_cluster_labels: every point's cluster label, int32 in the cloud's order -- the smallest record index of its
        connected component under `tolerance`, -1 for a non-finite point.  with_stats: (labels, the counts as a dict)."""
        out = np.empty(len(points), dtype=np.int32)
        st = ClusterStats()
        self._ck(lib().mm3d_cluster_labels(self._h, points._h, C.c_double(tolerance), out.ctypes.data_as(C.c_void_p), C.c_size_t(len(out)),
                                           C.byref(st)))
        return (out, st.as_dict()) if with_stats else out

    def removeSmallClusters(self, cloud: "Cloud", tolerance: float, method=ClusterMethod.MIN_SIZE, min_size: int = 100) -> "Cloud":
        """mm3d_remove_small_clusters: the points of the clusters of at least min_size points (MIN_SIZE), or of the largest
        cluster (LARGEST), in the cloud's order."""
        h = C.c_void_p()
        self._ck(lib().mm3d_remove_small_clusters(self._h, cloud._h, C.c_double(tolerance), int(method), int(min_size), C.byref(h)))
        return Cloud(self, h)

    def segmentPlanes(self, points: "Cloud", options=None, **kw):
        """mm3d_segment_planes: (labels int32[n] in the cloud's order -- the round of a record's plane, PLANE_NONE or
        PLANE_INVALID --, the planes as dicts, the counts as a dict).  A PlaneOptions, or its fields as keywords; the method is
        not read."""
        o = options if options is not None else PlaneOptions(**kw)
        out = np.empty(len(points), dtype=np.int32)
        arr = (Plane * 8)()
        n = C.c_int(0)
        st = PlaneStats()
        self._ck(lib().mm3d_segment_planes(self._h, points._h, C.byref(o), out.ctypes.data_as(C.c_void_p), C.c_size_t(len(out)), arr,
                                           C.byref(n), C.byref(st)))
        return out, [arr[i].as_dict() for i in range(n.value)], st.as_dict()

    def removePlanes(self, cloud: "Cloud", options=None, **kw) -> "Cloud":
        """mm3d_remove_planes: the records that lie on none of the planes found, in the cloud's order."""
        o = options if options is not None else PlaneOptions(**kw)
        h = C.c_void_p()
        self._ck(lib().mm3d_remove_planes(self._h, cloud._h, C.byref(o), C.byref(h)))
        return Cloud(self, h)

    def smoothDisplacements(self, points: "Cloud", radius: float, order: int = 2, min_neighbours: int = 6):
        """mm3d_smooth_displacements: (disp float64[n, 3], state int32[n], neighbours int32[n], the counts as a dict) of the
        moving-least-squares rule, in the cloud's order; a point that stays has a zero displacement."""
        n = len(points)
        disp = np.zeros((n, 3), dtype=np.float64)
        state = np.zeros(n, dtype=np.int32)
        count = np.zeros(n, dtype=np.int32)
        st = SmoothStats()
        self._ck(lib().mm3d_smooth_displacements(self._h, points._h, C.c_double(radius), int(order), int(min_neighbours),
                                                 disp.ctypes.data_as(C.c_void_p), state.ctypes.data_as(C.c_void_p),
                                                 count.ctypes.data_as(C.c_void_p), C.c_size_t(n), C.byref(st)))
        return disp, state, count, st.as_dict()

    def smoothCloud(self, cloud: "Cloud", radius: float, order: int = 2, min_neighbours: int = 6) -> "Cloud":
        """mm3d_smooth_cloud: the cloud with every valid point moved by the moving-least-squares rule, same size and order."""
        h = C.c_void_p()
        self._ck(lib().mm3d_smooth_cloud(self._h, cloud._h, C.c_double(radius), int(order), int(min_neighbours), C.byref(h)))
        return Cloud(self, h)

    def siftCertOctave(self, points: "Cloud", min_scale: float, octave: int):
        """Test hook (mm3d_debug_sift_cert_octave): the certified SIFT pass of one octave -- (val[n, 5], bound[n, 5]) with
        bound >= |the CPU path's float DoG - val|, or None when the octave does not exist."""
        n = C.c_size_t(0)
        self._ck(lib().mm3d_debug_sift_cert_octave(self._h, points._h, C.c_double(min_scale), int(octave), None, None, C.c_size_t(0), C.byref(n)))
        if n.value == 0:
            return None
        val = np.empty((n.value, 5), dtype=np.float32)
        bound = np.empty((n.value, 5), dtype=np.float32)
        self._ck(lib().mm3d_debug_sift_cert_octave(self._h, points._h, C.c_double(min_scale), int(octave), val.ctypes.data_as(C.c_void_p),
                                                   bound.ctypes.data_as(C.c_void_p), C.c_size_t(n.value), C.byref(n)))
        return val, bound

    def siftDogMarked(self, points: "Cloud", min_scale: float, octave: int, ids, small_capacity: bool = False) -> np.ndarray:
        """Test hook (mm3d_debug_sift_dog_marked): the exact float DoG of the points `ids` of one octave's cloud, float32[len(ids), 5],
        from the one-block-per-point kernel of the certified octaves.  small_capacity: the sort buffer of 128 keys (lists in
        distance bands).  Raises Mm3dError with status -4 when a point does not fit the buffer; rows never written are NaN."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        out = np.full((len(ids), 5), np.nan, dtype=np.float32)
        self._ck(lib().mm3d_debug_sift_dog_marked(self._h, points._h, C.c_double(min_scale), int(octave), ids.ctypes.data_as(C.c_void_p),
                                                  C.c_size_t(len(ids)), 1 if small_capacity else 0, out.ctypes.data_as(C.c_void_p)))
        return out

    def harrisResponse(self, points: "Cloud", normals: "Normals", radius: float) -> np.ndarray:
        """HarrisKeypoint3D::responseHarris of every point (what detectKeypoints(HARRIS) thresholds)."""
        out = np.zeros(max(len(points), 1), dtype=np.float32)
        self._ck(lib().mm3d_harris_response(self._h, points._h, normals._h, C.c_double(radius), out.ctypes.data_as(C.c_void_p)))
        return out[:len(points)]

    def computeLocalDescriptors(self, points: "Cloud", normals: "Normals", keypoints: "Cloud", descriptor,
                                feature_radius: float) -> "Descriptors":
        """Prunes `keypoints` in place like the reference (features.h:72-74)."""
        h = C.c_void_p()
        self._ck(lib().mm3d_compute_descriptors(self._h, points._h, normals._h, keypoints._h, int(descriptor),
                                                C.c_double(feature_radius), C.byref(h)))
        return Descriptors(self, h)

    # ---- matching.h ------------------------------------------------------------------------
    def findFeatureCorrespondences(self, source: "Descriptors", target: "Descriptors", k: int = 5):
        n = C.c_size_t()
        self._ck(lib().mm3d_find_correspondences(self._h, source._h, target._h, C.c_size_t(k), None, C.c_size_t(0),
                                                 C.byref(n)))
        out = np.empty(max(n.value, 1), dtype=CORR)
        self._ck(lib().mm3d_find_correspondences(self._h, source._h, target._h, C.c_size_t(k),
                                                 out.ctypes.data_as(C.c_void_p), C.c_size_t(len(out)), C.byref(n)))
        return out[:n.value].copy()

    def estimateTransformFromCorrespondences(self, source_keypoints, target_keypoints, correspondences,
                                             inlier_threshold: float):
        corr = np.ascontiguousarray(correspondences, dtype=CORR)
        T = np.zeros(16, dtype=np.float32)
        inl = np.empty(max(len(corr), 1), dtype=CORR)
        n = C.c_size_t()
        self._ck(lib().mm3d_estimate_transform_from_correspondences(
            self._h, source_keypoints._h, target_keypoints._h, corr.ctypes.data_as(C.c_void_p), C.c_size_t(len(corr)),
            C.c_double(inlier_threshold), T.ctypes.data_as(C.c_void_p), inl.ctypes.data_as(C.c_void_p),
            C.c_size_t(len(inl)), C.byref(n)))
        return _Tout(T), inl[:n.value].copy()

    def estimateTransformConsistency(self, source_keypoints, target_keypoints, correspondences, inlier_threshold: float,
                                     options=None, **kw):
        """mm3d_estimate_transform_consistency: (T, inliers, stats dict), whatever the context's setting."""
        o = options if options is not None else EstimatorOptions(**kw)
        corr = np.ascontiguousarray(correspondences, dtype=CORR)
        T = np.zeros(16, dtype=np.float32)
        inl = np.empty(max(len(corr), 1), dtype=CORR)
        n = C.c_size_t()
        st = EstimatorStats()
        self._ck(lib().mm3d_estimate_transform_consistency(
            self._h, source_keypoints._h, target_keypoints._h, corr.ctypes.data_as(C.c_void_p), C.c_size_t(len(corr)),
            C.c_double(inlier_threshold), C.byref(o), T.ctypes.data_as(C.c_void_p), inl.ctypes.data_as(C.c_void_p),
            C.c_size_t(len(inl)), C.byref(n), C.byref(st)))
        return _Tout(T), inl[:n.value].copy(), st.as_dict()

    def consistencyGraph(self, source_keypoints, target_keypoints, correspondences, inlier_threshold: float, options=None, **kw):
        """mm3d_debug_consistency: a dict of rows [C][ceil(C / 64)] uint64, deg [C], seeds [n_seeds] by rank, consensus
        [n_seeds][consensus] ascending and -1 padded, hypotheses [n_seeds][4][4] (row-major, as every transform here) and
        counts [n_seeds] (-1 without a hypothesis)."""
        o = options if options is not None else EstimatorOptions(**kw)
        corr = np.ascontiguousarray(correspondences, dtype=CORR)
        n_c = len(corr)
        W, H, K = (n_c + 63) // 64, min(int(o.seeds), n_c), int(o.consensus)
        rows = np.zeros((n_c, W), dtype=np.uint64)
        deg = np.zeros(n_c, dtype=np.int32)
        seeds = np.full(max(H, 1), -1, dtype=np.int32)
        cons = np.full((max(H, 1), K), -1, dtype=np.int32)
        hyp = np.zeros((max(H, 1), 16), dtype=np.float32)
        counts = np.full(max(H, 1), -1, dtype=np.int32)
        n = C.c_size_t()
        self._ck(lib().mm3d_debug_consistency(
            self._h, source_keypoints._h, target_keypoints._h, corr.ctypes.data_as(C.c_void_p), C.c_size_t(n_c),
            C.c_double(inlier_threshold), C.byref(o), rows.ctypes.data_as(C.c_void_p), deg.ctypes.data_as(C.c_void_p),
            seeds.ctypes.data_as(C.c_void_p), C.byref(n), cons.ctypes.data_as(C.c_void_p), hyp.ctypes.data_as(C.c_void_p),
            counts.ctypes.data_as(C.c_void_p)))
        m = int(n.value)
        return dict(rows=rows, deg=deg, seeds=seeds[:m].copy(), consensus=cons[:m].copy(),
                    hypotheses=hyp[:m].reshape(m, 4, 4).transpose(0, 2, 1).copy(), counts=counts[:m].copy())

    def estimateTransformFromDescriptorsSets(self, source_keypoints, source_descriptors, target_keypoints,
                                             target_descriptors, min_sample_distance, max_correspondence_distance,
                                             max_iterations):
        T = np.zeros(16, dtype=np.float32)
        self._ck(lib().mm3d_estimate_transform_from_descriptors(
            self._h, source_keypoints._h, source_descriptors._h, target_keypoints._h, target_descriptors._h,
            C.c_double(min_sample_distance), C.c_double(max_correspondence_distance), int(max_iterations),
            T.ctypes.data_as(C.c_void_p)))
        return _Tout(T)

    def estimateTransformPrerejective(self, source_keypoints, source_descriptors, target_keypoints, target_descriptors,
                                      inlier_distance, options=None, **kw):
        """mm3d_estimate_transform_prerejective: (T, stats dict), whatever the context's setting."""
        o = options if options is not None else AlignmentOptions(**kw)
        T = np.zeros(16, dtype=np.float32)
        st = AlignmentStats()
        self._ck(lib().mm3d_estimate_transform_prerejective(
            self._h, source_keypoints._h, source_descriptors._h, target_keypoints._h, target_descriptors._h,
            C.c_double(inlier_distance), C.byref(o), T.ctypes.data_as(C.c_void_p), C.byref(st)))
        return _Tout(T), st.as_dict()

    def prerejectiveSurvivors(self, source_keypoints, source_descriptors, target_keypoints, target_descriptors,
                              inlier_distance, options=None, cap=1 << 20, **kw):
        """mm3d_debug_prerejective_survivors: (rows [n][7] = h, i0 i1 i2, t0 t1 t2 in ascending h; their inlier counts;
        the number of survivors, which may exceed cap)."""
        o = options if options is not None else AlignmentOptions(**kw)
        rows = np.zeros((max(cap, 1), 7), dtype=np.int32)
        counts = np.zeros(max(cap, 1), dtype=np.int32)
        n = C.c_size_t()
        self._ck(lib().mm3d_debug_prerejective_survivors(
            self._h, source_keypoints._h, source_descriptors._h, target_keypoints._h, target_descriptors._h,
            C.c_double(inlier_distance), C.byref(o), rows.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
            C.c_size_t(cap), C.byref(n)))
        m = min(int(n.value), cap)
        return rows[:m].copy(), counts[:m].copy(), int(n.value)

    def estimateTransformICP(self, source_points, target_points, initial_guess, max_correspondence_distance,
                             outlier_rejection_threshold, max_iterations=100, transformation_epsilon=0.0):
        g = _T(initial_guess)
        T = np.zeros(16, dtype=np.float32)
        self._ck(lib().mm3d_estimate_transform_icp(
            self._h, source_points._h, target_points._h, g.ctypes.data_as(C.c_void_p),
            C.c_double(max_correspondence_distance), C.c_double(outlier_rejection_threshold), int(max_iterations),
            C.c_double(transformation_epsilon), T.ctypes.data_as(C.c_void_p)))
        self.last_icp_iterations = lib().mm3d_last_icp_iterations(self._h)
        return _Tout(T)

    def estimateTransformICPPlane(self, source_points, target_points, target_normals, initial_guess, max_correspondence_distance,
                                  max_iterations=100, transformation_epsilon=0.0):
        """mm3d_estimate_transform_icp_plane: point-to-plane ICP from initial_guess (target_normals: one per target point)."""
        g = _T(initial_guess)
        T = np.zeros(16, dtype=np.float32)
        self._ck(lib().mm3d_estimate_transform_icp_plane(
            self._h, source_points._h, target_points._h, target_normals._h, g.ctypes.data_as(C.c_void_p),
            C.c_double(max_correspondence_distance), int(max_iterations), C.c_double(transformation_epsilon),
            T.ctypes.data_as(C.c_void_p)))
        self.last_icp_iterations = lib().mm3d_last_icp_iterations(self._h)
        self.last_icp_converged = lib().mm3d_last_icp_converged(self._h)
        return _Tout(T)

    def estimateTransformICPRejecting(self, source_points, target_points, target_normals, initial_guess, max_correspondence_distance,
                                      options=None, max_iterations=100, transformation_epsilon=0.0, **kw):
        """mm3d_estimate_transform_icp_rejecting: ICP with correspondence rejection from initial_guess, whatever the context's
        setting.  target_normals None: the point-to-point estimate, else the point-to-plane one."""
        o = options if options is not None else IcpRejectionOptions(**kw)
        g = _T(initial_guess)
        T = np.zeros(16, dtype=np.float32)
        st = IcpRejectionStats()
        self._ck(lib().mm3d_estimate_transform_icp_rejecting(
            self._h, source_points._h, target_points._h, target_normals._h if target_normals is not None else None,
            g.ctypes.data_as(C.c_void_p), C.c_double(max_correspondence_distance), C.byref(o), int(max_iterations),
            C.c_double(transformation_epsilon), T.ctypes.data_as(C.c_void_p), C.byref(st)))
        self.last_icp_iterations = lib().mm3d_last_icp_iterations(self._h)
        self.last_icp_converged = lib().mm3d_last_icp_converged(self._h)
        return _Tout(T)

    def boundaryPoints(self, points, normals, radius, angle_deg=90.0, min_neighbours=3):
        """mm3d_boundary_points: (flags bool[n] in the points' order, their number)."""
        n = len(points)
        flags = np.zeros(max(n, 1), dtype=np.uint8)
        count = C.c_longlong(0)
        self._ck(lib().mm3d_boundary_points(self._h, points._h, normals._h, C.c_double(radius), C.c_double(angle_deg), int(min_neighbours),
                                            flags.ctypes.data_as(C.c_void_p), C.c_size_t(flags.size), C.byref(count)))
        return flags[:n].astype(bool), int(count.value)

    def estimateTransformICPRejectingGeometry(self, source_points, source_normals, target_points, target_normals, initial_guess,
                                              max_correspondence_distance, rejection=None, geometry=None, point_to_plane=False,
                                              max_iterations=100, transformation_epsilon=0.0):
        """mm3d_estimate_transform_icp_rejecting_geometry: ICP with correspondence rejection and its geometric step 1b from
        initial_guess, whatever the context's settings.  Returns (T, rejection stats dict, geometry stats dict)."""
        ro = rejection if rejection is not None else IcpRejectionOptions()
        go = geometry if geometry is not None else IcpGeometryOptions()
        g = _T(initial_guess)
        T = np.zeros(16, dtype=np.float32)
        rs, gs = IcpRejectionStats(), IcpGeometryStats()
        self._ck(lib().mm3d_estimate_transform_icp_rejecting_geometry(
            self._h, source_points._h, source_normals._h if source_normals is not None else None, target_points._h,
            target_normals._h if target_normals is not None else None, int(bool(point_to_plane)), g.ctypes.data_as(C.c_void_p),
            C.c_double(max_correspondence_distance), C.byref(ro), C.byref(go), int(max_iterations), C.c_double(transformation_epsilon),
            T.ctypes.data_as(C.c_void_p), C.byref(rs), C.byref(gs)))
        self.last_icp_iterations = lib().mm3d_last_icp_iterations(self._h)
        self.last_icp_converged = lib().mm3d_last_icp_converged(self._h)
        return _Tout(T), rs.as_dict(), gs.as_dict()

    def estimateTransformICPRobust(self, source_points, target_points, target_normals, initial_guess, max_correspondence_distance,
                                   options=None, max_iterations=100, transformation_epsilon=0.0, **kw):
        """mm3d_estimate_transform_icp_robust: ICP with a robust kernel from initial_guess, whatever the context's setting.
        target_normals None: the point-to-point estimate, else the point-to-plane one."""
        o = options if options is not None else IcpRobustOptions(**kw)
        g = _T(initial_guess)
        T = np.zeros(16, dtype=np.float32)
        st = IcpRobustStats()
        self._ck(lib().mm3d_estimate_transform_icp_robust(
            self._h, source_points._h, target_points._h, target_normals._h if target_normals is not None else None,
            g.ctypes.data_as(C.c_void_p), C.c_double(max_correspondence_distance), C.byref(o), int(max_iterations),
            C.c_double(transformation_epsilon), T.ctypes.data_as(C.c_void_p), C.byref(st)))
        self.last_icp_iterations = lib().mm3d_last_icp_iterations(self._h)
        self.last_icp_converged = lib().mm3d_last_icp_converged(self._h)
        return _Tout(T)

    def estimateTransformICPColor(self, source_points, target_points, target_normals, initial_guess, max_correspondence_distance,
                                  options=None, max_iterations=100, transformation_epsilon=0.0, **kw):
        """mm3d_estimate_transform_icp_color: coloured ICP from initial_guess, whatever the context's setting and options.enabled
        (options.gradient_radius > 0; target_normals: one per target point)."""
        o = options if options is not None else IcpColorOptions(**kw)
        g = _T(initial_guess)
        T = np.zeros(16, dtype=np.float32)
        self._ck(lib().mm3d_estimate_transform_icp_color(
            self._h, source_points._h, target_points._h, target_normals._h, g.ctypes.data_as(C.c_void_p),
            C.c_double(max_correspondence_distance), C.byref(o), int(max_iterations), C.c_double(transformation_epsilon),
            T.ctypes.data_as(C.c_void_p)))
        self.last_icp_iterations = lib().mm3d_last_icp_iterations(self._h)
        self.last_icp_converged = lib().mm3d_last_icp_converged(self._h)
        return _Tout(T)

    def estimateTransformICPGeneralized(self, source_points, source_normals, target_points, target_normals, initial_guess,
                                        max_correspondence_distance, max_iterations=100, transformation_epsilon=0.0, epsilon=None):
        """mm3d_estimate_transform_icp_generalized: generalized ICP from initial_guess, whatever the context's setting (each
        cloud's normals: one per point; epsilon: mm3d_icp_generalized_options_default's when None)."""
        o = IcpGeneralizedOptions() if epsilon is None else IcpGeneralizedOptions(epsilon=epsilon)
        g = _T(initial_guess)
        T = np.zeros(16, dtype=np.float32)
        self._ck(lib().mm3d_estimate_transform_icp_generalized(
            self._h, source_points._h, source_normals._h, target_points._h, target_normals._h, g.ctypes.data_as(C.c_void_p),
            C.c_double(max_correspondence_distance), C.byref(o), int(max_iterations), C.c_double(transformation_epsilon),
            T.ctypes.data_as(C.c_void_p)))
        self.last_icp_iterations = lib().mm3d_last_icp_iterations(self._h)
        self.last_icp_converged = lib().mm3d_last_icp_converged(self._h)
        return _Tout(T)

    def sampleIcpSource(self, points, normals, options=None, indices=True, **kw):
        """mm3d_sample_icp_source: (the sample as a Cloud, the kept points' indices in `points` -- None with indices=False) under
        the options, whatever the context's setting.  normals: one per point under NORMAL_SPACE, None under STRIDE."""
        o = options if options is not None else IcpSamplingOptions(**kw)
        h = C.c_void_p()
        idx = np.full(max(len(points), 1), -1, dtype=np.int32) if indices else None
        self._ck(lib().mm3d_sample_icp_source(self._h, points._h, normals._h if normals is not None else None, C.byref(o), C.byref(h),
                                              idx.ctypes.data_as(C.c_void_p) if indices else None, C.c_size_t(len(points) if indices else 0)))
        cloud = Cloud(self, h)
        return cloud, (idx[:len(cloud)].copy() if indices else None)

    def estimateTransformICPSampled(self, source_points, source_normals, target_points, target_normals, initial_guess,
                                    max_correspondence_distance, options=None, max_iterations=100, transformation_epsilon=0.0, **kw):
        """mm3d_estimate_transform_icp_sampled: mm3d_sample_icp_source of the source, then the point-to-point ICP (target_normals
        None) or the point-to-plane ICP on the sample, whatever the context's setting."""
        o = options if options is not None else IcpSamplingOptions(**kw)
        g = _T(initial_guess)
        T = np.zeros(16, dtype=np.float32)
        self._ck(lib().mm3d_estimate_transform_icp_sampled(
            self._h, source_points._h, source_normals._h if source_normals is not None else None, target_points._h,
            target_normals._h if target_normals is not None else None, C.byref(o), g.ctypes.data_as(C.c_void_p),
            C.c_double(max_correspondence_distance), int(max_iterations), C.c_double(transformation_epsilon),
            T.ctypes.data_as(C.c_void_p)))
        self.last_icp_iterations = lib().mm3d_last_icp_iterations(self._h)
        self.last_icp_converged = lib().mm3d_last_icp_converged(self._h)
        return _Tout(T)

    def estimateTransformNDT(self, source_points, target_points, initial_guess, options=None, max_iterations=100,
                             transformation_epsilon=0.0, **kw):
        """mm3d_estimate_transform_ndt: NDT from initial_guess, whatever the context's setting (options.resolution > 0)."""
        o = options if options is not None else RefineOptions(**kw)
        g = _T(initial_guess)
        T = np.zeros(16, dtype=np.float32)
        self._ck(lib().mm3d_estimate_transform_ndt(
            self._h, source_points._h, target_points._h, g.ctypes.data_as(C.c_void_p), C.byref(o), int(max_iterations),
            C.c_double(transformation_epsilon), T.ctypes.data_as(C.c_void_p)))
        self.last_icp_iterations = lib().mm3d_last_icp_iterations(self._h)
        self.last_icp_converged = lib().mm3d_last_icp_converged(self._h)
        return _Tout(T)

    def ndtVoxels(self, target_points, options=None, cap=1 << 20, **kw):
        """mm3d_debug_ndt_voxels: the target's voxel table in ascending (i, j, k) as a dict of arrays -- ijk [n][3], count [n],
        mean [n][3], icov [n][6] (xx xy xz yy yz zz; zeros when invalid), valid [n] -- and the number of voxels, which may exceed cap."""
        o = options if options is not None else RefineOptions(**kw)
        c = max(int(cap), 1)
        ijk = np.zeros((c, 3), dtype=np.int32)
        count = np.zeros(c, dtype=np.int32)
        mean = np.zeros((c, 3), dtype=np.float32)
        icov = np.zeros((c, 6), dtype=np.float32)
        valid = np.zeros(c, dtype=np.uint8)
        n = C.c_size_t()
        self._ck(lib().mm3d_debug_ndt_voxels(
            self._h, target_points._h, C.byref(o), ijk.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p),
            mean.ctypes.data_as(C.c_void_p), icov.ctypes.data_as(C.c_void_p), valid.ctypes.data_as(C.c_void_p), C.c_size_t(int(cap)),
            C.byref(n)))
        m = min(int(n.value), int(cap))
        return dict(ijk=ijk[:m].copy(), count=count[:m].copy(), mean=mean[:m].copy(), icov=icov[:m].copy(),
                    valid=valid[:m].astype(bool)), int(n.value)

    def estimateTransformCorrelative(self, source_points, source_normals, target_points, target_normals, options=None, **kw):
        """mm3d_estimate_transform_correlative: (T, stats dict), whatever the context's setting (options.cell > 0)."""
        o = options if options is not None else CoarseOptions(**kw)
        T = np.zeros(16, dtype=np.float32)
        st = CoarseStats()
        self._ck(lib().mm3d_estimate_transform_correlative(
            self._h, source_points._h, source_normals._h, target_points._h, target_normals._h, C.byref(o),
            T.ctypes.data_as(C.c_void_p), C.byref(st)))
        return _Tout(T), st.as_dict()

    def correlativeSignature(self, points, normals, options=None, cap=1 << 20, **kw):
        """mm3d_debug_correlative_signature: a dict of structure [n][3] (i, j, count), ground [n][3], ground_height [n] and
        coarse [n][2], each ascending in (i, j)."""
        o = options if options is not None else CoarseOptions(**kw)
        c = max(int(cap), 1)
        st = np.zeros((c, 3), dtype=np.int32)
        gr = np.zeros((c, 3), dtype=np.int32)
        gh = np.zeros(c, dtype=np.float32)
        co = np.zeros((c, 2), dtype=np.int32)
        n = (C.c_size_t * 3)()
        self._ck(lib().mm3d_debug_correlative_signature(
            self._h, points._h, normals._h, C.byref(o), st.ctypes.data_as(C.c_void_p), gr.ctypes.data_as(C.c_void_p),
            gh.ctypes.data_as(C.c_void_p), co.ctypes.data_as(C.c_void_p), C.c_size_t(c), n))
        if max(n) > c:
            raise RuntimeError("correlativeSignature: more cells than cap")
        return dict(structure=st[:n[0]].copy(), ground=gr[:n[1]].copy(), ground_height=gh[:n[1]].copy(), coarse=co[:n[2]].copy())

    def correlativeVotes(self, source_points, source_normals, target_points, target_normals, q, options=None, **kw):
        """mm3d_debug_correlative_votes: a dict of frame (Q, u_min, v_min, U, V), acc [U][V] of coarse yaw index q, cands
        [n][4] (q, u, v, votes) in rank order and scores [n][2G+1][2F+1][2F+1]."""
        o = options if options is not None else CoarseOptions(**kw)
        frame = (C.c_int * 5)()
        n = C.c_size_t()
        K, W, GW = int(o.candidates), 2 * int(o.cell_factor) + 1, 2 * int(o.yaw_factor) + 1
        cands = np.zeros((K, 4), dtype=np.int32)
        scores = np.zeros((K, GW, W, W), dtype=np.int32)
        args = (self._h, source_points._h, source_normals._h, target_points._h, target_normals._h, C.byref(o), int(q), frame)
        self._ck(lib().mm3d_debug_correlative_votes(*args, None, C.c_size_t(0), cands.ctypes.data_as(C.c_void_p),
                                                    scores.ctypes.data_as(C.c_void_p), C.c_size_t(K), C.byref(n)))
        U, V = int(frame[3]), int(frame[4])
        acc = np.zeros((U, V), dtype=np.int32)
        if U * V:
            self._ck(lib().mm3d_debug_correlative_votes(*args, acc.ctypes.data_as(C.c_void_p), C.c_size_t(U * V),
                                                        cands.ctypes.data_as(C.c_void_p), scores.ctypes.data_as(C.c_void_p),
                                                        C.c_size_t(K), C.byref(n)))
        m = int(n.value)
        return dict(frame=tuple(int(x) for x in frame), acc=acc, cands=cands[:m].copy(), scores=scores[:m].copy())

    def transformOverlap(self, source_points, target_points, transform, options=None, **kw) -> dict:
        """mm3d_transform_overlap: the overlap confidence of two clouds under `transform` (4 x 4) and its six counts, whatever
        the context's setting (options.voxel > 0)."""
        o = options if options is not None else ConfidenceOptions(**kw)
        T = _T(transform)
        st = OverlapStats()
        self._ck(lib().mm3d_transform_overlap(self._h, source_points._h, target_points._h, T.ctypes.data_as(C.c_void_p), C.byref(o),
                                              C.byref(st)))
        return st.as_dict()

    def debugOverlapTable(self, points, options=None, **kw) -> dict:
        """mm3d_debug_overlap_table: brick0 / bricks / view0 / views (3 ints each), words uint64 [bricks] and view uint8
        [views], both i-major."""
        o = options if options is not None else ConfidenceOptions(**kw)
        box = (C.c_int * 12)()
        self._ck(lib().mm3d_debug_overlap_table(self._h, points._h, C.byref(o), box, None, C.c_size_t(0), None, C.c_size_t(0)))
        b = [int(x) for x in box]
        words = np.zeros(tuple(b[3:6]), dtype=np.uint64)
        view = np.zeros(tuple(b[9:12]), dtype=np.uint8)
        if words.size:
            self._ck(lib().mm3d_debug_overlap_table(self._h, points._h, C.byref(o), box, words.ctypes.data_as(C.c_void_p),
                                                    C.c_size_t(words.size), view.ctypes.data_as(C.c_void_p), C.c_size_t(view.size)))
        return dict(brick0=tuple(b[0:3]), bricks=tuple(b[3:6]), view0=tuple(b[6:9]), views=tuple(b[9:12]), words=words, view=view)

    def estimateTransform(self, source_points, source_keypoints, source_descriptors, target_points,
                          target_keypoints, target_descriptors, method, refine, inlier_threshold,
                          max_correspondence_distance, max_iterations, matching_k, transform_epsilon):
        T = np.zeros(16, dtype=np.float32)
        self._ck(lib().mm3d_estimate_transform(
            self._h, source_points._h, source_keypoints._h, source_descriptors._h, target_points._h,
            target_keypoints._h, target_descriptors._h, int(method), int(bool(refine)), C.c_double(inlier_threshold),
            C.c_double(max_correspondence_distance), int(max_iterations), C.c_size_t(matching_k),
            C.c_double(transform_epsilon), T.ctypes.data_as(C.c_void_p)))
        return _Tout(T)

    def debugWavePrimitives(self, op, values):
        """mm3d_debug_wave_primitives: one wave reduction / scan of device_util.hpp and the shuffle loop it replaced on the
        same input (a multiple of 256 elements; float64 for op 0, float32 for 1, 5, 6, uint64 for 8, int32 otherwise).
        Returns (new, old), every lane's result."""
        dt = {0: np.float64, 1: np.float32, 5: np.float32, 6: np.float32, 8: np.uint64}.get(int(op), np.int32)
        v = np.ascontiguousarray(values, dtype=dt)
        new, old = np.empty_like(v), np.empty_like(v)
        self._ck(lib().mm3d_debug_wave_primitives(self._h, int(op), v.ctypes.data_as(C.c_void_p), len(v),
                                                  new.ctypes.data_as(C.c_void_p), old.ctypes.data_as(C.c_void_p)))
        return new, old

    def debugNnSearch(self, source_points, target_points, transform, range, convention, split):
        """mm3d_debug_nn_search: the ICP / score nearest-neighbour search point by point.  convention 0 reads `range` as ICP's
        max_correspondence_distance, 1 as transformScore's max_distance (compared with the squared distance); split 1 or 4 is
        forced.  Returns (idx int32[n], d2 float32[n], info dict) in the source's own order: idx -1 and d2 +inf for nothing
        in range and for non-finite source points."""
        n = len(source_points)
        idx = np.zeros(max(n, 1), dtype=np.int32)
        d2 = np.zeros(max(n, 1), dtype=np.float32)
        t = _T(transform)
        info = NnSearchInfo()
        self._ck(lib().mm3d_debug_nn_search(self._h, source_points._h, target_points._h, t.ctypes.data_as(C.c_void_p),
                                            C.c_double(range), int(convention), int(split), idx.ctypes.data_as(C.c_void_p),
                                            d2.ctypes.data_as(C.c_void_p), C.byref(info)))
        return idx[:n], d2[:n], info.as_dict()

    def debugHilbertOrder(self, points, min_cell=0.25):
        """mm3d_debug_hilbert_order: the Hilbert order and the wave work items of a fresh cloud.  Returns (order int32[finite
        points]: original index of every sorted point, items int32[m][2]: first sorted point and count per item)."""
        n = len(points)
        cap = n // 64 + 16386
        order = np.full(max(n, 1), -1, dtype=np.int32)
        items = np.zeros((cap, 2), dtype=np.int32)
        m = C.c_int(0)
        self._ck(lib().mm3d_debug_hilbert_order(self._h, points._h, C.c_float(min_cell), order.ctypes.data_as(C.c_void_p),
                                                items.ctypes.data_as(C.c_void_p), C.c_size_t(cap), C.byref(m)))
        order = order[:n]
        return order[order >= 0], items[:m.value]

    def debugCountingSort(self, keys, key_range, no_invalid_keys=False):
        """mm3d_debug_counting_sort: the voxel filter's counting sort on host keys.  Returns (keys_out uint32[n], idx_out
        uint32[n], too_long bool); entries behind the valid keys, and everything when too_long, read 0xFFFFFFFF."""
        k = np.ascontiguousarray(keys, dtype=np.uint32)
        ko, io = np.zeros(len(k), dtype=np.uint32), np.zeros(len(k), dtype=np.uint32)
        tl = C.c_int(0)
        self._ck(lib().mm3d_debug_counting_sort(self._h, k.ctypes.data_as(C.c_void_p), C.c_size_t(len(k)), C.c_uint64(int(key_range)),
                                                int(bool(no_invalid_keys)), ko.ctypes.data_as(C.c_void_p), io.ctypes.data_as(C.c_void_p),
                                                C.byref(tl)))
        return ko, io, bool(tl.value)

    def debugColorGradients(self, points, normals, options=None, **kw):
        """mm3d_debug_color_gradients: the gradient records of `points` with `normals`, float32[n][4]: gx gy gz I."""
        o = options if options is not None else IcpColorOptions(**kw)
        n = len(points)
        out = np.zeros((max(n, 1), 4), dtype=np.float32)
        self._ck(lib().mm3d_debug_color_gradients(self._h, points._h, normals._h, C.byref(o), out.ctypes.data_as(C.c_void_p)))
        return out[:n]

    def debugIcpRejection(self, source_points, target_points, transform, max_correspondence_distance, options=None, split=1, **kw):
        """mm3d_debug_icp_rejection: one iteration's correspondence stage at `transform`.  Returns (idx int32[n], d2 float32[n],
        kept bool[n], stats dict) in the source's own order."""
        o = options if options is not None else IcpRejectionOptions(**kw)
        n = len(source_points)
        idx = np.zeros(max(n, 1), dtype=np.int32)
        d2 = np.zeros(max(n, 1), dtype=np.float32)
        kept = np.zeros(max(n, 1), dtype=np.uint8)
        t = _T(transform)
        st = IcpRejectionStats()
        self._ck(lib().mm3d_debug_icp_rejection(self._h, source_points._h, target_points._h, t.ctypes.data_as(C.c_void_p),
                                                C.c_double(max_correspondence_distance), C.byref(o), int(split),
                                                idx.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p),
                                                kept.ctypes.data_as(C.c_void_p), C.byref(st)))
        return idx[:n], d2[:n], kept[:n].astype(bool), st.as_dict()

    def debugIcpGeometry(self, source_points, source_normals, target_points, target_normals, transform, max_correspondence_distance,
                         rejection=None, geometry=None, split=1):
        """mm3d_debug_icp_geometry: one iteration's correspondence stage with step 1b at `transform`.  Returns (idx int32[n], d2
        float32[n], reason uint8[n], rejection stats dict, geometry stats dict) in the source's own order."""
        ro = rejection if rejection is not None else IcpRejectionOptions()
        go = geometry if geometry is not None else IcpGeometryOptions()
        n = len(source_points)
        idx = np.zeros(max(n, 1), dtype=np.int32)
        d2 = np.zeros(max(n, 1), dtype=np.float32)
        reason = np.zeros(max(n, 1), dtype=np.uint8)
        t = _T(transform)
        rs, gs = IcpRejectionStats(), IcpGeometryStats()
        self._ck(lib().mm3d_debug_icp_geometry(
            self._h, source_points._h, source_normals._h if source_normals is not None else None, target_points._h,
            target_normals._h if target_normals is not None else None, t.ctypes.data_as(C.c_void_p),
            C.c_double(max_correspondence_distance), C.byref(ro), C.byref(go), int(split), idx.ctypes.data_as(C.c_void_p),
            d2.ctypes.data_as(C.c_void_p), reason.ctypes.data_as(C.c_void_p), C.byref(rs), C.byref(gs)))
        return idx[:n], d2[:n], reason[:n], rs.as_dict(), gs.as_dict()

    def debugIcpRobust(self, source_points, target_points, target_normals, transform, max_correspondence_distance, options=None, k=0,
                       split=1, **kw):
        """mm3d_debug_icp_robust: iteration k's search, weights and sums at `transform`, without the finalize.  Returns (idx
        int32[n], d2 float32[n], weight float64[n], sums float64[19 or 32], stats dict) in the source's own order."""
        o = options if options is not None else IcpRobustOptions(**kw)
        n = len(source_points)
        idx = np.zeros(max(n, 1), dtype=np.int32)
        d2 = np.zeros(max(n, 1), dtype=np.float32)
        w = np.zeros(max(n, 1), dtype=np.float64)
        sums = np.zeros(32 if target_normals is not None else 19, dtype=np.float64)
        t = _T(transform)
        st = IcpRobustStats()
        self._ck(lib().mm3d_debug_icp_robust(self._h, source_points._h, target_points._h,
                                             target_normals._h if target_normals is not None else None, t.ctypes.data_as(C.c_void_p),
                                             C.c_double(max_correspondence_distance), C.byref(o), int(k), int(split),
                                             idx.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p),
                                             sums.ctypes.data_as(C.c_void_p), C.byref(st)))
        return idx[:n], d2[:n], w[:n], sums, st.as_dict()

    def transformScore(self, source_points, target_points, transform, max_distance) -> float:
        t = _T(transform)
        s = C.c_double()
        self._ck(lib().mm3d_transform_score(self._h, source_points._h, target_points._h, t.ctypes.data_as(C.c_void_p),
                                            C.c_double(max_distance), C.byref(s)))
        return s.value

    # ---- map_merging.h ---------------------------------------------------------------------
    def estimateMapsTransforms(self, clouds, params: MapMergingParams, return_pairs: bool = False):
        """clouds: list of host numpy POINT arrays (or (ptr, n) tuples for HBM-resident inputs)."""
        n = len(clouds)
        keep = []
        views = (_View * max(n, 1))()
        for i, c in enumerate(clouds):
            if isinstance(c, tuple):                      # (ptr, n) packed 16-byte records, or (ptr, n, stride, rgba_offset)
                views[i] = _View(C.c_void_p(c[0]), c[1], c[2] if len(c) > 2 else 16, c[3] if len(c) > 3 else 12)
            else:
                a = np.ascontiguousarray(c, dtype=POINT)
                keep.append(a)
                views[i] = _View(a.ctypes.data_as(C.c_void_p), len(a), 16, 12)
        out = np.zeros((max(n, 1), 16), dtype=np.float32)
        pairs = np.zeros(max(n * (n - 1) // 2, 1), dtype=PAIR)
        n_out, n_pairs = C.c_size_t(), C.c_size_t()
        self._ck(lib().mm3d_estimate_maps_transforms(self._h, views, C.c_size_t(n), C.byref(params),
                                                     out.ctypes.data_as(C.c_void_p), C.byref(n_out),
                                                     pairs.ctypes.data_as(C.c_void_p), C.byref(n_pairs)))
        res = [_Tout(out[i]) for i in range(n_out.value)]
        return (res, pairs[:n_pairs.value].copy()) if return_pairs else res

    def composeMaps(self, clouds, transforms, resolution: float):
        n = len(clouds)
        if n == 0:
            return None                                  # nullptr (map_merging.h:97)
        if n != len(transforms):
            # the reference throws (R/src/map_merging.cpp:285-288)
            raise RuntimeError("composeMaps: clouds and transforms size must be the same.")
        arr = (C.c_void_p * n)(*[c._h for c in clouds])
        tr = np.ascontiguousarray(np.stack([_T(t) for t in transforms]))
        h = C.c_void_p()
        self._ck(lib().mm3d_compose_maps(self._h, arr, C.c_size_t(n), tr.ctypes.data_as(C.c_void_p), C.c_size_t(n),
                                         C.c_double(resolution), C.byref(h)))
        return Cloud(self, h)

    # ---- shardable pieces ------------------------------------------------------------------
    def mapFeatures(self, raw: "Cloud", params: MapMergingParams) -> "Map":
        h = C.c_void_p()
        self._ck(lib().mm3d_map_features(self._h, raw._h, C.byref(params), C.byref(h)))
        return Map(self, h)

    def mapFromParts(self, points: "Cloud", keypoints: "Cloud", desc: "Descriptors") -> "Map":
        h = C.c_void_p()
        self._ck(lib().mm3d_map_from_parts(self._h, points._h, keypoints._h, desc._h, C.byref(h)))
        for o in (points, keypoints, desc):
            o._owned = False                             # the map owns them now
        return Map(self, h)

    def mapPrepare(self, m: "Map", params: MapMergingParams) -> None:
        """mm3d_map_prepare: build the map's search structures now, so that pair estimates only read it
        (and may then run on several contexts at once)."""
        self._ck(lib().mm3d_map_prepare(self._h, m._h, C.byref(params)))

    def pairEstimate(self, source: "Map", target: "Map", params: MapMergingParams, execute: bool = True):
        r = np.zeros(1, dtype=PAIR)
        self._ck(lib().mm3d_pair_estimate(self._h, source._h, target._h, C.byref(params), int(execute),
                                          r.ctypes.data_as(C.c_void_p)))
        return r[0]

    def pairsSkip(self, sources, targets, params: MapMergingParams):
        """Replays the rand() draws of pairs this context does not execute (one call for the whole run)."""
        n = len(sources)
        if n == 0:
            return
        a = (C.c_void_p * n)(*[m._h for m in sources])
        b = (C.c_void_p * n)(*[m._h for m in targets])
        self._ck(lib().mm3d_pairs_skip(self._h, a, b, C.c_size_t(n), C.byref(params)))

    def shardBegin(self, clouds, params: MapMergingParams, rank: int, world: int) -> "Shard":
        """mm3d_shard_begin: the per-cloud loop for the maps `rank` owns, on this context's streams.
        clouds: host POINT arrays or (device ptr, n) tuples, all n of them (only the owned ones are read)."""
        n = len(clouds)
        keep = []
        views = (_View * max(n, 1))()
        for i, c in enumerate(clouds):
            if isinstance(c, tuple):
                views[i] = _View(C.c_void_p(c[0]), c[1], 16, 12)
            else:
                a = np.ascontiguousarray(c, dtype=POINT)
                keep.append(a)
                views[i] = _View(a.ctypes.data_as(C.c_void_p), len(a), 16, 12)
        h = C.c_void_p()
        self._ck(lib().mm3d_shard_begin(self._h, views, C.c_size_t(n), C.byref(params), int(rank), int(world), C.byref(h)))
        return Shard(self, h, n, int(params.descriptor_type))

    # ---- measurement -----------------------------------------------------------------------
    def profile(self, on: bool):
        self._ck(lib().mm3d_profile_enable(self._h, int(on)))

    def profile_reset(self):
        lib().mm3d_profile_reset(self._h)

    def profile_entries(self):
        out = {}
        for i in range(lib().mm3d_profile_count(self._h)):
            name, ms, n, b = C.c_char_p(), C.c_double(), C.c_uint64(), C.c_double()
            lib().mm3d_profile_entry(self._h, i, C.byref(name), C.byref(ms), C.byref(n), C.byref(b))
            out[name.value.decode()] = {"ms": ms.value, "launches": n.value, "bytes": b.value}
        return out


class Shard:
    """One rank's part of estimateMapsTransforms on N processes (include/mm3d.h, mm3d_shard_*)."""

    def __init__(self, ctx: "Context", h, n: int, descriptor_type: int):
        self._ctx, self._h, self.n, self.descriptor_type = ctx, h, n, descriptor_type

    def bundleSizes(self):
        """(n_points[n], n_keypoints[n]) of the maps this rank owns, zero elsewhere."""
        a, b = np.zeros(self.n, dtype=np.uint64), np.zeros(self.n, dtype=np.uint64)
        self._ctx._ck(lib().mm3d_shard_bundle_sizes(self._h, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))
        return a, b

    def bundleBytes(self, n_points: int, n_keypoints: int) -> int:
        f = lib().mm3d_shard_bundle_bytes
        f.restype = C.c_size_t
        return int(f(C.c_uint64(int(n_points)), C.c_uint64(int(n_keypoints)), int(self.descriptor_type)))

    def pack(self, i: int, dst_ptr: int):
        self._ctx._ck(lib().mm3d_shard_pack(self._h, C.c_size_t(i), C.c_void_p(dst_ptr)))

    def unpack(self, i: int, src_ptr: int, n_points: int, n_keypoints: int):
        self._ctx._ck(lib().mm3d_shard_unpack(self._h, C.c_size_t(i), C.c_void_p(src_ptr), C.c_uint64(int(n_points)),
                                              C.c_uint64(int(n_keypoints))))

    def unpackMany(self, items):
        """items: (map index, source pointer, n_points, n_keypoints) of the maps other ranks own; on the context's streams."""
        n = len(items)
        if n == 0:
            return
        maps = (C.c_size_t * n)(*[int(i[0]) for i in items])
        srcs = (C.c_void_p * n)(*[int(i[1]) for i in items])
        a = (C.c_uint64 * n)(*[int(i[2]) for i in items])
        b = (C.c_uint64 * n)(*[int(i[3]) for i in items])
        self._ctx._ck(lib().mm3d_shard_unpack_many(self._h, C.c_size_t(n), maps, srcs, a, b))

    def pairs(self):
        """(records of every live pair in the reference's order, mine[q]): the pairs whose target this rank owns
        are estimated, the other slots carry only the pair's indices."""
        cap = max(self.n * (self.n - 1) // 2, 1)
        rec = np.zeros(cap, dtype=PAIR)
        mine = np.zeros(cap, dtype=np.uint8)
        n = C.c_size_t()
        self._ctx._ck(lib().mm3d_shard_pairs(self._h, rec.ctypes.data_as(C.c_void_p), mine.ctypes.data_as(C.c_void_p),
                                             C.c_size_t(cap), C.byref(n)))
        return rec[:n.value].copy(), mine[:n.value].astype(bool)

    def end(self):
        if self._h:
            lib().mm3d_shard_end(self._h)
            self._h = None


def shardMapOwner(i: int, world: int) -> int:
    return int(lib().mm3d_shard_map_owner(C.c_size_t(i), int(world)))


def globalTransforms(pairs, confidence_threshold: float, n_clouds: int):
    """computeGlobalTransforms (R/src/map_merging.cpp:153-186); host only."""
    pairs = np.ascontiguousarray(pairs, dtype=PAIR)
    out = np.zeros((max(n_clouds, 1), 16), dtype=np.float32)
    n_out = C.c_size_t()
    st = lib().mm3d_global_transforms(pairs.ctypes.data_as(C.c_void_p), C.c_size_t(len(pairs)),
                                      C.c_double(confidence_threshold), C.c_size_t(n_clouds),
                                      out.ctypes.data_as(C.c_void_p), C.byref(n_out))
    if st != 0:
        raise Mm3dError(st, "mm3d_global_transforms")
    return [_Tout(out[i]) for i in range(n_out.value)]


class _Obj:
    _free = None

    def __init__(self, ctx: Context, h, owned=True):
        self.ctx, self._h, self._owned = ctx, h, owned

    def free(self):
        if self._h and self._owned and self.ctx._h:
            getattr(lib(), self._free)(self.ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Cloud(_Obj):
    _free = "mm3d_cloud_free"

    def __len__(self):
        return lib().mm3d_cloud_size(self._h)

    def numpy(self) -> np.ndarray:
        out = np.empty(len(self), dtype=POINT)
        self.ctx._ck(lib().mm3d_cloud_download(self.ctx._h, self._h, out.ctypes.data_as(C.c_void_p), C.c_size_t(16),
                                               C.c_size_t(12)))
        return out


class Normals(_Obj):
    _free = "mm3d_normals_free"

    def __len__(self):
        return lib().mm3d_normals_size(self._h)

    def numpy(self) -> np.ndarray:
        out = np.empty(len(self), dtype=NORMAL)
        self.ctx._ck(lib().mm3d_normals_download(self.ctx._h, self._h, out.ctypes.data_as(C.c_void_p), C.c_size_t(16)))
        return out


class Descriptors(_Obj):
    _free = "mm3d_desc_free"

    def __len__(self):
        return lib().mm3d_desc_size(self._h)

    @property
    def dim(self):
        return lib().mm3d_desc_dim(self._h)

    def numpy(self) -> np.ndarray:
        out = np.empty((len(self), self.dim), dtype=np.float32)
        self.ctx._ck(lib().mm3d_desc_download(self.ctx._h, self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def frames(self) -> np.ndarray:
        """SHOT only: the local reference frames [n, 9] (x, y, z axes), the rf field of pcl::SHOT1344."""
        out = np.empty((len(self), 9), dtype=np.float32)
        self.ctx._ck(lib().mm3d_desc_download_frames(self.ctx._h, self._h, out.ctypes.data_as(C.c_void_p)))
        return out


class Map(_Obj):
    _free = "mm3d_map_free"

    @property
    def points(self) -> Cloud:
        return Cloud(self.ctx, C.c_void_p(lib().mm3d_map_points(self._h)), owned=False)

    @property
    def keypoints(self) -> Cloud:
        return Cloud(self.ctx, C.c_void_p(lib().mm3d_map_keypoints(self._h)), owned=False)

    @property
    def descriptors(self) -> Descriptors:
        return Descriptors(self.ctx, C.c_void_p(lib().mm3d_map_descriptors(self._h)), owned=False)

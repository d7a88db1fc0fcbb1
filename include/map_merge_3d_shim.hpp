// map_merge_3d_shim.hpp -- the reference-side binding a maintainer adds to use libmm3d.so.
//
// Drop-in for the static library `map_merging` (R/CMakeLists.txt:67-74): it defines the SAME free
// functions with the SAME signatures as R/include/map_merge_3d/{features,matching,map_merging}.h
// and forwards each to the C ABI of include/mm3d.h.  map_merge_node.cpp, map_merge_tool.cpp and
// registration_visualisation.cpp compile unchanged against the reference's own headers and link
// this translation unit + libmm3d.so instead of features.cpp / matching.cpp / map_merging.cpp /
// graph.cpp.  Needs PCL and ROS headers (the reference's headers include them), so it is compiled
// only where they exist; this image has neither, hence the __has_include guard.
//
//   g++ -std=c++14 -I<ref>/include -Iinclude -DMM3D_SHIM_IMPLEMENTATION -c mm3d_shim.cpp   (a .cpp that
//   includes this header once), then link with -lmm3d.
#pragma once

#include <cmath>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "mm3d.h"

namespace map_merge_3d
{
namespace mm3d_shim
{
// MM3D_KEYPOINTS=uniform or uniform:<leaf in metres>: the estimation context's maps take uniform keypoints instead of the
// reference's detectors (mm3d_set_keypoints; without a leaf, the library's default fraction of descriptor_radius); reference
// or unset keeps the detectors.  Anything else throws, as a malformed MM3D_ICP or MM3D_ALIGN does.  (Outside the guard below:
// it needs neither PCL nor ROS, so it is checked where the rest of this header cannot be compiled.)
inline mm3d_keypoint_options parse_keypoints(const char *value)
{
  mm3d_keypoint_options o;
  o.source = MM3D_KEYPOINTS_REFERENCE;
  o.leaf = 0.0;
  const std::string v = value ? value : "";
  if (v.empty() || v == "reference") return o;
  bool ok = v.compare(0, 7, "uniform") == 0 && (v.size() == 7 || v[7] == ':');
  if (ok && v.size() > 7) {
    const char *s = v.c_str() + 8;
    char *end = nullptr;
    o.leaf = std::strtod(s, &end);
    ok = end != s && *end == '\0' && std::isfinite(o.leaf) && o.leaf > 0.0;
  }
  if (!ok) throw std::runtime_error("mm3d: MM3D_KEYPOINTS must be reference, uniform or uniform:<leaf in metres>, not '" + v + "'");
  o.source = MM3D_KEYPOINTS_UNIFORM;
  return o;
}
// MM3D_OUTLIERS=statistical, statistical:<mean_k> or statistical:<mean_k>:<stddev_mult>: the estimation context's maps are filtered
// by the statistical rule instead of the reference's radius filter (mm3d_set_outlier_filter; what is not given keeps
// mm3d_outlier_options_default's value, 16 and 2.0); reference or unset keeps removeOutliers.  Anything else throws.
inline mm3d_outlier_options parse_outliers(const char *value)
{
  mm3d_outlier_options o;
  o.method = MM3D_OUTLIERS_RADIUS;
  o.mean_k = 16;
  o.stddev_mult = 2.0;
  const std::string v = value ? value : "";
  if (v.empty() || v == "reference") return o;
  bool ok = v.compare(0, 11, "statistical") == 0 && (v.size() == 11 || v[11] == ':');
  if (ok && v.size() > 11) {
    const char *s = v.c_str() + 12;
    char *end = nullptr;
    const long k = std::strtol(s, &end, 10);
    ok = end != s && (*end == '\0' || *end == ':') && k >= 1 && k <= 64 && *s >= '0' && *s <= '9';
    o.mean_k = (int)k;
    if (ok && *end == ':') {
      s = end + 1;
      o.stddev_mult = std::strtod(s, &end);
      ok = end != s && *end == '\0' && std::isfinite(o.stddev_mult) && o.stddev_mult >= 0.0 && ((*s >= '0' && *s <= '9') || *s == '.');
    }
  }
  if (!ok)
    throw std::runtime_error("mm3d: MM3D_OUTLIERS must be reference, statistical, statistical:<mean_k 1 .. 64> or "
                             "statistical:<mean_k>:<stddev_mult >= 0>, not '" + v + "'");
  o.method = MM3D_OUTLIERS_STATISTICAL;
  return o;
}
// MM3D_CLUSTERS=min_size:<n>, min_size:<n>:<tolerance> or largest[:<tolerance>]: the small connected components of the estimation
// context's filtered maps are dropped (mm3d_set_cluster_filter; min_size alone keeps mm3d_cluster_options_default's 100, no
// tolerance means twice params.resolution); off or unset runs nothing.  Anything else throws.
inline mm3d_cluster_options parse_clusters(const char *value)
{
  mm3d_cluster_options o;
  o.method = MM3D_CLUSTERS_OFF;
  o.min_size = 100;
  o.tolerance = 0.0;
  const std::string v = value ? value : "";
  if (v.empty() || v == "off") return o;
  const bool largest = v.compare(0, 7, "largest") == 0 && (v.size() == 7 || v[7] == ':');
  const bool min_size = v.compare(0, 8, "min_size") == 0 && (v.size() == 8 || v[8] == ':');
  bool ok = largest || min_size;
  const size_t head = largest ? 7 : 8;
  if (ok && v.size() > head) {
    const char *s = v.c_str() + head + 1;
    char *end = nullptr;
    bool more = largest;                     // (largest: the tolerance is the only field)
    if (min_size) {
      const long k = std::strtol(s, &end, 10);
      ok = end != s && (*end == '\0' || *end == ':') && k >= 1 && k <= 2147483647L && *s >= '0' && *s <= '9';
      o.min_size = (int)k;
      more = ok && *end == ':';
      if (more) s = end + 1;
    }
    if (ok && more) {
      o.tolerance = std::strtod(s, &end);
      ok = end != s && *end == '\0' && std::isfinite(o.tolerance) && o.tolerance > 0.0 && ((*s >= '0' && *s <= '9') || *s == '.');
    }
  }
  if (!ok)
    throw std::runtime_error("mm3d: MM3D_CLUSTERS must be off, min_size:<n >= 1>, min_size:<n>:<tolerance > 0>, largest or "
                             "largest:<tolerance>, not '" + v + "'");
  o.method = largest ? MM3D_CLUSTERS_LARGEST : MM3D_CLUSTERS_MIN_SIZE;
  return o;
}
// MM3D_SMOOTH=mls, mls:<order> or mls:<order>:<radius>, each with @maps or @composed behind it if only one place is meant: moving
// least squares smooths the estimation context's filtered maps before their normals, and the composed map between two voxel
// passes (mm3d_set_smoothing; mls alone keeps mm3d_smooth_options_default's order 2, no radius means three times the resolution in
// force); off or unset runs nothing.  Anything else throws.
inline mm3d_smooth_options parse_smooth(const char *value)
{
  mm3d_smooth_options o;
  o.method = MM3D_SMOOTH_OFF;
  o.order = 2;
  o.min_neighbours = 6;
  o.where = MM3D_SMOOTH_MAPS | MM3D_SMOOTH_COMPOSED;
  o.radius = 0.0;
  const std::string v = value ? value : "";
  if (v.empty() || v == "off") return o;
  std::string head = v;
  const size_t at = v.find('@');
  bool ok = true;
  if (at != std::string::npos) {
    const std::string where = v.substr(at + 1);
    head = v.substr(0, at);
    if (where == "maps") o.where = MM3D_SMOOTH_MAPS;
    else if (where == "composed") o.where = MM3D_SMOOTH_COMPOSED;
    else ok = false;
  }
  ok = ok && head.compare(0, 3, "mls") == 0 && (head.size() == 3 || head[3] == ':');
  if (ok && head.size() > 3) {
    const char *s = head.c_str() + 4;
    char *end = nullptr;
    const long k = std::strtol(s, &end, 10);
    ok = end == s + 1 && (*end == '\0' || *end == ':') && (k == 1 || k == 2);
    o.order = (int)k;
    if (ok && *end == ':') {
      s = end + 1;
      o.radius = std::strtod(s, &end);
      ok = end != s && *end == '\0' && std::isfinite(o.radius) && o.radius > 0.0 && ((*s >= '0' && *s <= '9') || *s == '.');
    }
  }
  if (!ok)
    throw std::runtime_error("mm3d: MM3D_SMOOTH must be off, mls, mls:<order 1 or 2> or mls:<order>:<radius > 0>, with @maps or "
                             "@composed behind it at the most, not '" + v + "'");
  o.method = MM3D_SMOOTH_MLS;
  return o;
}
// MM3D_PLANES=remove or set_aside, then :<max_planes> and :<distance> if given, then @<x>,<y>,<z>,<degrees> or @any at most: the
// dominant planes of the estimation context's filtered maps leave, or are set aside while MM3D_CLUSTERS looks at the rest
// (mm3d_set_planes; what is not given keeps mm3d_plane_options_default's value: one plane, half of params.resolution, within 10
// degrees of z); off or unset runs nothing.  Anything else throws.
inline mm3d_plane_options parse_planes(const char *value)
{
  mm3d_plane_options o;
  o.method = MM3D_PLANES_OFF;
  o.max_planes = 1; o.samples = 1024; o.refit = 1; o.seed = 1u;
  o.distance = 0.0; o.min_fraction = 0.05;
  o.axis[0] = 0.0; o.axis[1] = 0.0; o.axis[2] = 1.0;
  o.max_angle_deg = 10.0;
  const std::string v = value ? value : "";
  if (v.empty() || v == "off") return o;
  const size_t at = v.find('@');
  const std::string head = v.substr(0, at), tail = at == std::string::npos ? "" : v.substr(at + 1);
  const bool remove = head.compare(0, 6, "remove") == 0 && (head.size() == 6 || head[6] == ':');
  const bool aside = head.compare(0, 9, "set_aside") == 0 && (head.size() == 9 || head[9] == ':');
  bool ok = remove || aside;
  const size_t name = remove ? 6 : 9;
  auto digit = [](char c) { return c >= '0' && c <= '9'; };
  if (ok && head.size() > name) {
    const char *s = head.c_str() + name + 1;
    char *end = nullptr;
    const long k = std::strtol(s, &end, 10);
    ok = end != s && (*end == '\0' || *end == ':') && k >= 1 && k <= 8 && digit(*s);
    o.max_planes = (int)k;
    if (ok && *end == ':') {
      s = end + 1;
      o.distance = std::strtod(s, &end);
      ok = end != s && *end == '\0' && std::isfinite(o.distance) && o.distance > 0.0 && (digit(*s) || *s == '.');
    }
  }
  if (ok && at != std::string::npos) {
    if (tail == "any") o.axis[2] = 0.0;
    else {
      double f[4];
      const char *s = tail.c_str();
      for (int k = 0; ok && k < 4; ++k) {
        char *end = nullptr;
        f[k] = std::strtod(s, &end);
        ok = end != s && std::isfinite(f[k]) && (digit(*s) || *s == '.' || *s == '-') && *end == (k < 3 ? ',' : '\0');
        s = end + 1;
      }
      ok = ok && (f[0] != 0.0 || f[1] != 0.0 || f[2] != 0.0) && f[3] >= 0.0 && f[3] <= 90.0;
      if (ok) { o.axis[0] = f[0]; o.axis[1] = f[1]; o.axis[2] = f[2]; o.max_angle_deg = f[3]; }
    }
  }
  if (!ok)
    throw std::runtime_error("mm3d: MM3D_PLANES must be off, remove or set_aside, then :<max_planes 1 .. 8> and :<distance > 0> if "
                             "wanted, then @<x>,<y>,<z>,<degrees 0 .. 90> or @any at most, not '" + v + "'");
  o.method = remove ? MM3D_PLANES_REMOVE : MM3D_PLANES_SET_ASIDE;
  return o;
}
// MM3D_REFINE=ndt or ndt:<resolution in metres>: the estimation context's pair stage refines with NDT in the ICP's place
// (mm3d_set_refinement; without a resolution, the library's default multiple of params.resolution; the other options keep
// mm3d_refine_options_default's values); icp or unset keeps the ICP that MM3D_ICP selects.  Anything else throws.
inline mm3d_refine_options parse_refine(const char *value)
{
  mm3d_refine_options o;
  o.method = MM3D_REFINE_ICP;
  o.resolution = 0.0;
  o.neighbours = 7;
  o.min_points = 6;
  o.regularisation = 0.01;
  const std::string v = value ? value : "";
  if (v.empty() || v == "icp") return o;
  bool ok = v.compare(0, 3, "ndt") == 0 && (v.size() == 3 || v[3] == ':');
  if (ok && v.size() > 3) {
    const char *s = v.c_str() + 4;
    char *end = nullptr;
    o.resolution = std::strtod(s, &end);
    ok = end != s && *end == '\0' && std::isfinite(o.resolution) && o.resolution > 0.0;
  }
  if (!ok) throw std::runtime_error("mm3d: MM3D_REFINE must be icp, ndt or ndt:<resolution in metres>, not '" + v + "'");
  o.method = MM3D_REFINE_NDT;
  return o;
}
// MM3D_COARSE=correlative or correlative:<cell in metres>: the estimation context's pairs take their initial estimate from the
// correlative yaw / shift search (mm3d_set_coarse_alignment; without a cell, the library's default multiple of
// params.resolution; the other options keep mm3d_coarse_options_default's values); none or unset keeps the estimate that
// estimation_method and MM3D_ALIGN select.  Anything else throws.
inline mm3d_coarse_options parse_coarse(const char *value)
{
  mm3d_coarse_options o;
  mm3d_coarse_options_default(&o);
  const std::string v = value ? value : "";
  if (v.empty() || v == "none") return o;
  bool ok = v.compare(0, 11, "correlative") == 0 && (v.size() == 11 || v[11] == ':');
  if (ok && v.size() > 11) {
    const char *s = v.c_str() + 12;
    char *end = nullptr;
    o.cell = std::strtod(s, &end);
    ok = end != s && *end == '\0' && std::isfinite(o.cell) && o.cell > 0.0;
  }
  if (!ok) throw std::runtime_error("mm3d: MM3D_COARSE must be none, correlative or correlative:<cell in metres>, not '" + v + "'");
  o.method = MM3D_COARSE_CORRELATIVE;
  return o;
}
// MM3D_CONFIDENCE=overlap or overlap:<voxel in metres>: the estimation context's pair records carry the overlap confidence, a
// fraction in [0, 1] that confidence_threshold is then compared with (mm3d_set_confidence; without a voxel, the library's
// default multiple of params.resolution; the other options keep mm3d_confidence_options_default's values); none or unset
// keeps the reference's 1 / transformScore.  Anything else throws.
inline mm3d_confidence_options parse_confidence(const char *value)
{
  mm3d_confidence_options o;
  o.method = MM3D_CONFIDENCE_REFERENCE;
  o.voxel = 0.0;
  o.min_points = 8;
  o.min_overlap = 0.05;
  o.view_margin = 0;
  const std::string v = value ? value : "";
  if (v.empty() || v == "none") return o;
  bool ok = v.compare(0, 7, "overlap") == 0 && (v.size() == 7 || v[7] == ':');
  if (ok && v.size() > 7) {
    const char *s = v.c_str() + 8;
    char *end = nullptr;
    o.voxel = std::strtod(s, &end);
    ok = end != s && *end == '\0' && std::isfinite(o.voxel) && o.voxel > 0.0;
  }
  if (!ok) throw std::runtime_error("mm3d: MM3D_CONFIDENCE must be none, overlap or overlap:<voxel in metres>, not '" + v + "'");
  o.method = MM3D_CONFIDENCE_OVERLAP;
  return o;
}
// Not available on a device list (its bundles carry no tables): overlap with MM3D_DEVICES set as well throws.
inline void check_confidence_devices(const mm3d_confidence_options &o, const char *devices)
{
  if (o.method == MM3D_CONFIDENCE_OVERLAP && devices && *devices)
    throw std::runtime_error("mm3d: MM3D_CONFIDENCE=overlap is not available with MM3D_DEVICES (a device list carries no tables)");
}
// MM3D_ICP_REJECT=<term>[+<term>...]: the estimation context's ICP rejects correspondences (mm3d_set_icp_rejection).  Terms:
// one_to_one, trimmed[:<overlap ratio in (0, 1]>], median[:<factor > 0>]; without a value, mm3d_icp_rejection_options_default's
// (0.5, 1.0).  none or unset rejects nothing.  trimmed and median together, a term twice, an unknown term or a value out of
// range throw, as a malformed MM3D_ICP does.
inline mm3d_icp_rejection_options parse_icp_reject(const char *value)
{
  mm3d_icp_rejection_options o;
  o.one_to_one = 0;
  o.distance = MM3D_REJECT_NONE;
  o.overlap_ratio = 0.5;
  o.min_correspondences = 0;
  o.median_factor = 1.0;
  const std::string v = value ? value : "";
  if (v.empty() || v == "none") return o;
  bool ok = true;
  for (size_t a = 0; ok && a <= v.size();) {
    size_t b = v.find('+', a);
    if (b == std::string::npos) b = v.size();
    const std::string term = v.substr(a, b - a);
    const size_t colon = term.find(':');
    const std::string name = term.substr(0, colon);
    double x = 0.0;
    if (colon != std::string::npos) {
      const char *s = term.c_str() + colon + 1;
      char *end = nullptr;
      x = std::strtod(s, &end);
      ok = end != s && *end == '\0' && std::isfinite(x) && x > 0.0;
    }
    if (name == "one_to_one") {
      ok = ok && colon == std::string::npos && !o.one_to_one;
      o.one_to_one = 1;
    } else if (name == "trimmed") {
      ok = ok && o.distance == MM3D_REJECT_NONE && (colon == std::string::npos || x <= 1.0);
      o.distance = MM3D_REJECT_TRIMMED;
      if (colon != std::string::npos) o.overlap_ratio = x;
    } else if (name == "median") {
      ok = ok && o.distance == MM3D_REJECT_NONE;
      o.distance = MM3D_REJECT_MEDIAN;
      if (colon != std::string::npos) o.median_factor = x;
    } else {
      ok = false;
    }
    a = b + 1;
  }
  if (!ok)
    throw std::runtime_error("mm3d: MM3D_ICP_REJECT must be none or terms joined by '+' out of one_to_one, trimmed[:<ratio>], "
                             "median[:<factor>] (trimmed and median exclude each other), not '" + v + "'");
  return o;
}
// Not available on a device list (its devices' pair loops run the ICP without rejection): an active value with MM3D_DEVICES throws.
inline void check_icp_reject_devices(const mm3d_icp_rejection_options &o, const char *devices)
{
  if ((o.one_to_one || o.distance != MM3D_REJECT_NONE) && devices && *devices)
    throw std::runtime_error("mm3d: MM3D_ICP_REJECT is not available with MM3D_DEVICES (a device list runs the ICP without rejection)");
}
// MM3D_ICP_REJECT_GEOMETRY=<term>[+<term>]: the estimation context's ICP drops correspondences by the maps' geometry
// (mm3d_set_icp_geometry_rejection).  Terms: boundary[:<radius in metres > 0>] (without a value: params.normal_radius),
// normals[:<degrees in (0, 90]>] (without a value: mm3d_icp_geometry_options_default's 45).  none or unset selects nothing.  A term
// twice, an unknown term or a value out of range throw, as a malformed MM3D_ICP_REJECT does.
inline mm3d_icp_geometry_options parse_icp_reject_geometry(const char *value)
{
  mm3d_icp_geometry_options o;
  o.boundary = 0;
  o.boundary_radius = 0.0;
  o.boundary_angle_deg = 90.0;
  o.boundary_min_neighbours = 3;
  o.normals = 0;
  o.normal_angle_deg = 45.0;
  const std::string v = value ? value : "";
  if (v.empty() || v == "none") return o;
  bool ok = true;
  for (size_t a = 0; ok && a <= v.size();) {
    size_t b = v.find('+', a);
    if (b == std::string::npos) b = v.size();
    const std::string term = v.substr(a, b - a);
    const size_t colon = term.find(':');
    const std::string name = term.substr(0, colon);
    double x = 0.0;
    if (colon != std::string::npos) {
      const char *s = term.c_str() + colon + 1;
      char *end = nullptr;
      x = std::strtod(s, &end);
      ok = end != s && *end == '\0' && std::isfinite(x) && x > 0.0;
    }
    if (name == "boundary") {
      ok = ok && !o.boundary;
      o.boundary = 1;
      if (colon != std::string::npos) o.boundary_radius = x;
    } else if (name == "normals") {
      ok = ok && !o.normals && (colon == std::string::npos || x <= 90.0);
      o.normals = 1;
      if (colon != std::string::npos) o.normal_angle_deg = x;
    } else {
      ok = false;
    }
    a = b + 1;
  }
  if (!ok)
    throw std::runtime_error("mm3d: MM3D_ICP_REJECT_GEOMETRY must be none or terms joined by '+' out of boundary[:<radius > 0>], "
                             "normals[:<degrees in (0, 90]>], not '" + v + "'");
  return o;
}
// Not available on a device list (its bundles carry neither normals nor flags): an active value with MM3D_DEVICES throws.  The
// other combinations the library refuses (coloured, generalized and robust ICP; normals with MM3D_ICP_SAMPLE) throw where the
// value is set, with the library's text.
inline void check_icp_reject_geometry_devices(const mm3d_icp_geometry_options &o, const char *devices)
{
  if ((o.boundary || o.normals) && devices && *devices)
    throw std::runtime_error("mm3d: MM3D_ICP_REJECT_GEOMETRY is not available with MM3D_DEVICES (a device list carries no normals or flags)");
}
// MM3D_ICP_ROBUST=<kernel>[:<scale>[:<scale_start>[:<anneal>[:<tuning>]]]]: the estimation context's ICP weights its correspondences
// (mm3d_set_icp_robust).  Kernels: l2, huber, cauchy, tukey, geman_mcclure; a value left out is
// mm3d_icp_robust_options_default's (0.05, 0, 0.5, 0).  none or unset selects nothing.  An unknown kernel, an empty or malformed
// value, a value out of range or a sixth field throw, as a malformed MM3D_ICP_REJECT does.
inline mm3d_icp_robust_options parse_icp_robust(const char *value)
{
  mm3d_icp_robust_options o;
  o.kernel = MM3D_ROBUST_OFF;
  o.scale = 0.05;
  o.scale_start = 0.0;
  o.anneal = 0.5;
  o.tuning = 0.0;
  const std::string v = value ? value : "";
  if (v.empty() || v == "none") return o;
  static const char *const names[] = {"l2", "huber", "cauchy", "tukey", "geman_mcclure"};
  double *const fields[] = {&o.scale, &o.scale_start, &o.anneal, &o.tuning};
  bool ok = true;
  int field = -1;
  for (size_t a = 0; ok && a <= v.size(); ++field) {
    size_t b = v.find(':', a);
    if (b == std::string::npos) b = v.size();
    const std::string term = v.substr(a, b - a);
    if (field < 0) {
      for (int k = 0; k < 5; ++k)
        if (term == names[k]) o.kernel = MM3D_ROBUST_L2 + k;
      ok = o.kernel != MM3D_ROBUST_OFF;
    } else if (field < 4) {
      char *end = nullptr;
      const double x = std::strtod(term.c_str(), &end);
      ok = !term.empty() && *end == '\0' && std::isfinite(x) && term.find_first_not_of("0123456789.eE+-") == std::string::npos;
      *fields[field] = x;
    } else {
      ok = false;
    }
    a = b + 1;
  }
  ok = ok && o.scale > 0.0 && (o.scale_start == 0.0 || o.scale_start >= o.scale) && o.anneal > 0.0 && o.anneal <= 1.0 && o.tuning >= 0.0;
  if (!ok)
    throw std::runtime_error("mm3d: MM3D_ICP_ROBUST must be none or <l2|huber|cauchy|tukey|geman_mcclure>[:<scale > 0>[:<scale_start, 0 or >= "
                             "scale>[:<anneal in (0, 1]>[:<tuning >= 0>]]]], not '" + v + "'");
  return o;
}
// Not available on a device list (its devices' pair loops run the ICP without a kernel), nor together with an active
// MM3D_ICP_REJECT, MM3D_ICP_COLOR, MM3D_ICP_GENERALIZED or MM3D_REFINE=ndt (the robust step has point-to-point's and
// point-to-plane's terms only): each combination throws.
inline void check_icp_robust_combinations(const mm3d_icp_robust_options &o, const mm3d_icp_rejection_options &reject,
                                          const mm3d_icp_color_options &color, const mm3d_icp_generalized_options &generalized,
                                          const mm3d_refine_options &refine, const char *devices)
{
  if (o.kernel == MM3D_ROBUST_OFF) return;
  if (devices && *devices)
    throw std::runtime_error("mm3d: MM3D_ICP_ROBUST is not available with MM3D_DEVICES (a device list runs the ICP without a robust kernel)");
  if (reject.one_to_one || reject.distance != MM3D_REJECT_NONE)
    throw std::runtime_error("mm3d: MM3D_ICP_ROBUST is not available with an active MM3D_ICP_REJECT (the robust ICP has no correspondence stage)");
  if (color.enabled)
    throw std::runtime_error("mm3d: MM3D_ICP_ROBUST is not available with an active MM3D_ICP_COLOR (the robust ICP has no colour term)");
  if (generalized.enabled)
    throw std::runtime_error("mm3d: MM3D_ICP_ROBUST is not available with an active MM3D_ICP_GENERALIZED (the robust ICP has no plane-to-plane term)");
  if (refine.method == MM3D_REFINE_NDT)
    throw std::runtime_error("mm3d: MM3D_ICP_ROBUST is not available with MM3D_REFINE=ndt (NDT has no correspondences to weight)");
}
// MM3D_ICP_COLOR=1 or <lambda>[:<radius in metres>]: the estimation context's pair stage runs coloured ICP (mm3d_set_icp_color).
// 1 alone: mm3d_icp_color_options_default's lambda (0.968) -- lambda 1 itself, point-to-plane's terms, is spelt 1.0 -- and, as
// without a radius, params.normal_radius.  0, none or unset leaves it off.  A lambda outside (0, 1], a radius that is not
// positive or anything else throws, as a malformed MM3D_ICP_REJECT does.
inline mm3d_icp_color_options parse_icp_color(const char *value)
{
  mm3d_icp_color_options o;
  o.enabled = 0;
  o.lambda_geometric = 0.968;
  o.gradient_radius = 0.0;
  o.min_neighbours = 4;
  const std::string v = value ? value : "";
  if (v.empty() || v == "0" || v == "none") return o;
  o.enabled = 1;
  if (v == "1") return o;
  const size_t colon = v.find(':');
  const std::string head = v.substr(0, colon);
  char *end = nullptr;
  o.lambda_geometric = std::strtod(head.c_str(), &end);
  bool ok = !head.empty() && *end == '\0' && o.lambda_geometric > 0.0 && o.lambda_geometric <= 1.0;
  if (ok && colon != std::string::npos) {
    const char *s = v.c_str() + colon + 1;
    o.gradient_radius = std::strtod(s, &end);
    ok = end != s && *end == '\0' && std::isfinite(o.gradient_radius) && o.gradient_radius > 0.0;
  }
  if (!ok)
    throw std::runtime_error("mm3d: MM3D_ICP_COLOR must be 0, 1 or <lambda in (0, 1]>[:<radius in metres>], not '" + v + "'");
  return o;
}
// Not available on a device list (its bundles carry no gradients) nor together with an active MM3D_ICP_REJECT (the rejecting
// reduction has no colour variant): either combination throws.
inline void check_icp_color_combinations(const mm3d_icp_color_options &o, const mm3d_icp_rejection_options &reject, const char *devices)
{
  if (!o.enabled) return;
  if (devices && *devices)
    throw std::runtime_error("mm3d: MM3D_ICP_COLOR is not available with MM3D_DEVICES (a device list carries no colour gradients)");
  if (reject.one_to_one || reject.distance != MM3D_REJECT_NONE)
    throw std::runtime_error("mm3d: MM3D_ICP_COLOR is not available with an active MM3D_ICP_REJECT (the rejecting ICP has no colour term)");
}
// MM3D_ICP_GENERALIZED=1 or <epsilon>: the estimation context's pair stage runs generalized ICP (mm3d_set_icp_generalized).
// 1 alone: mm3d_icp_generalized_options_default's epsilon (1e-3) -- epsilon 1 itself is spelt 1.0.  0, none or unset leaves it
// off.  An epsilon outside (0, 1] or anything else throws, as a malformed MM3D_ICP_COLOR does.
inline mm3d_icp_generalized_options parse_icp_generalized(const char *value)
{
  mm3d_icp_generalized_options o;
  o.enabled = 0;
  o.epsilon = 1e-3;
  const std::string v = value ? value : "";
  if (v.empty() || v == "0" || v == "none") return o;
  o.enabled = 1;
  if (v == "1") return o;
  char *end = nullptr;
  o.epsilon = std::strtod(v.c_str(), &end);
  if (!(end != v.c_str() && *end == '\0' && o.epsilon > 0.0 && o.epsilon <= 1.0))
    throw std::runtime_error("mm3d: MM3D_ICP_GENERALIZED must be 0, 1 or <epsilon in (0, 1]>, not '" + v + "'");
  return o;
}
// Not available on a device list (its bundles carry no normals), nor together with an active MM3D_ICP_REJECT or an active
// MM3D_ICP_COLOR (neither has a plane-to-plane variant): each combination throws.
inline void check_icp_generalized_combinations(const mm3d_icp_generalized_options &o, const mm3d_icp_rejection_options &reject,
                                               const mm3d_icp_color_options &color, const char *devices)
{
  if (!o.enabled) return;
  if (devices && *devices)
    throw std::runtime_error("mm3d: MM3D_ICP_GENERALIZED is not available with MM3D_DEVICES (a device list carries no normals)");
  if (reject.one_to_one || reject.distance != MM3D_REJECT_NONE)
    throw std::runtime_error("mm3d: MM3D_ICP_GENERALIZED is not available with an active MM3D_ICP_REJECT (the rejecting ICP has no plane-to-plane term)");
  if (color.enabled)
    throw std::runtime_error("mm3d: MM3D_ICP_GENERALIZED is not available with an active MM3D_ICP_COLOR (coloured ICP has no plane-to-plane term)");
}
// MM3D_ESTIMATOR=consistency or consistency:<seeds>: under MATCHING the estimation context's pairs take their initial estimate
// from the consistency graph of the correspondences (mm3d_set_estimator; without a number, mm3d_estimator_options_default's 64
// seeds; tolerance and consensus keep its values, 0 = inlier_threshold and 20).  ransac or unset keeps the reference's RANSAC.
// A seed count outside 1 .. 4096 or anything else throws, as a malformed MM3D_COARSE does.
inline mm3d_estimator_options parse_estimator(const char *value)
{
  mm3d_estimator_options o;
  o.method = MM3D_ESTIMATOR_RANSAC;
  o.tolerance = 0.0;
  o.seeds = 64;
  o.consensus = 20;
  const std::string v = value ? value : "";
  if (v.empty() || v == "ransac") return o;
  bool ok = v.compare(0, 11, "consistency") == 0 && (v.size() == 11 || v[11] == ':');
  if (ok && v.size() > 11) {
    const char *s = v.c_str() + 12;
    char *end = nullptr;
    const long n = std::strtol(s, &end, 10);
    ok = end != s && *end == '\0' && *s >= '0' && *s <= '9' && n >= 1 && n <= 4096;
    if (ok) o.seeds = (int)n;
  }
  if (!ok) throw std::runtime_error("mm3d: MM3D_ESTIMATOR must be ransac, consistency or consistency:<seeds in 1 .. 4096>, not '" + v + "'");
  o.method = MM3D_ESTIMATOR_CONSISTENCY;
  return o;
}
// Not available on a device list (its devices' pair loops run RANSAC): consistency with MM3D_DEVICES set as well throws.
inline void check_estimator_devices(const mm3d_estimator_options &o, const char *devices)
{
  if (o.method == MM3D_ESTIMATOR_CONSISTENCY && devices && *devices)
    throw std::runtime_error("mm3d: MM3D_ESTIMATOR=consistency is not available with MM3D_DEVICES (a device list's pair loops run RANSAC)");
}
// MM3D_ICP_SAMPLE=normal_space:<fraction>[:<bins>] or stride:<fraction>: the estimation context's ICP searches with a sample of
// the source map (mm3d_set_icp_sampling): that fraction of its valid points, in (0, 1]; bins 1, 2, 4 or 8 cells per axis of a
// face of the normal cube (without one: mm3d_icp_sampling_options_default's 4).  A method without a fraction takes the default
// 0.25.  none or unset keeps every point.  Anything else throws, as a malformed MM3D_ICP_COLOR does.
inline mm3d_icp_sampling_options parse_icp_sample(const char *value)
{
  mm3d_icp_sampling_options o;
  o.method = MM3D_ICP_SAMPLE_NONE;
  o.fraction = 0.25;
  o.max_points = 0;
  o.bins = 4;
  const std::string v = value ? value : "";
  if (v.empty() || v == "none") return o;
  const std::string::size_type c1 = v.find(':');
  const std::string name = v.substr(0, c1);
  bool ok = name == "normal_space" || name == "stride";
  o.method = name == "stride" ? MM3D_ICP_SAMPLE_STRIDE : MM3D_ICP_SAMPLE_NORMAL_SPACE;
  if (ok && c1 != std::string::npos) {
    const std::string::size_type c2 = v.find(':', c1 + 1);
    const std::string frac = v.substr(c1 + 1, c2 == std::string::npos ? std::string::npos : c2 - c1 - 1);
    char *end = nullptr;
    o.fraction = std::strtod(frac.c_str(), &end);
    ok = !frac.empty() && end == frac.c_str() + frac.size() && o.fraction > 0.0 && o.fraction <= 1.0;
    if (ok && c2 != std::string::npos) {
      const std::string b = v.substr(c2 + 1);
      ok = o.method == MM3D_ICP_SAMPLE_NORMAL_SPACE && (b == "1" || b == "2" || b == "4" || b == "8");
      if (ok) o.bins = b[0] - '0';
    }
  }
  if (!ok)
    throw std::runtime_error("mm3d: MM3D_ICP_SAMPLE must be none, normal_space[:<fraction in (0, 1]>[:<bins 1|2|4|8>]] or stride[:<fraction>], not '" + v + "'");
  return o;
}
// Not available on a device list (its devices' pair loops search with the whole source), nor together with MM3D_REFINE=ndt, an
// active MM3D_ICP_COLOR or MM3D_ICP_GENERALIZED (none of them reads a sample): each combination throws.
inline void check_icp_sample_combinations(const mm3d_icp_sampling_options &o, const mm3d_refine_options &refine,
                                          const mm3d_icp_color_options &color, const mm3d_icp_generalized_options &generalized,
                                          const char *devices)
{
  if (o.method == MM3D_ICP_SAMPLE_NONE) return;
  if (devices && *devices)
    throw std::runtime_error("mm3d: MM3D_ICP_SAMPLE is not available with MM3D_DEVICES (a device list's pair loops search with the whole source)");
  if (refine.method == MM3D_REFINE_NDT)
    throw std::runtime_error("mm3d: MM3D_ICP_SAMPLE is not available with MM3D_REFINE=ndt (NDT searches nothing)");
  if (color.enabled)
    throw std::runtime_error("mm3d: MM3D_ICP_SAMPLE is not available with an active MM3D_ICP_COLOR (coloured ICP reads the whole source)");
  if (generalized.enabled)
    throw std::runtime_error("mm3d: MM3D_ICP_SAMPLE is not available with an active MM3D_ICP_GENERALIZED (generalized ICP reads the whole source)");
}
}  // namespace mm3d_shim
}  // namespace map_merge_3d

#if defined(__has_include)
#if __has_include(<pcl/point_cloud.h>) && __has_include(<map_merge_3d/map_merging.h>)
#define MM3D_SHIM_AVAILABLE 1
#endif
#endif

#ifdef MM3D_SHIM_AVAILABLE

#include <map_merge_3d/map_merging.h>
#include <pcl/conversions.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "mm3d.h"

namespace map_merge_3d
{
namespace mm3d_shim
{
// MM3D_DEVICES="0,1,2,3,4,5,6,7" (or "all"): the node's ONE process uses that many GPUs -- estimateMapsTransforms is then
// sharded over them inside the library, the pair records gathered by one RCCL all-gather (mm3d_create_devices); no source
// change in the node.  Otherwise one GPU: MM3D_DEVICE (default 0).
inline mm3d_ctx *make_ctx(int streams, bool may_use_device_list = false)
{
  mm3d_ctx *p = nullptr;
  const char *list = may_use_device_list ? std::getenv("MM3D_DEVICES") : nullptr;
  if (list && *list) {
    std::vector<int> devs;
    if (std::string(list) == "all") {
      for (int d = 0; d < 64; ++d) {                       // as many as exist: creation fails at the first that does not
        mm3d_ctx *probe = nullptr;
        if (mm3d_create(d, &probe) != MM3D_OK) break;
        mm3d_destroy(probe);
        devs.push_back(d);
      }
    } else {
      for (const char *q = list; *q;) {
        devs.push_back(std::atoi(q));
        while (*q && *q != ',') ++q;
        if (*q == ',') ++q;
      }
    }
    if (devs.empty() || mm3d_create_devices(devs.data(), (int)devs.size(), &p) != MM3D_OK)
      throw std::runtime_error("mm3d: MM3D_DEVICES does not name usable MI355X devices");
  } else {
    const char *d = std::getenv("MM3D_DEVICE");
    if (mm3d_create(d ? std::atoi(d) : 0, &p) != MM3D_OK) throw std::runtime_error("mm3d: no MI355X device");
  }
  (void)mm3d_set_streams(p, streams);
  return p;
}
// Two engines per process, created on first use (the reference functions are stateless free
// functions; a context only caches device memory and carries the rand() replay).  A context
// serialises its calls, and the node runs mapCompositing (0.3 Hz) beside transformsEstimation
// (0.01 Hz, seconds long) under a MultiThreadedSpinner (R/src/map_merge_node.cpp:32-40,264-265),
// so composeMaps has a context of its own and never queues behind an estimation.
inline mm3d_ctx *ctx()
{
  // estimateMapsTransforms deals its per-cloud and per-pair loops to 16 HIP streams inside the
  // library (same bits as one stream, about twice the throughput); MM3D_STREAMS overrides
  // MM3D_MAP_CACHE=<maps> (default 0 = off): the node calls estimateMapsTransforms on a timer with every robot's latest map,
  // most of them unchanged since the last tick; with the cache on, an unchanged map's features (and, under MATCHING, its
  // pairs) are reused, bit for bit (mm3d_set_map_cache).  A device list has no cache: that MM3D_EUNSUPPORTED is ignored.
  // MM3D_ICP=point_to_plane: the pair stage refines with point-to-plane ICP instead of the reference's point-to-point
  // (mm3d_set_icp_method); point_to_point or unset keeps the reference's.  Not available on a device list: with MM3D_DEVICES
  // set as well this throws rather than quietly running point-to-point.
  // MM3D_ALIGN=prerejective: under SAC_IA the pair stage's initial alignment is the prerejective one (mm3d_set_alignment), with
  // MM3D_ALIGN_SAMPLES=<draws> if given; sac_ia or unset keeps the reference's.  Not available on a device list either.
  // MM3D_KEYPOINTS=uniform[:<leaf>]: parse_keypoints above; it works on a device list too.
  // MM3D_OUTLIERS=statistical[:<mean_k>[:<stddev_mult>]]: parse_outliers above; it works on a device list too.
  // MM3D_CLUSTERS=min_size:<n>[:<tolerance>] or largest[:<tolerance>]: parse_clusters above; it works on a device list too.
  // MM3D_PLANES=remove|set_aside[:<max_planes>[:<distance>]][@<x>,<y>,<z>,<degrees>|@any]: parse_planes above; it works on a device list too.
  // MM3D_SMOOTH=mls[:<order>[:<radius>]][@maps|@composed]: parse_smooth above; it works on a device list too.
  // MM3D_REFINE=ndt[:<resolution>]: parse_refine above.  Not available on a device list: ndt with MM3D_DEVICES set as well throws.
  // MM3D_COARSE=correlative[:<cell>]: parse_coarse above.  Not available on a device list: correlative with MM3D_DEVICES set as well throws.
  // MM3D_CONFIDENCE=overlap[:<voxel>]: parse_confidence above.  Not available on a device list: overlap with MM3D_DEVICES set as well throws.
  // MM3D_ICP_REJECT=one_to_one+trimmed:0.7 ...: parse_icp_reject above.  Not available on a device list: an active value with MM3D_DEVICES set as well throws.
  // MM3D_ICP_ROBUST=geman_mcclure:0.05[:<start>[:<anneal>[:<tuning>]]]: parse_icp_robust above.  Not available on a device list nor with an active MM3D_ICP_REJECT, MM3D_ICP_COLOR, MM3D_ICP_GENERALIZED or MM3D_REFINE=ndt: each throws.
  // MM3D_ICP_COLOR=1 or <lambda>[:<radius>]: parse_icp_color above.  Not available on a device list nor with an active MM3D_ICP_REJECT: either throws.
  // MM3D_ICP_GENERALIZED=1 or <epsilon>: parse_icp_generalized above.  Not available on a device list nor with an active MM3D_ICP_REJECT or MM3D_ICP_COLOR: each throws.
  // MM3D_ESTIMATOR=consistency[:<seeds>]: parse_estimator above.  Not available on a device list: consistency with MM3D_DEVICES set as well throws.
  // MM3D_ICP_SAMPLE=normal_space:0.25[:<bins>] or stride:0.1: parse_icp_sample above.  Not available on a device list nor with MM3D_REFINE=ndt, MM3D_ICP_COLOR or MM3D_ICP_GENERALIZED: each throws.
  static mm3d_ctx *c = [] {
    const mm3d_estimator_options estimator = parse_estimator(std::getenv("MM3D_ESTIMATOR"));
    check_estimator_devices(estimator, std::getenv("MM3D_DEVICES"));
    const mm3d_icp_rejection_options reject = parse_icp_reject(std::getenv("MM3D_ICP_REJECT"));
    check_icp_reject_devices(reject, std::getenv("MM3D_DEVICES"));
    const mm3d_icp_geometry_options reject_geometry = parse_icp_reject_geometry(std::getenv("MM3D_ICP_REJECT_GEOMETRY"));
    check_icp_reject_geometry_devices(reject_geometry, std::getenv("MM3D_DEVICES"));
    const mm3d_icp_color_options color = parse_icp_color(std::getenv("MM3D_ICP_COLOR"));
    check_icp_color_combinations(color, reject, std::getenv("MM3D_DEVICES"));
    const mm3d_icp_generalized_options generalized = parse_icp_generalized(std::getenv("MM3D_ICP_GENERALIZED"));
    check_icp_generalized_combinations(generalized, reject, color, std::getenv("MM3D_DEVICES"));
    const mm3d_confidence_options confidence = parse_confidence(std::getenv("MM3D_CONFIDENCE"));
    check_confidence_devices(confidence, std::getenv("MM3D_DEVICES"));
    const mm3d_coarse_options coarse = parse_coarse(std::getenv("MM3D_COARSE"));
    if (coarse.method == MM3D_COARSE_CORRELATIVE && std::getenv("MM3D_DEVICES") && *std::getenv("MM3D_DEVICES"))
      throw std::runtime_error("mm3d: MM3D_COARSE=correlative is not available with MM3D_DEVICES (a device list carries no signatures)");
    const mm3d_keypoint_options keypoints = parse_keypoints(std::getenv("MM3D_KEYPOINTS"));
    const mm3d_outlier_options outliers = parse_outliers(std::getenv("MM3D_OUTLIERS"));
    const mm3d_cluster_options clusters = parse_clusters(std::getenv("MM3D_CLUSTERS"));
    const mm3d_plane_options planes = parse_planes(std::getenv("MM3D_PLANES"));
    const mm3d_smooth_options smooth = parse_smooth(std::getenv("MM3D_SMOOTH"));
    mm3d_refine_options refine = parse_refine(std::getenv("MM3D_REFINE"));
    if (refine.method == MM3D_REFINE_NDT && std::getenv("MM3D_DEVICES") && *std::getenv("MM3D_DEVICES"))
      throw std::runtime_error("mm3d: MM3D_REFINE=ndt is not available with MM3D_DEVICES (a device list carries no voxel tables)");
    const mm3d_icp_robust_options robust = parse_icp_robust(std::getenv("MM3D_ICP_ROBUST"));
    check_icp_robust_combinations(robust, reject, color, generalized, refine, std::getenv("MM3D_DEVICES"));
    const mm3d_icp_sampling_options sampling = parse_icp_sample(std::getenv("MM3D_ICP_SAMPLE"));
    check_icp_sample_combinations(sampling, refine, color, generalized, std::getenv("MM3D_DEVICES"));
    const char *al = std::getenv("MM3D_ALIGN");
    const std::string align = al ? al : "";
    if (!align.empty() && align != "sac_ia" && align != "prerejective")
      throw std::runtime_error("mm3d: MM3D_ALIGN must be sac_ia or prerejective, not '" + align + "'");
    if (align == "prerejective" && std::getenv("MM3D_DEVICES") && *std::getenv("MM3D_DEVICES"))
      throw std::runtime_error("mm3d: MM3D_ALIGN=prerejective is not available with MM3D_DEVICES (the devices' pair loops run SAC-IA)");
    const char *icp = std::getenv("MM3D_ICP");
    const std::string icp_method = icp ? icp : "";
    if (!icp_method.empty() && icp_method != "point_to_point" && icp_method != "point_to_plane")
      throw std::runtime_error("mm3d: MM3D_ICP must be point_to_point or point_to_plane, not '" + icp_method + "'");
    const char *devices = std::getenv("MM3D_DEVICES");
    if (icp_method == "point_to_plane" && devices && *devices)
      throw std::runtime_error("mm3d: MM3D_ICP=point_to_plane is not available with MM3D_DEVICES (a device list carries no normals)");
    const char *s = std::getenv("MM3D_STREAMS");
    const int n = s ? std::atoi(s) : 16;
    mm3d_ctx *e = make_ctx(n >= 1 && n <= 64 ? n : 16, true);   // (the estimation engine is the one that may span several GPUs)
    const char *m = std::getenv("MM3D_MAP_CACHE");
    const int maps = m ? std::atoi(m) : 0;
    if (maps > 0) (void)mm3d_set_map_cache(e, maps);
    if (icp_method == "point_to_plane" && mm3d_set_icp_method(e, MM3D_ICP_POINT_TO_PLANE) != MM3D_OK)
      throw std::runtime_error(std::string("mm3d: ") + mm3d_last_error(e));
    if (align == "prerejective") {
      mm3d_alignment_options o;
      mm3d_alignment_options_default(&o);
      o.method = MM3D_ALIGN_PREREJECTIVE;
      if (const char *ns = std::getenv("MM3D_ALIGN_SAMPLES")) o.samples = std::atoi(ns);
      if (mm3d_set_alignment(e, &o) != MM3D_OK)
        throw std::runtime_error("mm3d: MM3D_ALIGN=prerejective was refused (MM3D_ALIGN_SAMPLES must be 1 .. 2^30)");
    }
    if (keypoints.source != MM3D_KEYPOINTS_REFERENCE && mm3d_set_keypoints(e, &keypoints) != MM3D_OK)
      throw std::runtime_error("mm3d: MM3D_KEYPOINTS was refused (the leaf must be a positive float with a finite reciprocal)");
    if (outliers.method != MM3D_OUTLIERS_RADIUS && mm3d_set_outlier_filter(e, &outliers) != MM3D_OK)
      throw std::runtime_error("mm3d: MM3D_OUTLIERS was refused (mean_k must be 1 .. 64, stddev_mult finite and not negative)");
    if (clusters.method != MM3D_CLUSTERS_OFF && mm3d_set_cluster_filter(e, &clusters) != MM3D_OK)
      throw std::runtime_error("mm3d: MM3D_CLUSTERS was refused (min_size must be at least 1, the tolerance finite and not negative)");
    if (planes.method != MM3D_PLANES_OFF && mm3d_set_planes(e, &planes) != MM3D_OK)
      throw std::runtime_error("mm3d: MM3D_PLANES was refused (max_planes must be 1 .. 8, the distance finite and not negative, the angle 0 .. 90)");
    if (smooth.method != MM3D_SMOOTH_OFF && mm3d_set_smoothing(e, &smooth) != MM3D_OK)
      throw std::runtime_error("mm3d: MM3D_SMOOTH was refused (the order must be 1 or 2, the radius finite and not negative)");
    if (refine.method != MM3D_REFINE_ICP && mm3d_set_refinement(e, &refine) != MM3D_OK)
      throw std::runtime_error("mm3d: MM3D_REFINE was refused (the resolution must be a positive float with a finite reciprocal)");
    if (coarse.method != MM3D_COARSE_NONE && mm3d_set_coarse_alignment(e, &coarse) != MM3D_OK)
      throw std::runtime_error("mm3d: MM3D_COARSE was refused (the cell must be a positive float with a finite reciprocal)");
    if (confidence.method != MM3D_CONFIDENCE_REFERENCE && mm3d_set_confidence(e, &confidence) != MM3D_OK)
      throw std::runtime_error("mm3d: MM3D_CONFIDENCE was refused (the voxel must be a positive float with a finite reciprocal)");
    if ((reject.one_to_one || reject.distance != MM3D_REJECT_NONE) && mm3d_set_icp_rejection(e, &reject) != MM3D_OK)
      throw std::runtime_error(std::string("mm3d: MM3D_ICP_REJECT was refused: ") + mm3d_last_error(e));
    if (robust.kernel != MM3D_ROBUST_OFF && mm3d_set_icp_robust(e, &robust) != MM3D_OK)
      throw std::runtime_error(std::string("mm3d: MM3D_ICP_ROBUST was refused: ") + mm3d_last_error(e));
    if (color.enabled && mm3d_set_icp_color(e, &color) != MM3D_OK)
      throw std::runtime_error(std::string("mm3d: MM3D_ICP_COLOR was refused: ") + mm3d_last_error(e));
    if (generalized.enabled && mm3d_set_icp_generalized(e, &generalized) != MM3D_OK)
      throw std::runtime_error(std::string("mm3d: MM3D_ICP_GENERALIZED was refused: ") + mm3d_last_error(e));
    if (estimator.method != MM3D_ESTIMATOR_RANSAC && mm3d_set_estimator(e, &estimator) != MM3D_OK)
      throw std::runtime_error(std::string("mm3d: MM3D_ESTIMATOR was refused: ") + mm3d_last_error(e));
    if (sampling.method != MM3D_ICP_SAMPLE_NONE && mm3d_set_icp_sampling(e, &sampling) != MM3D_OK)
      throw std::runtime_error(std::string("mm3d: MM3D_ICP_SAMPLE was refused: ") + mm3d_last_error(e));
    // (last: the library refuses it beside coloured, generalized and robust ICP, and its normals term beside a sampling)
    if ((reject_geometry.boundary || reject_geometry.normals) && mm3d_set_icp_geometry_rejection(e, &reject_geometry) != MM3D_OK)
      throw std::runtime_error(std::string("mm3d: MM3D_ICP_REJECT_GEOMETRY was refused: ") + mm3d_last_error(e));
    return e;
  }();
  return c;
}
inline mm3d_ctx *compose_ctx()
{
  // MM3D_SMOOTH with the composed map in it (parse_smooth): composeMaps smooths between two voxel passes
  static mm3d_ctx *c = [] {
    mm3d_ctx *e = make_ctx(1);
    const mm3d_smooth_options smooth = parse_smooth(std::getenv("MM3D_SMOOTH"));
    if (smooth.method != MM3D_SMOOTH_OFF && mm3d_set_smoothing(e, &smooth) != MM3D_OK)
      throw std::runtime_error("mm3d: MM3D_SMOOTH was refused (the order must be 1 or 2, the radius finite and not negative)");
    return e;
  }();
  return c;
}
inline void check(mm3d_ctx *c, int st)
{
  if (st != MM3D_OK) throw std::runtime_error(std::string("mm3d: ") + mm3d_last_error(c));
}
inline void check(int st) { check(ctx(), st); }
// pcl::PointXYZRGB is 32 bytes: x,y,z,pad | rgba,pad,pad,pad  -> stride 32, rgba_offset 16
inline mm3d_cloud *upload(const PointCloud &c, mm3d_ctx *on = nullptr)
{
  mm3d_ctx *e = on ? on : ctx();
  mm3d_cloud *h = nullptr;
  check(e, mm3d_cloud_create(e, c.points.data(), c.points.size(), sizeof(PointT), offsetof(PointT, rgba), &h));
  return h;
}
inline PointCloudPtr download(mm3d_cloud *h, mm3d_ctx *on = nullptr)
{
  mm3d_ctx *e = on ? on : ctx();
  PointCloudPtr out(new PointCloud);
  out->points.resize(mm3d_cloud_size(h));
  out->width = static_cast<uint32_t>(out->points.size());
  out->height = 1;
  out->is_dense = true;
  check(e, mm3d_cloud_download(e, h, out->points.data(), sizeof(PointT), offsetof(PointT, rgba)));
  return out;
}
inline mm3d_normals *upload(const SurfaceNormals &n)
{
  mm3d_normals *h = nullptr;
  // pcl::Normal is 32 bytes: nx,ny,nz,pad | curvature,... : repack to 16-byte records first
  std::vector<float> tmp(n.points.size() * 4);
  for (size_t i = 0; i < n.points.size(); ++i) {
    tmp[4 * i] = n.points[i].normal_x; tmp[4 * i + 1] = n.points[i].normal_y;
    tmp[4 * i + 2] = n.points[i].normal_z; tmp[4 * i + 3] = n.points[i].curvature;
  }
  check(mm3d_normals_create(ctx(), tmp.data(), n.points.size(), 16, &h));
  return h;
}
// PCLPointCloud2 <-> mm3d_desc: fields[0].name selects the descriptor (dispatch_descriptors.h:104-111)
inline int descriptor_from_field(const std::string &name)
{
  for (int d = 0; d < 6; ++d)
    if (name == mm3d_descriptor_field_name(d)) return d;
  throw std::runtime_error("unknown descriptor type");
}
inline mm3d_desc *upload(const LocalDescriptors &d)
{
  if (d.fields.empty()) throw std::runtime_error("descriptors must contain at least one field with descriptors.");
  const int type = descriptor_from_field(d.fields[0].name);
  const int dim = mm3d_descriptor_dim(type);
  const size_t n = static_cast<size_t>(d.width) * d.height;
  std::vector<float> tmp(n * dim);
  for (size_t i = 0; i < n; ++i)
    std::memcpy(&tmp[i * dim], &d.data[i * d.point_step + d.fields[0].offset], sizeof(float) * dim);
  mm3d_desc *h = nullptr;
  check(mm3d_desc_create(ctx(), tmp.data(), n, type, &h));
  return h;
}
inline Eigen::Matrix4f to_eigen(const float *T)
{
  return Eigen::Map<const Eigen::Matrix4f>(T);   // both column-major
}
inline mm3d_params to_params(const MapMergingParams &p)
{
  mm3d_params q;
  q.resolution = p.resolution; q.descriptor_radius = p.descriptor_radius;
  q.outliers_min_neighbours = p.outliers_min_neighbours; q.normal_radius = p.normal_radius;
  q.keypoint_type = static_cast<int>(p.keypoint_type); q.keypoint_threshold = p.keypoint_threshold;
  q.descriptor_type = static_cast<int>(p.descriptor_type); q.estimation_method = static_cast<int>(p.estimation_method);
  q.refine_transform = p.refine_transform; q.inlier_threshold = p.inlier_threshold;
  q.max_correspondence_distance = p.max_correspondence_distance; q.max_iterations = p.max_iterations;
  q.matching_k = p.matching_k; q.transform_epsilon = p.transform_epsilon;
  q.confidence_threshold = p.confidence_threshold; q.output_resolution = p.output_resolution;
  return q;
}
inline MapMergingParams from_params(const mm3d_params &q)
{
  MapMergingParams p;
  p.resolution = q.resolution; p.descriptor_radius = q.descriptor_radius;
  p.outliers_min_neighbours = q.outliers_min_neighbours; p.normal_radius = q.normal_radius;
  p.keypoint_type = static_cast<Keypoint>(q.keypoint_type); p.keypoint_threshold = q.keypoint_threshold;
  p.descriptor_type = static_cast<Descriptor>(q.descriptor_type);
  p.estimation_method = static_cast<EstimationMethod>(q.estimation_method);
  p.refine_transform = q.refine_transform != 0; p.inlier_threshold = q.inlier_threshold;
  p.max_correspondence_distance = q.max_correspondence_distance; p.max_iterations = q.max_iterations;
  p.matching_k = static_cast<size_t>(q.matching_k); p.transform_epsilon = q.transform_epsilon;
  p.confidence_threshold = q.confidence_threshold; p.output_resolution = q.output_resolution;
  return p;
}
// a ROS parameter that names an enum value: absent or empty keeps the default, an unknown
// name throws like enums::from_string (R/include/map_merge_3d/enum.h:58)
inline void enum_param(const ros::NodeHandle &n, const char *key, int (*parse)(const char *), int *value)
{
  std::string s;
  n.getParam(key, s);
  if (s.empty()) return;
  const int v = parse(s.c_str());
  if (v < 0) throw std::runtime_error("string is not a valid enum value: " + s);
  *value = v;
}
}  // namespace mm3d_shim

#ifdef MM3D_SHIM_IMPLEMENTATION

// map_merging.h:53, R/src/map_merging.cpp:10-54 -- the parsing itself lives behind the C ABI
// (mm3d_params_from_command_line) so that non-C++ callers get the same behaviour
MapMergingParams MapMergingParams::fromCommandLine(int argc, char **argv)
{
  mm3d_params q;
  if (mm3d_params_from_command_line(argc, argv, &q) != MM3D_OK)
    throw std::runtime_error("string is not a valid enum value");   // enums::from_string, enum.h:58
  return mm3d_shim::from_params(q);
}

// map_merging.h:60, R/src/map_merging.cpp:56-98 -- the same keys read from the node's parameters;
// a missing key keeps the default, matching_k is applied only when positive
MapMergingParams MapMergingParams::fromROSNode(const ros::NodeHandle &n)
{
  mm3d_params q;
  mm3d_params_default(&q);
  bool refine = q.refine_transform != 0;
  int k = -1;
  n.getParam("resolution", q.resolution);
  n.getParam("descriptor_radius", q.descriptor_radius);
  n.getParam("outliers_min_neighbours", q.outliers_min_neighbours);
  n.getParam("normal_radius", q.normal_radius);
  mm3d_shim::enum_param(n, "keypoint_type", mm3d_keypoint_from_string, &q.keypoint_type);
  n.getParam("keypoint_threshold", q.keypoint_threshold);
  mm3d_shim::enum_param(n, "descriptor_type", mm3d_descriptor_from_string, &q.descriptor_type);
  mm3d_shim::enum_param(n, "estimation_method", mm3d_estimation_method_from_string, &q.estimation_method);
  n.getParam("refine_transform", refine);
  n.getParam("inlier_threshold", q.inlier_threshold);
  n.getParam("max_correspondence_distance", q.max_correspondence_distance);
  n.getParam("max_iterations", q.max_iterations);
  n.getParam("matching_k", k);
  n.getParam("transform_epsilon", q.transform_epsilon);
  n.getParam("confidence_threshold", q.confidence_threshold);
  n.getParam("output_resolution", q.output_resolution);
  q.refine_transform = refine;
  if (k > 0) q.matching_k = static_cast<uint64_t>(k);
  return mm3d_shim::from_params(q);
}

// map_merging.h:62, R/src/map_merging.cpp:100-123 -- "name: value" lines, mm3d_params_to_string
std::ostream &operator<<(std::ostream &stream, const MapMergingParams &params)
{
  const mm3d_params q = mm3d_shim::to_params(params);
  std::vector<char> text(mm3d_params_to_string(&q, nullptr, 0));   // size includes the terminating NUL
  mm3d_params_to_string(&q, text.data(), text.size());
  return stream << text.data();
}

// R/include/map_merge_3d/features.h:34
PointCloudPtr downSample(const PointCloudConstPtr &input, double resolution)
{
  using namespace mm3d_shim;
  mm3d_cloud *in = upload(*input), *out = nullptr;
  check(mm3d_downsample(ctx(), in, resolution, &out));
  PointCloudPtr r = download(out);
  mm3d_cloud_free(ctx(), in); mm3d_cloud_free(ctx(), out);
  return r;
}

// features.h:45
PointCloudPtr removeOutliers(const PointCloudConstPtr &input, double radius, int min_neighbors)
{
  using namespace mm3d_shim;
  mm3d_cloud *in = upload(*input), *out = nullptr;
  check(mm3d_remove_outliers(ctx(), in, radius, min_neighbors, &out));
  PointCloudPtr r = download(out);
  mm3d_cloud_free(ctx(), in); mm3d_cloud_free(ctx(), out);
  return r;
}

// features.h:97
SurfaceNormalsPtr computeSurfaceNormals(const PointCloudConstPtr &input, double radius)
{
  using namespace mm3d_shim;
  mm3d_cloud *in = upload(*input);
  mm3d_normals *n = nullptr;
  check(mm3d_compute_normals(ctx(), in, radius, &n));
  std::vector<float> tmp(mm3d_normals_size(n) * 4);
  check(mm3d_normals_download(ctx(), n, tmp.data(), 16));
  SurfaceNormalsPtr out(new SurfaceNormals);
  out->points.resize(tmp.size() / 4);
  out->width = static_cast<uint32_t>(out->points.size()); out->height = 1; out->is_dense = true;
  for (size_t i = 0; i < out->points.size(); ++i) {
    out->points[i].normal_x = tmp[4 * i]; out->points[i].normal_y = tmp[4 * i + 1];
    out->points[i].normal_z = tmp[4 * i + 2]; out->points[i].curvature = tmp[4 * i + 3];
    if (!std::isfinite(tmp[4 * i])) out->is_dense = false;
  }
  mm3d_cloud_free(ctx(), in); mm3d_normals_free(ctx(), n);
  return out;
}

// features.h:65
PointCloudPtr detectKeypoints(const PointCloudConstPtr &points, const SurfaceNormalsPtr &normals, Keypoint type,
                              double threshold, double radius, double resolution)
{
  using namespace mm3d_shim;
  mm3d_cloud *in = upload(*points), *kp = nullptr;
  mm3d_normals *n = normals ? upload(*normals) : nullptr;
  check(mm3d_detect_keypoints(ctx(), in, n, static_cast<int>(type), threshold, radius, resolution, &kp));
  PointCloudPtr r = download(kp);
  mm3d_cloud_free(ctx(), in); mm3d_cloud_free(ctx(), kp);
  if (n) mm3d_normals_free(ctx(), n);
  return r;
}

// features.h:83 -- prunes `keypoints` in place like the reference (features.cpp:137-141)
LocalDescriptorsPtr computeLocalDescriptors(const PointCloudConstPtr &points, const SurfaceNormalsPtr &normals,
                                            const PointCloudPtr &keypoints, Descriptor descriptor, double feature_radius)
{
  using namespace mm3d_shim;
  mm3d_cloud *in = upload(*points), *kp = upload(*keypoints);
  mm3d_normals *n = upload(*normals);
  mm3d_desc *d = nullptr;
  check(mm3d_compute_descriptors(ctx(), in, n, kp, static_cast<int>(descriptor), feature_radius, &d));
  *keypoints = *download(kp);
  const int dim = mm3d_desc_dim(d);
  const size_t cnt = mm3d_desc_size(d);
  LocalDescriptorsPtr out(new LocalDescriptors);
  out->fields.resize(1);
  out->fields[0].name = mm3d_descriptor_field_name(static_cast<int>(descriptor));
  out->fields[0].offset = 0; out->fields[0].datatype = pcl::PCLPointField::FLOAT32; out->fields[0].count = dim;
  out->point_step = sizeof(float) * dim; out->width = static_cast<uint32_t>(cnt); out->height = 1;
  out->row_step = out->point_step * out->width; out->is_dense = true;
  out->data.resize(out->row_step);
  check(mm3d_desc_download(ctx(), d, reinterpret_cast<float *>(out->data.data())));
  mm3d_cloud_free(ctx(), in); mm3d_cloud_free(ctx(), kp); mm3d_normals_free(ctx(), n); mm3d_desc_free(ctx(), d);
  return out;
}

// matching.h:26
CorrespondencesPtr findFeatureCorrespondences(const LocalDescriptorsPtr &source_descriptors,
                                              const LocalDescriptorsPtr &target_descriptors, size_t k)
{
  using namespace mm3d_shim;
  mm3d_desc *s = upload(*source_descriptors), *t = upload(*target_descriptors);
  size_t n = 0;
  check(mm3d_find_correspondences(ctx(), s, t, k, nullptr, 0, &n));
  std::vector<mm3d_corr> buf(n ? n : 1);
  check(mm3d_find_correspondences(ctx(), s, t, k, buf.data(), buf.size(), &n));
  CorrespondencesPtr out(new Correspondences);
  for (size_t i = 0; i < n; ++i) out->emplace_back(buf[i].index_query, buf[i].index_match, buf[i].distance);
  mm3d_desc_free(ctx(), s); mm3d_desc_free(ctx(), t);
  return out;
}

// matching.h:44
Eigen::Matrix4f estimateTransformFromCorrespondences(const PointCloudPtr &source_keypoints, const PointCloudPtr &target_keypoints,
                                                     const CorrespondencesPtr &correspondences, CorrespondencesPtr &inliers,
                                                     double inlier_threshold)
{
  using namespace mm3d_shim;
  mm3d_cloud *s = upload(*source_keypoints), *t = upload(*target_keypoints);
  std::vector<mm3d_corr> c(correspondences->size()), inl(correspondences->size() + 1);
  for (size_t i = 0; i < c.size(); ++i) c[i] = {(*correspondences)[i].index_query, (*correspondences)[i].index_match, (*correspondences)[i].distance};
  float T[16]; size_t n = 0;
  check(mm3d_estimate_transform_from_correspondences(ctx(), s, t, c.data(), c.size(), inlier_threshold, T, inl.data(), inl.size(), &n));
  inliers.reset(new Correspondences);
  for (size_t i = 0; i < n; ++i) inliers->emplace_back(inl[i].index_query, inl[i].index_match, inl[i].distance);
  mm3d_cloud_free(ctx(), s); mm3d_cloud_free(ctx(), t);
  return to_eigen(T);
}

// matching.h:68
Eigen::Matrix4f estimateTransformFromDescriptorsSets(const PointCloudPtr &source_keypoints, const LocalDescriptorsPtr &source_descriptors,
                                                     const PointCloudPtr &target_keypoints, const LocalDescriptorsPtr &target_descriptors,
                                                     double min_sample_distance, double max_correspondence_distance, int max_iterations)
{
  using namespace mm3d_shim;
  mm3d_cloud *s = upload(*source_keypoints), *t = upload(*target_keypoints);
  mm3d_desc *sd = upload(*source_descriptors), *td = upload(*target_descriptors);
  float T[16];
  check(mm3d_estimate_transform_from_descriptors(ctx(), s, sd, t, td, min_sample_distance, max_correspondence_distance, max_iterations, T));
  mm3d_cloud_free(ctx(), s); mm3d_cloud_free(ctx(), t); mm3d_desc_free(ctx(), sd); mm3d_desc_free(ctx(), td);
  return to_eigen(T);
}

// matching.h:94
Eigen::Matrix4f estimateTransformICP(const PointCloudPtr &source_points, const PointCloudPtr &target_points,
                                     const Eigen::Matrix4f &initial_guess, double max_correspondence_distance,
                                     double outlier_rejection_threshold, int max_iterations, double transformation_epsilon)
{
  using namespace mm3d_shim;
  mm3d_cloud *s = upload(*source_points), *t = upload(*target_points);
  float T[16];
  check(mm3d_estimate_transform_icp(ctx(), s, t, initial_guess.data(), max_correspondence_distance, outlier_rejection_threshold,
                                    max_iterations, transformation_epsilon, T));
  mm3d_cloud_free(ctx(), s); mm3d_cloud_free(ctx(), t);
  return to_eigen(T);
}

// matching.h:129
Eigen::Matrix4f estimateTransform(const PointCloudPtr &source_points, const PointCloudPtr &source_keypoints,
                                  const LocalDescriptorsPtr &source_descriptors, const PointCloudPtr &target_points,
                                  const PointCloudPtr &target_keypoints, const LocalDescriptorsPtr &target_descriptors,
                                  EstimationMethod method, bool refine, double inlier_threshold, double max_correspondence_distance,
                                  int max_iterations, size_t matching_k, double transform_epsilon)
{
  using namespace mm3d_shim;
  mm3d_cloud *sp = upload(*source_points), *sk = upload(*source_keypoints), *tp = upload(*target_points), *tk = upload(*target_keypoints);
  mm3d_desc *sd = upload(*source_descriptors), *td = upload(*target_descriptors);
  float T[16];
  check(mm3d_estimate_transform(ctx(), sp, sk, sd, tp, tk, td, static_cast<int>(method), refine, inlier_threshold,
                                max_correspondence_distance, max_iterations, matching_k, transform_epsilon, T));
  for (mm3d_cloud *c : {sp, sk, tp, tk}) mm3d_cloud_free(ctx(), c);
  mm3d_desc_free(ctx(), sd); mm3d_desc_free(ctx(), td);
  return to_eigen(T);
}

// matching.h:150
double transformScore(const PointCloudPtr &source_points, const PointCloudPtr &target_points, const Eigen::Matrix4f &transform,
                      double max_distance)
{
  using namespace mm3d_shim;
  mm3d_cloud *s = upload(*source_points), *t = upload(*target_points);
  double score = 0;
  check(mm3d_transform_score(ctx(), s, t, transform.data(), max_distance, &score));
  mm3d_cloud_free(ctx(), s); mm3d_cloud_free(ctx(), t);
  return score;
}

// map_merging.h:85 -- the whole hot path in one call; clouds go to the device once
std::vector<Eigen::Matrix4f> estimateMapsTransforms(const std::vector<PointCloudConstPtr> &clouds, const MapMergingParams &params)
{
  using namespace mm3d_shim;
  // R/src/map_merging.cpp:192-197: nothing to estimate, the clouds are not touched (and no device is needed)
  if (clouds.empty()) return {};
  if (clouds.size() == 1) return {Eigen::Matrix4f::Identity()};
  std::vector<mm3d_cloud_view> views(clouds.size());
  for (size_t i = 0; i < clouds.size(); ++i) {
    // a robot that is subscribed but has no map yet hands over nullptr (map_merge_node.cpp:171)
    views[i].points = clouds[i] ? clouds[i]->points.data() : nullptr;
    views[i].n = clouds[i] ? clouds[i]->points.size() : 0;
    views[i].stride = sizeof(PointT);
    views[i].rgba_offset = offsetof(PointT, rgba);
  }
  std::vector<float> out(16 * clouds.size());
  size_t n_out = 0;
  const mm3d_params p = to_params(params);
  check(mm3d_estimate_maps_transforms(ctx(), views.data(), views.size(), &p, out.data(), &n_out, nullptr, nullptr));
  std::vector<Eigen::Matrix4f> result(n_out);
  for (size_t i = 0; i < n_out; ++i) result[i] = to_eigen(&out[16 * i]);
  return result;
}

// map_merging.h:99 -- on the compositing context (see mm3d_shim::compose_ctx)
PointCloudPtr composeMaps(const std::vector<PointCloudConstPtr> &clouds, const std::vector<Eigen::Matrix4f> &transforms, double resolution)
{
  using namespace mm3d_shim;
  if (clouds.empty()) return nullptr;
  if (clouds.size() != transforms.size())
    throw new std::runtime_error("composeMaps: clouds and transforms size must be the same.");   // a pointer, like the reference
  size_t total = 0;
  for (const auto &c : clouds) total += c ? c->points.size() : 0;
  if (total == 0) {                                // nothing to transform or voxelise: an empty cloud, no device needed
    PointCloudPtr empty(new PointCloud);
    empty->is_dense = true;
    return empty;
  }
  mm3d_ctx *e = compose_ctx();
  const PointCloud none;
  std::vector<mm3d_cloud *> h(clouds.size());
  std::vector<float> T(16 * clouds.size());
  for (size_t i = 0; i < clouds.size(); ++i) {
    h[i] = upload(clouds[i] ? *clouds[i] : none, e);
    std::memcpy(&T[16 * i], transforms[i].data(), sizeof(float) * 16);
  }
  mm3d_cloud *out = nullptr;
  check(e, mm3d_compose_maps(e, h.data(), h.size(), T.data(), transforms.size(), resolution, &out));
  PointCloudPtr r = download(out, e);
  for (mm3d_cloud *c : h) mm3d_cloud_free(e, c);
  mm3d_cloud_free(e, out);
  return r;
}

#endif  // MM3D_SHIM_IMPLEMENTATION
}  // namespace map_merge_3d

#endif  // MM3D_SHIM_AVAILABLE

// types.hpp -- device-resident objects behind the opaque C handles, and the stage entry points
// shared between the translation units of libmm3d.
//
// HBM layout:
//   cloud points   float4 {x, y, z, rgba-bits}            16 B / point, reference order
//   normals        float4 {nx, ny, nz, curvature}         16 B / point, same order
//   descriptors    float  [n][dim] row-major              (FPFH: 132 B / keypoint)
//   grid           cell_start int32[dx*dy*dz + 1] (x fastest) + a cell-sorted copy of the points
//                  whose .w carries the ORIGINAL index, so a (y,z) row of cells is one contiguous
//                  span of candidates.
#pragma once

#include "common.hpp"

namespace mm3d {
struct DeviceSet;
struct IcpMethodBase;
struct AlignMethodBase;
struct KeypointSourceBase;
struct CoarseMethodBase;
struct ConfidenceMethodBase;
struct EstimatorMethodBase;
struct IcpSamplerBase;
struct OutlierFilterBase;
struct ClusterFilterBase;
struct SmootherBase;
struct PlaneFilterBase;
struct IcpGeometryBase;

// The opt-in stages of a context's pipeline (mm3d_set_icp_method, mm3d_set_alignment, mm3d_set_keypoints, mm3d_set_refinement,
// mm3d_set_coarse_alignment, mm3d_set_confidence, mm3d_set_icp_rejection, mm3d_set_icp_robust, mm3d_set_icp_color, mm3d_set_icp_generalized,
// mm3d_set_estimator, mm3d_set_icp_sampling, mm3d_set_outlier_filter, mm3d_set_cluster_filter, mm3d_set_smoothing, mm3d_set_planes): a null method = the reference's stage.  The methods are process-wide
// objects of their kernel files that hold no state and are not owned.  Every context has its own copy of the record; only
// select_stage (stage_rules.hpp) changes one, and it and mm3d_set_streams hand the root's copy to the helpers.
struct StageSelection {
  const IcpMethodBase *icp = nullptr;                  // point-to-plane in the place of point-to-point
  const AlignMethodBase *align = nullptr;              // the initial estimate under SAC_IA
  const KeypointSourceBase *keypoints = nullptr;       // where a map's keypoints come from
  const IcpMethodBase *refine = nullptr;               // what takes the ICP's place (NDT); `icp` keeps its own value beside it
  const CoarseMethodBase *coarse = nullptr;            // what takes the initial estimate's place
  const ConfidenceMethodBase *confidence = nullptr;    // what a pair record's confidence is
  const IcpMethodBase *color = nullptr;                // coloured ICP in the place of `icp`'s, which keeps its own value beside it
  const IcpMethodBase *generalized = nullptr;          // generalized ICP in the place of `icp`'s, which keeps its own value beside it
  const EstimatorMethodBase *estimator = nullptr;      // the initial estimate under MATCHING: the consistency graph in RANSAC's place
  const IcpSamplerBase *sampler = nullptr;             // what the ICP searches with: a sample of the source map in the place of all of it
  const OutlierFilterBase *outliers = nullptr;         // what filters a down-sampled map in removeOutliers' place
  const ClusterFilterBase *clusters = nullptr;         // what drops the small connected components of the filtered map
  const SmootherBase *smoother = nullptr;              // what smooths a filtered map before its normals, and the composed map
  const PlaneFilterBase *planes = nullptr;             // what takes the dominant planes out of the filtered map, before the cluster filter
  const IcpGeometryBase *geometry = nullptr;           // what binds a pair's boundary flags and normals for the rejecting step's step 1b
  mm3d_alignment_options align_options;
  mm3d_keypoint_options keypoint_options;
  mm3d_refine_options refine_options;
  mm3d_coarse_options coarse_options;
  mm3d_confidence_options confidence_options;
  mm3d_icp_rejection_options reject_options;           // the ICP's correspondence rejection: no method object, the jobs carry them
  mm3d_icp_robust_options robust_options;              // the ICP's robust kernel: no method object, the jobs carry them
  mm3d_icp_color_options color_options;
  mm3d_icp_generalized_options generalized_options;
  mm3d_estimator_options estimator_options;
  mm3d_icp_sampling_options sampling_options;
  mm3d_outlier_options outlier_options;
  mm3d_cluster_options cluster_options;
  mm3d_smooth_options smooth_options;                  // `where` says which places ask the smoother
  mm3d_plane_options plane_options;
  mm3d_icp_geometry_options geometry_options;
  // A stage's pointer is non-null exactly while its options make it active; what that means is its row's predicate in
  // stage_rules.cpp, which the setters' edits and the three members below read.
  StageSelection();                                    // capi.cpp: the options are the sixteen mm3d_*_options_default's
  // the ICP of the pair stage rejects correspondences (mm3d_set_icp_rejection)
  bool rejecting() const;
  // the rejecting step drops correspondences by the maps' geometry too (mm3d_set_icp_geometry_rejection)
  bool geometric() const;
  // the ICP of the pair stage weights its correspondences (mm3d_set_icp_robust)
  bool robust() const;
  int icp_method() const;                              // MM3D_ICP_*
  // the pair's initial estimate is the prerejective alignment's
  bool prerejective(const mm3d_params *p) const { return !coarse && align && p->estimation_method == MM3D_EST_SAC_IA; }
  // the pair's initial estimate is the consistency graph's (MATCHING draws nothing from rand(): replay_method is as it was)
  bool consistency(const mm3d_params *p) const { return !coarse && estimator && p->estimation_method == MM3D_EST_MATCHING; }
  // The estimation method as the rand() replay sees it: neither the prerejective nor the correlative alignment draws from
  // rand(), which is MATCHING's case in pair_rand_replay
  int replay_method(const mm3d_params *p) const { return coarse || prerejective(p) ? (int)MM3D_EST_MATCHING : (int)p->estimation_method; }
  // such a pair is estimated by pairs_estimate_batch alone (pair_estimate_impl hands it a batch of one)
  bool batch_only(const mm3d_params *p) const { return icp || refine || coarse || confidence || color || generalized || rejecting() || geometric() || robust() || prerejective(p) || consistency(p) || sampler; }
};

// The feature / pair cache of mm3d_estimate_maps_transforms (mm3d_set_map_cache; the concrete class is map_cache.cpp's).  The
// drivers in capi.cpp only see this interface, so the host code links without it (tests/host_san).  One call at a time -- the
// context's lock: begin, then lookups and inserts from any worker thread of the call, then commit (the call succeeded) or
// abort (it did not: the cache is left exactly as it was before the call).
struct MapCacheBase {
  virtual ~MapCacheBase() = default;
  // sel: the call's stage selection (what keys a map's features and a pair's record besides the parameters)
  virtual void begin(size_t n_maps, const mm3d_params *p, const StageSelection &sel) = 0;
  // map `slot`'s packed upload `raw` (non-empty, on c's stream): the cached bundle, borrowed for the call, or null.  One launch and
  // one wait on c (a second compare-only launch and wait when the digest names another candidate than the slot's last entry).
  virtual const mm3d_map *lookup(Context *c, size_t slot, const mm3d_cloud *raw) = 0;
  // the bundle built from `raw` after lookup(slot) missed, complete on the device: the cache owns both from here on (the raw
  // points are kept for the exact compares of later calls)
  virtual void insert(size_t slot, std::unique_ptr<mm3d_cloud> raw, mm3d_map *m) = 0;
  // pair (source slot, target slot) of this call from generator state rnd (read under SAC_IA only): true and *out = the
  // record, with this call's indices, when one is reused
  virtual bool pair_lookup(size_t s, size_t t, const GlibcRand &rnd, mm3d_pair_result *out) = 0;
  virtual void pair_insert(size_t s, size_t t, const GlibcRand &rnd, const mm3d_pair_result &r) = 0;
  virtual void commit() = 0;
  virtual void abort() noexcept = 0;
};
}  // namespace mm3d

// the opaque C handles are these structs
struct mm3d_ctx : mm3d::Context {
  // mm3d_set_map_cache: null = off (the drivers take their plain path).  Owned by this context; never set on helpers or peers.
  mm3d::MapCacheBase *map_cache = nullptr;
  mm3d::StageSelection sel;
  // what the selected stages report of the most recent pair (mm3d_last_alignment_stats, mm3d_last_coarse_stats, mm3d_last_confidence_stats)
  mm3d_alignment_stats last_align_stats{0, 0, 0, -1, 0, 0};
  mm3d_coarse_stats last_coarse_stats{0, 0, 0, 0, 0, -1, 0, 0};
  mm3d_overlap_stats last_confidence_stats{0, 0, 0, 0, 0, 0, 0.0};
  mm3d_icp_rejection_stats last_reject_stats{0, 0, 0, INFINITY, 0, 0};   // (mm3d_last_icp_rejection_stats)
  mm3d_icp_robust_stats last_robust_stats{0, 0, 0.0, 0.0, 0, 0};         // (mm3d_last_icp_robust_stats)
  mm3d_icp_geometry_stats last_geometry_stats{0, 0, 0, 0, 0};            // (mm3d_last_icp_geometry_stats)
  mm3d_estimator_stats last_estimator_stats{0, 0, 0, 0, -1, -1, 0};      // (mm3d_last_estimator_stats)
  mm3d_icp_sampling_stats last_sampling_stats{0, 0, 0, 0, 0};            // (mm3d_last_icp_sampling_stats)
  mm3d_outlier_stats last_outlier_stats{0, 0, 0, 0, 0.0, 0.0, 0.0};      // (mm3d_last_outlier_stats)
  mm3d_cluster_stats last_cluster_stats{0, 0, 0, 0, 0, 0};               // (mm3d_last_cluster_stats)
  mm3d_smooth_stats last_smooth_stats{0, 0, 0, 0, 0, 0, 0.0};            // (mm3d_last_smooth_stats)
  mm3d_plane_stats last_plane_stats{0, 0, 0, 0, 0, 0, 0, 0, 0};          // (mm3d_last_plane_stats)
  mm3d_plane last_planes[8] = {};                                        // (mm3d_last_planes: the first last_plane_stats.planes of them)
  // mm3d_set_streams: helper contexts (one HIP stream + one host thread each while a call is running)
  // that mm3d_estimate_maps_transforms deals maps and pairs to; owned by this context
  std::vector<mm3d_ctx *> helpers;
  // mm3d_create_devices: the root contexts of the OTHER devices of the list (this context is the first device's); each has
  // its own helpers.  mm3d_estimate_maps_transforms then shards its two loops over the devices inside the library
  // (capi.cpp::estimate_maps_devices) and gathers the pair records through RCCL (devices.cpp).  Owned by this context.
  std::vector<mm3d_ctx *> peers;
  mm3d::DeviceSet *device_set = nullptr;                 // non-null exactly for contexts made by mm3d_create_devices
  // diagnostics of the most recent mm3d_estimate_maps_transforms (mm3d_last_run_*)
  double last_features_s = 0.0, last_total_s = 0.0;      // when the last map was ready / when the call returned
  double last_exchange_s = 0.0, last_pairs_s = 0.0, last_gather_s = 0.0;   // several devices: bundles moved / pairs done (slowest device) / the RCCL gather alone
  std::vector<size_t> last_points, last_keypoints;       // per input cloud, after filtering / after pruning
};

namespace mm3d {

struct GridView {
  float minx, miny, minz;
  float inv;   // 1 / cell
  float cell;
  int dx, dy, dz;
  const int *cell_start;
  const float4 *pts;   // cell-sorted; .w = original index bits
  int n;
  const unsigned char *dt;   // optional: Chebyshev distance (in cells, capped) to the nearest occupied cell
  int dt_cap;                // values > dt_cap are stored as 255
  // optional merged neighbourhood lists: nb_pts[nb_start[c] .. nb_start[c+1]) = every point of the
  // (2 nb_R + 1)^3 block of cells around cell c, so a fixed-radius query reads ONE contiguous span
  const int *nb_start;
  // .w = distance of the entry from the centre of cell c, and the list ascends in it: a nearest-point scan
  // stops once .w minus the cell's half diagonal exceeds what it still looks for.  (A list too long to
  // sort in LDS keeps stencil order and .w = 0: it is scanned to the end.)
  const float4 *nb_pts;
  int nb_R;
};

struct Grid {
  float cell = 0.f;
  float mn[3] = {0, 0, 0};
  int dims[3] = {1, 1, 1};
  DevBuf<int> cell_start;
  DevBuf<float4> sorted;
  int n = 0;
  DevBuf<unsigned char> dt;   // built on demand by grid_ensure_dt
  int dt_cap = 0;
  DevBuf<int> nb_start;       // built on demand by grid_ensure_nblists
  DevBuf<float4> nb_pts;      // x, y, z, distance from the list's cell centre
  int nb_R = 0;
  std::mutex cache_mu;        // grid_ensure_dt / grid_ensure_nblists
  GridView view() const
  {
    GridView v;
    v.minx = mn[0]; v.miny = mn[1]; v.minz = mn[2];
    v.inv = 1.0f / cell; v.cell = cell;
    v.dx = dims[0]; v.dy = dims[1]; v.dz = dims[2];
    v.cell_start = cell_start.get(); v.pts = sorted.get(); v.n = n;
    v.dt = dt.get(); v.dt_cap = dt_cap;
    v.nb_start = nb_start.get(); v.nb_pts = nb_pts.get(); v.nb_R = nb_R;
    return v;
  }
};

// The target side of NDT (ndt.hip, mm3d_set_refinement): one Gaussian per voxel of the global lattice, and a dense index over
// the voxel bounding box of the finite points, so that a lookup is one load.  48 B per occupied voxel plus 4 B per index cell.
struct NdtTable {
  double resolution = 0.0, regularisation = 0.0;   // what it was built with (a map's table is rebuilt when these change)
  int min_points = 0;
  float inv = 0.f;                                 // 1.0f / (float)resolution
  float mn[3] = {0, 0, 0};                         // the smallest voxel index per axis (an integer-valued float)
  int dims[3] = {0, 0, 0};                         // index cells per axis; cell ((i * dims[1]) + j) * dims[2] + k
  int n_voxels = 0;
  DevBuf<float4> rec;      // [n_voxels][3], ascending (i, j, k): {mean, valid} {P xx xy xz yy} {P yz zz, count bits, 0}
  DevBuf<int> index;       // [dims[0] * dims[1] * dims[2]]: the voxel's record, -1 = empty
};

// What the correlative alignment keeps of a map (align_correlative.hip, mm3d_set_coarse_alignment): the 2-D cells of its
// vertical structure and of its ground on the global lattice, as lists for the source role and as dense maps over the cell box
// of its counted points, padded by one cell, for the target role.
struct CoarseSignature {
  mm3d_coarse_options opt{};                       // what it was made with, cell resolved (a map's is remade when these change)
  float c = 0.f, inv = 0.f;                        // (float)cell, 1.0f / c
  int n_struct = 0, n_ground = 0;                  // fine structure cells, ground cells
  int mn[2] = {0, 0}, dims[2] = {0, 0};            // the dense frame: cell (i, j) is word (i - mn[0]) * dims[1] + (j - mn[1])
  int cmn[2] = {0, 0}, cdims[2] = {0, 0};          // the frame of the coarse cells
  DevBuf<int4> scells;     // [n_struct] (i, j, count, 0), ascending (i, j)
  DevBuf<int4> gcells;     // [n_ground] (i, j, count, height bits)
  DevBuf<int2> ccells;     // coarse cells (I, J), ascending; their number is n_coarse[0], on the device
  DevBuf<int> n_coarse;
  DevBuf<unsigned char> dil;   // dense: the structure cells dilated by one cell
  DevBuf<float> gh;            // dense: a ground cell's height, NaN elsewhere
};

// What the overlap confidence keeps of a map (confidence_overlap.hip, mm3d_set_confidence): which voxels of the global lattice
// lie within one voxel of a point, one bit each in 4 x 4 x 4 bricks, and which 8-voxel view cells the map has seen, one byte
// each; both dense over the brick box of the finite points.  8 B per brick plus 1 B per view cell.
struct OverlapTable {
  double voxel = 0.0;                              // what it was built with (a map's table is rebuilt when these change)
  int min_points = 0, view_margin = 0;
  float inv = 0.f;                                 // 1.0f / (float)voxel
  int b0[3] = {0, 0, 0}, nb[3] = {0, 0, 0};        // the brick box: minimum and extent; word ((bi-b0i) * nb[1] + (bj-b0j)) * nb[2] + (bk-b0k)
  int c0[3] = {0, 0, 0}, nc[3] = {0, 0, 0};        // the view-cell box, in the same order
  size_t n_finite = 0;                             // the cloud's finite points
  DevBuf<unsigned long long> near;                 // [nb[0] * nb[1] * nb[2]]
  DevBuf<unsigned char> view;                      // [nc[0] * nc[1] * nc[2]]
};

// What coloured ICP keeps of a map (icp_color.hip, mm3d_set_icp_color): per point the colour gradient on the tangent plane and
// the intensity, in the points' order.  16 B per point beside the 16 B of the normals they are made from.
struct ColorGradients {
  double radius = 0.0;                             // what it was built with (a map's records are rebuilt when these change)
  int min_neighbours = 0;
  size_t n = 0;
  DevBuf<float4> rec;                              // [n] (gx, gy, gz, I)
};

// What the boundary rejector keeps of a map (icp_geometry.hip, mm3d_set_icp_geometry_rejection): one flag per point, in the points'
// order.  1 B per point beside the 16 B of the normals they are made from.
struct BoundaryFlags {
  double radius = 0.0, angle_deg = 0.0;            // what they were made with, radius resolved (a map's flags are remade when these change)
  int min_neighbours = 0;
  size_t n = 0;
  long long n_boundary = 0;
  DevBuf<unsigned char> flags;                     // [n]
};

}  // namespace mm3d

struct mm3d_cloud {
  mm3d::DevBuf<float4> pts;
  size_t n = 0;
  // lazily computed, under cache_mu: several contexts (streams) may ask the same cloud for a structure that
  // mm3d_map_prepare did not build; the first builds it (and drains its stream), the others wait
  std::recursive_mutex cache_mu;
  bool have_bbox = false;
  float bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0};
  size_t n_finite = 0;
  std::map<int, std::unique_ptr<mm3d::Grid>> grids;   // key: cell size in units of 1e-4 m
  std::vector<float4> host;                            // host copy (keypoint clouds only)
  mm3d::DevBuf<float4> hil_pts;                        // finite points in Hilbert order, .w = original index
  mm3d::DevBuf<uint32_t> hil_keys;                     // their sort keys: (Hilbert index of the 0.25 m column << 10) | z cell
  mm3d::DevBuf<int2> wave_items;                       // {first point, count <= 64}: one compact patch per wave
  int n_wave_items = 0;
  // > 0: the points are centroids of distinct voxels of a VoxelGrid with this leaf (downsample made the cloud, or a filter kept
  // a subset of such a cloud), none farther than two leaves from a member of its voxel (checked on the device where the
  // centroids were formed).  A grid cell of side C then holds at most (floor(C / leaf) + 6)^3 of them, and cloud_grid need not
  // ask the device whether a cell outgrew its counting sort.  0: unknown (a caller's raw cloud, a copy from a peer).
  float voxel_leaf = 0.f;
  // the points were replaced (descriptor pruning): everything derived from them goes
  void reset_caches()
  {
    grids.clear(); host.clear(); have_bbox = false; n_finite = 0;
    hil_pts = mm3d::DevBuf<float4>(); hil_keys = mm3d::DevBuf<uint32_t>(); wave_items = mm3d::DevBuf<int2>(); n_wave_items = 0;
  }
};

struct mm3d_normals {
  mm3d::DevBuf<float4> nrm;
  size_t n = 0;
};

struct mm3d_desc {
  mm3d::DevBuf<float> data;
  size_t n = 0;
  int dim = 0;
  int type = 0;
  // target-side operands of the MFMA k-NN (column sums + centred, augmented, MFMA-ordered rows):
  // they depend on this set alone, so a map that is the target of 15 pairs prepares them once
  // (desc_knn_prepare_target, called from mm3d_map_prepare)
  mm3d::DevBuf<float> knn_colsum, knn_Bp;
  std::mutex cache_mu;        // desc_knn_prepare_target
  // the rows' Euclidean norms in ascending order and the row index of each (the exact fallback of the k-NN only
  // visits targets whose norm is within the current k-th distance of the query's: | |a| - |b| | <= |a - b|)
  mm3d::DevBuf<uint32_t> knn_nsort, knn_nperm;
  // SHOT only: the local reference frames (x, y, z axes, 9 floats per row) -- the "rf" field of
  // pcl::SHOT1344; not part of the point representation that matching reads
  mm3d::DevBuf<float> rf;
};

namespace mm3d {
// What ICP source sampling keeps of a map (icp_sample.hip, mm3d_set_icp_sampling): the sample as a cloud of its own, which carries
// the query order the ICP searches with like any other cloud.  16 B per sampled point plus that copy.
struct IcpSample {
  mm3d_icp_sampling_options opt{};                 // what it was made with (a map's sample is remade when these change)
  std::unique_ptr<mm3d_cloud> cloud;
  mm3d_icp_sampling_stats stats{0, 0, 0, 0, 0};
};
}  // namespace mm3d

// A map owns its parts: whoever holds the map frees all of them with `delete m` (mm3d_map_from_parts adopts the caller's).
struct mm3d_map {
  mm3d_cloud *points = nullptr;
  mm3d_cloud *keypoints = nullptr;
  mm3d_desc *desc = nullptr;
  // What the opt-in stages keep of the points, null until one asks: made and replaced through map_kept (map_kept.hpp) alone,
  // by mm3d_map_prepare or a pair's first use of the map.
  std::unique_ptr<mm3d_normals> normals;            // (normal_radius) point-to-plane, coloured and generalized ICP, the correlative signature
  std::unique_ptr<mm3d::NdtTable> ndt;              // NDT's voxel Gaussians
  std::unique_ptr<mm3d::CoarseSignature> coarse;    // the correlative alignment's signature
  std::unique_ptr<mm3d::OverlapTable> overlap;      // the overlap confidence's table
  std::unique_ptr<mm3d::ColorGradients> color;      // coloured ICP's gradient records
  std::unique_ptr<mm3d::IcpSample> icp_sample;      // the source sample of the ICP
  std::unique_ptr<mm3d::BoundaryFlags> boundary;    // the boundary rejector's flags
  mm3d_map() = default;
  mm3d_map(const mm3d_map &) = delete;
  mm3d_map &operator=(const mm3d_map &) = delete;
  ~mm3d_map() { delete points; delete keypoints; delete desc; }
};

namespace mm3d {

// grid.hip
void cloud_bbox(Context *c, mm3d_cloud *cl);
const Grid &cloud_grid(Context *c, const mm3d_cloud *cl, float cell);
// per-cell Chebyshev distance transform (capped at R cells), cached on the grid
void grid_ensure_dt(Context *c, const Grid &g, int R);
// per-cell merged candidate lists over the (2R+1)^3 block of cells, cached on the grid
void grid_ensure_nblists(Context *c, const Grid &g, int R);
// Hilbert-ordered copy of the finite points (.w = original index) + wave work items, cached on the cloud
// min_cell: lower bound of the Hilbert cell (a work item never straddles a block of 8 x 8 cells); callers whose cloud is
// sparser than 0.1 m (SIFT's later octaves) pass a larger one so that their items still hold 64 points
void cloud_hilbert(Context *c, const mm3d_cloud *cl, float min_cell = 0.25f);
mm3d_cloud *cloud_from_device(Context *c, DevBuf<float4> &&pts, size_t n);
mm3d_cloud *cloud_from_memory(Context *c, const void *src, size_t n, size_t stride, size_t rgba_off);
void cloud_download(Context *c, const mm3d_cloud *cl, void *dst, size_t stride, size_t rgba_off);
// wait = false: the copy is enqueued and the caller waits for the stream itself before the vector is read (by anybody)
const std::vector<float4> &cloud_host(Context *c, const mm3d_cloud *cl, bool wait = true);
// ordered compaction: keeps in[i] where flags[i] != 0, preserving order; returns kept count
size_t compact_points(Context *c, const float4 *in, const int *flags, size_t n, DevBuf<float4> &out, unsigned *box_host = nullptr);   // box_host: 7 words for cloud_set_bbox
void cloud_set_bbox(mm3d_cloud *cl, const unsigned box[7]);
// out holds m points in a buffer of `bound`: moved to a buffer of m when that one is large and mostly empty (grid.hip has the rule)
void refit_points(Context *c, DevBuf<float4> &out, size_t m, size_t bound);
// the points of `in` whose flag is set, in order, as a new cloud with its box (one wait); the input's voxel_leaf when asked
mm3d_cloud *cloud_of_kept(Context *c, const mm3d_cloud *in, const int *flags, bool inherits_leaf, size_t *kept = nullptr);
void exclusive_scan_int(Context *c, const int *in, int *out, size_t n);
// one chained-scan launch's share of the context's scan state (grid.hip::scan_prepare; scan_fused.hpp)
constexpr int kScanItems = 16, kScanTile = 256 * kScanItems;
struct ScanLaunchState { unsigned long long *status; unsigned *ticket; unsigned ticket_base, epoch, tiles; };
ScanLaunchState scan_prepare(Context *c, size_t n);
void counting_sort_pairs_u32(Context *c, const uint32_t *keys, int n, uint64_t key_range, uint32_t *keys_out, uint32_t *idx_out,
                             int *too_long, bool no_invalid_keys = false);
// The search-structure kernels' A/B switches ("Dependent-load chains"): -DMM3D_...=0 builds the earlier form.
#ifndef MM3D_ITEM_NEXT
#define MM3D_ITEM_NEXT 1        // a work item's length from the fused scan's head masks, not from a walk over the keys
#endif
#ifndef MM3D_PLACE_PAIRS
#define MM3D_PLACE_PAIRS 1      // the counting sorts scatter (key, index) pairs: the placing kernels read one level
#endif
#ifndef MM3D_VOXEL_FUSED
#define MM3D_VOXEL_FUSED 1      // the voxel filter's keys come with their histogram; too_long shares the counts' fill
#endif
#ifndef MM3D_HIL_BOX
#define MM3D_HIL_BOX 1          // the Hilbert columns' table is sized by the cloud's box (4^k columns), not 2^20
#endif
// The counting sort in two halves, for a caller whose own kernel makes the keys (filters.hip: the voxel key comes with its
// histogram).  begin: the bins of key_range, the counts and the too_long word zeroed by ONE fill, the ranks' buffer.  The
// caller's launch writes keys[i] and ranks[i] = atomicAdd(&counts[keys[i] / divisor], 1) for every key but 0xFFFFFFFF;
// finish scans, scatters and places as counting_sort_pairs_u32 does.  too_long() is read after the caller's next wait, while
// the object lives.
struct CountingSort {
  uint32_t divisor = 1;
  int nbins = 0;
  DevBuf<int> counts;             // nbins + 2: the bins, the scan's total, too_long
  DevBuf<uint32_t> ranks;
  int *too_long() const { return counts.get() + nbins + 1; }
};
CountingSort counting_sort_begin(Context *c, int n, uint64_t key_range);
void counting_sort_finish(Context *c, const CountingSort &cs, const uint32_t *keys, int n, uint32_t *keys_out, uint32_t *idx_out, bool no_invalid_keys);
void iota_u32(Context *c, uint32_t *v, int n);       // v[i] = i (the radix fallbacks' values)
void sort_pairs_u32(Context *c, const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout,
                    size_t n, int end_bit);

// filters.hip
mm3d_cloud *downsample(Context *c, const mm3d_cloud *in, double resolution);
bool downsample_is_identity(Context *c, const mm3d_cloud *in, double resolution);   // would downsample() return `in` bit for bit? (one small launch + a wait)
mm3d_cloud *remove_outliers(Context *c, const mm3d_cloud *in, double radius, int min_neighbours);
mm3d_cloud *transform_concat(Context *c, const mm3d_cloud *const *clouds, size_t n, const float *T);

// normals.hip
mm3d_normals *compute_normals(Context *c, const mm3d_cloud *in, double radius);

// sift.hip
mm3d_cloud *detect_keypoints_sift(Context *c, const mm3d_cloud *points, double min_scale, int nr_octaves, int nr_scales, double min_contrast,
                                  double normals_radius = 0.0, mm3d_normals **normals_out = nullptr, float grid_cell_hint = 0.0f);   // (+ the points' normals, fused when possible;
                                  // grid_cell_hint: cell of a grid the caller will build on `points` anyway)
void normals_of_items(Context *c, const mm3d_cloud *in, const Grid &g, double radius, const int *ov_items, const int *ov_count_dev, int n_overflow,
                      float4 *out);

// harris.hip
mm3d_cloud *detect_keypoints_harris(Context *c, const mm3d_cloud *points, const mm3d_normals *normals, double threshold,
                                    double radius);
void harris_response(Context *c, const mm3d_cloud *points, const mm3d_normals *normals, double radius, DevBuf<float> &out);

// fpfh.hip
mm3d_desc *compute_fpfh(Context *c, const mm3d_cloud *points, const mm3d_normals *normals,
                        mm3d_cloud *keypoints, double radius);
// test hook: atan2_fast(y, x) of the certified SPFH bins on device arrays (mm3d_debug_libm fn 9)
void debug_atan2_fast(Context *c, const float *x_dev, const float *y_dev, int n, float *out_dev);

// pfh.hip
mm3d_desc *compute_pfh(Context *c, const mm3d_cloud *points, const mm3d_normals *normals,
                       mm3d_cloud *keypoints, double radius);

mm3d_desc *compute_pfhrgb(Context *c, const mm3d_cloud *points, const mm3d_normals *normals,
                          mm3d_cloud *keypoints, double radius);

// test hooks of the four kernels that keep a neighbour list in LDS (pfh.hip holds the state; mm3d_debug_feature_lds_cap,
// mm3d_debug_feature_overflow).  family: 0 PFH / PFHRGB, 1 SHOT, 2 SC3D, 3 the Harris refinement.
int feature_lds_cap(int compiled);                          // the capacity the first launch is given
void feature_overflow_note(int family, int rows, int cap);  // a scratch pass of `rows` rows with `cap` entries each

void debug_libm(Context *c, int fn, const float *x_host, const float *y_host, int n, float *out_host);
void debug_float_chain(Context *c, const float *incr_host, const unsigned *hits_host, int n, float *out_host);
// sift.hip, test hooks of the certified SIFT decision (sift_cert.hpp): the unsorted scale space of ONE octave -- val* and the
// bound B per point and DoG column, [n][5] by the octave cloud's index -- and the process-wide statistics
size_t debug_sift_cert_octave(Context *c, const mm3d_cloud *points, double min_scale, int octave, float *val_host, float *bound_host, size_t capacity);
void debug_sift_cert_stats(long long *out, int reset);
void debug_sift_cert_min(int n);     // test hook: octaves of at least n points are certified (< 0: the default / MM3D_SIFT_CERT_MIN)

// rsd.hip
mm3d_desc *compute_rsd(Context *c, const mm3d_cloud *points, const mm3d_normals *normals,
                       mm3d_cloud *keypoints, double radius);

// sc3d.hip
mm3d_desc *compute_sc3d(Context *c, const mm3d_cloud *points, const mm3d_normals *normals,
                        mm3d_cloud *keypoints, double radius);

// shot.hip
mm3d_desc *compute_shot(Context *c, const mm3d_cloud *points, const mm3d_normals *normals,
                        mm3d_cloud *keypoints, double radius);

// desc_knn.hip
// k nearest rows of B for every row of A (squared L2, FLANN accumulation order); idx -1 padded
void desc_knn(Context *c, const mm3d_desc *A, const mm3d_desc *B, int k, DevBuf<int> &idx, DevBuf<float> &d2);
// cache the target-side operands of B on the set itself (a no-op for small or already prepared sets)
void desc_knn_prepare_target(Context *c, const mm3d_desc *B);
// the same for a subset of A's rows given as a device index list; result row r belongs to rows[r]
struct KnnRows { const mm3d_desc *A; const int *rows_dev; int n_rows; };
void desc_knn_rows_multi(Context *c, const KnnRows *srcs, int n_srcs, const mm3d_desc *B, int k, DevBuf<int> &idx, DevBuf<float> &d2);
void desc_knn_rows(Context *c, const mm3d_desc *A, const int *rows_dev, int n_rows, const mm3d_desc *B, int k,
                   DevBuf<int> &idx, DevBuf<float> &d2);

// registration.hip
struct IcpResult { float T[16]; int iterations; int converged; };
struct PairTail { float T[16]; int iterations; int converged; int n_corr; double score; };
// one pair of a batch of ICP + score tails (icp_score_batch): inputs (the common ones, then what each method's
// prepare_target or a stage-level call binds for its step), then the result
struct IcpScoreJob {
  const mm3d_cloud *src = nullptr, *tgt = nullptr;
  const float *guess_dev = nullptr;     // the guess on the device, or
  float guess_host[16] = {0};           // on the host
  PairTail out{};
  bool closed = false;
  const mm3d_normals *tgt_normals = nullptr;   // point-to-plane ICP: the target's normals, in its order
  const NdtTable *tgt_ndt = nullptr;           // NDT: the target's voxel table, and how many voxels a point reads (1 or 7)
  int ndt_neighbours = 7;
  // correspondence rejection (mm3d_set_icp_rejection; icp_reject.hip): non-null = the point-to-point and point-to-plane ICP run
  // the rejecting correspondence stage with these options (the same for every job of a batch), even when they reject nothing;
  // NDT does not read it.  reject_stats: the last iteration's counts.
  const mm3d_icp_rejection_options *reject = nullptr;
  mm3d_icp_rejection_stats reject_stats{0, 0, 0, INFINITY, 0, 0};
  // geometric rejectors (mm3d_set_icp_geometry_rejection; icp_geometry.hip, icp_reject.hip): non-null (with `reject` non-null) = the
  // rejecting step runs its step 1b with these options (the same for every job of a batch).  tgt_boundary: the target's flags on
  // the device, in its order (boundary == 1); the normals test reads src_normals and tgt_normals.  geometry_stats: the last
  // iteration's counts.
  const mm3d_icp_geometry_options *geometry = nullptr;
  const unsigned char *tgt_boundary = nullptr;
  long long tgt_boundary_points = 0;
  const mm3d_normals *geo_tgt_normals = nullptr;   // (tgt_normals stays what selects and feeds the point-to-plane rows)
  mm3d_icp_geometry_stats geometry_stats{0, 0, 0, 0, 0};
  // robust kernel (mm3d_set_icp_robust; icp_robust.hip): non-null = the point-to-point and point-to-plane ICP run the robust step
  // with these options (the same for every job of a batch); the other methods do not read it.  robust_stats: the last
  // iteration's counts.
  const mm3d_icp_robust_options *robust = nullptr;
  mm3d_icp_robust_stats robust_stats{0, 0, 0.0, 0.0, 0, 0};
  // coloured ICP (mm3d_set_icp_color; icp_color.hip): the target's gradient records on the device, in its order, and the weight
  // of the geometric rows (the same for every job of a batch)
  const float4 *tgt_color = nullptr;
  double color_lambda = 1.0;
  // generalized ICP (mm3d_set_icp_generalized; icp_generalized.hip): the source's normals, in its order, and epsilon (the same
  // for every job of a batch)
  const mm3d_normals *src_normals = nullptr;
  double generalized_epsilon = 1e-3;
  // source sampling (mm3d_set_icp_sampling; icp_sample.hip): what the ICP searches with in src's place, null = src itself.  The
  // score stays over src.
  const mm3d_cloud *icp_src = nullptr;
  const mm3d_cloud *icp_source() const { return icp_src ? icp_src : src; }
};
struct IcpStep;      // nn_core.hpp
// The ICP + score tail of a batch of pairs (nn.hip) with `method`'s ICP; null: the reference's point-to-point ICP.  When the ICP
// runs and the jobs carry rejection options, a method that can reject correspondences does; when they carry a robust kernel, the
// point-to-point and point-to-plane ICP run icp_robust.hip's step.  The score stays point-to-point.
void icp_score_batch(Context *c, const IcpMethodBase *method, IcpScoreJob *jobs, int n_jobs, bool run_icp, double max_corr_dist,
                     int max_iterations, double eps, bool want_score, double score_max_distance);
// What stands in the place of the pair stage's point-to-point ICP on a context: point-to-plane (mm3d_set_icp_method,
// icp_plane.hip), coloured ICP (mm3d_set_icp_color, icp_color.hip), generalized ICP (mm3d_set_icp_generalized,
// icp_generalized.hip) or NDT (mm3d_set_refinement, ndt.hip).  Like MapCacheBase,
// the drivers in capi.cpp only see this interface, so the host code links without the kernels (tests/host_san); a null
// pointer on the context means the reference's point-to-point ICP.
struct IcpMethodBase {
  virtual ~IcpMethodBase() = default;
  virtual int method() const = 0;                        // MM3D_ICP_*
  // this method's side of one icp_score_batch; reject: the batch's rejection options, or null.  Point-to-plane makes the
  // rejecting step with normals then; NDT and coloured ICP do not read it.
  virtual std::unique_ptr<IcpStep> step(const mm3d_icp_rejection_options *reject) const = 0;
  // what the method keeps on a target map beyond its search structures (point-to-plane's normals, NDT's voxel table, the
  // gradient records): made when missing or stale (map_kept.hpp; no wait when it is there), and bound to `job` when there is one
  virtual void prepare_target(mm3d_ctx *, const mm3d_map *, const mm3d_params *, IcpScoreJob *) const = 0;
  // the same for a pair's source map (generalized ICP's normals); the others keep nothing on a source
  virtual void prepare_source(mm3d_ctx *, const mm3d_map *, const mm3d_params *, IcpScoreJob *) const {}
};
inline int StageSelection::icp_method() const { return icp ? icp->method() : MM3D_ICP_POINT_TO_POINT; }
struct PairFront;
// The initial alignment of a context's pair stage under SAC_IA (mm3d_set_alignment; the one concrete class is
// align_prerej.hip's).  Like IcpMethodBase, the drivers in capi.cpp only see this interface, so the host code links without
// the new kernels (tests/host_san); a null pointer on the context means the reference's SAC-IA.
struct AlignMethodBase {
  virtual ~AlignMethodBase() = default;
  // the target-side structures a pair reads of a map's keypoints (mm3d_map_prepare)
  virtual void prepare(Context *c, const mm3d_cloud *kp, double inlier_distance) const = 0;
  // estimate_pair_front's SAC_IA branch with this method: f.dT0 / f.on_device, or the identity in f.T0
  virtual void front(Context *c, const mm3d_alignment_options &o, unsigned seed, const mm3d_cloud *skp, const mm3d_desc *sd,
                     const mm3d_cloud *tkp, const mm3d_desc *td, double inlier_distance, PairFront &f,
                     mm3d_alignment_stats *stats) const = 0;
};
// Where a whole-map call takes a map's keypoints from instead of detectKeypoints (mm3d_set_keypoints; the one concrete class
// is keypoints_uniform.hip's).  Like IcpMethodBase, the drivers in capi.cpp only see this interface, so the host code links
// without the new kernels (tests/host_san); a null pointer on the context means the reference's detectors.
struct KeypointSourceBase {
  virtual ~KeypointSourceBase() = default;
  virtual int source() const = 0;                        // MM3D_KEYPOINTS_*
  // the keypoints of the filtered cloud `points`, a new cloud complete on c's stream (one wait: its size)
  virtual mm3d_cloud *keypoints(Context *c, const mm3d_cloud *points, double leaf) const = 0;
};
// What takes the place of a pair's initial estimate (mm3d_set_coarse_alignment; the one concrete class is
// align_correlative.hip's).  Like AlignMethodBase, the drivers only see this interface, so the host code links without the
// new kernels (tests/host_san); a null pointer on the context means the estimate that estimation_method selects.
struct CoarseMethodBase {
  virtual ~CoarseMethodBase() = default;
  // the map's signature at the context's options (and the normals it is made from), made when missing or stale (map_kept.hpp)
  virtual void prepare(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p) const = 0;
  // the pair's initial estimate: f.dT0 / f.on_device, or the identity in f.T0
  virtual void front(mm3d_ctx *ctx, const mm3d_map *s, const mm3d_map *t, const mm3d_params *p, PairFront &f, mm3d_coarse_stats *stats) const = 0;
};
// What a pair record's confidence is when it is not the reference's (mm3d_set_confidence; the one concrete class is
// confidence_overlap.hip's).  Like CoarseMethodBase, the drivers and pair_estimate.cpp only see this interface, so the host
// code links without the new kernels (tests/host_san); a null pointer on the context means 1 / transformScore.
struct ConfidencePair { const mm3d_map *s, *t; const float *T; double confidence; };   // T: the pair's transform on the host, 16 floats
struct ConfidenceMethodBase {
  virtual ~ConfidenceMethodBase() = default;
  // the map's table at the context's options, made when missing or stale (map_kept.hpp)
  virtual void prepare(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p) const = 0;
  // the confidences of a batch of pairs at their host transforms: one launch, one wait; stats (may be null) receives the
  // last pair's counts
  virtual void score(mm3d_ctx *ctx, ConfidencePair *pairs, size_t n, const mm3d_params *p, mm3d_overlap_stats *stats) const = 0;
};
// What takes RANSAC's place behind estimation_method = MATCHING (mm3d_set_estimator; the one concrete class is
// estimate_consistency.hip's).  Like AlignMethodBase, the drivers and pair_estimate.cpp only see this interface, so the host
// code links without the new kernels (tests/host_san); a null pointer on the context means the reference's RANSAC.
struct EstimatorMethodBase {
  virtual ~EstimatorMethodBase() = default;
  // estimate_pair_front's MATCHING branch with this method: findFeatureCorrespondences, then the estimate in f.T0 and f.counts
  virtual void front(Context *c, const mm3d_estimator_options &o, const mm3d_cloud *skp, const mm3d_desc *sd, const mm3d_cloud *tkp,
                     const mm3d_desc *td, double inlier_threshold, size_t matching_k, PairFront &f, mm3d_estimator_stats *stats) const = 0;
};
// What the pair stage's ICP searches with when it is not the whole source map (mm3d_set_icp_sampling; the one concrete class is
// icp_sample.hip's).  Like IcpMethodBase, the drivers and pair_estimate.cpp only see this interface, so the host code links
// without the new kernels (tests/host_san); a null pointer on the context means every point of the source.
struct IcpSamplerBase {
  virtual ~IcpSamplerBase() = default;
  // the map's sample at the context's options (and, under NORMAL_SPACE, the normals it is made from), made when missing or stale
  // (map_kept.hpp; no wait when it is there); stats (may be null) receives what it was made with
  virtual const mm3d_cloud *sample(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p, mm3d_icp_sampling_stats *stats) const = 0;
};
// What filters a down-sampled map in removeOutliers' place behind the whole-map calls (mm3d_set_outlier_filter; the one concrete
// class is outliers_statistical.hip's).  Like KeypointSourceBase, the drivers and pair_estimate.cpp only see this interface, so the
// host code links without the new kernels (tests/host_san); a null pointer on the context means the reference's radius filter.
struct OutlierFilterBase {
  virtual ~OutlierFilterBase() = default;
  virtual int method() const = 0;                        // MM3D_OUTLIERS_*
  // the kept records of `in` in its order, a new cloud complete on c's stream (one wait: its size); stats (may be null)
  // receives the counts and the threshold
  virtual mm3d_cloud *filter(Context *c, const mm3d_cloud *in, const mm3d_outlier_options &o, mm3d_outlier_stats *stats) const = 0;
};
// What drops the small connected components of a map's filtered cloud behind the whole-map calls (mm3d_set_cluster_filter; the one
// concrete class is clusters_euclidean.hip's).  Like OutlierFilterBase, the drivers and pair_estimate.cpp only see this interface,
// so the host code links without the new kernels (tests/host_san); a null pointer on the context means that no such step runs.
struct ClusterFilterBase {
  virtual ~ClusterFilterBase() = default;
  // the kept records of `in` in its order, a new cloud complete on c's stream (one wait: its size); o.tolerance == 0 stands for
  // 2 * resolution; stats (may be null) receives the counts
  virtual mm3d_cloud *filter(Context *c, const mm3d_cloud *in, const mm3d_cluster_options &o, double resolution, mm3d_cluster_stats *stats) const = 0;
};
// What smooths a map's filtered cloud before its normals, and the composed map between its two voxel passes (mm3d_set_smoothing; the
// one concrete class is smooth_mls.hip's).  Like ClusterFilterBase, pair_estimate.cpp and capi.cpp only see this interface, so the
// host code links without the new kernels (tests/host_san); a null pointer on the context means that no such step runs.
struct SmootherBase {
  virtual ~SmootherBase() = default;
  // the records of `in` in its order, every valid one moved by the rule, a new cloud complete on c's stream (one wait: the
  // counts) whose voxel_leaf is 0; o.radius == 0 stands for 3 * resolution; stats (may be null) receives the counts
  virtual mm3d_cloud *smooth(Context *c, const mm3d_cloud *in, const mm3d_smooth_options &o, double resolution, mm3d_smooth_stats *stats) const = 0;
};
// What takes the dominant planes out of a map's filtered cloud behind the whole-map calls (mm3d_set_planes; the one concrete class
// is planes_ransac.hip's).  Like ClusterFilterBase, pair_estimate.cpp only sees this interface, so the host code links without
// the new kernels (tests/host_san); a null pointer on the context means that no such step runs.  The cluster filter comes with
// the call, since MM3D_PLANES_SET_ASIDE composes the two: the composition stays inside the kernel file.
struct PlaneFilterBase {
  virtual ~PlaneFilterBase() = default;
  // The map's cloud after the plane stage AND the cluster filter (`clusters` may be null: none selected), complete on c's stream.
  // REMOVE: the records without a plane, then the cluster filter on them.  SET_ASIDE: the plane records in the cloud's order, then
  // the cluster filter's result on the rest; without a cluster filter nothing runs and `in` is returned as a plain copy of the
  // pointer (the caller keeps its cloud).  o.distance == 0 stands for resolution / 2.  stats and planes (8 records) receive the
  // plane stage's counts and planes, cluster_stats (may be null) the cluster filter's.
  virtual mm3d_cloud *filter(Context *c, mm3d_cloud *in, const mm3d_plane_options &o, double resolution, const ClusterFilterBase *clusters,
                             const mm3d_cluster_options &cluster_options, mm3d_plane_stats *stats, mm3d_plane *planes,
                             mm3d_cluster_stats *cluster_stats) const = 0;
};
// What binds the geometric rejectors' operands to a pair (mm3d_set_icp_geometry_rejection; the one concrete class is
// icp_geometry.hip's).  Like IcpSamplerBase, the drivers and pair_estimate.cpp only see this interface, so the host code links
// without the new kernels (tests/host_san); a null pointer on the context means an inactive selection.
struct IcpGeometryBase {
  virtual ~IcpGeometryBase() = default;
  // the map's normals and, under `boundary`, its flags at the context's options, made when missing or stale (map_kept.hpp)
  virtual void prepare(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p) const = 0;
  // the same for a pair's two maps, bound to `job`: geometry, tgt_boundary, src_normals, geo_tgt_normals
  virtual void bind(mm3d_ctx *ctx, const mm3d_map *s, const mm3d_map *t, const mm3d_params *p, IcpScoreJob *job) const = 0;
};
struct PairCounts { int n_correspondences = 0, n_inliers = 0, icp_correspondences = 0; };
// ICP (optional) from a guess on the device (guess_dev != null) or on the host, then transformScore
// (optional) of the result, with one host synchronisation
PairTail icp_score(Context *c, const mm3d_cloud *src, const mm3d_cloud *tgt, const float *guess_dev, const float guess_host[16],
                   bool run_icp, double max_corr_dist, int max_iterations, double eps, bool want_score,
                   double score_max_distance);
IcpResult icp(Context *c, const mm3d_cloud *src, const mm3d_cloud *tgt, const float guess[16],
              double max_corr_dist, int max_iterations, double eps);
double transform_score(Context *c, const mm3d_cloud *src, const mm3d_cloud *tgt, const float T[16],
                       double max_distance);
// hypothesis scoring
void ransac_count(Context *c, const float4 *src_kp, const float4 *tgt_kp, const int *idx_src,
                  const int *idx_tgt, int n_corr, const float *T_all /* H*16 device */, int H,
                  double thr2, int *counts /* device H */);
// SAC-IA scoring of a batch of pairs (models from the replayed samples, truncated errors, their ordered sums, the
// first minimum): everything is device memory of the caller's, asynchronous
struct SacPair {
  const mm3d_cloud *src_kp, *tgt_kp;
  const int *samp;        // H*3: sampled source keypoints
  const int *corr_ref;    // H*3: index into nn
  const int *nn;          // k-NN table of the sampled rows
  float *T_best;          // out: the winning model, 16 floats
};
void sacia_score_batch(Context *c, const SacPair *pairs, int n, int H, float corr_thresh);
void debug_sacia_stats(long long out[4], int reset, int collect);
// build (and cache on the clouds) every search structure pair estimates with these parameters read
void prepare_pair_search(Context *c, const mm3d_cloud *points, double max_corr_dist, double score_max_distance);
void prepare_sacia_target(Context *c, const mm3d_cloud *kp, float corr_thresh);

// host_pipeline.cpp
size_t find_correspondences(Context *c, const mm3d_desc *s, const mm3d_desc *t, size_t k, std::vector<mm3d_corr> &out);
size_t ransac_transform(Context *c, const mm3d_cloud *skp, const mm3d_cloud *tkp, const mm3d_corr *corr,
                        size_t n_corr, double inlier_threshold, float T[16], std::vector<mm3d_corr> &inliers);
// What RANSAC's best model bT goes through (matching.cpp:127-140), shared with the consistency estimator: the correspondences
// within thr2 under bT in index order, failure (0, T and inliers as they were) below three of them or on an identity model,
// else umeyama_f32 over them into T.  is / it: the correspondences' keypoint indices, checked by the caller.
size_t ransac_model_tail(const std::vector<float4> &skp, const std::vector<float4> &tkp, const mm3d_corr *corr, const std::vector<int> &is,
                         const std::vector<int> &it, const float bT[16], double thr2, float T[16], std::vector<mm3d_corr> &inliers);
// T_dev == nullptr: the winning transform is returned in T (host).  Otherwise, when the device path
// ran, *T_dev receives it (16 floats on the device), T is left at identity and true is returned.
bool sac_ia(Context *c, const mm3d_cloud *skp, const mm3d_desc *sd, const mm3d_cloud *tkp, const mm3d_desc *td,
            double min_sample_distance, double max_corr_dist, int max_iterations, float T[16], bool execute,
            DevBuf<float> *T_dev = nullptr);
void sac_ia_draws(GlibcRand &rnd, const std::vector<float4> &skp, int ns, float min_sample_distance, int H, int kk, int *samp,
                  int *pick);
// advances rnd by the rand() draws one estimateTransform(source -> any non-empty target) consumes (host only)
void pair_rand_replay(GlibcRand &rnd, int method, const std::vector<float4> &skp_host, double inlier_threshold, int max_iterations);
// estimateTransform + (optionally) transformScore of the result; returns the ICP iteration count
// estimateTransform up to its initial estimate (correspondences + RANSAC, or SAC-IA): T0 on the host, or dT0 on the device
struct PairFront {
  float T0[16];
  DevBuf<float> dT0;
  bool on_device = false;
  PairCounts counts;
  // SAC-IA between its steps (sac_ia_replay / sac_ia_knn / sac_ia_finish): the replayed samples (samp | corr_ref |
  // rows, device) and the k-NN table of the sampled rows (its own buffer, or a slice of a batch's)
  DevBuf<int> sac_idx, sac_nn;
  DevBuf<float> sac_nd;
  const int *sac_nn_ptr = nullptr;
  int sac_rows = 0;          // distinct sampled rows
  int sac_h = 0;             // hypotheses to score; 0: nothing to do (too few keypoints, or not executed)
};
// SAC-IA in steps, so that several pairs can share launches: replay = the rand() stream and the upload of the
// sampled rows; knn = the descriptor k-NN of the sampled rows of every pair with the SAME target (td) as one search;
// finish = sacia_score_batch over the prepared pairs
void sac_ia_replay(Context *c, const mm3d_cloud *skp, const mm3d_desc *sd, const mm3d_cloud *tkp, const mm3d_desc *td,
                   double min_sample_distance, int max_iterations, bool execute, PairFront &f);
struct SacPrepared { const mm3d_cloud *skp, *tkp; const mm3d_desc *sd, *td; PairFront *front; };
void sac_ia_knn(Context *c, SacPrepared *same_target, int n, DevBuf<int> &nn_owner, DevBuf<float> &nd_owner);
void sac_ia_finish(Context *c, SacPrepared *pairs, int n, double max_corr_dist);
void estimate_pair_front(Context *c, const mm3d_cloud *skp, const mm3d_desc *sd, const mm3d_cloud *tkp, const mm3d_desc *td, int method,
                         double inlier_threshold, double max_corr_dist, int max_iterations, size_t matching_k, bool execute, PairFront &f);
int estimate_pair(Context *c, const mm3d_cloud *sp, const mm3d_cloud *skp, const mm3d_desc *sd, const mm3d_cloud *tp,
                  const mm3d_cloud *tkp, const mm3d_desc *td, int method, int refine, double inlier_threshold,
                  double max_corr_dist, int max_iterations, size_t matching_k, double eps, float T[16], bool execute,
                  bool want_score, double score_max_distance, double *score, PairCounts *counts = nullptr);
int estimate_transform(Context *c, const mm3d_cloud *sp, const mm3d_cloud *skp, const mm3d_desc *sd,
                       const mm3d_cloud *tp, const mm3d_cloud *tkp, const mm3d_desc *td, int method, int refine,
                       double inlier_threshold, double max_corr_dist, int max_iterations, size_t matching_k,
                       double eps, float T[16], bool execute);
int global_transforms(const mm3d_pair_result *pairs, size_t n_pairs, double thr, size_t n_clouds, float *out,
                      size_t *n_out);

// map_cache.hip
struct CloudDigest { unsigned long long h0 = 0, h1 = 0; bool equal = false; };
// one pass over n packed records at `a` (device, c's stream; ends in a wait): their 128-bit digest (want_digest) and whether
// they equal the n records at `hint` bit for bit (hint != null; equal is false without one)
CloudDigest cloud_digest_compare(Context *c, const float4 *a, const float4 *hint, size_t n, bool want_digest);

// devices.cpp (host only): one process, several GPUs
// The RCCL communicators of a device list (ncclCommInitAll) and what the devices exchange: the maps' bundles, pulled by the
// device that needs them with hipMemcpyPeerAsync over xGMI, and the pair records, all-gathered with ncclAllGather.
struct DeviceSet;
DeviceSet *device_set_create(const int *devices, int n);          // throws Error; distinct devices get a communicator each
void device_set_destroy(DeviceSet *ds);
bool device_set_has_comms(const DeviceSet *ds);                   // false only for the duplicate-device test hook
// a copy of `src` (which lives on src_device) on c's device: points, bounding box and the source-side search structures
// (Hilbert query copy, work items, their keys), and the host copy when `src` has one.  Asynchronous on c's stream.
mm3d_cloud *cloud_clone_from_peer(Context *c, const mm3d_cloud *src, int src_device);
mm3d_desc *desc_clone_from_peer(Context *c, const mm3d_desc *src, int src_device);
// rank r contributes send[r] (its records, `slots` of them, zero padded); out receives world * slots records, rank by rank,
// as they arrived on roots[0]'s device.  One ncclAllGather per rank inside one group; returns the seconds it took.
double gather_pair_records(DeviceSet *ds, const std::vector<mm3d_ctx *> &roots, const std::vector<std::vector<mm3d_pair_result>> &send,
                           size_t slots, std::vector<mm3d_pair_result> &out);

// linalg (host)
void umeyama_f32(const float *src, const float *dst, int n, float T[16]);
void umeyama_f64(const double *src, const double *dst, int n, double T[16]);
void mat4_mul(const float A[16], const float B[16], float out[16]);
void mat4_inverse(const float A[16], float out[16]);
void eigen33_values(const float cov[9], float evals[3]);

}  // namespace mm3d

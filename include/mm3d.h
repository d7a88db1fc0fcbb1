/*
 * mm3d.h -- C ABI of libmm3d.so, the MI355X (gfx950) registration engine that replaces the
 * hot path of map_merge_3d (static library `map_merging`, R/CMakeLists.txt:67-74).
 *
 * The reference has no FFI: its seam is the C++ free-function API in
 * R/include/map_merge_3d/{features,matching,map_merging}.h.  Every entry point below names the
 * reference declaration it replaces; include/map_merge_3d_shim.hpp shows the C++ forwarding
 * layer a maintainer links instead of the static library.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types; nothing throws across the boundary;
 *     every function returns an mm3d_status (MM3D_OK == 0) and mm3d_last_error() gives text.
 *   - "points" are pcl::PointXYZRGB payloads: float x,y,z at byte 0 and uint32 rgba
 *     (0xAARRGGBB, PCL byte order b,g,r,a) at byte `rgba_offset`, `stride` bytes apart.
 *     pcl::PointXYZRGB itself is stride 32 / rgba_offset 16; packed records are 16 / 12.
 *     Source pointers may be host or device (HBM) addresses.
 *   - 4x4 transforms are column-major float[16] (Eigen::Matrix4f storage); the all-zero matrix
 *     is the reference's "could not be estimated" sentinel (matching.h:41-42, map_merging.h:81-83).
 *   - enums carry the reference's integer values (features.h:20-24,49; matching.h:103).
 *   - one estimation at a time per context (internally serialised); contexts are independent.
 */
#ifndef MM3D_H_
#define MM3D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  MM3D_OK = 0,
  MM3D_EINVAL = -1,        /* bad argument (also: unknown enum string, like enums::from_string) */
  MM3D_EDEVICE = -2,       /* HIP runtime / device failure */
  MM3D_ENOMEM = -3,
  MM3D_EUNSUPPORTED = -4,  /* a size outside what the kernels are built for: an ordered-sum neighbourhood of more than 16384 points,
                              an SPFH neighbourhood of more than 65535, nr_scales != 3 (INTEGRATION.md "Size limits") */
  MM3D_ECAPACITY = -5      /* caller buffer too small; required size is reported */
} mm3d_status;

/* R/include/map_merge_3d/features.h:20-24 (ENUM_CLASS(Descriptor, PFH, PFHRGB, FPFH, RSD, SHOT, SC3D)) */
typedef enum { MM3D_DESC_PFH = 0, MM3D_DESC_PFHRGB, MM3D_DESC_FPFH, MM3D_DESC_RSD, MM3D_DESC_SHOT, MM3D_DESC_SC3D } mm3d_descriptor;
/* R/include/map_merge_3d/features.h:49 */
typedef enum { MM3D_KP_SIFT = 0, MM3D_KP_HARRIS } mm3d_keypoint;
/* R/include/map_merge_3d/matching.h:103 */
typedef enum { MM3D_EST_MATCHING = 0, MM3D_EST_SAC_IA } mm3d_estimation_method;
/* the ICP of the pair stage (mm3d_set_icp_method; not an enum of the reference's: it has point-to-point only) */
typedef enum { MM3D_ICP_POINT_TO_POINT = 0, MM3D_ICP_POINT_TO_PLANE = 1 } mm3d_icp_method;

/* enums::to_string / enums::from_string (R/include/map_merge_3d/enum.h:30-67) and the
 * PointCloud2 field-name table of R/src/dispatch_descriptors.h:38-48. */
const char *mm3d_descriptor_name(int d);              /* "PFH" ... or NULL */
int mm3d_descriptor_from_string(const char *s);       /* value or MM3D_EINVAL */
const char *mm3d_descriptor_field_name(int d);        /* "pfh","pfhrgb","fpfh","r_min","shot","shape_context" */
int mm3d_descriptor_dim(int d);                       /* 125, 250, 33, 2, 1344, 1980 */
const char *mm3d_keypoint_name(int k);
int mm3d_keypoint_from_string(const char *s);
const char *mm3d_estimation_method_name(int m);
int mm3d_estimation_method_from_string(const char *s);

/* MapMergingParams, field for field (R/include/map_merge_3d/map_merging.h:28-44). */
typedef struct {
  double resolution;
  double descriptor_radius;
  int outliers_min_neighbours;
  double normal_radius;
  int keypoint_type;
  double keypoint_threshold;
  int descriptor_type;
  int estimation_method;
  int refine_transform;
  double inlier_threshold;
  double max_correspondence_distance;
  int max_iterations;
  uint64_t matching_k;
  double transform_epsilon;
  double confidence_threshold;
  double output_resolution;
} mm3d_params;
/* the defaults of map_merging.h:28-44 (dependent defaults evaluated from resolution = 0.1) */
void mm3d_params_default(mm3d_params *p);
/* MapMergingParams::fromCommandLine (R/src/map_merging.cpp:10-54): "--name value", unknown
 * options ignored, matching_k applied only if > 0; bad enum string -> MM3D_EINVAL. */
int mm3d_params_from_command_line(int argc, const char *const *argv, mm3d_params *p);
/* operator<<(ostream, MapMergingParams) (R/src/map_merging.cpp:100-123); returns bytes needed. */
size_t mm3d_params_to_string(const mm3d_params *p, char *buf, size_t cap);

typedef struct { int32_t index_query, index_match; float distance; } mm3d_corr; /* pcl::Correspondence */

typedef struct mm3d_ctx mm3d_ctx;
typedef struct mm3d_cloud mm3d_cloud;      /* device-resident PointCloud<PointXYZRGB> */
typedef struct mm3d_normals mm3d_normals;  /* device-resident PointCloud<Normal> */
typedef struct mm3d_desc mm3d_desc;        /* device-resident descriptors (PCLPointCloud2 payload) */

/* ---- context -------------------------------------------------------------------------- */
int mm3d_create(int device, mm3d_ctx **out);
/* One process, several GPUs.  The reference's callers are single processes (MapMerge3d::transformsEstimation, a ROS timer
 * callback: R/src/map_merge_node.cpp:133-153; map_merge_tool's main: R/src/map_merge_tool.cpp:37-38), so the multi-GPU form
 * of the path sits behind the same entry point: a context made from a device list runs mm3d_estimate_maps_transforms
 * sharded over those devices INSIDE the library -- features by map owner, the other maps' bundles pulled GPU to GPU
 * (hipMemcpyPeerAsync over xGMI), pairs by target owner, ONE RCCL all-gather (ncclAllGather, communicators from
 * ncclCommInitAll) of the 104-byte pair records, pose graph on the host -- with the bits of one device.  Every other entry
 * point of such a context works on its first device.  mm3d_set_streams applies to every device of the list.
 * Creating the communicators takes seconds (once, here); librccl.so.1 is loaded by this call (a context made by mm3d_create
 * never needs it).  A device listed twice is MM3D_EINVAL (test hook:
 * MM3D_DEVICES_ALLOW_DUPLICATES=1 admits it, the records are then gathered through host memory instead of RCCL, which
 * refuses a device twice; mm3d_devices_use_rccl tells). */
int mm3d_create_devices(const int *devices, int n_devices, mm3d_ctx **out);
int mm3d_device_count(const mm3d_ctx *ctx);          /* 1 for a context made by mm3d_create */
int mm3d_device_at(const mm3d_ctx *ctx, int i);      /* the i-th device of the list, or MM3D_EINVAL */
int mm3d_devices_use_rccl(const mm3d_ctx *ctx);      /* 1: pair records travel through ncclAllGather; 0: plain context or the test hook */
void mm3d_destroy(mm3d_ctx *ctx);
const char *mm3d_last_error(const mm3d_ctx *ctx);   /* ctx == NULL: why this thread's last mm3d_create / mm3d_create_devices failed */
/* diagnostics of the most recent ICP run on this context (pcl::Registration::nr_iterations_, converged_) */
int mm3d_last_icp_iterations(const mm3d_ctx *ctx);
int mm3d_last_icp_converged(const mm3d_ctx *ctx);
/* debug counters (cost a host sync per call when on): descriptor k-NN rows that failed the MFMA
 * certificate and were redone by the exact kernel, out of all rows, since the last reset */
void mm3d_set_debug(mm3d_ctx *ctx, int on);
long long mm3d_debug_knn_fallback_rows(mm3d_ctx *ctx);
long long mm3d_debug_knn_rows(mm3d_ctx *ctx);
/* which routes the descriptor k-NN took on this context while mm3d_set_debug was on: one bit per route, read and cleared */
#define MM3D_KNN_PATH_SMALL 1u      /* small problems: plain brute force */
#define MM3D_KNN_PATH_LIST 2u       /* rows of 2 / 33 floats: candidate lists, every candidate re-ranked */
#define MM3D_KNN_PATH_FILTER 4u     /* rows of 2 / 33 floats against many targets: the threshold filter */
#define MM3D_KNN_PATH_LIST_WIDE 8u  /* rows of 125 floats: candidate lists, the pruned re-rank */
#define MM3D_KNN_PATH_WIDE_BF16 16u /* rows beyond 128 floats: the split-bf16 selector */
#define MM3D_KNN_PATH_WIDE_F32 32u  /* rows beyond 128 floats: the f32 selector (MM3D_KNN_WIDE_BF16=0) */
#define MM3D_KNN_PATH_ANY 64u       /* k beyond 16 */
unsigned mm3d_debug_knn_paths(mm3d_ctx *ctx);
/* host waits for the context's stream (and its mm3d_set_streams workers') since the context was made: out[0] = their number,
 * out[1] = nanoseconds spent in them */
void mm3d_debug_waits(mm3d_ctx *ctx, long long out[2]);
/* test hook: out[i] = the float sum "0 + incr[i] + incr[i] + ..." (hits[i] additions) as the PFH kernels
 * replay it for a histogram bin (PFHEstimation: "histogram[h] += hist_incr" once per pair) */
int mm3d_debug_float_chain(mm3d_ctx *ctx, const float *incr, const unsigned *hits, int n, float *out);
/* test hook: out[i] = the device's restatement of glibc's expf (fn 0), atanf (1), sinf (2), cosf (3) of x[i] or
 * atan2f(y[i], x[i]) (4) -- csrc/libm_exact.hpp, the functions the CPU path's PCL calls through libm */
int mm3d_debug_libm(mm3d_ctx *ctx, int fn, const float *x, const float *y, int n, float *out);
/* (fn 5: the raw v_exp_f32, 2^x, of the certified SIFT pass.
 *  fn 6: expf (|x| < 88) as the SIFT kernels call it: the 2^(i/32) table staged in LDS, no range checks (sift.hip).
 *  fn 7: lm::fdiv_const(x, y, (float)(1.0 / (double)y)), the division by a constant of the SIFT weights, with the
 *        reciprocal prepared as sift.hip prepares SiftScales::rcp.
 *  fn 8: acos_abs_greater(x, y) as 1.0f / 0.0f: computePairFeatures' "acos(fabs(x)) > acos(fabs(y))" in double.
 *  fn 9: atan2_fast(y, x), the polynomial arc tangent of the certified SPFH bins (fpfh.hip).
 *  fn 10, 11: the raw v_rsq_f32 and v_rcp_f32 of x.)
 * test hook: per pair i of (p1[4 i], n1[4 i]) and (p2[4 i], n2[4 i]) (x, y, z, w records), out[11 i ..] = the bits of f1, f2, f3
 * of the SPFH's exact pair features, their branch (0 no switch, 1 switched, 2 f4 == 0: the oracle's mo_pair_features code),
 * the exact path's three bins, the certified path's (pair_bins_fast) ok flag and its three bins (csrc/fpfh.hip) */
int mm3d_debug_pair_bins(mm3d_ctx *ctx, const float *p1, const float *n1, const float *p2, const float *n2, int n, int *out);
/* test hook, host code only (no context, no device): out[i] = the float chain "0 + incr[i] + incr[i] + ..." (hits[i] additions,
 * round to nearest even) as the SPFH kernel's epilogue replays it for a bin, in O(binades) (csrc/spfh_replay.hpp) */
void mm3d_debug_spfh_replay(const float *incr, const unsigned *hits, int n, float *out);
/* test hook: every wave-wide reduction / scan of csrc/device_util.hpp (DPP / permlane network) next to the shuffle loop it
 * replaced (kept in csrc/libm_debug.hip), on the same input: n elements (a multiple of 256: whole blocks of four waves), every
 * lane's result of the new form in out_new and of the old one in out_old, element type as the input's.
 * op 0 wave_sum(double), 1 wave_sum(float), 2 wave_sum(int) -- lane 0 of every wave holds the sum;
 * op 3 wave_min_int, 4 wave_max_int, 5 wave_min_f, 6 wave_max_f, 8 wave_min_u64 (uint64) -- every lane holds the result;
 * op 7 wave_scan_incl(int), the inclusive prefix sum. */
/* test hook: SAC-IA's error kernel takes k source keypoints per thread (1, 2, 4 or 8) in every launch from now on, whatever
 * its size; 0: chosen by the launch's size again; negative: no change.  Returns the count large launches use. */
int mm3d_debug_sacia_queries_per_thread(int k);
int mm3d_debug_wave_primitives(mm3d_ctx *ctx, int op, const void *in, int n, void *out_new, void *out_old);
/*
 * test hooks of the certified SIFT decision (csrc/sift_cert.hpp; the later octaves of detectKeypoints(SIFT),
 * R/src/features.cpp:45-62): the unsorted scale space of octave `octave` (0-based) on `points` -- val[5 i + s] and
 * bound[5 i + s] >= |the CPU path's float DoG - val| for point i of the octave's cloud -- *n_out = that cloud's size
 * (nothing is written when it exceeds capacity; 0: no such octave); and process-wide counters since the last reset:
 * out[0] octaves decided on the certified path, [1] their points, [2] points that took the exact sorted-list path,
 * [3] points left open by the first pass, [4] octaves sent back to the sorted-list path, [5] bound violations (must be 0),
 * [6] points still open after the second pass (must be 0), [7] work items the unsorted pass could not stage */
int mm3d_debug_sift_cert_octave(mm3d_ctx *ctx, const mm3d_cloud *points, double min_scale, int octave, float *val, float *bound,
                                size_t capacity, size_t *n_out);
void mm3d_debug_sift_cert_stats(long long out[8], int reset);
/* test hook: octaves of at least n points take the certified path (default 15 000, MM3D_SIFT_CERT_MIN; n < 0 restores it) */
void mm3d_debug_sift_cert_min(int n);
/* test hook: the exact DoG of single points as the certified octaves compute it for the points their certificate leaves open
 * (csrc/sift.hip::k_sift_dog_marked, one block per point).  The cloud of octave `octave` is built as
 * mm3d_debug_sift_cert_octave builds it; out[5 k + s] receives the CPU path's float DoG(ids[k], s) -- the raw values, before
 * anything is packed.  small_capacity != 0: the instantiation whose sort buffer holds 128 keys instead of 2048, so that
 * ordinary neighbour lists are worked in several distance bands.  n_ids == 0 does nothing.  MM3D_EINVAL: no such octave, an id
 * outside its cloud; MM3D_EUNSUPPORTED: a point has more neighbours at ONE distance than the sort buffer holds (its row is
 * left as it was, the other rows are written). */
int mm3d_debug_sift_dog_marked(mm3d_ctx *ctx, const mm3d_cloud *points, double min_scale, int octave, const int *ids, size_t n_ids,
                               int small_capacity, float *out);
/* test hook: the leaf of the VoxelGrid whose centroids the cloud's points are known to be (downSample's output and
 * removeOutliers' subset of it, R/src/features.cpp:19-40; every centroid within two leaves of a member of its voxel), 0 when
 * nothing is known -- what lets a grid build on the cloud skip its "did a cell outgrow the counting sort" wait */
float mm3d_debug_cloud_voxel_leaf(const mm3d_cloud *cloud);
/* test hook, process-wide like mm3d_debug_icp_rejection_split: the neighbour capacity the FIRST launch of the four kernels
 * that keep a neighbour list in LDS is given -- PFH / PFHRGB, SHOT, SC3D (1024 each) and the Harris corner refinement (2048).
 * A keypoint with more neighbours goes to the second launch of the same kernel with its list in global scratch; the LDS
 * arrays keep their size and the scratch pass is sized as always.  0 = the compile-time capacities; otherwise a power of two
 * from 64 to 2048, and a kernel whose own capacity is smaller keeps its own.  Anything else changes nothing.  Returns the
 * PREVIOUS value. */
int mm3d_debug_feature_lds_cap(int cap);
/* test hook: process-wide counters of that second launch since the last reset, two per kernel family in the order PFH / PFHRGB,
 * SHOT, SC3D, Harris refinement: out[2 f] the rows handed to the scratch pass, out[2 f + 1] the largest scratch capacity per
 * row chosen (PFH: the largest neighbour count; SHOT, SC3D: the power of two from 1024 that holds it; Harris: the power of two
 * from 2048 that holds twice it).  Both are values the host downloads anyway: counting adds no launch and no wait. */
void mm3d_debug_feature_overflow(long long out[8], int reset);
/* test / study hook of SAC-IA's certified pick (csrc/registration.hip::k_sacia_select; R/src/matching.cpp:142-194 ->
 * SampleConsensusInitialAlignment keeps the hypothesis of the lowest error sum): process-wide counters since the last reset --
 * out[0] pairs scored, [1] pairs whose winner the sums in double decided (no float chain was run), [2] candidate hypotheses
 * the intervals left, [3] float chains run.  collect = 1 / 0 switches the collection on / off (it costs a wait per batch;
 * MM3D_SACIA_STATS in the environment switches it on for the whole process), collect < 0 leaves it as it is */
void mm3d_debug_sacia_stats(long long out[4], int reset, int collect);
/* test / study hook: the descriptor k-NN of findFeatureCorrespondences (R/src/matching.cpp:50-75) on raw rows of width `dim`
 * -- the widths of the reference's descriptors (2, 33, 125, 250, 1344, 1980) and 352, pcl::SHOT352's shape, which the reference
 * does not bind (dispatch_descriptors.h:44-46 binds SHOT1344) but BASELINE.json configs[3] names: idx / d2 receive na x k
 * nearest target rows in FLANN's (distance, index) order, exact */
int mm3d_debug_desc_knn(mm3d_ctx *ctx, const float *a, size_t na, const float *b, size_t nb, int dim, int k, int *idx, float *d2);
/* test hook: the exact nearest-neighbour search behind mm3d_estimate_transform_icp and mm3d_transform_score (csrc/nn_search_body.hpp),
 * point by point.  Every source point is carried by the column-major T and searched in `target` within `range`, read as
 * convention 0: a distance, ICP's max_correspondence_distance; 1: mm3d_transform_score's max_distance, compared with the
 * SQUARED distance.  The largest squared distance in range, the search radius, the grid cell and the ring limit are derived
 * as those two entry points derive them.  split: 1 = one work item per wave, 4 = one per block (the library picks by the
 * source's size; here it is forced).  Per source point, in the caller's order: idx = the nearest target point's index (ties:
 * the lowest) or -1 for nothing in range and for a non-finite source point, d2 = the float squared distance the search holds,
 * +inf where idx is -1.  info (optional) receives what was derived; cell = 0 and n_items = 0 when there was nothing to
 * search (an empty or all-non-finite cloud). */
typedef struct mm3d_nn_search_info {
  float max_d2;        /* d2 <= max_d2 is in range */
  float rmax;          /* the radius the search proves */
  float cell;          /* the target grid's cell */
  float origin[3];     /* the grid's corner: the target's bounding-box minimum */
  int dims[3];         /* cells per axis */
  int max_ring;        /* a query whose cell is farther than this from every occupied cell (max-norm, in cells) is not searched */
  int n_items;         /* work items (<= 64 source points each) of the source */
} mm3d_nn_search_info;
int mm3d_debug_nn_search(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target, const float T[16], double range,
                         int convention, int split, int *idx, float *d2, mm3d_nn_search_info *info);
/* test hook: the Hilbert order and the wave work items of a cloud as every neighbourhood stage uses them (csrc/grid.hip:
 * cloud_hilbert).  The cell is max(0.25, min_cell, largest box side / 1023); the finite points are sorted, stably, by (Hilbert
 * index of their x, y column << 10 | z cell); a work item starts at the first point, at every change of the 8 x 8 column block
 * (key >> 16) and at every 64th point.  order[cloud size]: the original index of the j-th sorted point, -1 behind the finite
 * points.  items[items_cap][2]: {first sorted point, count <= 64} per item; *n_items of them (an error if more than items_cap:
 * cloud size / 64 + 16386 always suffices).  The cloud must not have been used by a stage yet: the order is cached on it. */
int mm3d_debug_hilbert_order(mm3d_ctx *ctx, const mm3d_cloud *cloud, float min_cell, int *order, int *items, size_t items_cap, int *n_items);
/* test hook: the counting sort behind the voxel filter (csrc/grid.hip) on n > 0 host keys, each below key_range <= 2^32 - 1 or
 * 0xFFFFFFFF (a point in no voxel: it stays out of the result; not allowed with no_invalid_keys != 0, the caller's promise
 * that there is none).  keys_out / idx_out [n]: the valid keys in ascending order, ties by ascending index, and their indices;
 * entries behind them read 0xFFFFFFFF.  A bin (key / ceil(key_range / 2^22)) that holds more than 1024 keys sets *too_long,
 * and nothing is sorted: both arrays read 0xFFFFFFFF throughout. */
int mm3d_debug_counting_sort(mm3d_ctx *ctx, const uint32_t *keys, size_t n, uint64_t key_range, int no_invalid_keys, uint32_t *keys_out,
                             uint32_t *idx_out, int *too_long);
/* SAC-IA draws from libc rand() in the reference (process-global, glibc seed 1).  The context
 * carries its own replay of that generator; mm3d_srand re-seeds it (srand semantics). */
void mm3d_srand(mm3d_ctx *ctx, unsigned seed);
/* Number of HIP streams (each with its own memory pool and, while a call runs, its own host thread)
 * that mm3d_estimate_maps_transforms deals the per-cloud and per-pair loops of
 * map_merging.cpp:212-242,256-269 to.  1 (the default) = the reference's sequential loops on one
 * stream.  One pair is a chain of dependent kernels that cannot fill an MI355X by itself; 16 streams
 * roughly double the throughput.  The results do not depend on the setting, bit for bit: every
 * stream replays the rand() draws of the pairs it does not run.  When many pairs are ready at once (many small
 * maps) a stream takes up to 16 of them that share their target and runs them as one batch (one descriptor
 * search, one launch per step for all of them); the results are the sequential loop's all the same.
 * A stream's host thread polls and naps while it waits for the device (about 0.2 of a core per busy stream; MM3D_WAIT=spin
 * makes it spin): far more streams than the process has CPUs (a container's quota counts) slow everything down, and the
 * device runs four kernels at a time anyway.  1 <= n <= 64. */
int mm3d_set_streams(mm3d_ctx *ctx, int n_streams);
int mm3d_get_streams(const mm3d_ctx *ctx);
/* diagnostics of the most recent mm3d_estimate_maps_transforms on this context: seconds from entry
 * until the last map's features existed and until the call returned; per input cloud, the number
 * of points after downSample + removeOutliers and of keypoints after descriptor pruning (returns
 * the number of clouds; at most `capacity` entries are written) */
int mm3d_last_run_stage_seconds(const mm3d_ctx *ctx, double *features_s, double *total_s);
/* the same for a device-list context: seconds from entry until the slowest device had pulled the other maps' bundles, until
 * the slowest device had finished its pairs, and the duration of the RCCL gather of the pair records alone */
int mm3d_last_run_device_seconds(const mm3d_ctx *ctx, double *exchange_s, double *pairs_s, double *gather_s);
size_t mm3d_last_run_map_sizes(const mm3d_ctx *ctx, size_t *points, size_t *keypoints, size_t capacity);
/* Feature / pair cache of mm3d_estimate_maps_transforms (off by default).  max_maps > 0 keeps the bundles of up to max_maps
 * distinct input clouds and the pair records among them; 0 turns it off and frees it.  The results of every call are the
 * bits of the same call on a context without a cache in the same generator state, and so is the generator state it leaves.
 *   - A map hits when its n packed records (x, y, z, rgba as mm3d_cloud_create packs them; the padding of wider records does
 *     not count, floats compare as bits) equal a cached cloud's, byte for byte, and every parameter the per-cloud loop reads
 *     is the same (resolution, descriptor_radius, outliers_min_neighbours, normal_radius, keypoint_type, keypoint_threshold,
 *     descriptor_type, max_correspondence_distance, estimation_method).  The slot does not matter: maps may be reordered,
 *     added, or passed twice.  Deciding costs one device pass over the uploaded records and one wait per map; a hit runs
 *     nothing else on the device for that map.  Null and empty clouds are never cached.
 *   - A pair record is reused when both its maps hit (in the same source -> target order) and the parameters the pair loop
 *     reads are the same (estimation_method, refine_transform, inlier_threshold, max_correspondence_distance,
 *     max_iterations, matching_k, transform_epsilon) -- and, under SAC_IA, the rand() state it starts from: without
 *     mm3d_srand to the same seed before each call the generator has moved on, and SAC_IA reuses the features only.
 *     The draws of a reused pair are replayed, so the generator ends where it would have.  confidence_threshold and
 *     output_resolution are read by neither key: the pose graph runs on every call.
 *   - Memory: each cached map keeps its packed input records on the device (16 B per point, 8 MB for 500 000 points) next
 *     to its filtered points, keypoints, descriptor rows and search structures.
 *   - Least recently used maps are evicted (at the end of a call; a call's own maps are never evicted while it runs),
 *     and with them every pair record that names them; at most 4 * max_maps^2 pair records are kept.  A call that fails
 *     leaves the cache as it was.  The cache survives mm3d_set_streams and goes with mm3d_destroy.
 * MM3D_EINVAL: ctx NULL or max_maps < 0; MM3D_EUNSUPPORTED: a device-list context (mm3d_create_devices).  Not for
 * mm3d_shard_* or mm3d_compose_maps. */
int mm3d_set_map_cache(mm3d_ctx *ctx, int max_maps);
int mm3d_get_map_cache(const mm3d_ctx *ctx);               /* max_maps, 0 when off or ctx NULL */
void mm3d_map_cache_clear(mm3d_ctx *ctx);                  /* drops every cached map and pair record */
/* out[0] map hits, [1] map misses, [2] pairs reused, [3] pairs computed (of calls that succeeded), [4] maps held now, [5] device
 * bytes held by the cache (raw copies, filtered points, keypoints, descriptor rows and their search structures, as of the
 * last call); counters since the last reset (reset != 0 resets them after reading).  All zero when the cache is off. */
int mm3d_map_cache_stats(const mm3d_ctx *ctx, long long out[6], int reset);   /* MM3D_EINVAL for NULL */
/* ICP of the pair stage (off the reference's path; MM3D_ICP_POINT_TO_POINT, the reference's, by default).
 * MM3D_ICP_POINT_TO_PLANE: PCL's IterativeClosestPoint with TransformationEstimationPointToPlaneLLS, the target's normals
 * being exactly mm3d_compute_normals(target points, normal_radius).  The loop is the point-to-point one in every respect
 * but the estimate: the source transformed by the current T in float, the exact float nearest neighbour accepted at
 * d2 <= max_correspondence_distance^2, fewer than 3 correspondences stop (not converged), T <- Tinc * T in float, and the
 * convergence tests of DefaultConvergenceCriteria (max_iterations -- reported as converged, as in PCL --, the rotation /
 * translation of Tinc against transform_epsilon, the change of the mean point-to-point d2 below 1e-12).  The estimate: for
 * each correspondence (s = transformed source point, d = target point, n = its normal) whose normal is finite, the row
 * [a, b, c, nx, ny, nz] with a = nz sy - ny sz, b = nx sz - nz sx, c = ny sx - nx sy and r = n.d - n.s; AtA and Atr are
 * summed in double, AtA x = Atr is solved in double, and Tinc = [Rz(x2) Ry(x1) Rx(x0) | x3 x4 x5].  A correspondence whose
 * normal is not finite counts (and its d2 enters the MSE) but adds no row.  The sign of a normal does not matter (AtA and
 * Atr do not change under n -> -n).  Unlike PCL, a degenerate system is defined: with fewer than 6 rows, or a pivot of the
 * (unpivoted LDLt) solve at or below 1e-12 * trace(AtA) / 6 -- a single plane, a line --, the loop stops, not converged,
 * with T as it was before that iteration (PCL inverts the singular matrix).
 *   - Applies to the ICP of mm3d_estimate_maps_transforms (every driver, with or without the map cache) and of
 *     mm3d_pair_estimate; transformScore (the pair's confidence) stays point-to-point.  mm3d_estimate_transform_icp and
 *     mm3d_estimate_transform mirror reference functions that take no normals: they stay point-to-point whatever the setting.
 *   - Maps keep their normals (mm3d_map_features made them anyway) and mm3d_map_prepare makes them for maps that lack them
 *     (mm3d_map_from_parts, maps made while the context was point-to-point); a pair whose target has none makes them on
 *     first use.  Memory: 16 B per filtered point of every map, cached maps included (mm3d_set_map_cache), and only
 *     while the setting is point-to-plane.
 *   - The setting reaches the context's mm3d_set_streams helpers, in either order of the two calls.  Results are
 *     bit-identical for every stream count, batch and cache setting, as for point-to-point.
 * MM3D_EINVAL: ctx NULL or an unknown method; MM3D_EUNSUPPORTED: a device-list context (mm3d_create_devices), whose bundles
 * carry no normals -- nor does mm3d_shard_begin, which returns MM3D_EUNSUPPORTED on a point-to-plane context. */
int mm3d_set_icp_method(mm3d_ctx *ctx, int method);
int mm3d_get_icp_method(const mm3d_ctx *ctx);              /* MM3D_ICP_*, MM3D_EINVAL for NULL */
/* Initial alignment of the pair stage where params.estimation_method == SAC_IA (off the reference's path;
 * MM3D_ALIGN_SAC_IA, the reference's, by default; MATCHING is untouched).  MM3D_ALIGN_PREREJECTIVE runs the algorithm of
 * pcl::SampleConsensusPrerejective (Buch et al., ICRA 2013) -- the algorithm, not its random stream: no parity is claimed --
 * on the inputs SAC-IA gets (keypoints, descriptors, inlier distance = max_correspondence_distance), wholly on the device:
 *   - Table: the k' = min(k, n_target) nearest target descriptors of every source keypoint (findFeatureCorrespondences'
 *     exact search), nearest first.
 *   - Draw h, 0 <= h < samples, from six 64-bit words w_j = mix(((seed << 32) | h) + (j + 1) * 0x9E3779B97F4A7C15 mod 2^64),
 *     mix = splitmix64's finaliser (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 *     z ^= z >> 31), seed = the last mm3d_srand value (1 without one; 0 counts as 1, as srand does), and
 *     bounded(w, n) = ((w >> 32) * n) >> 32.  Three distinct source keypoints: i0 = bounded(w0, ns); i1 = bounded(w1, ns - 1),
 *     plus one if >= i0; i2 = bounded(w2, ns - 2), plus one if >= min(i0, i1), then plus one if >= max(i0, i1).  Their
 *     targets: table[i_j][bounded(w_{3+j}, k')].  The stream is a function of (seed, h, ns, k') alone: not of the pair's
 *     place in the pair loop, the stream count, batching or the cache.  It consumes NOTHING from the context's rand() replay,
 *     so mm3d_pair_estimate(execute = 0) and mm3d_pairs_skip advance nothing for such a pair.
 *   - Prerejection: for each of the three edges, the squared lengths ds (source) and dt (target), ((dx dx + dy dy) + dz dz)
 *     in double on the float coordinates; the draw survives when ds > 0, dt > 0 and min(ds, dt) >= similarity^2 max(ds, dt)
 *     on all three -- the edge-length ratio min / max >= similarity -- and its three targets are distinct.  Anything not
 *     finite fails the test.
 *   - Hypothesis of a survivor: Umeyama's closed form without scale on the three pairs (means, covariance and the 3x3 SVD in
 *     double), rounded to a float 4x4.
 *   - Score: every source keypoint transformed in float, its exact float nearest target keypoint (a grid of the target's
 *     keypoints, built by mm3d_map_prepare); an inlier when d2 <= (float)(inlier distance^2).  Per hypothesis the inlier
 *     count (integer) and the inliers' d2 sum (double, in a fixed order: bit-identical whatever else runs).
 *   - Pick: among the hypotheses with count >= 1 and count >= inlier_fraction * ns, the lowest mean inlier d2; ties to the
 *     lower h.  Then one refit -- Umeyama in double over all the winner's (keypoint, nearest target) inlier pairs --, scored
 *     the same way and kept when it has more inliers, or as many and a mean d2 not larger.  converged = 1.
 *     If no hypothesis reaches the fraction: the one with the most inliers (ties to the lower h), no refit, converged = 0.
 *     No survivor at all, or fewer than three keypoints on either side: the identity (SAC-IA's guess), converged = 0.
 *     The pair goes on to ICP and its record as after SAC-IA, converged or not.
 *   - Results are bit-identical for every stream count, batch, driver and cache setting, and after mm3d_srand to the same seed.
 *   - The map cache's pair key holds the method and its four options, and for a prerejective pair the seed in place of the
 *     rand() state: such a record is reused without mm3d_srand between the calls. */
typedef enum { MM3D_ALIGN_SAC_IA = 0, MM3D_ALIGN_PREREJECTIVE = 1 } mm3d_align_method;
typedef struct mm3d_alignment_options {
  int method;                 /* MM3D_ALIGN_* */
  int samples;                /* raw draws, 1 .. 2^30 */
  int k;                      /* candidate matches per source keypoint, 1 .. 64 (10: SAC-IA's k_correspondences) */
  double similarity;          /* edge-length ratio a draw must reach, 0 .. 1 */
  double inlier_fraction;     /* of the source keypoints, 0 .. 1 */
} mm3d_alignment_options;
typedef struct mm3d_alignment_stats {
  long long draws;            /* samples */
  long long survivors;        /* draws that passed the prerejection */
  long long hypotheses_scored;/* survivors, plus one for the refit when it ran */
  long long winner_h;         /* the chosen draw, -1 when there was none */
  int winner_inliers;         /* inliers of the returned transform */
  int converged;              /* 1 when a hypothesis reached inlier_fraction */
} mm3d_alignment_stats;
/* method MM3D_ALIGN_SAC_IA, samples 2^16 (DESIGN.md section 7c has the measurement), k 10, similarity 0.9, inlier_fraction 0.25 */
void mm3d_alignment_options_default(mm3d_alignment_options *o);
/* MM3D_EINVAL: ctx or options NULL, an unknown method, a value outside its range above (the values are checked whatever the
 * method).  MM3D_EUNSUPPORTED: MM3D_ALIGN_PREREJECTIVE on a device-list context (mm3d_create_devices); mm3d_shard_begin
 * returns MM3D_EUNSUPPORTED on a prerejective context.  The setting reaches the context's mm3d_set_streams helpers, in
 * either order of the two calls. */
int mm3d_set_alignment(mm3d_ctx *ctx, const mm3d_alignment_options *options);
int mm3d_get_alignment(const mm3d_ctx *ctx, mm3d_alignment_options *options);      /* MM3D_EINVAL for NULL */
/* The alignment of the last pair that mm3d_pair_estimate or the one-stream mm3d_estimate_maps_transforms ran with
 * MM3D_ALIGN_PREREJECTIVE on this context (all zero, winner_h -1, before the first).  MM3D_EINVAL for NULL. */
int mm3d_last_alignment_stats(const mm3d_ctx *ctx, mm3d_alignment_stats *stats);
/* Where the whole-map calls take a map's keypoints from (off the reference's path; MM3D_KEYPOINTS_REFERENCE, the reference's
 * detectKeypoints(params.keypoint_type), by default).  With MM3D_KEYPOINTS_UNIFORM every place that runs detectKeypoints
 * behind a whole-map call -- mm3d_map_features, mm3d_estimate_maps_transforms on one stream or many, on a device list
 * (mm3d_create_devices) and mm3d_shard_begin -- takes mm3d_uniform_keypoints(the filtered points, leaf) instead: no detector,
 * an evenly spaced subset of the cloud (what PCL's own alignment tutorials describe with pcl::UniformSampling), so that a map
 * without colour or corners still has keypoints and two independent samplings of one surface have keypoints within about one
 * leaf of each other.  params.keypoint_type and params.keypoint_threshold are then not read (values outside the enum still
 * answer MM3D_EINVAL); mm3d_params does not change.  The normals come from their stand-alone launch (SIFT's fused first octave
 * does not run); descriptors, their pruning of the keypoints, either estimation method, either alignment and either ICP are
 * the existing code on the new keypoint cloud.  The stand-alone mm3d_detect_keypoints is untouched.
 *   - leaf > 0: the spacing in metres; 0: params.descriptor_radius / 2 (DESIGN.md section 7d has the measurement).
 *   - The setting reaches the context's mm3d_set_streams helpers in either order of the two calls, and every device of a
 *     device-list context; only a map's features change, and those travel in the bundles, so device lists and shards carry it.
 *     Every rank of a sharded call must use the same setting.  Results are bit-identical for every stream count, driver and
 *     cache setting.
 *   - The map cache's map key holds (source, leaf): a bundle of one source is never served to the other. */
typedef enum { MM3D_KEYPOINTS_REFERENCE = 0, MM3D_KEYPOINTS_UNIFORM = 1 } mm3d_keypoint_source;
typedef struct mm3d_keypoint_options {
  int source;                 /* MM3D_KEYPOINTS_* */
  double leaf;                /* > 0; 0 = descriptor_radius / 2, see above */
} mm3d_keypoint_options;
void mm3d_keypoint_options_default(mm3d_keypoint_options *o);     /* source MM3D_KEYPOINTS_REFERENCE, leaf 0 */
/* MM3D_EINVAL: ctx or options NULL, an unknown source, a leaf that is neither 0 nor one mm3d_uniform_keypoints takes (the
 * value is checked whatever the source). */
int mm3d_set_keypoints(mm3d_ctx *ctx, const mm3d_keypoint_options *options);
int mm3d_get_keypoints(const mm3d_ctx *ctx, mm3d_keypoint_options *options);        /* MM3D_EINVAL for NULL */
/* What filters a down-sampled map before anything else looks at it (off the reference's path; MM3D_OUTLIERS_RADIUS, the
 * reference's removeOutliers(descriptor_radius, outliers_min_neighbours), by default).  The radius filter is a fixed density
 * threshold: a map somewhat sparser than its two numbers assume is deleted whole.  With MM3D_OUTLIERS_STATISTICAL every place
 * that runs removeOutliers behind a whole-map call -- mm3d_map_features, mm3d_estimate_maps_transforms on one stream or many, on
 * a device list (mm3d_create_devices) and mm3d_shard_begin -- takes mm3d_remove_outliers_statistical(the down-sampled points,
 * mean_k, stddev_mult) instead: the density-adaptive filter that users of pcl::StatisticalOutlierRemoval and Open3D's
 * remove_statistical_outlier expect.  params.outliers_min_neighbours is then not read by the filter; descriptor_radius keeps
 * every other role; mm3d_params does not change.  The stand-alone mm3d_remove_outliers is untouched.
 *   The rule, for a cloud of n records, mean_k in 1 .. 64 and stddev_mult finite and >= 0 (no parity with PCL's class is
 *   claimed):
 *   1. A point is valid when its three coordinates are finite.  Invalid points are never kept, never counted and never anybody's
 *      neighbour.  n_valid counts the valid points.
 *   2. k' = min(mean_k, n_valid - 1).  If n_valid <= 1, every valid point is kept and the statistics are zero.
 *   3. For a valid point i, take the k' smallest values of the multiset { d2(i, j) : j valid, j != i }, where
 *      d2 = (dx * dx + dy * dy) + dz * dz in float, every operation rounded to nearest, nothing contracted.  A duplicate point
 *      has d2 = 0 and is a neighbour.  d_i = (sum of sqrt((double)d2)) / k', summed in double in ascending order of d2.  Which
 *      of several equal distances is taken cannot change d_i, so the rule names no tie-break.
 *   4. S = sum d_i and Q = sum d_i^2 over the valid points, in double, in a fixed order that depends on the cloud alone (blocks
 *      of 4096 consecutive records: lane l of 256 adds records l, l + 256, ... in that order, the lanes by a fixed tree, the
 *      blocks in ascending order), never on stream count, batch, cache, driver or device.  mu = S / n_valid;
 *      var = max(0, (Q - S * S / n_valid) / (n_valid - 1)), PCL's formula; sigma = sqrt(var); t = mu + stddev_mult * sigma.
 *   5. Point i is kept iff it is valid and d_i <= t.  The result is the kept 16-byte records in the cloud's order, colour
 *      included.
 *   - mean_k is capped at 64: one wave's width on this hardware, and above PCL's tutorial value (50) and Open3D's (20).
 *   - The defaults (16, 2.0) removed 97 - 100 % of 150 points planted in the free space of a 4 000-point room and kept at least
 *     99.9 % of the room (DESIGN.md section 7n has the table).
 *   - The setting reaches the context's mm3d_set_streams helpers in either order of the two calls, and every device of a
 *     device-list context; only a map's features change, and those travel in the bundles, so device lists and shards carry it.
 *     Every rank of a sharded call must use the same setting.  Nothing is drawn from rand().  Results are bit-identical for
 *     every stream count, driver, batch and cache setting.
 *   - The map cache's map key holds (method, mean_k, stddev_mult), zeros under MM3D_OUTLIERS_RADIUS: a radius-filtered bundle
 *     is never served for a statistical one, nor one of other options. */
typedef enum { MM3D_OUTLIERS_RADIUS = 0, MM3D_OUTLIERS_STATISTICAL = 1 } mm3d_outlier_method;
typedef struct mm3d_outlier_options {
  int method;                 /* MM3D_OUTLIERS_* */
  int mean_k;                 /* 1 .. 64 */
  double stddev_mult;         /* finite, >= 0 */
} mm3d_outlier_options;
void mm3d_outlier_options_default(mm3d_outlier_options *o);       /* MM3D_OUTLIERS_RADIUS, 16, 2.0 */
/* MM3D_EINVAL: ctx or options NULL, an unknown method, mean_k outside 1 .. 64, stddev_mult negative or not finite (the values
 * are checked whatever the method). */
int mm3d_set_outlier_filter(mm3d_ctx *ctx, const mm3d_outlier_options *options);
int mm3d_get_outlier_filter(const mm3d_ctx *ctx, mm3d_outlier_options *options);   /* MM3D_EINVAL for NULL */
typedef struct mm3d_outlier_stats {
  long long points, valid, kept;      /* n, n_valid, the size of the result */
  int k;                              /* k' */
  double mean, stddev, threshold;     /* mu, sigma, t */
} mm3d_outlier_stats;
/* The statistical filter's last run on this context: mm3d_remove_outliers_statistical, or mm3d_map_features under
 * MM3D_OUTLIERS_STATISTICAL (all zero before the first).  MM3D_EINVAL for NULL. */
int mm3d_last_outlier_stats(const mm3d_ctx *ctx, mm3d_outlier_stats *stats);
/* What removes the small connected components of a filtered map (off the reference's path; MM3D_CLUSTERS_OFF by default: nothing
 * runs).  Both outlier filters are density tests: a person, another robot or a floating fragment of a bad scan is a compact,
 * dense blob in free space and passes them.  With a method selected, every place that filters a map behind a whole-map call --
 * mm3d_map_features, mm3d_estimate_maps_transforms on one stream or many, on a device list (mm3d_create_devices) and
 * mm3d_shard_begin -- runs mm3d_remove_small_clusters(the cloud that left the outlier filter, radius or statistical, tolerance,
 * method, min_size) before the normals: Euclidean clustering as users of pcl::EuclideanClusterExtraction and Open3D's
 * cluster_dbscan expect it.  A map that the cluster filter empties is handled like one the outlier filter emptied.  mm3d_params
 * does not change; the stand-alone mm3d_remove_outliers* are untouched.
 *   The rule, for a cloud of n 16-byte records and a tolerance finite and > 0 (no parity with PCL's class is claimed: PCL takes
 *   a kd-tree radius search in float, and its cluster order is an artefact of it):
 *   1. A point is valid when its three coordinates are finite.  Invalid points are never kept, never counted in a cluster and
 *      never anybody's neighbour; their label is -1.
 *   2. Two valid points i != j are adjacent iff (double)d2 <= tolerance * tolerance, the product formed in double, where
 *      d2 = (dx * dx + dy * dy) + dz * dz in float, every operation rounded to nearest, nothing contracted (the d2 of the
 *      statistical filter).  Duplicate points are adjacent.
 *   3. A cluster is a connected component of that graph.  Its label is the smallest record index, in the cloud's own order,
 *      among its members; its size is the number of its members.  So the labels depend neither on launch geometry, nor on the
 *      cell-sorted order the device works in, nor on which lane won an atomic.
 *   4. MM3D_CLUSTERS_MIN_SIZE keeps a valid point iff its cluster's size is at least min_size (>= 1; 1 keeps exactly the valid
 *      points).  MM3D_CLUSTERS_LARGEST keeps the members of the largest cluster, among clusters of equal size the one with the
 *      smallest label; an empty cloud, or one with no valid point, gives an empty result.  The result is the kept records in
 *      the cloud's order, colour included.
 *   - options.tolerance == 0 means 2 * params.resolution behind the whole-map calls: two centroids of face-adjacent voxels of
 *     the down-sampled cloud are always closer than that, so a densely sampled surface stays one cluster whatever its
 *     orientation.
 *   - The setting reaches the context's mm3d_set_streams helpers in either order of the two calls, and every device of a
 *     device-list context; only a map's features change, and those travel in the bundles, so device lists and shards carry it.
 *     Every rank of a sharded call must use the same setting.  Nothing is drawn from rand().  The result is an integer function
 *     of the cloud alone: bit-identical for every stream count, driver, batch and cache setting.
 *   - The map cache's map key holds (method, min_size, tolerance), zeros under MM3D_CLUSTERS_OFF. */
typedef enum { MM3D_CLUSTERS_OFF = 0, MM3D_CLUSTERS_MIN_SIZE = 1, MM3D_CLUSTERS_LARGEST = 2 } mm3d_cluster_method;
typedef struct mm3d_cluster_options {
  int method;                 /* MM3D_CLUSTERS_* */
  int min_size;               /* >= 1; read by MM3D_CLUSTERS_MIN_SIZE */
  double tolerance;           /* metres, finite and >= 0; 0 = 2 * params.resolution */
} mm3d_cluster_options;
void mm3d_cluster_options_default(mm3d_cluster_options *o);       /* MM3D_CLUSTERS_OFF, 100, 0.0 */
/* MM3D_EINVAL: ctx or options NULL, an unknown method, min_size < 1, a tolerance negative or not finite (the values are checked
 * whatever the method).  After a refused call the selection is what it was. */
int mm3d_set_cluster_filter(mm3d_ctx *ctx, const mm3d_cluster_options *options);
int mm3d_get_cluster_filter(const mm3d_ctx *ctx, mm3d_cluster_options *options);   /* MM3D_EINVAL for NULL */
typedef struct mm3d_cluster_stats {
  long long points, valid, kept;      /* n, the valid points, the size of the result (mm3d_cluster_labels: the valid points) */
  long long clusters, kept_clusters;  /* components, and those of them that were kept (mm3d_cluster_labels: all) */
  long long largest;                  /* the size of the largest cluster, 0 without a valid point */
} mm3d_cluster_stats;
/* The cluster filter's last run on this context: mm3d_remove_small_clusters, or mm3d_map_features with a method selected (all
 * zero before the first).  MM3D_EINVAL for NULL. */
int mm3d_last_cluster_stats(const mm3d_ctx *ctx, mm3d_cluster_stats *stats);
/* What takes the dominant planes out of a filtered map (off the reference's path; MM3D_PLANES_OFF by default: nothing runs).  The
 * cluster filter removes what floats; a person, a robot or a chair stands on the floor, and through the floor it is connected to
 * every wall.  With a method selected, every place that filters a map behind a whole-map call -- mm3d_map_features,
 * mm3d_estimate_maps_transforms on one stream or many, on a device list (mm3d_create_devices) and mm3d_shard_begin -- runs the
 * rule below on the cloud that left the outlier filter, radius or statistical:
 *   MM3D_PLANES_REMOVE     the plane records leave; the cluster filter, if selected, then runs on what is left.  What users of
 *                          pcl::SACSegmentation and Open3D's segment_plane do to the ground of an outdoor map before matching.
 *   MM3D_PLANES_SET_ASIDE  with a cluster filter selected, the cluster filter runs on the records labelled MM3D_PLANE_NONE; the
 *                          map is the set-aside plane records in the cloud's order, followed by the cluster filter's result, which
 *                          is in the cloud's order too; invalid records are dropped.  Without a cluster filter nothing runs and
 *                          the map is what it would be with MM3D_PLANES_OFF.
 * A map that the stage empties is handled like one the outlier filter emptied.  MLS smoothing, normals, keypoints and descriptors
 * are the existing stages on the new cloud.  mm3d_params does not change.
 *   The rule, for a cloud of n 16-byte records (no parity with pcl::SACSegmentation is claimed: its random stream and its model
 *   refinement are not reproduced):
 *   1. A record is valid when its three coordinates are finite.  Invalid records get the label MM3D_PLANE_INVALID; they are never
 *      drawn, never counted and never kept.  n_valid counts the valid ones.
 *   2. The stop threshold is T = max(3, ceil(min_fraction * (double)n_valid)).
 *   3. Round p = 0 .. max_planes - 1 works on R_p, the valid records that have no plane yet, in the cloud's order, m = |R_p|.
 *      m < 3 ends the rule.
 *   4. Word j of draw h of round p is mix((((uint64)seed << 32) | ((uint64)p << 24) | h) + (j + 1) * 0x9E3779B97F4A7C15 mod 2^64),
 *      mix being splitmix64's finaliser as mm3d_set_alignment states it, and bounded(w, n) = ((w >> 32) * n) >> 32.  Three distinct
 *      ranks in R_p, by the prerejective alignment's recipe: i0 = bounded(w0, m); i1 = bounded(w1, m - 1), plus one if >= i0;
 *      i2 = bounded(w2, m - 2), plus one if >= min(i0, i1), then plus one if >= max(i0, i1).  The stream is a function of
 *      (seed, p, h, m) alone: nothing is drawn from the context's rand() replay, mm3d_srand has no say.
 *   5. With a, b, c the three records, everything from here on in double, every operation rounded to nearest, nothing contracted:
 *      u = (double)b - (double)a and v = (double)c - (double)a per coordinate; nrm = u x v, each component u_i * v_j - u_j * v_i;
 *      len2 = (nx*nx + ny*ny) + nz*nz.  The draw is degenerate unless len2 > 1e-12 * ((u.u) * (v.v)), the dots written
 *      (x*x + y*y) + z*z: collinear records and duplicates.  With a non-zero axis the draw is off axis unless
 *      dn * dn >= (c2 * len2) * aa, where dn = (nx*ax + ny*ay) + nz*az, aa = (ax*ax + ay*ay) + az*az and
 *      c2 = cos(max_angle_deg * pi / 180)^2 from the host's libm cos (the degenerate test comes first).  Degenerate and off-axis
 *      draws have no count and cannot win; stats.degenerate and stats.off_axis count them over all rounds, stats.draws all draws.
 *   6. The count of a surviving draw is the number of q in R_p with s * s <= (distance * distance) * len2, where
 *      s = (nx*dx + ny*dy) + nz*dz and d = (double)q - (double)a per coordinate.  No square root and no division: an integer.
 *   7. The winner is the highest count, ties to the lower h.  Without a surviving draw, or with the winner's count below T, the
 *      rule ends and round p finds no plane.  stats.rounds counts the rounds that drew, this last one included.
 *   8. With refit == 1, over the winner's inliers: N, S = sum q and P = sum q q^T with q = (double)p_i - (double)a, summed in
 *      double in a fixed order that depends on R_p alone (blocks of 4096 ranks: a lane's sixteen in ascending order, the wave's
 *      fixed tree, the four waves in order, the blocks in order); mu = S / N, C = P / N - mu mu^T; lambda0 <= lambda1 <= lambda2
 *      and the unit eigenvector n' of lambda0 by cyclic Jacobi in double.  The refit plane goes through c = (double)a + mu; its
 *      inliers over R_p are the q with |s'| <= distance, s' = (n'x*dx + n'y*dy) + n'z*dz and d = (double)q - c.  It is adopted iff
 *      the trace is > 0, lambda1 - lambda0 > 1e-6 * trace, everything is finite, with an axis (n'.axis)^2 >= c2 * aa, and it has
 *      at least as many inliers as the hypothesis.  Otherwise the hypothesis plane and its inliers stand.
 *   9. The adopted plane's inliers get the label p.  planes[p] holds the unit normal, d with n.x + d = 0 in world coordinates
 *      (d = -((nx*ax + ny*ay) + nz*az) through a, or through c after a refit), the inlier count, the winning h and whether the
 *      refit was adopted.  The hypothesis' normal is nrm / sqrt(len2).  Sign with an axis: n.axis >= 0; without one: nz > 0, or
 *      nz == 0 and ny > 0, or both zero and nx > 0.
 *   - Why 1024 draws by default: a plane that holds the share f of the remaining points is missed with probability at most
 *     (1 - f^3)^samples: below 3e-4 for f = 0.2, not negligible for f = 0.1, where a user raises samples.
 *   - Why the test is relative to a: the differences of two floats are exact in double, so the rule does not care how far the map
 *     is from the origin.
 *   - options.distance == 0 means params.resolution / 2 behind the whole-map calls.
 *   - The setting reaches the context's mm3d_set_streams helpers in either order of the two calls, and every device of a
 *     device-list context; only a map's points change, and those travel in the bundles, so device lists and shards carry it.
 *     Every rank of a sharded call must use the same setting.  replay_method and batch_only stay as they are.  The result is
 *     bit-identical for every stream count, driver, batch and cache setting, the planes' doubles included.
 *   - The map cache's map key holds all nine option fields, zeros under MM3D_PLANES_OFF. */
typedef enum { MM3D_PLANES_OFF = 0, MM3D_PLANES_REMOVE = 1, MM3D_PLANES_SET_ASIDE = 2 } mm3d_plane_method;
enum { MM3D_PLANE_NONE = -1, MM3D_PLANE_INVALID = -2 };           /* labels that name no plane */
typedef struct mm3d_plane_options {
  int method;              /* MM3D_PLANES_* (not read by the stage calls) */
  int max_planes;          /* 1 .. 8 */
  int samples;             /* draws per plane, 1 .. 65536 */
  int refit;               /* 0 or 1 */
  unsigned seed;           /* any value */
  double distance;         /* metres, finite, >= 0; 0 = params.resolution / 2 behind the whole-map calls */
  double min_fraction;     /* of the cloud's valid points, 0 .. 1 */
  double axis[3];          /* finite; the zero vector = any orientation */
  double max_angle_deg;    /* 0 .. 90 */
} mm3d_plane_options;      /* 72 bytes */
typedef struct mm3d_plane { double normal[3]; double d; long long inliers; int draw; int refit; } mm3d_plane;   /* 48 bytes */
typedef struct mm3d_plane_stats { long long points, valid, on_planes, kept, draws, degenerate, off_axis; int planes; int rounds; } mm3d_plane_stats;
void mm3d_plane_options_default(mm3d_plane_options *o);   /* OFF, 1, 1024, 1, 1, 0.0, 0.05, (0, 0, 1), 10.0 */
/* MM3D_EINVAL: ctx or options NULL, an unknown method, and any value outside its range above (the values are checked whatever
 * the method).  After a refused call the selection is what it was. */
int mm3d_set_planes(mm3d_ctx *ctx, const mm3d_plane_options *options);
int mm3d_get_planes(const mm3d_ctx *ctx, mm3d_plane_options *options);   /* MM3D_EINVAL for NULL */
/* The plane stage's last run on this context: mm3d_remove_planes, or mm3d_map_features with a method selected (all zero, no plane,
 * before the first).  mm3d_last_planes copies min(*n, capacity) records; MM3D_EINVAL for NULL or a negative capacity. */
int mm3d_last_plane_stats(const mm3d_ctx *ctx, mm3d_plane_stats *stats);
int mm3d_last_planes(const mm3d_ctx *ctx, mm3d_plane *planes, int capacity, int *n);
/* What smooths a map's points (off the reference's path; MM3D_SMOOTH_OFF by default: nothing runs).  Moving least squares: every
 * point is moved onto the Gaussian-weighted plane fitted to its neighbours within a radius, or onto the quadratic fitted over
 * that plane.  Two places ask it, each behind a bit of `where`:
 *   MM3D_SMOOTH_MAPS      every place that builds a map behind a whole-map call -- mm3d_map_features, mm3d_estimate_maps_transforms
 *                         on one stream or many, on a device list (mm3d_create_devices) and mm3d_shard_begin -- runs
 *                         mm3d_smooth_cloud(the cloud that left the outlier filter and the cluster filter, radius, order,
 *                         min_neighbours) before the normals; keypoints and descriptors are the existing stages on the new cloud.
 *                         After the filters, because a stray blob would pull the surface towards itself.
 *   MM3D_SMOOTH_COMPOSED  mm3d_compose_maps on this context returns downsample(smooth(downsample(cat, res), radius), res): where
 *                         two maps overlap, the ICP's residual leaves two copies of every wall a few centimetres apart, and one
 *                         voxel pass keeps both.  The first pass bounds the density the fit sees, the last turns the fused
 *                         layers back into one point per voxel.  Without the bit, or OFF, the call is the reference's, byte for byte.
 * mm3d_params does not change.  No parity with pcl::MovingLeastSquares is claimed: PCL fits an unweighted plane, drops points with
 * few neighbours and carries upsampling modes; none of that is here.
 *   The rule, for a cloud of n 16-byte records, a radius r finite and > 0, an order 1 or 2 and min_neighbours >= 3:
 *   1. A record is valid when its three coordinates are finite.  An invalid record is copied unchanged, is nobody's neighbour and
 *      has state INVALID.
 *   2. The neighbours of a valid point i are the valid j with (double)d2 <= r * r, the product formed in double, where
 *      d2 = (dx * dx + dy * dy) + dz * dz in float, every operation rounded to nearest, nothing contracted (the d2 of the
 *      statistical filter and the cluster filter).  Point i itself and exact duplicates count.  count_i is their number; with
 *      count_i < min_neighbours the state is FEW and the point stays.
 *   3. Everything from here on is in double, in coordinates relative to the query point, q_j = (double)p_j - (double)p_i per
 *      coordinate -- exact differences, so the rule does not care how far the map is from the origin.
 *      w_j = exp(-(double)d2_j / (r * r)); mu = sum(w q) / sum(w); C = sum(w (q - mu)(q - mu)^T) / sum(w);
 *      lambda0 <= lambda1 <= lambda2 the eigenvalues of C, n a unit eigenvector of lambda0 (its sign does not matter).  The state
 *      is DEGENERATE and the point stays when the trace is not > 0, when lambda1 - lambda0 <= 1e-6 * trace, or when anything is
 *      not finite: a line, a single repeated point.  The foot of the plane is o = (mu . n) n, the query point projected on it.
 *   4. Order 1: the displacement is o, the state PLANE.
 *   5. Order 2 needs count_i >= 6; with fewer, step 4.  With any orthonormal u, v perpendicular to n (the fitted value at the
 *      origin does not depend on the choice: the full quadratic basis is closed under rotation) and, per neighbour, e = q - o,
 *      a = e.u / r, b = e.v / r, h = e.n: minimise sum w (c0 + c1 a + c2 b + c3 a^2 + c4 a b + c5 b^2 - h)^2 through the normal
 *      equations M c = g, solved by an unpivoted LDLt.  A pivot at or below 1e-9 * trace(M) / 6 means singular (points on one
 *      conic): step 4.  The displacement is o + c0 n, the state POLYNOMIAL; if it is not finite or longer than r, step 4.
 *   6. The output record is (float)((double)p + displacement) per coordinate, the colour untouched; same n, same order.
 *   - options.radius == 0 means 3 * the resolution in force (params.resolution for the maps, mm3d_compose_maps' for the composed
 *     map): a voxel-filtered surface then has about 28 neighbours per point, enough for six coefficients, and the ball is still
 *     thinner than a wall is from its neighbour.
 *   - The result is a function of the cloud and the four numbers alone: the sums run in the cell-sorted order of the stage's grid
 *     with lane-strided partials and a fixed tree, never in the order of an atomic or of the launch geometry -- bit-identical for
 *     every stream count, batch, driver and cache setting.  The sums stream: a ball that holds every point of the cloud is legal.
 *   - The smoothed cloud is no voxel grid's output any more, and is not treated as one by the stages behind it.
 *   - The setting reaches the context's mm3d_set_streams helpers in either order of the two calls, and every device of a
 *     device-list context; only a map's points change, and those travel in the bundles, so device lists and shards carry it.
 *     Every rank of a sharded call must use the same setting.  Nothing is drawn from rand().
 *   - The map cache's map key holds (method, order, min_neighbours, radius), zeros unless the method is MLS and MM3D_SMOOTH_MAPS
 *     is set. */
typedef enum { MM3D_SMOOTH_OFF = 0, MM3D_SMOOTH_MLS = 1 } mm3d_smooth_method;
enum { MM3D_SMOOTH_MAPS = 1, MM3D_SMOOTH_COMPOSED = 2 };          /* bits of `where` */
enum { MM3D_SMOOTH_INVALID = 0, MM3D_SMOOTH_FEW = 1, MM3D_SMOOTH_DEGENERATE = 2, MM3D_SMOOTH_PLANE = 3, MM3D_SMOOTH_POLYNOMIAL = 4 };   /* a record's state */
typedef struct mm3d_smooth_options {
  int method;          /* MM3D_SMOOTH_* */
  int order;           /* 1 or 2 */
  int min_neighbours;  /* >= 3 */
  int where;           /* MM3D_SMOOTH_MAPS | MM3D_SMOOTH_COMPOSED, not 0 */
  double radius;       /* finite, >= 0; 0 = 3 * the resolution in force */
} mm3d_smooth_options;                                            /* 24 bytes */
void mm3d_smooth_options_default(mm3d_smooth_options *o);         /* OFF, 2, 6, MAPS | COMPOSED, 0.0 */
/* MM3D_EINVAL: ctx or options NULL, an unknown method, an order other than 1 and 2, min_neighbours < 3, `where` 0 or with an
 * unknown bit, a radius negative or not finite (the values are checked whatever the method).  After a refused call the selection
 * is what it was.  No context is refused. */
int mm3d_set_smoothing(mm3d_ctx *ctx, const mm3d_smooth_options *options);
int mm3d_get_smoothing(const mm3d_ctx *ctx, mm3d_smooth_options *options);   /* MM3D_EINVAL for NULL */
typedef struct mm3d_smooth_stats {
  long long points, valid, few, degenerate, plane, polynomial;   /* n, the valid records, and those of them in each state */
  double max_displacement;                                       /* the longest displacement, 0 when nothing moved */
} mm3d_smooth_stats;
/* The smoothing's last run on this context: mm3d_smooth_cloud, mm3d_map_features or mm3d_compose_maps with the method selected (all
 * zero before the first).  MM3D_EINVAL for NULL. */
int mm3d_last_smooth_stats(const mm3d_ctx *ctx, mm3d_smooth_stats *stats);
/* What refines a pair's initial estimate where params.refine_transform is set (off the reference's path; MM3D_REFINE_ICP by
 * default: the ICP that mm3d_set_icp_method selects, which mm3d_get_icp_method keeps answering whatever the refinement is).
 * MM3D_REFINE_NDT runs the Normal Distributions Transform in the ICP's place: a Gauss-Newton form of point-to-distribution
 * NDT (Biber & Strasser 2003; Magnusson 2009).  The target is summarised once per map as one Gaussian per voxel, and a source
 * point finds its terms by computing an index: no search, and a cost per iteration that does not grow with the target's
 * density.  The voxel side sets the basin of convergence; max_correspondence_distance is not read by it.  No parity with
 * pcl::NormalDistributionsTransform is claimed: PCL clamps the covariance's eigenvalues, mixes in the d1 / d2 outlier
 * constants and steps by a More-Thuente line search; none of that is here (audit row 16b).
 *   Voxel table of the target.  r_f = (float)resolution, inv = 1.0f / r_f.  The voxel of a finite point is
 *   (floorf(x * inv), floorf(y * inv), floorf(z * inv)) on the GLOBAL lattice anchored at the origin, as in
 *   mm3d_uniform_keypoints; non-finite points belong to no voxel.  Per voxel with count >= min_points, everything in double
 *   over the voxel's points in ascending input index (position l of that order goes to partial sum l mod 64, each partial
 *   ascending, and the 64 partials are added by a fixed tree): the mean mu; the covariance
 *   S = sum (p - mu)(p - mu)^T / (count - 1), two-pass; S' = S + regularisation * (trace S / 3) * I; P = S'^-1 by the
 *   closed-form adjugate.  mu and P are rounded to float once.  The voxel has no Gaussian when count < min_points, when
 *   trace S is not > 0, or when anything is not finite.
 *   One iteration.  For every finite source point, s = the point transformed by the current float T (the ICP's float rule).
 *   For its own voxel -- and, with neighbours = 7, the six face neighbours -- where that voxel has a Gaussian, in double:
 *   q = s - mu, m = q^T P q, w = exp(-m / 2); a term whose m is not finite adds nothing.  With J = [-[s]x | I] (the
 *   parametrisation of the point-to-plane row), H = sum w J^T P J, g = -sum w J^T P q, sum w, the number of terms and the
 *   number of points with at least one term are summed in double in a fixed order (per point first: J^T (sum w P) J and
 *   -J^T (sum w P q)).  H x = g is solved by point-to-plane's unpivoted LDLt with its degeneracy rule: a pivot at or below
 *   1e-12 * trace H / 6, or fewer than 6 terms, stops the loop, not converged, with T unchanged.  Tinc = [Rz(x2) Ry(x1) Rx(x0) |
 *   x3 x4 x5], T <- Tinc * T in float, then DefaultConvergenceCriteria's three tests as the ICP runs them, with
 *   F = sum w / (number of finite source points) in the place of the mean d2.
 *   - Applies to the refinement of mm3d_estimate_maps_transforms (one stream or many, with or without the map cache) and of
 *     mm3d_pair_estimate.  In the pair record icp_iterations is NDT's iteration count, icp_correspondences the number of
 *     source points that had at least one term in the last iteration, and confidence stays the point-to-point transformScore.
 *     mm3d_last_icp_iterations / mm3d_last_icp_converged report on NDT runs.
 *   - resolution > 0: the voxel side in metres; 0: 10 * params.resolution (DESIGN.md section 7e has the measurement).
 *   - mm3d_map_prepare builds a map's table on an NDT context; a pair whose target has none, or one of other options, builds
 *     it on first use.  Memory: 48 B per occupied voxel plus 4 B per cell of the voxel bounding box of the finite points,
 *     cached maps included.  Size limit: that box may hold at most 2^26 cells (MM3D_EUNSUPPORTED from the call beyond it).
 *   - The setting reaches the context's mm3d_set_streams helpers in either order of the two calls.  Results are bit-identical
 *     for every stream count, batch, split and cache setting, and through mm3d_estimate_transform_ndt from the same guess.
 *   - The map cache's pair key holds the method and, under NDT, its four options: records of different refinements are
 *     never shared. */
typedef enum { MM3D_REFINE_ICP = 0, MM3D_REFINE_NDT = 1 } mm3d_refine_method;
typedef struct mm3d_refine_options {
  int method;                 /* MM3D_REFINE_*; ICP = whatever mm3d_set_icp_method says */
  double resolution;          /* voxel side in metres, > 0; 0 = 10 * params.resolution, see above */
  int neighbours;             /* 1: the point's own voxel; 7: it and its six face neighbours */
  int min_points;             /* a voxel with fewer finite points has no Gaussian; >= 4 */
  double regularisation;      /* kappa above, 0 < kappa <= 1 */
} mm3d_refine_options;
void mm3d_refine_options_default(mm3d_refine_options *o);         /* MM3D_REFINE_ICP, 0, 7, 6, 0.01 */
/* MM3D_EINVAL: ctx or options NULL, an unknown method, a value outside its range above or a resolution that is neither 0 nor a
 * positive finite float with a finite reciprocal (the values are checked whatever the method).  MM3D_EUNSUPPORTED:
 * MM3D_REFINE_NDT on a device-list context (mm3d_create_devices), whose bundles carry no voxel tables -- nor does
 * mm3d_shard_begin, which returns MM3D_EUNSUPPORTED on an NDT context. */
int mm3d_set_refinement(mm3d_ctx *ctx, const mm3d_refine_options *options);
int mm3d_get_refinement(const mm3d_ctx *ctx, mm3d_refine_options *options);        /* MM3D_EINVAL for NULL */

/* ---- cloud objects -------------------------------------------------------------------- */
int mm3d_cloud_create(mm3d_ctx *ctx, const void *points, size_t n, size_t stride, size_t rgba_offset,
                      mm3d_cloud **out);
size_t mm3d_cloud_size(const mm3d_cloud *c);
int mm3d_cloud_download(mm3d_ctx *ctx, const mm3d_cloud *c, void *dst, size_t stride, size_t rgba_offset);
void mm3d_cloud_free(mm3d_ctx *ctx, mm3d_cloud *c);
size_t mm3d_normals_size(const mm3d_normals *n);
/* 16-byte records nx,ny,nz,curvature (pcl::Normal payload) */
int mm3d_normals_download(mm3d_ctx *ctx, const mm3d_normals *n, void *dst, size_t stride);
int mm3d_normals_create(mm3d_ctx *ctx, const void *normals, size_t n, size_t stride, mm3d_normals **out);
void mm3d_normals_free(mm3d_ctx *ctx, mm3d_normals *n);
size_t mm3d_desc_size(const mm3d_desc *d);
int mm3d_desc_dim(const mm3d_desc *d);
int mm3d_desc_type(const mm3d_desc *d);
int mm3d_desc_download(mm3d_ctx *ctx, const mm3d_desc *d, float *dst /* size*dim */);
/* SHOT only: the local reference frames, 9 floats per row (x, y, z axes) = the "rf" field of
 * pcl::SHOT1344; MM3D_EINVAL for other descriptor types. */
int mm3d_desc_download_frames(mm3d_ctx *ctx, const mm3d_desc *d, float *dst /* size*9 */);
int mm3d_desc_create(mm3d_ctx *ctx, const float *data, size_t n, int descriptor_type, mm3d_desc **out);
void mm3d_desc_free(mm3d_ctx *ctx, mm3d_desc *d);

/* ---- features.h ----------------------------------------------------------------------- */
/* downSample (R/include/map_merge_3d/features.h:34, R/src/features.cpp:17-27) */
int mm3d_downsample(mm3d_ctx *ctx, const mm3d_cloud *in, double resolution, mm3d_cloud **out);
/* removeOutliers (features.h:45, features.cpp:31-43) */
int mm3d_remove_outliers(mm3d_ctx *ctx, const mm3d_cloud *in, double radius, int min_neighbours,
                         mm3d_cloud **out);
/* computeSurfaceNormals (features.h:97, features.cpp:168-179) */
int mm3d_compute_normals(mm3d_ctx *ctx, const mm3d_cloud *in, double radius, mm3d_normals **out);
/* detectKeypoints (features.h:65, features.cpp:85-96): SIFT (features.cpp:45-62; normals and radius are
 * not used) or HARRIS (features.cpp:64-83: HarrisKeypoint3D on the given normals, non-maximum suppression
 * and refinement on, threshold, radius).  An invalid enum is UB in the reference (falls off the
 * switch); here MM3D_EINVAL. */
int mm3d_detect_keypoints(mm3d_ctx *ctx, const mm3d_cloud *points, const mm3d_normals *normals,
                          int type, double threshold, double radius, double resolution,
                          mm3d_cloud **keypoints);
/* Uniform keypoints (not a reference function; mm3d_set_keypoints puts it behind the whole-map calls): a subset of the
 * records of `points`, unchanged (x, y, z and the rgba bits), in ascending input index -- of every occupied voxel of the
 * GLOBAL lattice of side leaf (anchored at the origin, not at the cloud's minimum) the point nearest the voxel's centre.
 * To the operation, every one a single IEEE float operation rounded to nearest, nothing contracted:
 *   - leaf_f = (float)leaf, inv = 1.0f / leaf_f.
 *   - A point is finite when x, y and z are.  Non-finite points are never keypoints and belong to no voxel.
 *   - The voxel of a finite point is (i, j, k) = (floorf(x * inv), floorf(y * inv), floorf(z * inv)), as downSample forms
 *     its keys.  The three are kept as the floats floorf returns (integer-valued, -0.0f equal to 0.0f; +-inf when the
 *     product overflows).
 *   - cx = (i + 0.5f) * leaf_f (one add, one multiply), likewise cy, cz; dx = x - cx, dy, dz;
 *     d2 = (dx * dx + dy * dy) + dz * dz.  d2 is >= +0 or +inf, never NaN.
 *   - The keypoint of an occupied voxel is its point with the smallest d2, ties to the smallest input index: the minimum of
 *     the 64-bit keys float_bits(d2) << 32 | index.
 *   - Extent rule, as VoxelGrid's: with d_a = (max index - min index) + 1 over the finite points on
 *     axis a, if d_x * d_y * d_z is not <= INT32_MAX (an infinite index included), every finite point is a keypoint.
 *   - MM3D_EINVAL: a NULL argument; leaf not finite or <= 0, or leaf_f or inv not a positive finite float (a leaf below
 *     about 3e-39 or above 3.4e38).  An empty cloud gives an empty cloud and MM3D_OK.
 * No parity with pcl::UniformSampling is claimed: PCL 1.8 takes the point nearest the integer voxel INDEX (i, j, k) read as
 * a position, not nearest a centre, and anchors its lattice at the cloud's minimum; the rule above is deliberately the
 * sensible one (audit row 16a).  The result does not depend on launch geometry or on the order in which
 * anything arrives: all minima are integer minima.  One host wait, for the keypoint count. */
int mm3d_uniform_keypoints(mm3d_ctx *ctx, const mm3d_cloud *points, double leaf, mm3d_cloud **out);
/* Statistical outlier removal (not a reference function; mm3d_set_outlier_filter states the rule and puts it behind the
 * whole-map calls).  mm3d_knn_mean_distances is step 3 alone: out[i] = d_i in the cloud's order, NaN for an invalid point (and
 * for every point when n_valid <= 1).  mm3d_remove_outliers_statistical is the whole rule on a caller's cloud, whatever the
 * context's setting; the result keeps the input's voxel lattice and carries the kept points' bounding box, as
 * mm3d_remove_outliers' does.  One host wait each beyond what the cloud's bounding box and its grid cost (none for a
 * down-sampled cloud at a small mean_k; a caller's raw cloud waits for its box, and a grid cell of more than ten voxel leaves,
 * mean_k of about 40 and above, for the grid's own check).
 *   - MM3D_EINVAL: a NULL argument; mean_k outside 1 .. 64; stddev_mult negative or not finite; a cloud of 2^31 points or more.
 *     MM3D_ECAPACITY: capacity below mm3d_cloud_size(points).  An empty cloud gives MM3D_OK and an empty result.
 *   - An exact k'-nearest search over the library's cell-sorted grid; the result does not depend on the grid's cell, on launch
 *     geometry or on the order in which anything arrives. */
int mm3d_knn_mean_distances(mm3d_ctx *ctx, const mm3d_cloud *points, int mean_k, double *out, size_t capacity);
int mm3d_remove_outliers_statistical(mm3d_ctx *ctx, const mm3d_cloud *in, int mean_k, double stddev_mult, mm3d_cloud **out);
/* Diagnostics of the k'-nearest search, process-wide, collected on contexts with mm3d_set_debug on (a host wait per call):
 * out[0] queries, out[1] those that looked past their first 3 x 3 x 3 box of cells, out[2] those a second launch served. */
void mm3d_debug_outlier_search(long long out[3], int reset);
/* Euclidean clustering (not a reference function; mm3d_set_cluster_filter states the rule and puts it behind the whole-map
 * calls).  mm3d_cluster_labels is steps 1 - 3 alone: labels[i] = the smallest record index of point i's cluster, -1 for an
 * invalid point, in the cloud's order; stats (may be NULL) receives the counts, with nothing removed.
 * mm3d_remove_small_clusters is the whole rule on a caller's cloud, whatever the context's setting, and leaves its counts for
 * mm3d_last_cluster_stats; the result keeps the input's voxel lattice and carries the kept points' bounding box, as
 * mm3d_remove_outliers' does.  One host wait each beyond what the cloud's bounding box and its grid cost.
 *   - MM3D_EINVAL: a NULL argument (stats excepted); a tolerance that is not finite or not > 0; an unknown method or
 *     MM3D_CLUSTERS_OFF; min_size < 1 (checked whatever the method); capacity below mm3d_cloud_size(points); a cloud of 2^31
 *     points or more.  An empty cloud gives MM3D_OK and an empty result.
 *   - Connected components by a lock-free union-find over the record indices, the candidates of a point taken from the
 *     library's cell-sorted grid at a cell just above the tolerance (for a cloud spread over kilometres the cell grows, and
 *     with it the candidates per point: the result depends neither on the cell, nor on launch geometry, nor on the order in
 *     which anything arrives).  No size is refused: a cell that holds thousands of points -- a raw scan that was not
 *     voxelised -- is processed correctly, and the scan is quadratic in the points of such a cell. */
int mm3d_cluster_labels(mm3d_ctx *ctx, const mm3d_cloud *points, double tolerance, int *labels, size_t capacity, mm3d_cluster_stats *stats);
int mm3d_remove_small_clusters(mm3d_ctx *ctx, const mm3d_cloud *in, double tolerance, int method, int min_size, mm3d_cloud **out);
/* Plane segmentation by RANSAC (not a reference function; mm3d_set_planes states the rule and puts it behind the whole-map
 * calls).  mm3d_segment_planes is the rule on a caller's cloud, whatever the context's setting: labels receives, in the cloud's
 * order, the round p of a record's plane, MM3D_PLANE_NONE or MM3D_PLANE_INVALID; planes the *n_planes records found; stats (may
 * be NULL) the counts.  mm3d_remove_planes returns the records labelled MM3D_PLANE_NONE, in the cloud's order, colour included,
 * and leaves its counts and planes for mm3d_last_plane_stats and mm3d_last_planes; the result keeps the input's voxel lattice and
 * carries the kept points' bounding box, as mm3d_remove_outliers' does.  options.method is not read.  One host wait each: every
 * round is enqueued, a round that finds no plane raises a flag on the device at which the later rounds' kernels return, and
 * nothing comes back before the end, whatever samples and max_planes are.
 *   - MM3D_EINVAL: a NULL argument (stats excepted); an option outside its range; distance not > 0; capacity below
 *     mm3d_cloud_size(points); a cloud of 2^31 points or more.  `planes` must have room for options.max_planes records.  An
 *     empty cloud gives MM3D_OK, no plane and an empty result.
 *   - samples x m point-to-plane tests per round, in double as the rule states them: a block keeps its points in registers and
 *     walks the hypotheses, the lanes' votes folded by ballot into integer counts, so no order can move them. */
int mm3d_segment_planes(mm3d_ctx *ctx, const mm3d_cloud *points, const mm3d_plane_options *options, int *labels, size_t capacity,
                        mm3d_plane *planes, int *n_planes, mm3d_plane_stats *stats);
int mm3d_remove_planes(mm3d_ctx *ctx, const mm3d_cloud *in, const mm3d_plane_options *options, mm3d_cloud **out);
/* Moving-least-squares smoothing (not a reference function; mm3d_set_smoothing states the rule and puts it behind the whole-map
 * calls).  mm3d_smooth_displacements is steps 1 - 5 alone, in the cloud's order: disp receives 3 n doubles, zero where the point
 * stays; state (may be NULL) the n states MM3D_SMOOTH_INVALID .. MM3D_SMOOTH_POLYNOMIAL; neighbours (may be NULL) the n count_i,
 * 0 for an invalid record; stats (may be NULL) the counts.  mm3d_smooth_cloud is the whole rule on a caller's cloud, whatever the
 * context's setting, and leaves its counts for mm3d_last_smooth_stats.  One host wait each beyond what the cloud's bounding box
 * and its grid cost.
 *   - MM3D_EINVAL: a NULL argument (state, neighbours and stats excepted); a radius that is not finite or not > 0; an order other
 *     than 1 and 2; min_neighbours < 3; a cloud of 2^31 points or more.  MM3D_ECAPACITY: capacity below mm3d_cloud_size(points).
 *     An empty cloud gives MM3D_OK, an empty result and zero stats.
 *   - A wave per point on the library's cell-sorted grid at a cell just above the radius (for a cloud spread over kilometres the
 *     cell grows, and with it the candidates per point, never the neighbours).  No size is refused: the sums stream, and a ball
 *     that holds thousands of points is quadratic in them. */
int mm3d_smooth_displacements(mm3d_ctx *ctx, const mm3d_cloud *points, double radius, int order, int min_neighbours,
                              double *disp, int *state, int *neighbours, size_t capacity, mm3d_smooth_stats *stats);
int mm3d_smooth_cloud(mm3d_ctx *ctx, const mm3d_cloud *in, double radius, int order, int min_neighbours, mm3d_cloud **out);
/* The Harris response of every point (HarrisKeypoint3D::responseHarris, what detectKeypoints(HARRIS)
 * thresholds and suppresses); dst receives mm3d_cloud_size(points) floats. */
int mm3d_harris_response(mm3d_ctx *ctx, const mm3d_cloud *points, const mm3d_normals *normals, double radius,
                         float *dst);
/* computeLocalDescriptors (features.h:83, features.cpp:99-166).  Like the reference it prunes
 * keypoints whose descriptor is not finite: *keypoints is replaced IN PLACE by the pruned cloud.
 * All six rows of the dispatch table are built: PFH (dispatch_descriptors.h:38, the reference's
 * default), PFHRGB (:39), FPFH (:40), RSD (:43), SHOT (:46, i.e. SHOTColorEstimation / SHOT1344:
 * 352 shape + 992 colour bins) and SC3D (:47); other values -> MM3D_EINVAL. */
int mm3d_compute_descriptors(mm3d_ctx *ctx, const mm3d_cloud *points, const mm3d_normals *normals,
                             mm3d_cloud *keypoints, int descriptor, double feature_radius,
                             mm3d_desc **out);

/* ---- matching.h ----------------------------------------------------------------------- */
/* findFeatureCorrespondences (matching.h:26, matching.cpp:31-108).  Two-call protocol: with
 * out == NULL only *n is written. */
int mm3d_find_correspondences(mm3d_ctx *ctx, const mm3d_desc *source, const mm3d_desc *target, size_t k,
                              mm3d_corr *out, size_t cap, size_t *n);
/* estimateTransformFromCorrespondences (matching.h:44, matching.cpp:110-140) */
int mm3d_estimate_transform_from_correspondences(mm3d_ctx *ctx, const mm3d_cloud *source_keypoints,
                                                 const mm3d_cloud *target_keypoints, const mm3d_corr *corr,
                                                 size_t n_corr, double inlier_threshold, float T[16],
                                                 mm3d_corr *inliers, size_t cap, size_t *n_inliers);
/* estimateTransformFromDescriptorsSets, SAC-IA (matching.h:68, matching.cpp:142-194) */
int mm3d_estimate_transform_from_descriptors(mm3d_ctx *ctx, const mm3d_cloud *source_keypoints,
                                             const mm3d_desc *source_descriptors,
                                             const mm3d_cloud *target_keypoints,
                                             const mm3d_desc *target_descriptors, double min_sample_distance,
                                             double max_correspondence_distance, int max_iterations,
                                             float T[16]);
/* estimateTransformICP (matching.h:94, matching.cpp:196-221) */
int mm3d_estimate_transform_icp(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target,
                                const float initial_guess[16], double max_correspondence_distance,
                                double outlier_rejection_threshold, int max_iterations,
                                double transformation_epsilon, float T[16]);
/* Point-to-plane ICP (mm3d_set_icp_method states the loop and the estimate) from initial_guess, whatever the context's
 * setting.  target_normals: one per target point, in its order (mm3d_compute_normals of the target, or the caller's).
 * MM3D_EINVAL when their count differs from the target's.  mm3d_last_icp_iterations / mm3d_last_icp_converged report on it;
 * a degenerate system returns MM3D_OK, not converged, with T = the transform before the degenerate iteration. */
int mm3d_estimate_transform_icp_plane(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target,
                                      const mm3d_normals *target_normals, const float initial_guess[16],
                                      double max_correspondence_distance, int max_iterations, double transformation_epsilon,
                                      float T[16]);
/* NDT (mm3d_set_refinement states the table and the loop) from initial_guess, whatever the context's setting and
 * options->method; options->resolution must be > 0 here.  mm3d_last_icp_iterations / mm3d_last_icp_converged report on it; a
 * degenerate system returns MM3D_OK, not converged, with T = the transform before the degenerate iteration.  MM3D_EINVAL: a
 * NULL argument, options out of range, a resolution that is not positive and finite; MM3D_EUNSUPPORTED: a target whose voxel
 * bounding box needs more than 2^26 index cells. */
int mm3d_estimate_transform_ndt(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target, const float initial_guess[16],
                                const mm3d_refine_options *options, int max_iterations, double transformation_epsilon,
                                float T[16]);
/* test hook of the above: the target's voxel table in ascending (i, j, k) -- i first --, voxels with and without a Gaussian
 * alike; at most cap rows of each array.  icov: xx xy xz yy yz zz, zeros when the voxel has no Gaussian (valid = 0).
 * *n_voxels receives their number, which may exceed cap. */
int mm3d_debug_ndt_voxels(mm3d_ctx *ctx, const mm3d_cloud *target, const mm3d_refine_options *options, int *ijk /* [cap][3] */,
                          int *count, float *mean /* [cap][3] */, float *icov /* [cap][6] */, unsigned char *valid, size_t cap,
                          size_t *n_voxels);
/* The prerejective alignment (mm3d_set_alignment states it) of two keypoint sets with their descriptors, whatever the
 * context's setting and options->method.  stats may be NULL.  Fewer than three keypoints on either side, or no surviving
 * draw: MM3D_OK, T = identity, converged = 0.  MM3D_EINVAL: a NULL argument, options out of range, inlier_distance not a
 * positive finite number, descriptor sets that do not match their keypoints. */
int mm3d_estimate_transform_prerejective(mm3d_ctx *ctx, const mm3d_cloud *source_keypoints, const mm3d_desc *source_descriptors,
                                         const mm3d_cloud *target_keypoints, const mm3d_desc *target_descriptors,
                                         double inlier_distance, const mm3d_alignment_options *options, float T[16],
                                         mm3d_alignment_stats *stats);
/* test / study hook of the above: the survivors of the prerejection in ascending h, at most cap rows of
 * (h, source i0 i1 i2, target t0 t1 t2) into rows[cap][7]; counts (may be NULL) receives each scored row's inlier count.
 * *n_survivors receives their number, which may exceed cap. */
int mm3d_debug_prerejective_survivors(mm3d_ctx *ctx, const mm3d_cloud *source_keypoints, const mm3d_desc *source_descriptors,
                                      const mm3d_cloud *target_keypoints, const mm3d_desc *target_descriptors,
                                      double inlier_distance, const mm3d_alignment_options *options, int *rows, int *counts,
                                      size_t cap, size_t *n_survivors);
/* estimateTransform (matching.h:129, matching.cpp:223-257) */
int mm3d_estimate_transform(mm3d_ctx *ctx, const mm3d_cloud *source_points, const mm3d_cloud *source_keypoints,
                            const mm3d_desc *source_descriptors, const mm3d_cloud *target_points,
                            const mm3d_cloud *target_keypoints, const mm3d_desc *target_descriptors,
                            int method, int refine, double inlier_threshold,
                            double max_correspondence_distance, int max_iterations, size_t matching_k,
                            double transform_epsilon, float T[16]);
/* transformScore (matching.h:150, matching.cpp:259-268) */
int mm3d_transform_score(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target,
                         const float T[16], double max_distance, double *score);

/* ---- map_merging.h -------------------------------------------------------------------- */
typedef struct { const void *points; size_t n; size_t stride; size_t rgba_offset; } mm3d_cloud_view;
/* TransformEstimate (R/src/graph.h:24-36) plus the integer observables of the pair: what
 * registration_visualisation prints as "cross-matches count" / "inliers count"
 * (R/src/registration_visualisation.cpp:129-130; both 0 for SAC_IA, which has neither) and the ICP trace
 * (pcl::Registration::nr_iterations_ and the number of correspondences of its last iteration). */
typedef struct {
  uint64_t source_idx, target_idx;
  float transform[16];
  double confidence;
  int32_t icp_iterations;
  int32_t n_correspondences;   /* findFeatureCorrespondences(...)->size()          (MATCHING) */
  int32_t n_inliers;           /* inliers->size() of estimateTransformFromCorrespondences (MATCHING) */
  int32_t icp_correspondences; /* correspondences within max_correspondence_distance in the last ICP iteration */
} mm3d_pair_result;

/* estimateMapsTransforms (map_merging.h:85, map_merging.cpp:188-275).
 * out_T has room for n*16 floats; *n_out = 0 for no cloud, 1 (identity) for one cloud,
 * otherwise `max pair index + 1` like the reference (map_merging.cpp:168) -- or n with all-zero
 * matrices when no pair survives (the reference is UB there).  pairs (optional, capacity
 * n*(n-1)/2) receives the pairwise estimates in pair order. */
int mm3d_estimate_maps_transforms(mm3d_ctx *ctx, const mm3d_cloud_view *clouds, size_t n,
                                  const mm3d_params *params, float *out_T, size_t *n_out,
                                  mm3d_pair_result *pairs, size_t *n_pairs);
/* composeMaps (map_merging.h:99, map_merging.cpp:277-305): *out = NULL for n == 0 (nullptr in
 * the reference); n != n_transforms -> MM3D_EINVAL (the reference throws).  On a context with mm3d_set_smoothing's
 * MM3D_SMOOTH_COMPOSED the result is smoothed between two voxel passes (see there); otherwise it is the reference's. */
int mm3d_compose_maps(mm3d_ctx *ctx, const mm3d_cloud *const *clouds, size_t n, const float *transforms,
                      size_t n_transforms, double resolution, mm3d_cloud **out);

/* ---- the same path in shardable pieces (one process per GPU; see bench.py) -------------- */
typedef struct mm3d_map mm3d_map;   /* per-map bundle: filtered cloud + keypoints + descriptors */
/* the per-cloud loop body of map_merging.cpp:212-242 */
int mm3d_map_features(mm3d_ctx *ctx, const mm3d_cloud *raw, const mm3d_params *params, mm3d_map **out);
const mm3d_cloud *mm3d_map_points(const mm3d_map *m);
const mm3d_cloud *mm3d_map_keypoints(const mm3d_map *m);
const mm3d_desc *mm3d_map_descriptors(const mm3d_map *m);
int mm3d_map_from_parts(mm3d_ctx *ctx, mm3d_cloud *points, mm3d_cloud *keypoints, mm3d_desc *desc,
                        mm3d_map **out);            /* takes ownership (feature exchange between ranks) */
/* Builds every search structure that pair estimates with `params` read from this map (point and
 * keypoint grids with their distance transforms, the Hilbert-ordered query copy, the host copy of
 * the keypoints).  Optional -- they are otherwise built lazily by the first pair that needs them --
 * but after it mm3d_pair_estimate only READS the map, so one map may serve pairs running on
 * several contexts (streams) at once.  Call it on the context that created the map. */
int mm3d_map_prepare(mm3d_ctx *ctx, mm3d_map *m, const mm3d_params *params);
void mm3d_map_free(mm3d_ctx *ctx, mm3d_map *m);
/* the per-pair loop body of map_merging.cpp:256-269.  execute == 0 only advances the context's
 * rand() replay exactly as the pair would (ranks that do not own the pair stay in lock-step with
 * the reference's single global stream). */
int mm3d_pair_estimate(mm3d_ctx *ctx, const mm3d_map *source, const mm3d_map *target,
                       const mm3d_params *params, int execute, mm3d_pair_result *out);
/* The rand() draws of n consecutive pairs of that loop that this context does NOT execute (what
 * mm3d_pair_estimate(execute = 0) does for one pair, in one call and without touching the device): keeps the
 * context's generator where the reference's sequential loop would have it. */
int mm3d_pairs_skip(mm3d_ctx *ctx, const mm3d_map *const *sources, const mm3d_map *const *targets, size_t n,
                    const mm3d_params *params);
/* computeGlobalTransforms (map_merging.cpp:153-186 + graph.cpp); host only, needs no device. */
int mm3d_global_transforms(const mm3d_pair_result *pairs, size_t n_pairs, double confidence_threshold,
                           size_t n_clouds, float *out_T, size_t *n_out);

/* ---- the same job on N processes, one per GPU, driven from inside the library ------------------------
 * estimateMapsTransforms' two loops shard naturally: maps are independent in the per-cloud loop
 * (map_merging.cpp:212-242), pairs in the per-pair loop (:256-269).  The caller only moves bytes between
 * its ranks (bench.py: torch.distributed over RCCL): one all-gather of feature bundles, one of pair records.
 *   1. mm3d_shard_begin: the per-cloud loop for the maps this rank owns (mm3d_shard_map_owner), on the
 *      context's streams (mm3d_set_streams), including the target-side search structures of those maps;
 *   2. mm3d_shard_bundle_sizes / mm3d_shard_pack: an owned map's bundle -- a 256-byte header, filtered points
 *      (16-byte records), keypoints (16-byte records), descriptors (rows of float), and both clouds once more in
 *      the library's Hilbert query order with their work items (the source role of ICP / score / SAC-IA scoring
 *      reads them in that order: the owner has it, a receiver would have to sort) -- contiguously at `dst`
 *      (device or host; mm3d_shard_bundle_bytes(points, keypoints, descriptor) bytes: every part at the size the
 *      two counts allow, opaque to the caller and only valid between ranks of one library build);
 *      after the exchange mm3d_shard_unpack hands every other map's bundle over (copies and one wait, no kernel);
 *   3. mm3d_shard_pairs: every live pair in the reference's order with the pairs whose TARGET this rank owns
 *      estimated on the context's streams (mine[q] = 1), the others zero; the rand() stream of the
 *      reference's single sequential loop is replayed on every rank, so the union over the ranks equals the
 *      one-process result bit for bit;
 *   4. the merged records go to mm3d_global_transforms on every rank. */
typedef struct mm3d_shard mm3d_shard;
int mm3d_shard_map_owner(size_t map, int world);   /* 0 1 .. w-1 w-1 .. 1 0 0 1 ..: evens out the pairs per target owner */
int mm3d_shard_begin(mm3d_ctx *ctx, const mm3d_cloud_view *clouds, size_t n, const mm3d_params *params, int rank, int world,
                     mm3d_shard **out);
int mm3d_shard_bundle_sizes(const mm3d_shard *sh, uint64_t *n_points /* [n] */, uint64_t *n_keypoints /* [n] */);   /* 0 for maps not owned */
size_t mm3d_shard_bundle_bytes(uint64_t n_points, uint64_t n_keypoints, int descriptor_type);
int mm3d_shard_pack(mm3d_shard *sh, size_t map, void *dst);
int mm3d_shard_unpack(mm3d_shard *sh, size_t map, const void *src, uint64_t n_points, uint64_t n_keypoints);
/* the same for several maps at once, dealt to the context's streams */
int mm3d_shard_unpack_many(mm3d_shard *sh, size_t count, const size_t *maps, const void *const *srcs, const uint64_t *n_points,
                           const uint64_t *n_keypoints);
int mm3d_shard_pairs(mm3d_shard *sh, mm3d_pair_result *pairs, unsigned char *mine, size_t capacity, size_t *n_pairs);
void mm3d_shard_end(mm3d_shard *sh);

/* ---- measurement ---------------------------------------------------------------------- */
/* per-kernel HIP-event timing on the context's own stream (bench.py roofline leg) */
int mm3d_profile_enable(mm3d_ctx *ctx, int on);
void mm3d_profile_reset(mm3d_ctx *ctx);
/* number of distinct kernels recorded; names via mm3d_profile_entry */
int mm3d_profile_count(mm3d_ctx *ctx);
int mm3d_profile_entry(mm3d_ctx *ctx, int i, const char **name, double *total_ms, uint64_t *launches,
                       double *algorithmic_bytes);
int mm3d_synchronize(mm3d_ctx *ctx);

/* ---- correlative coarse alignment ------------------------------------------------------- */
/* Where a pair's INITIAL estimate comes from (off the reference's path; MM3D_COARSE_NONE by default: whatever
 * params.estimation_method and mm3d_set_alignment say).  MM3D_COARSE_CORRELATIVE reads no keypoint and no descriptor: the
 * maps come from robots that know gravity, so the unknown part of a pair's pose is close to a yaw and a shift in the plane.
 * EVERY yaw and shift is scored on a coarse 2-D occupancy of the vertical structure (walls: points whose normal is near
 * horizontal), the best few are refined on the fine grid, and height and residual tilt are read off the two ground surfaces.
 * Nothing is drawn at random; all scores are integer counts, so the result does not depend on launch geometry or arrival
 * order.  No such estimator is in PCL or in the reference: no parity is claimed (audit row 16c).
 * To the operation -- every float step is a single IEEE operation rounded to nearest, nothing contracted:
 *   Signature of a map (once per map and option set).  c = (float)cell, inv = 1.0f / c.  A point counts when x, y, z and
 *   the three components of its normal are finite.  Its 2-D cell is (i, j) = (floorf(x * inv), floorf(y * inv)) on the
 *   GLOBAL lattice anchored at the origin.  A fine STRUCTURE cell has >= min_points counted points with
 *   fabsf(n_z) <= (float)wall_nz; a GROUND cell has >= min_points counted points with fabsf(n_z) >= (float)ground_nz, and its
 *   height is the mean z in double over those points in ascending input index (position l of that order goes to partial
 *   sum l mod 64, each partial ascending, and the 64 partials are added by the fixed tree of the NDT voxel table), rounded to
 *   float once.  The COARSE structure cells are the distinct (floor(i / F), floor(j / F)) of the structure cells (floor
 *   division, F = cell_factor).  All lists ascend in (i, j), i first.  For the target role the structure cells are also kept
 *   as a dense map DILATED by one cell (a cell is set when it or one of its 8 neighbours is a structure cell), beside a
 *   dense map of the ground heights.  Size limit: the 2-D box of the counted points' cells may hold at most 2^24 cells.
 *   Coarse vote.  cs[k] = (float)cos(2 pi k / yaw_steps), sn[k] = (float)sin(2 pi k / yaw_steps), the angle and the
 *   functions evaluated in double on the host.  C = c * (float)F, invC = 1.0f / C, G = yaw_factor, Q = yaw_steps / G.  For
 *   every coarse yaw index q (k = q G), every source coarse cell (I, J) with centre p = (((float)I + 0.5f) * C,
 *   ((float)J + 0.5f) * C) and every target coarse cell with centre t formed alike: r = (cs px - sn py, sn px + cs py),
 *   d = t - r, (u, v) = (floorf(dx * invC + 0.5f), floorf(dy * invC + 0.5f)), acc[q][u][v] += 1.  The accumulator spans a
 *   box of (u, v) that the two maps' cell boxes bound, U x V cells; Q U V may be at most 2^26 (MM3D_EUNSUPPORTED beyond).
 *   Candidates.  A cell is a candidate when it has >= 1 vote and no OTHER cell of its 3 x 3 x 3 neighbourhood (cyclic in q,
 *   clipped in u and v) has more votes, or as many and a lower linear index (q U + u') V + v' (u', v' counted from the box's
 *   minimum).  The `candidates` best are kept: votes descending, then linear index ascending.
 *   Fine score.  For every kept candidate (rank order), every g in [-G, G] (k = (q G + g) mod yaw_steps) and every (a, b) in
 *   [-F, F]^2 the shift is s = ((float)(u F + a) * c, (float)(v F + b) * c) and the score is the number of source fine
 *   structure cells (i, j) whose centre p = (((float)i + 0.5f) * c, ((float)j + 0.5f) * c), rotated to r as above and
 *   shifted, x' = rx + sx, y' = ry + sy, falls in a set cell (floorf(x' * inv), floorf(y' * inv)) of the target's dilated
 *   map.  The winner is the highest score, ties to the lowest (rank, g, a, b).  candidates (2G + 1) (2F + 1)^2 must stay below
 *   2^31 (MM3D_EUNSUPPORTED beyond).
 *   Height and tilt.  At the winner every source ground cell's centre is carried over the same way; where
 *   (floorf(x' * inv), floorf(y' * inv)) is a ground cell of the target, d = (double)h_target - (double)h_source.  With n such
 *   cells, position l of the source's list order goes to partial sum l mod 256, each partial ascending, and the partials are
 *   added by a fixed tree, all in double: n, sums of x', y', x'x', x'y', y'y', d, x'd, y'd.  With n >= 16 the 3 x 3 normal
 *   equations of d ~ alpha x' + beta y' + gamma (unknowns in that order) are solved by an unpivoted LDLt; a pivot at or below
 *   1e-12 * trace / 3 (the rule of the point-to-plane solve) makes the system degenerate.  A degenerate system, n < 16, a
 *   result that is not finite or a slope sqrt(alpha^2 + beta^2) above tan 20 deg gives alpha = beta = 0 and gamma = the
 *   mean d (0 with n = 0).
 *   Transform.  In double: T = Trans(0, 0, gamma) * Rx(atan beta) * Ry(-atan alpha) * [Rz | s], Rz from the table's floats
 *   (cs[k], sn[k]) of the winner, cos(atan a) = 1 / sqrt(1 + a^2) and sin(atan a) = a / sqrt(1 + a^2); the third row of
 *   Rx Ry is then (alpha, beta sqrt(1 + alpha^2), 1) / (sqrt(1 + alpha^2) sqrt(1 + beta^2)): the fitted plane to first order, and the
 *   refinement takes the rest.  Rounded to a float 4 x 4 once (column-major, as every transform of this header).
 *   Outcome.  converged = (double)score >= accept_fraction * (double)source_cells.  A winner that is not converged is still
 *   handed on, as the prerejective alignment does.  No structure cell on either side: the identity, converged = 0, yaw_index -1.
 *   - Behind the whole-map calls: with MM3D_COARSE_CORRELATIVE a pair's initial estimate is this one, whatever
 *     params.estimation_method and mm3d_set_alignment say -- mm3d_estimate_maps_transforms on one stream or many, with or
 *     without the map cache, and mm3d_pair_estimate.  The pair goes on to the configured refinement and to its record as
 *     after SAC-IA; n_correspondences and n_inliers are 0.  Nothing is taken from the rand() replay:
 *     mm3d_pair_estimate(execute = 0) and mm3d_pairs_skip advance nothing.  A map's features are still computed, and which
 *     pairs are live does not change.
 *   - cell > 0: the fine cell side in metres; 0: 5 * params.resolution.
 *   - mm3d_map_prepare makes a map's signature from the normals the map build has anyway; a pair whose map has none, or one
 *     of other options, makes it on first use (a map without normals gets them as point-to-plane's targets do).
 *   - The setting reaches the context's mm3d_set_streams helpers in either order of the two calls.  Results are bit-identical
 *     for every stream count, batch and cache setting, and through mm3d_estimate_transform_correlative on the same inputs.
 *   - The map cache's pair key holds the method and, under it, every option. */
typedef enum { MM3D_COARSE_NONE = 0, MM3D_COARSE_CORRELATIVE = 1 } mm3d_coarse_method;
typedef struct mm3d_coarse_options {
  int method;            /* MM3D_COARSE_* */
  double cell;           /* fine cell side in metres, > 0; 0 = 5 * params.resolution */
  int cell_factor;       /* F: a coarse cell is F x F fine cells, 1 .. 16 */
  int yaw_steps;         /* fine yaw steps per turn, 8 .. 7200 */
  int yaw_factor;        /* G: a coarse yaw step is G fine ones; yaw_steps % G == 0 */
  int candidates;        /* coarse maxima that are refined, 1 .. 1024 */
  double wall_nz;        /* a point is structure when |n_z| <= wall_nz, 0 .. 1 */
  double ground_nz;      /* a point is ground when |n_z| >= ground_nz, wall_nz < ground_nz <= 1 */
  int min_points;        /* points of a class a cell needs, >= 1 */
  double accept_fraction;/* converged when score >= accept_fraction * source structure cells, 0 .. 1 */
} mm3d_coarse_options;
typedef struct mm3d_coarse_stats {
  int source_cells, target_cells;   /* fine structure cells */
  int coarse_votes;                 /* of the winner's candidate */
  int candidates;                   /* refined */
  int score;                        /* the winner's */
  int yaw_index;                    /* fine step, 0 .. yaw_steps-1; -1: none */
  int ground_pairs;                 /* cells in the plane fit */
  int converged;
} mm3d_coarse_stats;
void mm3d_coarse_options_default(mm3d_coarse_options *o);   /* NONE, 0, 4, 720, 6, 32, 0.5, 0.9, 3, 0.25 */
/* MM3D_EINVAL: ctx or options NULL, an unknown method, a value outside its range above, a cell that is neither 0 nor a
 * positive finite float with a finite reciprocal (the values are checked whatever the method).  MM3D_EUNSUPPORTED:
 * MM3D_COARSE_CORRELATIVE on a device-list context (mm3d_create_devices), whose bundles carry no signatures -- nor does
 * mm3d_shard_begin, which returns MM3D_EUNSUPPORTED on a correlative context. */
int mm3d_set_coarse_alignment(mm3d_ctx *ctx, const mm3d_coarse_options *options);
int mm3d_get_coarse_alignment(const mm3d_ctx *ctx, mm3d_coarse_options *options);   /* MM3D_EINVAL for NULL */
/* of the most recent correlative alignment this context ran (a pair of a whole-map call on one stream, or the call below) */
int mm3d_last_coarse_stats(const mm3d_ctx *ctx, mm3d_coarse_stats *stats);
/* The correlative alignment of two clouds with their normals (one per point, in its order), whatever the context's setting
 * and options->method; options->cell must be > 0 here.  stats may be NULL.  MM3D_EINVAL: a NULL argument, options out of
 * range, normals whose count differs from their cloud's; MM3D_EUNSUPPORTED: a size limit above. */
int mm3d_estimate_transform_correlative(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_normals *source_normals,
                                        const mm3d_cloud *target, const mm3d_normals *target_normals,
                                        const mm3d_coarse_options *options, float T[16], mm3d_coarse_stats *stats);
/* test hook: a map's signature.  structure [cap][3] = (i, j, count), ground [cap][3] = (i, j, count) with ground_height
 * [cap], coarse [cap][2] = (I, J), each ascending in (i, j); at most cap rows of each (arrays may be NULL with cap = 0).
 * n[3] receives the three counts, which may exceed cap. */
int mm3d_debug_correlative_signature(mm3d_ctx *ctx, const mm3d_cloud *points, const mm3d_normals *normals,
                                     const mm3d_coarse_options *options, int *structure, int *ground, float *ground_height,
                                     int *coarse, size_t cap, size_t n[3]);
/* test hook: the search of a pair.  frame[5] = {Q, u_min, v_min, U, V}; acc (may be NULL) receives the U x V accumulator
 * of coarse yaw index q when acc_cap >= U V; cands [cand_cap][4] = (q, u, v, votes) in rank order, u and v as the rule
 * counts them (not from the box's minimum); scores [cand_cap][2G+1][2F+1][2F+1] the fine score cube of each; *n_cands the
 * number refined, at most options->candidates.  A pair without structure cells: frame all 0, *n_cands = 0. */
int mm3d_debug_correlative_votes(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_normals *source_normals,
                                 const mm3d_cloud *target, const mm3d_normals *target_normals,
                                 const mm3d_coarse_options *options, int q, int frame[5], int *acc, size_t acc_cap, int *cands,
                                 int *scores, size_t cand_cap, size_t *n_cands);

/* ---- overlap confidence (off the reference's path) ---------------------------------------
 * What a pair record's `confidence` is.  MM3D_CONFIDENCE_REFERENCE (the default) is the reference's 1 / transformScore, bit
 * for bit as before.  MM3D_CONFIDENCE_OVERLAP replaces it by a two-way voxel agreement of the two maps under the pair's
 * transform: search-free (one index computation and two loads per point), normalised to the overlap, and integer-valued up
 * to one final division.  It has no PCL counterpart and claims no parity (audit row 16d; section 7g).
 * THIS CONFIDENCE LIVES IN [0, 1]: params.confidence_threshold is then a fraction, not a reciprocal mean squared distance.
 *   Lattice.  r_f = (float)voxel, inv = 1.0f / r_f.  The voxel of a coordinate x is (int)floorf(x * inv) (one float multiply)
 *   on the GLOBAL lattice anchored at the origin, as in mm3d_set_refinement and mm3d_uniform_keypoints.  Per axis, brick
 *   b = v >> 2 and view cell c = v >> 3 (arithmetic shifts: floor division).
 *   Table of a map, from its finite points only, once per map and option set:
 *     occ(v):  some finite point lies in voxel v.
 *     near(v): occ(u) for some u with max|u - v| <= 1 (the 27 voxels around v).
 *     cnt(c):  the number of finite points whose view cell is c;  seen(c) = cnt(c) >= min_points.
 *     view(c): view_margin = 0: seen(c);  view_margin = 1: seen(c') for some c' with max|c' - c| <= 1.
 *   Storage is dense over the brick box of the finite points: per axis bricks [(v_lo - 1) >> 2, (v_hi + 1) >> 2], v_lo / v_hi
 *   the voxels of the cloud's bounding box minimum / maximum.  One uint64 word per brick holds its 4 x 4 x 4 voxels of near:
 *   voxel (i, j, k) is bit (i&3) | ((j&3)<<2) | ((k&3)<<4) of word ((bi-b0i)*nj + (bj-b0j))*nk + (bk-b0k).  One byte per view
 *   cell holds view, over the view cells [b0 >> 1, b1 >> 1] that the brick box touches, widened by one cell on every side
 *   when view_margin = 1, in the same (i-major) order.  Everything outside the two boxes reads as 0.  Memory: 8 B per brick
 *   plus 1 B per view cell, cached maps included.  Limits, decided before anything is allocated, both MM3D_EUNSUPPORTED: more
 *   than 2^24 words; a voxel index of magnitude >= 2^30.
 *   One direction A -> B under a float matrix M.  For every finite point p of A: s = M p by the ICP's float rule (unfused
 *   multiplies and adds, x then y then z then the translation).  A point with a non-finite s, or with |s * inv| >= 2^30 on
 *   any axis, counts for nothing.  Otherwise v = its voxel; if view_B(v >> 3): in += 1, and if in addition near_B(v): hit += 1.
 *   Two directions.  source -> target uses M = T.  target -> source uses the rigid inverse, formed on the host in double from
 *   T's float entries: R' = R^T, t'_r = -((R_0r t_0 + R_1r t_1) + R_2r t_2), rounded to float once, last row 0 0 0 1.  A T with
 *   a non-finite entry, or the all-zero matrix, gives all counts 0 and confidence 0.
 *   Confidence.  n_s, n_t = the finite point counts.  It is 0.0 when in_st == 0, in_ts == 0,
 *   (double)in_st < min_overlap * (double)n_s or (double)in_ts < min_overlap * (double)n_t; otherwise
 *   min((double)hit_st / (double)in_st, (double)hit_ts / (double)in_ts).
 *   - voxel: 0, or a positive finite float with a finite reciprocal; 0 means 2 * params.resolution.  min_points >= 1.
 *     0 <= min_overlap <= 1.  view_margin 0 or 1.
 *   - Applies to mm3d_estimate_maps_transforms (one stream or many, with or without the map cache) and mm3d_pair_estimate:
 *     the record's confidence is the overlap confidence at the record's transform; every other field is what it would have
 *     been, and nothing is taken from the rand() replay.  The reference's transformScore is then not run at all.
 *   - mm3d_map_prepare builds a map's table on an overlap context; a pair needs BOTH maps' tables, and either is built on first
 *     use when missing or made with other options.
 *   - The setting reaches the context's mm3d_set_streams helpers in either order of the two calls.  All counts are integer
 *     sums: identical for every launch shape, batch, stream count and cache setting, and through mm3d_transform_overlap.
 *   - The map cache's pair key holds the method and, under overlap, its four options. */
typedef enum { MM3D_CONFIDENCE_REFERENCE = 0, MM3D_CONFIDENCE_OVERLAP = 1 } mm3d_confidence_method;
typedef struct mm3d_confidence_options {
  int method;            /* MM3D_CONFIDENCE_* */
  double voxel;          /* voxel side in metres, > 0; 0 = 2 * params.resolution */
  int min_points;        /* a view cell with fewer finite points has not been seen; >= 1 */
  double min_overlap;    /* the share of a map's finite points that must fall in the other's view, 0 .. 1 */
  int view_margin;       /* 0: a view cell counts when seen; 1: when it or one of its 26 neighbours is */
} mm3d_confidence_options;
typedef struct mm3d_overlap_stats {
  long long points_st, in_st, hit_st;   /* source -> target: finite source points, in the target's view, near a target voxel */
  long long points_ts, in_ts, hit_ts;   /* target -> source */
  double confidence;
} mm3d_overlap_stats;
void mm3d_confidence_options_default(mm3d_confidence_options *o);   /* REFERENCE, 0, 8, 0.05, 0 */
/* MM3D_EINVAL: ctx or options NULL, an unknown method, a value outside its range above (the values are checked whatever the
 * method).  MM3D_EUNSUPPORTED: MM3D_CONFIDENCE_OVERLAP on a device-list context (mm3d_create_devices), whose bundles carry
 * no tables -- nor does mm3d_shard_begin, which returns MM3D_EUNSUPPORTED on an overlap context. */
int mm3d_set_confidence(mm3d_ctx *ctx, const mm3d_confidence_options *options);
int mm3d_get_confidence(const mm3d_ctx *ctx, mm3d_confidence_options *options);      /* MM3D_EINVAL for NULL */
/* of the most recent pair this context scored itself (the last pair of a whole-map call on one stream, or the call below) */
int mm3d_last_confidence_stats(const mm3d_ctx *ctx, mm3d_overlap_stats *stats);
/* The overlap confidence of two clouds under T (column-major, as in the pair record), whatever the context's setting and
 * options->method; options->voxel must be > 0 here.  Builds throw-away tables.  stats receives the counts and the
 * confidence.  MM3D_EINVAL: a NULL argument, options out of range; MM3D_EUNSUPPORTED: a limit above. */
int mm3d_transform_overlap(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target, const float T[16],
                           const mm3d_confidence_options *options, mm3d_overlap_stats *stats);
/* test hook: a cloud's table.  box[12] = brick box minimum (3) and extent (3), view box minimum (3) and extent (3); words
 * receives the near words when word_cap >= their number, view the bytes when view_cap >= theirs (either may be NULL with a
 * cap of 0).  A cloud without a finite point: box all 0. */
int mm3d_debug_overlap_table(mm3d_ctx *ctx, const mm3d_cloud *cloud, const mm3d_confidence_options *options, int box[12],
                             unsigned long long *words, size_t word_cap, unsigned char *view, size_t view_cap);

/* ---------------------------------------------------------------- opt-in ICP correspondence rejection
 * mm3d_set_icp_rejection lets the pair stage's ICP ignore correspondences: PCL's CorrespondenceRejectorOneToOne,
 * CorrespondenceRejectorTrimmed and CorrespondenceRejectorMedianDistance, the three that need nothing but the correspondences.
 * With the default options (nothing rejected) the selection is inactive and the pair stage runs the kernels it always ran.
 * The rule, for ONE iteration of the loop that mm3d_set_icp_method states (everything else is that loop):
 *   1. match     a finite source point is carried by the current float T; its exact float nearest target point is found (ties
 *                to the lowest index); it is matched when d2 <= max_d2 (the float the ICP accepts at).
 *   2. one_to_one  of all matched source points that share a target point, the one with the smallest 64-bit key
 *                float_bits(d2) << 32 | original source index survives (an integer minimum: no arrival order shows).
 *   3. distance  over the n survivors' d2 (non-negative, so its float bits order as the values do):
 *       TRIMMED  k = max(min_correspondences, (long long)(overlap_ratio * (double)n)).  k >= n: nothing is cut.  k == 0:
 *                everything is cut.  Otherwise tau is the k-th smallest d2 and every survivor with d2 <= tau is kept: ties at tau
 *                are all kept, so kept >= k.  (PCL cuts its sorted list at k with an unspecified tie order: no parity is claimed.)
 *       MEDIAN   m is the survivor d2 of 0-based rank n / 2 in ascending order; a survivor is kept when
 *                (double)d2 <= (double)m * median_factor.
 *                tau and m are exact order statistics (a radix select on the device, no host round trip in an iteration).
 *   4. estimate  the sums of the selected estimate (point-to-point's 17 terms, point-to-plane's 30) run over the kept
 *                correspondences only, in the order the default kernels add them, and the default finalize kernels run on
 *                them: with nothing rejected the result is the default ICP's, bit for bit.  The "fewer than 3" stop, the MSE
 *                of the convergence test and icp_correspondences all count kept correspondences.
 * Results are bit-identical for every stream count, batch and cache setting.  Applies to the ICP of
 * mm3d_estimate_maps_transforms and mm3d_pair_estimate, with either mm3d_set_icp_method; NDT (mm3d_set_refinement) does not
 * read the setting, nor do mm3d_estimate_transform_icp, mm3d_estimate_transform_icp_plane, mm3d_estimate_transform,
 * transformScore or the overlap confidence.  Working memory per pair of a batch: 8 B per source point, 8 B per target point
 * under one_to_one, 4 KiB of histograms. */
typedef enum { MM3D_REJECT_NONE = 0, MM3D_REJECT_TRIMMED = 1, MM3D_REJECT_MEDIAN = 2 } mm3d_reject_distance;
typedef struct mm3d_icp_rejection_options {
  int one_to_one;            /* 0 / 1 */
  int distance;              /* MM3D_REJECT_* */
  double overlap_ratio;      /* TRIMMED: 0 < rho <= 1 */
  int min_correspondences;   /* TRIMMED: keep at least this many, >= 0 */
  double median_factor;      /* MEDIAN: > 0, finite */
} mm3d_icp_rejection_options;
typedef struct mm3d_icp_rejection_stats {  /* of the LAST iteration that ran */
  long long matched;         /* finite source points whose nearest target point has d2 <= max_d2 */
  long long after_one_to_one;/* == matched when one_to_one is 0 */
  long long kept;            /* == the pair record's icp_correspondences */
  float threshold_d2;        /* tau (TRIMMED) or m (MEDIAN); +inf when distance is NONE, when nothing was cut or when there
                              * was no survivor; -1 when TRIMMED cut everything (k == 0) */
  int iterations, converged;
} mm3d_icp_rejection_stats;
void mm3d_icp_rejection_options_default(mm3d_icp_rejection_options *o);   /* 0, NONE, 0.5, 0, 1.0 (PCL's own defaults) */
/* The selection is active when one_to_one || distance != MM3D_REJECT_NONE.  MM3D_EINVAL: ctx or options NULL, one_to_one not
 * 0 / 1, an unknown distance, a value outside its range above (the values are checked whatever the selection).
 * MM3D_EUNSUPPORTED: an active selection on a device-list context (mm3d_create_devices), or while coloured ICP
 * (mm3d_set_icp_color) or generalized ICP (mm3d_set_icp_generalized) is enabled; mm3d_shard_begin returns
 * MM3D_EUNSUPPORTED on a context with an active selection.  The setting reaches the context's mm3d_set_streams helpers, in
 * either order, and is part of the map cache's pair key while active. */
int mm3d_set_icp_rejection(mm3d_ctx *ctx, const mm3d_icp_rejection_options *options);
int mm3d_get_icp_rejection(const mm3d_ctx *ctx, mm3d_icp_rejection_options *options);   /* MM3D_EINVAL for NULL */
/* of the most recent pair whose ICP this context ran with rejection (the last pair of a whole-map call on one stream, or the
 * call below); all zero, threshold_d2 +inf, before there was one */
int mm3d_last_icp_rejection_stats(const mm3d_ctx *ctx, mm3d_icp_rejection_stats *stats);
/* ICP with the rule above from initial_guess, whatever the context's setting: the correspondence stage of the rule runs even
 * when `options` reject nothing.  target_normals NULL: the point-to-point estimate; else the point-to-plane one (normals in
 * the target's order).  stats may be NULL.  MM3D_EINVAL: a NULL argument, options out of range, normals whose count differs
 * from the target's. */
int mm3d_estimate_transform_icp_rejecting(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target,
                                          const mm3d_normals *target_normals, const float initial_guess[16],
                                          double max_correspondence_distance, const mm3d_icp_rejection_options *options,
                                          int max_iterations, double transformation_epsilon, float T[16],
                                          mm3d_icp_rejection_stats *stats);
/* test hook: ONE iteration's correspondence stage (steps 1 - 3) at T.  Per source point, in the caller's order: the matched
 * target index (-1: none), the float d2 (+inf: none) and whether the correspondence was kept.  split: 1 or 4, as in
 * mm3d_debug_nn_search.  stats (may be NULL): the counts and the threshold; iterations and converged are 0. */
int mm3d_debug_icp_rejection(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target, const float T[16],
                             double max_correspondence_distance, const mm3d_icp_rejection_options *options, int split, int *idx,
                             float *d2, unsigned char *kept, mm3d_icp_rejection_stats *stats);
/* test hook, process-wide like mm3d_debug_sacia_queries_per_thread: 0 = one or four work items per block chosen by size, as
 * everywhere; 1 or 4 = forced in every rejecting launch from now on; negative = no change.  Returns the value in force. */
int mm3d_debug_icp_rejection_split(int split);

/* ---------------------------------------------------------------- opt-in geometric ICP rejectors
 * mm3d_set_icp_geometry_rejection adds two rejectors that read the maps' geometry to the correspondence stage above: a
 * correspondence is dropped when its TARGET point lies on the edge of the target's surface (Turk and Levoy 1994; PCL's
 * BoundaryEstimation with CorrespondenceRejectionBoundaryPoints), and when the two points' normals disagree (PCL's
 * CorrespondenceRejectorSurfaceNormal).  The algorithms, not their floats: no parity with PCL is claimed.  With the default
 * options the selection is inactive and the pair stage runs the kernels it always ran.
 *
 * The boundary flag of point i of a cloud with one normal n per point, radius r, angle theta, minimum k.  All arithmetic is
 * double, every step is ONE IEEE operation, nothing is contracted; differences of two floats promoted to double are exact, so
 * the rule does not see how far the map is from the origin.
 *   - i gets flag 0 unless its coordinates and its normal are finite and the normal is not (0, 0, 0).
 *   - Its neighbours are the points j with finite coordinates, delta = p_j - p_i != 0 and (dx dx + dy dy) + dz dz <= r * r.
 *   - Tangent frame, no square root, no division: e is the coordinate axis of the smallest |n_k| (ties to the lowest k),
 *     u = e x n, v = n x u, each component (a b) - (c d).
 *   - The direction of j is (x, y) = (u . delta, v . delta), a dot being (a b + c d) + e f.  x == 0 && y == 0 (a neighbour
 *     along the normal) is no direction and is skipped.
 *   - c = cos(theta) from the host's libm, but exactly 0 at 90 and exactly -1 at 180; c2 = c * c.  With cross = ax by - ay bx,
 *     dot = ax bx + ay by, direction b FILLS THE WEDGE of direction a when
 *       b lies counter-clockwise of a by an angle in (0, 180]:  cross > 0 || (cross == 0 && dot < 0),       and that angle
 *       is at most theta:   c >= 0:  dot >= 0 && dot * dot >= c2 * ((a . a) * (b . b))
 *                           c <  0:  dot >= 0 || dot * dot <= c2 * ((a . a) * (b . b)).
 *   - i is a boundary point iff it has at least k directions and SOME direction's wedge is filled by no other direction:
 *     PCL's "largest angular gap > theta" as an existence test.  No sort, no atan2, no sum: the flag does not depend on the
 *     order in which neighbours arrive.  A gap of exactly theta is no boundary.
 *
 * Step 1b of the rejection rule above, between "match" and "one_to_one".  A matched correspondence (source point s, target
 * point t) is dropped
 *     with reason 1 when boundary is set and t's flag is set; else
 *     with reason 2 when normals is set and the normals disagree: m = R n_s in float, R the rotation of the current float T,
 *                   each component (R_k0 nx + R_k1 ny) + R_k2 nz; then in double d = (mx tx + my ty) + mz tz, and they AGREE
 *                   when d * d >= c2n * (((mx mx + my my) + mz mz) * ((tx tx + ty ty) + tz tz)), c2n = cos(normal_angle_deg)^2
 *                   (exactly 0 at 90).  |cos|, because every map orients its normals towards its own origin.  A non-finite or
 *                   zero normal on either side disagrees.
 * A dropped correspondence does not compete for one-to-one ownership and is in no order statistic; steps 2 - 4 run on the
 * rest, unchanged, and the rejection statistics' `matched` counts the rest.  With nothing dropped the result is that of the
 * rejection rule alone, bit for bit. */
typedef struct mm3d_icp_geometry_options {
  int boundary;                 /* 0 / 1: drop a correspondence whose TARGET point is a boundary point */
  double boundary_radius;       /* metres, finite, >= 0; 0 = params.normal_radius behind the whole-map calls */
  double boundary_angle_deg;    /* (0, 180]; PCL's default is 90 */
  int boundary_min_neighbours;  /* >= 3 (PCL: fewer than 3 neighbours is never a boundary) */
  int normals;                  /* 0 / 1: drop a correspondence whose two normals disagree */
  double normal_angle_deg;      /* (0, 90] */
} mm3d_icp_geometry_options;
typedef struct mm3d_icp_geometry_stats {   /* of the LAST iteration that ran */
  long long matched, on_boundary, normal_mismatch, passed;   /* passed = matched - on_boundary - normal_mismatch */
  long long target_boundary_points;                          /* flagged points of the target map (0 when boundary is 0) */
} mm3d_icp_geometry_stats;
void mm3d_icp_geometry_options_default(mm3d_icp_geometry_options *o);   /* 0, 0.0, 90, 3, 0, 45 */
/* The selection is active when boundary || normals; an active selection makes the pair stage's point-to-point and
 * point-to-plane ICP take the rejecting step even when mm3d_set_icp_rejection rejects nothing.  Behind the whole-map calls the
 * normals are the maps' (normal_radius) and a map keeps its flags (made by mm3d_map_prepare or on first use, remade when radius,
 * angle or minimum change).  MM3D_EINVAL: a NULL argument, a value outside its range above (checked whatever the bits are).
 * MM3D_EUNSUPPORTED: an active selection on a device-list context (mm3d_create_devices); while coloured, generalized or robust
 * ICP is enabled (each of which in turn refuses while this selection is active); normals == 1 while an ICP source sampling is
 * set (mm3d_set_icp_sampling, which in turn refuses then: a sample has no normals of its own; boundary alone combines with
 * it); mm3d_shard_begin returns MM3D_EUNSUPPORTED on a context with an active selection.  NDT does not read the setting, nor
 * do mm3d_estimate_transform_icp*, mm3d_estimate_transform, the score and the overlap confidence.  The six fields are part of
 * the map cache's pair key while active. */
int mm3d_set_icp_geometry_rejection(mm3d_ctx *ctx, const mm3d_icp_geometry_options *options);
int mm3d_get_icp_geometry_rejection(const mm3d_ctx *ctx, mm3d_icp_geometry_options *options);   /* MM3D_EINVAL for NULL */
/* of the most recent pair whose ICP this context ran with an active selection (or the stage call below); zeros before */
int mm3d_last_icp_geometry_stats(const mm3d_ctx *ctx, mm3d_icp_geometry_stats *stats);
/* The boundary flags of the rule above for every point of `points` with `normals` (one per point), in the caller's order:
 * flags[i] = 0 / 1 for i < the cloud's size, which `capacity` must reach; *n_boundary (may be NULL) their sum.  Correct for
 * any neighbourhood size.  MM3D_EINVAL: a NULL argument, radius not finite or <= 0, angle outside (0, 180], min_neighbours
 * < 3, normals whose count differs, a capacity too small. */
int mm3d_boundary_points(mm3d_ctx *ctx, const mm3d_cloud *points, const mm3d_normals *normals, double radius, double angle_deg,
                         int min_neighbours, unsigned char *flags, size_t capacity, long long *n_boundary);
/* ICP with the rejection rule and its step 1b from initial_guess, whatever the context's settings.  point_to_plane 0 / 1 selects
 * the estimate.  source_normals may be NULL when normals == 0; target_normals may be NULL when neither bit nor point_to_plane
 * needs them (boundary needs them: the flags are made here, with boundary_radius, which must be > 0).  Either stats may be
 * NULL.  MM3D_EINVAL: a NULL argument otherwise, options out of range, normals whose count differs from their cloud's. */
int mm3d_estimate_transform_icp_rejecting_geometry(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_normals *source_normals,
                                                   const mm3d_cloud *target, const mm3d_normals *target_normals, int point_to_plane,
                                                   const float initial_guess[16], double max_correspondence_distance,
                                                   const mm3d_icp_rejection_options *rejection_options,
                                                   const mm3d_icp_geometry_options *geometry_options, int max_iterations,
                                                   double transformation_epsilon, float T[16],
                                                   mm3d_icp_rejection_stats *rejection_stats, mm3d_icp_geometry_stats *geometry_stats);
/* test hook: ONE iteration's correspondence stage (steps 1, 1b, 2, 3) at T, operands as in the call above.  Per source point, in
 * the caller's order: the nearest target index (-1: none within the distance, or a non-finite source point), the float d2
 * (+inf: none) and a reason: 0 kept, 1 boundary, 2 normals, 3 one-to-one, 4 distance (none within
 * max_correspondence_distance, or cut by TRIMMED / MEDIAN).  split: 1 or 4.  Either stats may be NULL. */
int mm3d_debug_icp_geometry(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_normals *source_normals, const mm3d_cloud *target,
                            const mm3d_normals *target_normals, const float T[16], double max_correspondence_distance,
                            const mm3d_icp_rejection_options *rejection_options, const mm3d_icp_geometry_options *geometry_options,
                            int split, int *idx, float *d2, unsigned char *reason, mm3d_icp_rejection_stats *rejection_stats,
                            mm3d_icp_geometry_stats *geometry_stats);
/* test hook, process-wide like mm3d_debug_feature_lds_cap: the directions a wave of the boundary kernel keeps in LDS; a
 * neighbourhood with more takes the path that streams the other directions again from the grid.  cap in [1, 512] sets it, 0
 * restores the compiled value (512), negative = no change.  Returns the value in force. */
int mm3d_debug_boundary_lds_cap(int cap);

/* ---------------------------------------------------------------- opt-in robust ICP
 * mm3d_set_icp_robust gives the pair stage's ICP a robust loss: every matched correspondence enters the estimate with an
 * M-estimator weight of its Euclidean d2 at a scale that is fixed before the iteration runs (a table that the host builds, so
 * the weight is computed in the kernel that searches and sums: one fused launch and the finalize per iteration, no
 * correspondence array, no select).  Geman-McClure on an annealed scale is Fast Global Registration's objective (Zhou, Park,
 * Koltun, ECCV 2016) applied to ICP correspondences; it is the configuration whose recovery the tests assert.  Huber, Cauchy
 * and Tukey ship with their measured table and no promise.  With kernel OFF (the default) the
 * selection is inactive and the pair stage runs the kernels it always ran.
 * The rule, for ONE iteration, 0-based index k, of the loop that mm3d_set_icp_method states (everything else is that loop):
 *   1. match     step 1 of the rejection rule above, unchanged: a finite source point is carried by the current float T; its
 *                exact float nearest target point is found (ties to the lowest index); it is matched when d2 <= max_d2.
 *   2. scale     in double: s_0 = scale_start, s_{k+1} = s_k * anneal (IEEE multiplies, no pow); sigma_k = max(scale, s_k).
 *                scale_start = 0 means no annealing: sigma_k = scale for every k.  The table of sigma_k, k < max_iterations,
 *                is built on the host and uploaded once per batch.  final_k is sigma_k == scale.  (L2 reads no scale: its
 *                table holds `scale` throughout, so every iteration is final.)
 *   3. weight    in double: h = sigma_k * tuning, u2 = (double)d2 / (h * h), and
 *                L2 w = 1;  HUBER w = 1 if u2 <= 1, else 1 / sqrt(u2);  CAUCHY w = 1 / (1 + u2);
 *                TUKEY w = (1 - u2) * (1 - u2) if u2 < 1, else 0;  GEMAN_MCCLURE w = 1 / ((1 + u2) * (1 + u2)).
 *                tuning = 0 selects 1.345 (HUBER), 2.385 (CAUCHY), 4.685 (TUKEY) and 1.0 (GEMAN_MCCLURE, L2).
 *   4. estimate  the default kernels' terms (point-to-point's 17, point-to-plane's 30), each multiplied by w in double --
 *                w * ((double)bqx * p.x), the d2 term w * (double)d2, the count term w -- are summed in the default kernels'
 *                order, and sum w normalises the moments.  Both estimates weight by the match's Euclidean d2, the number the
 *                rejectors threshold on.  A point-to-plane row needs a finite normal, as always; the "six rows" test counts
 *                the rows with w > 0.  Two further sums are integers: `matched`, and `weighted`, the matches with w > 0.
 *                The "fewer than 3" stop and icp_correspondences count `weighted`.  The MSE of the convergence test is
 *                sum w d2 / sum w.
 *   5. convergence  the max_iterations stop always applies; the rotation / translation test and the MSE test apply only in
 *                iterations with final_k, so an annealing run cannot stop on a scale it is about to leave.  (The MSE of an
 *                iteration without final_k is not recorded either: the first final_k iteration compares with DBL_MAX.)
 * With kernel L2 the result, the iteration count and `converged` are the default ICP's, bit for bit, for either estimate.
 * Results are bit-identical for every stream count, batch and cache setting.  Applies to the ICP of
 * mm3d_estimate_maps_transforms and mm3d_pair_estimate with either mm3d_set_icp_method, and composes with
 * mm3d_set_icp_sampling (the robust step searches with the sample); mm3d_estimate_transform_icp,
 * mm3d_estimate_transform_icp_plane, transformScore and the overlap confidence do not read the setting.  Working memory per
 * pair of a batch: 8 B per iteration of the scale table, shared by the batch; nothing per point. */
typedef enum {
  MM3D_ROBUST_OFF = 0, MM3D_ROBUST_L2 = 1, MM3D_ROBUST_HUBER = 2, MM3D_ROBUST_CAUCHY = 3, MM3D_ROBUST_TUKEY = 4,
  MM3D_ROBUST_GEMAN_MCCLURE = 5
} mm3d_robust_kernel;
typedef struct mm3d_icp_robust_options {
  int kernel;                /* MM3D_ROBUST_* */
  double scale;              /* metres, > 0 and finite: the scale every run ends on */
  double scale_start;        /* metres: 0 (no annealing), or >= scale and finite */
  double anneal;             /* 0 < a <= 1 */
  double tuning;             /* >= 0 and finite; 0 = the kernel's constant above */
} mm3d_icp_robust_options;
typedef struct mm3d_icp_robust_stats {  /* of the LAST iteration that ran */
  long long matched;         /* finite source points whose nearest target point has d2 <= max_d2 */
  long long weighted;        /* of those, the ones with w > 0: == the pair record's icp_correspondences */
  double weight_sum;         /* sum w */
  double scale;              /* that iteration's sigma_k (0 when none ran) */
  int iterations, converged;
} mm3d_icp_robust_stats;
void mm3d_icp_robust_options_default(mm3d_icp_robust_options *o);   /* OFF, 0.05, 0, 0.5, 0 */
/* The selection is active when kernel != MM3D_ROBUST_OFF.  MM3D_EINVAL: ctx or options NULL, an unknown kernel, a value outside
 * its range above (the values are checked whatever the selection).  MM3D_EUNSUPPORTED: an active selection on a device-list
 * context (mm3d_create_devices), or while a correspondence rejection (mm3d_set_icp_rejection), coloured ICP
 * (mm3d_set_icp_color), generalized ICP (mm3d_set_icp_generalized) or NDT (mm3d_set_refinement) is active -- each of which in
 * turn refuses to become active while a robust kernel is selected; mm3d_shard_begin returns MM3D_EUNSUPPORTED on a context
 * with an active selection.  The setting reaches the context's mm3d_set_streams helpers, in either order, and is part of the
 * map cache's pair key while active. */
int mm3d_set_icp_robust(mm3d_ctx *ctx, const mm3d_icp_robust_options *options);
int mm3d_get_icp_robust(const mm3d_ctx *ctx, mm3d_icp_robust_options *options);   /* MM3D_EINVAL for NULL */
/* of the most recent pair whose ICP this context ran with a robust kernel (the last pair of a whole-map call on one stream, or
 * the call below); all zero before there was one */
int mm3d_last_icp_robust_stats(const mm3d_ctx *ctx, mm3d_icp_robust_stats *stats);
/* ICP with the rule above from initial_guess, whatever the context's setting.  options->kernel OFF runs as L2.  target_normals
 * NULL: the point-to-point estimate; else the point-to-plane one (normals in the target's order).  stats may be NULL.
 * MM3D_EINVAL: a NULL argument, options out of range, normals whose count differs from the target's. */
int mm3d_estimate_transform_icp_robust(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target,
                                       const mm3d_normals *target_normals, const float initial_guess[16],
                                       double max_correspondence_distance, const mm3d_icp_robust_options *options,
                                       int max_iterations, double transformation_epsilon, float T[16],
                                       mm3d_icp_robust_stats *stats);
/* test hook: iteration k's search, weights and sums at T, without the finalize.  Per source point, in the caller's order: the
 * matched target index (-1: none), the float d2 (+inf: none) and the double weight (0: none).  sums (may be NULL): the
 * iteration's totals as the finalize kernel forms them, 19 doubles (the 17 point-to-point terms, matched, weighted) or, with
 * normals, 32 (the 30 point-to-plane terms, matched, weighted).  split: 1 or 4, as in mm3d_debug_nn_search.  k >= 0.  stats (may
 * be NULL): the counts, sum w and sigma_k; iterations and converged are 0. */
int mm3d_debug_icp_robust(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target, const mm3d_normals *target_normals,
                          const float T[16], double max_correspondence_distance, const mm3d_icp_robust_options *options, int k,
                          int split, int *idx, float *d2, double *weight, double *sums, mm3d_icp_robust_stats *stats);
/* test hook, process-wide like mm3d_debug_icp_rejection_split: 0 = one or four work items per block chosen by size, as
 * everywhere; 1 or 4 = forced in every robust launch from now on; negative = no change.  Returns the value in force. */
int mm3d_debug_icp_robust_split(int split);

/* ---------------------------------------------------------------- opt-in coloured ICP
 * mm3d_set_icp_color puts a photometric term beside point-to-plane's in the pair stage's ICP (Park, Zhou, Koltun, "Colored Point
 * Cloud Registration Revisited", ICCV 2017; Open3D's registration_colored_icp is the known implementation, and no parity with it
 * is claimed).  Planes leave a pose open along themselves -- a corridor one direction, a floor with a wall two -- and
 * point-to-plane then stops at its degeneracy rule with T unchanged; the texture on such surfaces constrains exactly those
 * directions.  Disabled (the default), the pair stage runs the kernels it always ran.
 * Intensity: for rgba bits with bytes r, g, b, I = (float)((double)(299 r + 587 g + 114 b) / 255000.0), in [0, 1].
 * The gradient record of a target point i, float4 (gx, gy, gz, I_i), made once per map and option set from the map's normals:
 *   neighbours  the finite points j != i with float d2 = (dx dx + dy dy) + dz dz <= (float)(radius * radius), radius =
 *               gradient_radius, or params.normal_radius when that is 0.  A non-finite point or normal, or fewer than
 *               min_neighbours neighbours, gives g = 0.
 *   otherwise, in double: e = p_j - p_i, u = e - (e.n) n, w = I_j - I_i; M = sum u u^T + k^2 n n^T (k the neighbour count: the
 *               soft constraint g.n = 0), b = sum u w; M g = b by an unpivoted 3x3 LDLt; a pivot at or below 1e-12 trace(M) / 3
 *               gives g = 0; g is rounded to float once.  The order of the sums is a function of the cloud and the radius alone.
 * One iteration is mm3d_set_icp_method's in every respect but the terms.  Per matched source point, in double: s the
 * float-transformed point, q the target point, n and (g, I_t) the target's normal and record, I_s from the source point's rgba;
 *   vG = [s x n, n], rG = n.q - n.s                                       (point-to-plane's expressions)
 *   e = s - q, h = e.n, m = g - (g.n) n, pred = I_t + g.(e - h n), rC = I_s - pred, vC = [s x m, m]
 * and with mu = 1 - lambda_geometric the AtA term (i, j) is lambda (vG_i vG_j) + mu (vC_i vC_j), the Atr term i the same with
 * rG and rC; the squared distances, the correspondence count and the row count are point-to-plane's.  A correspondence whose
 * normal is not finite counts and adds no row; a zero gradient adds a zero colour row.  With lambda_geometric == 1 the terms are
 * point-to-plane's own and the result is mm3d_estimate_transform_icp_plane's, bit for bit.
 * Enabled, the pair stage's ICP is the coloured one whatever mm3d_set_icp_method says (mm3d_get_icp_method keeps answering its
 * own value); NDT (mm3d_set_refinement) does not read the setting, transformScore stays point-to-point, the overlap confidence
 * is untouched and nothing is drawn from rand().  mm3d_estimate_transform_icp and mm3d_estimate_transform_icp_plane do not see
 * the setting.  Results are bit-identical for every stream count, batch and cache setting.  Memory: 16 B per filtered point of a
 * map beside the 16 B of its normals. */
typedef struct mm3d_icp_color_options {
  int enabled;             /* 0 / 1 */
  double lambda_geometric; /* weight of the geometric rows, 0 < lambda <= 1; the photometric rows get 1 - lambda */
  double gradient_radius;  /* metres, > 0; 0 = params.normal_radius */
  int min_neighbours;      /* a point with fewer neighbours in the radius has a zero gradient; >= 4 */
} mm3d_icp_color_options;
void mm3d_icp_color_options_default(mm3d_icp_color_options *o);   /* 0, 0.968, 0, 4 (lambda: Open3D's default) */
/* MM3D_EINVAL: ctx or options NULL, enabled not 0 / 1, a value outside its range above (checked whatever `enabled` is).
 * MM3D_EUNSUPPORTED: enabled on a device-list context (mm3d_create_devices), or while a correspondence rejection is active
 * (mm3d_set_icp_rejection, which in turn refuses an active selection while colour is enabled) or generalized ICP is enabled
 * (mm3d_set_icp_generalized, likewise); mm3d_shard_begin returns
 * MM3D_EUNSUPPORTED on a context with colour enabled.  The setting reaches the context's mm3d_set_streams helpers, in either
 * order, and is part of the map cache's pair key while enabled. */
int mm3d_set_icp_color(mm3d_ctx *ctx, const mm3d_icp_color_options *options);
int mm3d_get_icp_color(const mm3d_ctx *ctx, mm3d_icp_color_options *options);   /* MM3D_EINVAL for NULL */
/* coloured ICP with the rule above from initial_guess, whatever options->enabled and the context's setting say; the target's
 * records are made from target_normals (in the target's order) for this call.  MM3D_EINVAL: a NULL argument, options out of
 * range, gradient_radius not > 0 (there are no parameters to take it from), normals whose count differs from the target's. */
int mm3d_estimate_transform_icp_color(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target,
                                      const mm3d_normals *target_normals, const float initial_guess[16],
                                      double max_correspondence_distance, const mm3d_icp_color_options *options,
                                      int max_iterations, double transformation_epsilon, float T[16]);
/* test hook: the gradient records of `points` with `normals` (gradient_radius > 0), out = [n][4]: gx gy gz I, in the points' order */
int mm3d_debug_color_gradients(mm3d_ctx *ctx, const mm3d_cloud *points, const mm3d_normals *normals,
                               const mm3d_icp_color_options *options, float *out);
/* test hook, process-wide like mm3d_debug_icp_rejection_split: 0 = one or four work items per block chosen by size, as
 * everywhere; 1 or 4 = forced in every coloured launch from now on; negative = no change.  Returns the value in force. */
int mm3d_debug_icp_color_split(int split);

/* ---------------------------------------------------------------- opt-in generalized ICP
 * mm3d_set_icp_generalized makes the pair stage's ICP plane-to-plane (Segal, Haehnel, Thrun, "Generalized-ICP", RSS 2009; PCL's
 * GeneralizedIterativeClosestPoint and Open3D's registration_generalized_icp are the known implementations, and no parity with
 * either is claimed).  Two maps sample the same surfaces differently, so a nearest neighbour is rarely the same surface point:
 * point-to-point is pulled along the surface by the sampling, and a source point near an edge that matches the neighbouring face
 * pulls point-to-plane.  Here a correspondence is weighted by the inverse of the sum of both surfaces' covariances, each the
 * disc I - (1 - epsilon) n n^T of its normal (PCL's R diag(1, 1, epsilon) R^T): an in-plane slide costs nothing, and a match
 * across two faces counts only along their common edge.  The covariances follow from the normals a map keeps already: nothing
 * new is made or stored per map.  Disabled (the default), the pair stage runs the kernels it always ran.
 * One iteration is mm3d_set_icp_method's in every respect but the 6x6 system: the float transform of the source by T, the exact
 * float nearest neighbour accepted at d2 <= max_d2, fewer than 3 correspondences -> stop, not converged, T <- Tinc * T in float
 * with Tinc = [Rz(gamma) Ry(beta) Rx(alpha) | t], and DefaultConvergenceCriteria's three tests.  Per matched source point i (its
 * index in the source's own order), in double: s the float-transformed point, q the target point, n_s and n_t the two normals.
 * A normal is usable when its three components are finite and n.n = (nx nx + ny ny) + nz nz > 0; its unit vector is
 * n / sqrt(n.n); the sign does not matter.  With both usable:
 *   m     = R n_s, R the 3x3 of T promoted to double, m_r = (R_r0 n_0 + R_r1 n_1) + R_r2 n_2 (not renormalised)
 *   Sigma = 2 I - (1 - epsilon) (n_t n_t^T + m m^T)                   (eigenvalues in [2 epsilon, 2])
 *   W     = Sigma^-1, the adjugate over the determinant
 *   e     = q - s,  J = [-[s]x | I3],  x = (alpha, beta, gamma, tx, ty, tz)
 * and the correspondence adds J^T W J to AtA, J^T W e to Atr, d2 to the squared distances, 1 to the correspondences and 3 to
 * the rows.  With either normal unusable it adds d2 and the 1 only (point-to-plane's rule for a non-finite normal).  The
 * solve, its degeneracy rule (fewer than 6 rows, or an LDLt pivot at or below 1e-12 trace / 6: stop, not converged, T as it
 * was) and the tail are point-to-plane's own.
 * Enabled, the pair stage's ICP is the generalized one whatever mm3d_set_icp_method says (mm3d_get_icp_method keeps answering
 * its own value), with both maps' normals at params.normal_radius; NDT (mm3d_set_refinement) does not read the setting,
 * transformScore stays point-to-point, the overlap confidence is untouched and nothing is drawn from rand().  The other stage
 * entry points do not see the setting.  Results are bit-identical for every stream count, batch and cache setting.  Memory:
 * the 16 B per filtered point of a map's normals. */
typedef struct mm3d_icp_generalized_options {
  int enabled;             /* 0 / 1 */
  double epsilon;          /* a surface's covariance along its normal, 0 < epsilon <= 1 (1: both covariances I, point-to-point's weights) */
} mm3d_icp_generalized_options;
void mm3d_icp_generalized_options_default(mm3d_icp_generalized_options *o);   /* 0, 1e-3 (PCL's gicp_epsilon) */
/* MM3D_EINVAL: ctx or options NULL, enabled not 0 / 1, epsilon outside (0, 1] or not finite (checked whatever `enabled` is).
 * MM3D_EUNSUPPORTED: enabled on a device-list context (mm3d_create_devices), or while a correspondence rejection is active
 * (mm3d_set_icp_rejection) or coloured ICP is enabled (mm3d_set_icp_color), each of which in turn refuses an active selection
 * while this is enabled; mm3d_shard_begin returns MM3D_EUNSUPPORTED on a context with it enabled.  The setting reaches the
 * context's mm3d_set_streams helpers, in either order, and is part of the map cache's pair key while enabled. */
int mm3d_set_icp_generalized(mm3d_ctx *ctx, const mm3d_icp_generalized_options *options);
int mm3d_get_icp_generalized(const mm3d_ctx *ctx, mm3d_icp_generalized_options *options);   /* MM3D_EINVAL for NULL */
/* generalized ICP with the rule above from initial_guess, whatever options->enabled and the context's setting say; each cloud's
 * normals in that cloud's order.  MM3D_EINVAL: a NULL argument, epsilon out of range, normals whose count differs from their
 * cloud's. */
int mm3d_estimate_transform_icp_generalized(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_normals *source_normals,
                                            const mm3d_cloud *target, const mm3d_normals *target_normals,
                                            const float initial_guess[16], double max_correspondence_distance,
                                            const mm3d_icp_generalized_options *options, int max_iterations,
                                            double transformation_epsilon, float T[16]);
/* test hook, process-wide like mm3d_debug_icp_color_split: 0 = one or four work items per block chosen by size, as everywhere;
 * 1 or 4 = forced in every generalized launch from now on; negative = no change.  Returns the value in force. */
int mm3d_debug_icp_generalized_split(int split);

/* ---------------------------------------------------------------- opt-in consistency-graph estimation under MATCHING
 * mm3d_set_estimator replaces the RANSAC behind estimation_method = MATCHING (pcl's CorrespondenceRejectorSampleConsensus:
 * 1 000 three-point samples, clean with probability w^3 at an inlier share w, so blind below about 10 %) by a deterministic
 * estimator over the rigidity of the correspondence set: two correct correspondences preserve the distance between their
 * points, a wrong one does so only by chance, so the graph of pairwise length-compatible correspondences holds the inliers as a
 * clique (Leordeanu and Hebert, "A spectral technique for correspondence problems using pairwise constraints", ICCV 2005; Chen
 * et al., "SC2-PCR", CVPR 2022).  It draws nothing from rand() nor from the RANSAC's mt19937.
 * The rule.  Inputs: C correspondences (s_i, t_i, .) in the order of findFeatureCorrespondences, the two keypoint clouds,
 * inlier_threshold and the options; p_i / q_i = the float coordinates of source keypoint s_i / target keypoint t_i, widened to
 * double.  All arithmetic is one IEEE operation per written operation (the library is built with -ffp-contract=off).
 *  1. Compatibility.  tau = options.tolerance, or inlier_threshold when it is 0; t2 = tau tau.  For i != j:
 *     da = (dx dx + dy dy) + dz dz on p_i - p_j, db likewise on q_i - q_j, and A_ij = 1 exactly when s_i != s_j, t_i != t_j,
 *     da > t2, db > t2 and e e <= 4.0 (da db) with e = (da + db) - t2 -- which is | |p_i-p_j| - |q_i-q_j| | <= tau without a
 *     square root.  Anything non-finite fails, because every comparison is false.  A is symmetric with a zero diagonal, kept as
 *     bit rows of ceil(C / 64) 64-bit words: bit j of row i is in word j / 64, bit j % 64; bits at and beyond C are zero.
 *  2. Degree.  deg_i = sum_j A_ij.
 *  3. Seeds.  The correspondences with deg_i >= 2, ordered by (deg descending, i ascending); the first
 *     min(options.seeds, their number) are kept, and the position in that list is the seed's rank.
 *  4. Second order, per seed s.  S_sj = A_sj ? popcount(row_s & row_j) : 0, the number of correspondences compatible with both.
 *     The consensus set K_s is s together with the options.consensus - 1 indices j of largest S_sj >= 1, ties to the lower j;
 *     it is read in ascending index order.  A seed with |K_s| < 3 has no hypothesis.
 *  5. Hypothesis.  Umeyama without scale over the pairs of K_s: the sums in double, in ascending index order, the SVD core of
 *     the library at precision 1e-12 (as the prerejective refit), the result rounded once to a float 4x4.
 *  6. Score.  The number of the C correspondences within the threshold under the hypothesis, as RANSAC counts them: the float
 *     transform, d2 < inlier_threshold^2.
 *  7. Pick.  The hypothesis with the most inliers, ties to the lower rank.  Its transform goes through what RANSAC's best model
 *     goes through: the inliers in correspondence order, failure below three inliers or on an identity model, the float
 *     Umeyama over the inliers.  No seed or no hypothesis: the all-zero matrix with no inliers, the reference's "could not be
 *     estimated".
 *  8. Limits.  C < 3 gives the zero matrix; C > 32 768 gives MM3D_EUNSUPPORTED (the bit rows would pass 128 MB per pair in
 *     flight).
 * Results are bit-identical whatever else runs: every decision is an integer or a comparison of fixed-order doubles, so they
 * do not depend on the stream count, the batch, the driver, the map cache or mm3d_srand.
 * The stage applies where params.estimation_method == MATCHING and no coarse alignment is selected, in
 * mm3d_estimate_maps_transforms and mm3d_pair_estimate; a pair record's n_correspondences and n_inliers mean what they mean
 * under RANSAC.  mm3d_estimate_transform and mm3d_estimate_transform_from_correspondences stay the reference's. */
typedef enum { MM3D_ESTIMATOR_RANSAC = 0, MM3D_ESTIMATOR_CONSISTENCY = 1 } mm3d_estimator_method;
typedef struct mm3d_estimator_options {
  int method;              /* mm3d_estimator_method */
  double tolerance;        /* tau of step 1, >= 0; 0 = inlier_threshold */
  int seeds;               /* 1..4096 */
  int consensus;           /* 3..64: |K_s| at most */
} mm3d_estimator_options;
void mm3d_estimator_options_default(mm3d_estimator_options *o);   /* RANSAC, 0, 64, 20 */
/* MM3D_EINVAL: ctx or options NULL, an unknown method, or a value out of range (checked whatever the method).
 * MM3D_EUNSUPPORTED: CONSISTENCY on a device-list context (mm3d_create_devices); mm3d_shard_begin returns MM3D_EUNSUPPORTED on
 * a context with it selected.  The setting reaches the context's mm3d_set_streams helpers, in either order, and is part of the
 * map cache's pair key while selected. */
int mm3d_set_estimator(mm3d_ctx *ctx, const mm3d_estimator_options *options);
int mm3d_get_estimator(const mm3d_ctx *ctx, mm3d_estimator_options *options);   /* MM3D_EINVAL for NULL */
typedef struct mm3d_estimator_stats {
  long long correspondences;   /* C */
  long long edges;             /* sum of deg / 2 */
  long long seeds;             /* seeds kept (step 3) */
  long long hypotheses;        /* seeds with a hypothesis (step 4) */
  int winner_index;            /* the winning seed's correspondence, -1: none */
  int winner_rank;             /* its rank, -1: none */
  int winner_inliers;          /* its count of step 6 */
} mm3d_estimator_stats;
/* of the context's most recent pair estimated with the stage selected */
int mm3d_last_estimator_stats(const mm3d_ctx *ctx, mm3d_estimator_stats *stats);
/* the rule above on a caller's correspondences, whatever options->method and the context's setting say; the arguments of
 * mm3d_estimate_transform_from_correspondences, the options and the statistics (may be NULL).  MM3D_EINVAL: a NULL argument,
 * options out of range, a correspondence index out of range; MM3D_EUNSUPPORTED: n_corr > 32 768. */
int mm3d_estimate_transform_consistency(mm3d_ctx *ctx, const mm3d_cloud *source_keypoints, const mm3d_cloud *target_keypoints,
                                        const mm3d_corr *corr, size_t n_corr, double inlier_threshold,
                                        const mm3d_estimator_options *options, float T[16], mm3d_corr *inliers, size_t cap,
                                        size_t *n_inliers, mm3d_estimator_stats *stats);
/* test hook: the intermediate results of the same call (any output may be NULL).  With W = ceil(n_corr / 64) and
 * H = min(options->seeds, n_corr): rows [n_corr][W] the bit rows, deg [n_corr], seeds [H] by rank (-1 padded) and their number,
 * consensus [H][options->consensus] ascending (-1 padded), hypotheses [H][16] column-major floats (zero without one),
 * counts [H] (-1 without a hypothesis).  n_corr < 3 leaves everything untouched but *n_seeds = 0. */
int mm3d_debug_consistency(mm3d_ctx *ctx, const mm3d_cloud *source_keypoints, const mm3d_cloud *target_keypoints,
                           const mm3d_corr *corr, size_t n_corr, double inlier_threshold, const mm3d_estimator_options *options,
                           unsigned long long *rows, int *deg, int *seeds, size_t *n_seeds, int *consensus, float *hypotheses,
                           int *counts);

/* ---------------------------------------------------------------- opt-in ICP source sampling
 * mm3d_set_icp_sampling makes the pair stage's ICP search a SAMPLE of the source map instead of every point of it: the step that
 * PCL offers as NormalSpaceSampling and Open3D as a down-sampling before registration_icp.  Every other opt-in widens what
 * registers; this one reduces what the ICP has to look at.  MM3D_ICP_SAMPLE_NORMAL_SPACE (Rusinkiewicz and Levoy, "Efficient
 * variants of the ICP algorithm", 3DIM 2001; no parity with PCL's class is claimed) keeps the same number of points from every
 * direction a surface faces, so the few points of a door frame or a kerb have their say beside the many of the floor;
 * MM3D_ICP_SAMPLE_STRIDE keeps evenly spaced valid points in the cloud's order.  MM3D_ICP_SAMPLE_NONE, the default: the pair
 * stage runs what it always ran.
 * The rule.  Everything is integer arithmetic, or an IEEE f32 multiply and a compare: no division of floats, no libm.
 *  1. Valid points.  Under STRIDE a point is valid when its three coordinates are finite; under NORMAL_SPACE its normal's three
 *     components must be finite too, and not all zero (-0 is zero).  Invalid points are never sampled; n_valid counts the valid.
 *  2. Buckets.  STRIDE has the one bucket 0.  NORMAL_SPACE has 3 bins^2 of them, bins in {1, 2, 4, 8}: the face a is the index of
 *     the normal's largest |component|, ties to the lowest index; s = n_a, b = (a + 1) % 3, c = (a + 2) % 3.  Antipodes fold -- n
 *     and -n share a bucket, both constrain the same plane: q = n_b when s > 0 and -n_b when s < 0, r = |s|.  The cell is
 *     cu = #{k in 1 .. bins - 1 : q >= e_k r}, the edge e_k = -1 + 2 k / bins being exact in f32 and e_k r ONE rounded f32
 *     multiply; cv is the same from n_c.  The bucket is (a bins + cu) bins + cv.
 *  3. Budget.  m = min(n_valid, floor(fraction n_valid)), the product in double; m = min(m, max_points) when max_points > 0;
 *     m is at least 1 when n_valid > 0.
 *  4. Water-fill.  With c_b the buckets' counts, L is the largest integer in [0, max c_b] with sum min(c_b, L) <= m, and
 *     take_b = min(c_b, L); the m - sum take_b that remain (fewer than there are buckets with c_b > L) go one each to the buckets
 *     with c_b > L, in ascending bucket index.  sum take_b = m exactly, and a bucket with c_b <= L is taken whole.
 *  5. Selection.  A valid point has the rank r among its bucket's points, from 0, in the cloud's order.  It is kept exactly when
 *     floor((r + 1) take_b / c_b) > floor(r take_b / c_b), in 64-bit integers: take_b points of the bucket, evenly spaced.
 *  6. The sample is the kept points in the cloud's order (the 16-byte records, colour included), a cloud of its own.
 * Selected, a pair's ICP searches the target with the SOURCE map's sample -- made with the map's normals at params.normal_radius
 * under NORMAL_SPACE, kept on the map, remade when the options change, built by mm3d_map_prepare or on the map's first use as a
 * source -- and is in every other respect the ICP it was: mm3d_set_icp_method's point-to-point or point-to-plane, with or without
 * mm3d_set_icp_rejection.  By construction the result is mm3d_sample_icp_source followed by the stage call on the sample.  A
 * pair record's icp_correspondences (and the rejection's statistics) then count SAMPLED points.  transformScore -- the pair's
 * confidence -- and the overlap confidence stay over the full source.  params.refine_transform 0 runs no ICP and no sampling.
 * A pair whose source has no valid point takes the ICP's empty-search path: the guess, no iterations, confidence 1 / DBL_MAX.
 * Nothing is drawn from rand(); results are bit-identical for every stream count, batch and cache setting.  Memory: 16 B per
 * sampled point plus its query copy, per map. */
typedef enum { MM3D_ICP_SAMPLE_NONE = 0, MM3D_ICP_SAMPLE_STRIDE = 1, MM3D_ICP_SAMPLE_NORMAL_SPACE = 2 } mm3d_icp_sample_method;
typedef struct mm3d_icp_sampling_options {
  int method;              /* mm3d_icp_sample_method */
  double fraction;         /* of the valid points, 0 < fraction <= 1 */
  int max_points;          /* >= 0; 0 = no cap */
  int bins;                /* 1, 2, 4 or 8 cells per axis of a face (NORMAL_SPACE) */
} mm3d_icp_sampling_options;
void mm3d_icp_sampling_options_default(mm3d_icp_sampling_options *o);   /* NONE, 0.25, 0, 4 */
/* MM3D_EINVAL: ctx or options NULL, an unknown method, fraction outside (0, 1], bins not 1 / 2 / 4 / 8, max_points < 0 (checked
 * whatever the method).  MM3D_EUNSUPPORTED: a method other than NONE on a device-list context (mm3d_create_devices), or while
 * NDT (mm3d_set_refinement), coloured ICP (mm3d_set_icp_color) or generalized ICP (mm3d_set_icp_generalized) is selected, each of
 * which in turn refuses its selection while a sampling method is set; mm3d_shard_begin returns MM3D_EUNSUPPORTED on a context
 * with one.  The setting reaches the context's mm3d_set_streams helpers, in either order, and is part of the map cache's pair
 * key while a method is set. */
int mm3d_set_icp_sampling(mm3d_ctx *ctx, const mm3d_icp_sampling_options *options);
int mm3d_get_icp_sampling(const mm3d_ctx *ctx, mm3d_icp_sampling_options *options);   /* MM3D_EINVAL for NULL */
typedef struct mm3d_icp_sampling_stats {
  long long points;            /* of the cloud */
  long long valid;             /* n_valid */
  long long sampled;           /* m */
  int buckets;                 /* buckets with c_b > 0 */
  int level;                   /* L */
} mm3d_icp_sampling_stats;
/* of the most recent sample this context made or fetched from a map (a stage call below, or a pair's source) */
int mm3d_last_icp_sampling_stats(const mm3d_ctx *ctx, mm3d_icp_sampling_stats *stats);
/* The rule above on a caller's cloud, whatever the context's setting: *out receives the sample (free it with mm3d_cloud_free; its
 * size is m), indices (may be NULL) the kept points' indices in `points`, ascending, at most `capacity` of them.  normals: one
 * per point under NORMAL_SPACE; not read, and may be NULL, under STRIDE.  MM3D_EINVAL: a NULL argument, options out of range or
 * of method NONE, normals whose count differs from the points'. */
int mm3d_sample_icp_source(mm3d_ctx *ctx, const mm3d_cloud *points, const mm3d_normals *normals,
                           const mm3d_icp_sampling_options *options, mm3d_cloud **out, int *indices, size_t capacity);
/* mm3d_sample_icp_source of the source followed by mm3d_estimate_transform_icp (target_normals NULL) or
 * mm3d_estimate_transform_icp_plane on the sample, from initial_guess, whatever the context's setting; options of method NONE
 * run the ICP on the source as it is.  mm3d_last_icp_iterations / mm3d_last_icp_converged report on it.  A source without a valid
 * point: MM3D_OK, T = initial_guess, no iterations.  MM3D_EINVAL: a NULL argument other than the two normals where they are not
 * read, options out of range, normals whose count differs from their cloud's. */
int mm3d_estimate_transform_icp_sampled(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_normals *source_normals,
                                        const mm3d_cloud *target, const mm3d_normals *target_normals,
                                        const mm3d_icp_sampling_options *options, const float initial_guess[16],
                                        double max_correspondence_distance, int max_iterations, double transformation_epsilon,
                                        float T[16]);

#ifdef __cplusplus
}
#endif
#endif /* MM3D_H_ */

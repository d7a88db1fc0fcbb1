// nn_core.hpp -- what the ICP / score tail of a pair estimate is made of, shared by nn.hip (the batch driver, the point-to-point
// ICP and the score) and the files that put another ICP in its place (icp_plane.hip, icp_color.hip, icp_generalized.hip, icp_reject.hip, icp_robust.hip, ndt.hip):
// the search knobs, the ICP state, the job layout and the wave helpers of the kernels; and, for the host, the set-up of one
// search (NnSearch) and the interface through which a variant takes part in a batch (IcpStep).  The search itself is
// nn_search_body.hpp (see there); how an iteration ends -- the partials, the totals, the estimate, the convergence step -- is
// icp_tail.hpp, one text for every variant's kernels.
#pragma once
#include <cfloat>
#include <cstddef>
#include <type_traits>

#include "device_util.hpp"
#include "linalg_shared.hpp"

namespace mm3d {

constexpr int kAcc = 17;     // sum p(3) | sum q(3) | sum q p^T (9, row = q) | sum d2 | count
#ifndef MM3D_NN_TILE
#define MM3D_NN_TILE 256
#endif
#ifndef MM3D_NN_WPE
#define MM3D_NN_WPE 4
#endif
#ifdef MM3D_NN_WPE
#define MM3D_NN_ATTR __attribute__((amdgpu_waves_per_eu(MM3D_NN_WPE, MM3D_NN_WPE)))
#else
#define MM3D_NN_ATTR
#endif
constexpr int kTile = MM3D_NN_TILE;   // staged target points per wave and tile (8 KiB of LDS)
#ifndef MM3D_NN_ROWS_PER_LANE
#define MM3D_NN_ROWS_PER_LANE 4
#endif
// MM3D_NN_PREFETCH=1: the next tile's gathers are issued into registers before this tile is scanned.  Measured and left off:
// 16 more VGPRs (112: four waves per SIMD instead of five for the ICP variant) for a latency that the other resident waves
// already cover -- headline 955 against 960 map-pairs/s, 64 x 50 k 10 250 against 10 520 (interleaved A/B, round 4).
#ifndef MM3D_NN_PREFETCH
#define MM3D_NN_PREFETCH 0
#endif
#ifndef MM3D_NN_TIGHT_BOX
#define MM3D_NN_TIGHT_BOX 1
#endif
#ifndef MM3D_NN_SHELL
#define MM3D_NN_SHELL 1
#endif
#ifndef MM3D_NN_LOWER_BOUND
#define MM3D_NN_LOWER_BOUND 1
#endif
#ifndef MM3D_NN_CORNERS
#define MM3D_NN_CORNERS 1
#endif
constexpr bool kPrefetch = MM3D_NN_PREFETCH != 0;
constexpr int kRowsPerLane = MM3D_NN_ROWS_PER_LANE;   // row headers a lane reads per chunk
constexpr int kRows = kWave * kRowsPerLane;           // rows of the box per chunk (power of two: the slot -> row search halves it)

#ifdef MM3D_NN_STATS
// (static: one per translation unit; mm3d_debug_nn_stats reads nn.hip's)
static __device__ unsigned long long g_nn_stats[64];   // 0 waves, 1 passes, 2 row chunks, 3 staged points, 4 active lanes at pass, 5 rows, 6 max wave cycles, 7 sum wave cycles, 8.. log2 histogram of wave cycles
#define MM3D_STAT(i_, v_) do { if (MM3D_NN_STATS == 1 && lane == 0) atomicAdd(&g_nn_stats[i_], (unsigned long long)(v_)); } while (0)
#define MM3D_TICK(var_) const long long var_ = wall_clock64()
// (phase ticks are summed in registers and flushed once per wave: an atomic per chunk on one word slowed the kernel threefold)
#define MM3D_TOCK(i_, from_) do { stat_ticks[(i_) - 32] += wall_clock64() - (from_); } while (0)
#else
#define MM3D_STAT(i_, v_)
#define MM3D_TICK(var_)
#define MM3D_TOCK(i_, from_)
#endif

struct IcpState {
  float T[16];      // cumulative transform applied to the original source points (starts at the guess)
  float Tinc[16];
  double prev_mse;
  double rot_thresh, trans_thresh;
  int iters, done, converged, n_corr, max_iter;
  int scored;      // the score of the final transform has been taken (k_score_finalize)
};

// One (source cloud, target grid) search of a launch: blockIdx.y picks the job, so the searches of several map
// pairs that are ready at the same time share one launch (many small maps: a launch per pair leaves most of the
// chip idle, and only four launches run at a time).
struct NnJob {
  const float4 *src;          // source points in Hilbert order
  const int2 *items;          // their work items
  int n_items, nblocks;       // blocks this job uses of the launch's grid.x
  int split;                  // 1: one work item per block (partials per item), 0: four items per block
  GridView g;                 // target grid
  const float4 *tgt_ref;      // target points in reference order
  IcpState *st;               // ICP: the pair's state; score: T is read from its head (or from Tc)
  const float *Tc;            // score: the transform, when it is not the ICP state's
  double *partials;           // [nblocks][kAcc]
  double *out;                // score: {sum d2, count}
  int max_ring;
};

// (wave-uniform, in a scalar register: device_util.hpp's DPP reductions)
__device__ __forceinline__ int wave_min_i(int v) { return wave_min_int(v); }
__device__ __forceinline__ int wave_max_i(int v) { return wave_max_int(v); }
// LDS written by some lanes of a wave and read by others: order the accesses for the compiler;
// the hardware executes one wave's DS operations in order.
__device__ __forceinline__ void wave_lds_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Partial sums of "block" b as the four-items-per-block kernels write them.  The one-item-per-block kernels leave
// one partial per item; adding four neighbours here, in the order those kernels' last step does, gives the same
// bits -- so which variant ran (a choice that depends on what else was ready at the time) never shows in a result.
template <int NACC>
__device__ __forceinline__ double nn_block_partial_n(const double *__restrict__ p, int b, int k, int split, int n_items)
{
  if (!split) return p[(size_t)b * NACC + k];
  const int i = b * 4;
  double v = p[(size_t)i * NACC + k];
  v += (i + 1 < n_items) ? p[(size_t)(i + 1) * NACC + k] : 0.0;
  v += (i + 2 < n_items) ? p[(size_t)(i + 2) * NACC + k] : 0.0;
  v += (i + 3 < n_items) ? p[(size_t)(i + 3) * NACC + k] : 0.0;
  return v;
}

// What a search derives from its range: the largest squared distance that is still a correspondence, the radius the
// search has to prove (with the slack that covers its own rounding) and the radius the target's grid is built for.
struct NnRange { float max_d2, rmax; double radius; };
NnRange nn_range_icp(double max_corr_dist);
NnRange nn_range_score(double max_distance);
// one work item per block (the kernels' SPLIT 4) for a source of so few items, and the blocks a job then takes
bool nn_split_items(int n_items);
inline unsigned nn_blocks(int n_items, bool split) { return split ? (unsigned)n_items : div_up(n_items, 4); }

// What a search of `src` in `tgt` needs on the host.  src is null when there is nothing to search (an empty cloud, no finite
// source point); grid is null then, when the target has no finite point, and when no range was given (NDT reads no grid).
struct NnSearch {
  const float4 *src = nullptr;      // the source in Hilbert order,
  const int2 *items = nullptr;      // its work items,
  int ns = 0, n_items = 0;          // its finite points and how many items they make
  const float4 *tgt_ref = nullptr;  // the target in reference order
  const Grid *grid = nullptr;       // the target's grid at the range's cell, its distance transform built out to
  int max_ring = 0;                 // this ring
};
// builds what is missing of it on the clouds' caches (cloud_hilbert, cloud_grid, grid_ensure_dt)
NnSearch nn_search(Context *c, const mm3d_cloud *src, const mm3d_cloud *tgt, const NnRange *range);
NnJob nn_job(const NnSearch &s, bool split, unsigned nblocks, IcpState *st, const float *Tc, double *partials, double *out);

// One ICP variant's side of a batch of pairs (nn.hip's icp_batch).  The batch owns what is common: the live pairs, the split,
// the states, the ICP and score NnJobs, the one pinned block, the chunked iterations with their speculative score, the one
// copy back and wait per round.  It asks the step for the rest, in this order: check per pair, the sizes, begin, bind per pair,
// upload, iterate per iteration, close per pair.
struct IcpLaunch {
  const NnJob *jobs_dev;            // the batch's ICP jobs
  int count;
  unsigned grid_x;                  // the largest job's blocks
  bool split;
  float max_d2, rmax;
  double bytes, finalize_bytes;     // profile table: bytes_per_point over the batch; the partials
};
struct IcpStep {
  virtual ~IcpStep() = default;
  int acc = kAcc;                   // doubles per block of partials
  bool searches = true;             // reads the target's grid and follows the batch's split (NDT: neither; four items per block)
  int forced_split = 0;             // test hook: 0 (by size), 1 or 4
  virtual double bytes_per_point(const IcpScoreJob &J) const = 0;   // profile table
  virtual void check(const IcpScoreJob &) const {}                  // throws when the pair lacks the variant's operand
  // Asked before the batch's one pin() (a second request could replace the arena): host bytes for B pairs, a multiple of 16,
  // and bytes that ride behind the IcpStates in the state copies, up and back
  virtual size_t pinned_bytes(int B) const { return 0; }
  virtual size_t record_bytes(int B) const { return 0; }
  // the step's device arrays for the B live pairs; its part of the pinned block; the bytes behind the states on both sides
  virtual void begin(Context *c, const IcpScoreJob *const *live, int B, char *pinned, void *rec_host, void *rec_dev) {}
  virtual void bind(int b, const NnJob &q, const IcpScoreJob &J) {}  // pair b, from its filled ICP job
  virtual void upload(Context *c) {}
  virtual void iterate(Context *c, const IcpLaunch &L) = 0;         // the search / reduction launches and the finalize launch
  virtual void close(int b, const IcpState &h, IcpScoreJob &J) {}   // pair b has finished: h and the records are final
};
// a step's job array: the host image in the batch's pinned block and the device copy
template <class Job>
struct StepJobs {
  DevBuf<Job> dev;
  Job *host = nullptr;
  static size_t bytes(int B) { return (sizeof(Job) * B + 15) & ~(size_t)15; }
  char *begin(Context *c, int B, char *pinned)
  {
    dev = DevBuf<Job>(c, (size_t)B);
    host = (Job *)pinned;
    return pinned + bytes(B);
  }
  void upload(Context *c) { MM3D_HIP(hipMemcpyAsync(dev.get(), host, sizeof(Job) * dev.size(), hipMemcpyHostToDevice, c->stream)); }
};

// nn.hip: k_icp_finalize over NnJobs (the rejecting step without normals ends an iteration with it)
void icp_point_finalize(Context *c, const NnJob *jobs_dev, int count, double bytes);

// point-to-plane ICP (icp_plane.hip): the search job plus the target's normals, in the target's reference order (tgt_ref's).
// Coloured ICP, generalized ICP and the rejecting step with normals keep such an array too: k_icp_plane_finalize reads it.
struct NnPlaneJob {
  NnJob nn;                   // nn.partials: [nblocks][kPlaneAcc]
  const float4 *nrm;
};
// AtA upper triangle (21) | Atr (6) | sum d2 | correspondences | rows with a finite normal
constexpr int kPlaneAcc = 30;
inline void icp_plane_check(const IcpScoreJob &J)
{
  if (!J.tgt_normals || J.tgt_normals->n != J.tgt->n)
    throw Error(MM3D_EINVAL, "point-to-plane ICP: the target's normals do not match its points");
}
inline NnPlaneJob icp_plane_job(const NnJob &q, const IcpScoreJob &J)
{
  return NnPlaneJob{q, J.tgt_normals ? (const float4 *)J.tgt_normals->nrm.get() : nullptr};
}
// icp_plane.hip: k_icp_plane_finalize over NnPlaneJobs; the method, for a stage-level call that has normals
void icp_plane_finalize(Context *c, const NnPlaneJob *jobs_dev, int count, double finalize_bytes);
const IcpMethodBase *icp_plane_method();

// icp_reject.hip (mm3d_set_icp_rejection): the step that puts a correspondence stage between the search and the sums of the
// point-to-point ICP or, with normals, of point-to-plane; geometry (mm3d_set_icp_geometry_rejection): non-null = with step 1b,
// whose operands the jobs carry
std::unique_ptr<IcpStep> icp_reject_step(const mm3d_icp_rejection_options &opt, bool normals, const mm3d_icp_geometry_options *geometry = nullptr);
// icp_geometry.hip: the boundary flags of `points` with `normals` (device, the points' order) by the rule of include/mm3d.h into
// flags_dev [points->n]; asynchronous on c's stream
void boundary_flags(Context *c, const mm3d_cloud *points, const float4 *normals_dev, double radius, double angle_deg, int min_neighbours,
                    unsigned char *flags_dev);
// ... and their number, after a wait
long long boundary_count(Context *c, const unsigned char *flags_dev, size_t n);
bool icp_geometry_options_valid(const mm3d_icp_geometry_options *o);

// icp_robust.hip (mm3d_set_icp_robust): the step whose fused search weights every match by an M-estimator of its d2 before the
// sums of the point-to-point ICP or, with normals, of point-to-plane; max_iterations sizes its table of scales
std::unique_ptr<IcpStep> icp_robust_step(const mm3d_icp_robust_options &opt, bool normals, int max_iterations);

}  // namespace mm3d

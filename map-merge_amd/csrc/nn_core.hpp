// nn_core.hpp -- what the ICP / score kernels of nn.hip (k_nn_wave) and the point-to-plane ICP kernel of icp_plane.hip
// (k_icp_plane_wave) share: the search knobs, the ICP state, the job layout and the wave helpers.  The search itself is
// nn_search_body.hpp (see there).
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

// point-to-plane ICP (icp_plane.hip): the search job plus the target's normals, in the target's reference order (tgt_ref's)
struct NnPlaneJob {
  NnJob nn;                   // nn.partials: [nblocks][kPlaneAcc]
  const float4 *nrm;
};
// AtA upper triangle (21) | Atr (6) | sum d2 | correspondences | rows with a finite normal
constexpr int kPlaneAcc = 30;
// one point-to-plane ICP iteration of a batch (icp_corr_reduce's and icp_finalize's counterparts): the search + reduction
// launch, then the solve / accumulate / convergence launch, on the same IcpState protocol as icp_score_batch's
void icp_plane_step(Context *c, const NnPlaneJob *jobs_dev, int count, unsigned grid_x, bool split, float max_d2, float rmax,
                    double bytes, double finalize_bytes);


// NDT (ndt.hip): the job's source side and state (nn.g, nn.tgt_ref and nn.max_ring are not read; nn.split is 0: always four work
// items per block, so nn.partials is [ceil(n_items / 4)][kNdtAcc] whatever the batch), and the target's voxel table
struct NdtJob {
  NnJob nn;
  const float4 *rec;          // NdtTable::rec
  const int *index;           // NdtTable::index
  float inv, mn[3];
  int dims[3];
  int neighbours;             // 1 or 7
  int n_src;                  // finite source points: the divisor of the convergence test's mean weight
};
// H upper triangle (21) | g (6) | sum w | terms | points with at least one term
constexpr int kNdtAcc = 30;
// one NDT iteration of a batch: the lookup + reduction launch, then the solve / accumulate / convergence launch, on the same
// IcpState protocol as icp_score_batch's
void ndt_step(Context *c, const NdtJob *jobs_dev, int count, unsigned grid_x, double bytes, double finalize_bytes);

// ICP with correspondence rejection (icp_reject.hip, mm3d_set_icp_rejection).  What one pair's selection leaves behind, on the
// device beside the pair's IcpState and back on the host in the copy that brings the states: the counts of the last iteration
// that ran and the state of the radix select (prefix / rank BEFORE pass q of four 8-bit passes over the d2 bits).
struct RejRecord {
  unsigned matched, survivors, kept;
  unsigned tau_bits;          // TRIMMED: tau; MEDIAN: m (valid when cut == 0)
  int cut;                    // 0: cut at tau_bits, 1: nothing is cut, 2: everything is cut
  unsigned prefix[4], rank[4];
};
// the search job plus the rejecting stage's working memory; nn.partials: [nblocks][kAcc], or [nblocks][kPlaneAcc] with normals
struct NnRejectJob {
  NnJob nn;
  const float4 *nrm;          // point-to-plane: the target's normals (tgt_ref's order); null: point-to-point
  int2 *corr;                 // [n_src], at the point's place in the Hilbert-ordered source: {target index (-1: none;
                              // -2 - index: lost its target under one_to_one), d2 bits}
  unsigned long long *owner;  // one_to_one: [n_tgt] smallest key d2 bits << 32 | original source index per target point
  unsigned *hist;             // [4][256]
  RejRecord *rec;
  int n_src;                  // finite source points
};
// One iteration's correspondence stage and sums for a batch: begin, search, the select's passes, the reduction into nn.partials
// in the default kernels' layout and order.  The caller runs the default finalize kernel afterwards (k_icp_finalize over its
// NnJobs, icp_plane_finalize over its NnPlaneJobs).  owner_all / owner_bytes: the batch's owner arrays as one region.
void icp_reject_step(Context *c, const NnRejectJob *jobs_dev, int count, unsigned grid_x, unsigned max_src, bool split, bool plane,
                     float max_d2, float rmax, const mm3d_icp_rejection_options &opt, unsigned long long *owner_all, size_t owner_bytes,
                     double bytes);
// icp_plane.hip: k_icp_plane_finalize alone
void icp_plane_finalize(Context *c, const NnPlaneJob *jobs_dev, int count, double finalize_bytes);
// mm3d_debug_icp_rejection_split: 0 (by size), 1 or 4
int icp_reject_forced_split();
// mm3d_debug_icp_rejection: begin, search and the select's passes for ONE job, then every source point's decision at its original index
void icp_reject_debug(Context *c, const NnRejectJob *job_dev, unsigned grid_x, unsigned n_src, int n_items, bool split, float max_d2, float rmax,
                      const mm3d_icp_rejection_options &opt, unsigned long long *owner, size_t owner_bytes, int *out_idx, float *out_d2,
                      unsigned char *out_kept);
bool icp_rejection_options_valid(const mm3d_icp_rejection_options *o);

// coloured ICP (icp_color.hip, mm3d_set_icp_color): the point-to-plane job plus the target's gradient records and the source's
// reference points (their rgba).  pl.nn.partials: [nblocks][kPlaneAcc], read by k_icp_plane_finalize over the NnPlaneJobs.
struct NnColorJob {
  NnPlaneJob pl;
  const float4 *rec;          // the target's records (gx, gy, gz, I), in tgt_ref's order
  const float4 *src_ref;      // the source's points in reference order (nn.src's .w indexes them)
};
// one coloured iteration's search + reduction launch for a batch; the caller runs icp_plane_finalize afterwards.  lambda: the
// weight of the geometric rows (the photometric ones get 1 - lambda; 1: point-to-plane's terms, bit for bit)
void icp_color_step(Context *c, const NnColorJob *jobs_dev, int count, unsigned grid_x, bool split, float max_d2, float rmax, double lambda,
                    double bytes);
// mm3d_debug_icp_color_split: 0 (by size), 1 or 4
int icp_color_forced_split();
bool icp_color_options_valid(const mm3d_icp_color_options *o);

}  // namespace mm3d

// nn.hip -- ICP and transformScore: exact 1-NN of every (transformed) source point in the target
// grid, fused with the reduction the caller needs (K12/K13 in SURVEY 2.2).
//
// estimateTransformICP  R/src/matching.cpp:196-221 -> pcl::IterativeClosestPoint (point-to-point,
//                       TransformationEstimationSVD/Umeyama, DefaultConvergenceCriteria)
// transformScore        R/src/matching.cpp:259-268 -> TransformationValidationEuclidean
//
// Wave-cooperative search.  A wave owns one work item of the source's Hilbert order (<= 64 points
// forming a compact patch), so the cells its queries can touch form a small box of the target grid.  The wave
//   1. reads one distance-transform byte per lane (how many cells to the nearest occupied cell;
//      out of range -> that lane is done),
//   2. takes the bounding box of its lanes' cells, grows it by the largest radius any lane needs,
//   3. streams the box's rows (contiguous spans of the cell-sorted target) through LDS with
//      coalesced 16-byte loads, 512 points per tile,
//   4. every lane scans the tile out of LDS (same address for all lanes = broadcast reads; the tile is
//      kept per component, so four candidates are one 16-byte read and their distances pack),
//   5. a lane is finished when its best distance is within what the box provably covers; otherwise
//      the box grows once more to the radius that lane needs.
// Candidate traffic is therefore LDS traffic; HBM sees the source once (16 B/point) and each target
// span once per wave.  The ICP iteration stays two launches and no host round trip:
// icp_corr_reduce (this search + 17 double partial sums per block through wave shuffles) and
// icp_finalize (Umeyama by 3x3 Jacobi SVD, accumulate, PCL's convergence tests, all on the device).
// Algorithmic traffic: 12 B per source point per iteration.
#include "capi_guard.hpp"
#include "nn_core.hpp"

namespace mm3d {

// MODE 0: ICP (transform from the device state, accumulate Umeyama moments)
// MODE 1: transformScore (transform from Tc, accumulate sum d2 / count for d2 <= max_d2)
// SPLIT 1: one work item per wave, four items per block.
// SPLIT 4: one work item per BLOCK: its four waves hold the same 64 points and the same box, each stages and
//          scans a quarter of the box's candidates, and the four minima meet in LDS after every pass.  Same
//          result, a quarter of the time per item: for a source of a few hundred items (a 50 k point map) the
//          chip is mostly idle and the kernel's duration IS one wave's scan.
template <int MODE, int SPLIT>
__global__ void __launch_bounds__(256) MM3D_NN_ATTR
k_nn_wave(const NnJob *__restrict__ jobs, float max_d2, float rmax)
{
  const NnJob &job = jobs[blockIdx.y];
  if ((int)blockIdx.x >= job.nblocks) return;            // the grid is as wide as the batch's largest job
  const float4 *__restrict__ src = job.src;
  const int2 *__restrict__ items = job.items;
  const int n_items = job.n_items;
  const GridView g = job.g;
  const float4 *__restrict__ tgt_ref = job.tgt_ref;
  const IcpState *__restrict__ st = job.st;
  const float *__restrict__ Tc = job.Tc ? job.Tc : job.st->T;
  double *__restrict__ partials = job.partials;
  const int max_ring = job.max_ring;
  __shared__ float Ts[16];
  __shared__ double red[4][kAcc];
  // staged candidates, one array per component: four candidates' x (y, z, index) are ONE 16-byte
  // broadcast read, and the distance arithmetic of candidate pairs packs into v_pk_* instructions
  __shared__ __attribute__((aligned(16))) float s_cx[4][kTile], s_cy[4][kTile], s_cz[4][kTile];
  __shared__ __attribute__((aligned(16))) unsigned s_cw[4][kTile];
  __shared__ int s_off[4][kRows];
  __shared__ int s_beg[4][kRows];
  __shared__ unsigned long long s_merge[SPLIT == 4 ? 4 : 1][64];
  if (MODE == 0 && st->done) return;
  // the score of a pair's ICP result: once, in the first round after its ICP has finished
  if (MODE == 1 && st && (!st->done || st->scored)) return;
  if (threadIdx.x < 16) Ts[threadIdx.x] = (MODE == 0) ? st->T[threadIdx.x] : Tc[threadIdx.x];
  __syncthreads();
#include "nn_search_body.hpp"
  if (SPLIT == 4 && wave != 0) return;     // the four waves hold the same result
  double acc[kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; ++k) acc[k] = 0.0;
  if (valid && best <= max_d2) {   // false for INFINITY / NaN
    if (MODE == 0) {
      const float4 bq = tgt_ref[(unsigned)(bkey & 0xffffffffull)];
      const float bqx = bq.x, bqy = bq.y, bqz = bq.z;
      acc[0] = p.x; acc[1] = p.y; acc[2] = p.z;
      acc[3] = bqx; acc[4] = bqy; acc[5] = bqz;
      acc[6] = (double)bqx * p.x; acc[7] = (double)bqx * p.y; acc[8] = (double)bqx * p.z;
      acc[9] = (double)bqy * p.x; acc[10] = (double)bqy * p.y; acc[11] = (double)bqy * p.z;
      acc[12] = (double)bqz * p.x; acc[13] = (double)bqz * p.y; acc[14] = (double)bqz * p.z;
    }
    acc[15] = best;
    acc[16] = 1.0;
  }
  // A wave none of whose points found a neighbour in range adds seventeen zeros: it writes them without the seventeen
  // reductions (each six shuffle steps on a double).  With the headline's initial poses that is a good part of the waves.
  const bool any_corr = ballot(valid && best <= max_d2) != 0ull;       // wave-uniform
  if (SPLIT == 4) {
#pragma unroll
    for (int k = 0; k < kAcc; ++k) {
      const double v = ((MODE == 0 || k >= 15) && any_corr) ? wave_sum(acc[k]) : 0.0;
      if (lane == 0) partials[(size_t)bid * kAcc + k] = v;
    }
    return;
  }
#pragma unroll
  for (int k = (MODE == 0 ? 0 : 15); k < kAcc; ++k) {
    const double v = any_corr ? wave_sum(acc[k]) : 0.0;
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kAcc) {
    const int k = threadIdx.x;
    double v = 0.0;
    if (MODE == 0 || k >= 15) v = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    partials[(size_t)bid * kAcc + k] = v;
  }
}

// The search alone, per point (test hook mm3d_debug_nn_search): nn_search_body.hpp's keyed search (MODE 0) for one job, and
// each valid lane's result -- the winner's original index and the d2 the lane holds, or -1 / +inf -- stored at the source
// point's ORIGINAL index (src[i].w).  A third compile of the shared body (the same tokens, its own machine code); the
// tests tie k_nn_wave's sums to what it returns.
template <int SPLIT>
__global__ void __launch_bounds__(256) MM3D_NN_ATTR
k_nn_probe(const NnJob *__restrict__ jobs, float max_d2, float rmax, int *__restrict__ out_idx, float *__restrict__ out_d2)
{
  constexpr int MODE = 0;
  const NnJob &job = jobs[0];
  if ((int)blockIdx.x >= job.nblocks) return;
  const float4 *__restrict__ src = job.src;
  const int2 *__restrict__ items = job.items;
  const int n_items = job.n_items;
  const GridView g = job.g;
  const float *__restrict__ Tc = job.Tc;
  const int max_ring = job.max_ring;
  __shared__ float Ts[16];
  __shared__ __attribute__((aligned(16))) float s_cx[4][kTile], s_cy[4][kTile], s_cz[4][kTile];
  __shared__ __attribute__((aligned(16))) unsigned s_cw[4][kTile];
  __shared__ int s_off[4][kRows];
  __shared__ int s_beg[4][kRows];
  __shared__ unsigned long long s_merge[SPLIT == 4 ? 4 : 1][64];
  if (threadIdx.x < 16) Ts[threadIdx.x] = Tc[threadIdx.x];
  __syncthreads();
#include "nn_search_body.hpp"
  if (SPLIT == 4 && wave != 0) return;     // the four waves hold the same result
  if (valid) {
    const int o = __float_as_int(src[i].w);
    const bool found = (unsigned)bkey != 0xffffffffu;
    out_idx[o] = found ? (int)(unsigned)bkey : -1;
    out_d2[o] = found ? best : INFINITY;
  }
}

// one block: reduce partials, Umeyama, accumulate, convergence (DefaultConvergenceCriteria)
// Partial sums of "block" b as the four-items-per-block kernel writes them.  The one-item-per-block kernel leaves
// one partial per item; adding four neighbours here, in the order that kernel's last step does, gives the same
// bits -- so which variant ran (a choice that depends on what else was ready at the time) never shows in a result.
__device__ __forceinline__ double nn_block_partial(const double *__restrict__ p, int b, int k, int split, int n_items)
{
  if (!split) return p[(size_t)b * kAcc + k];
  const int i = b * 4;
  double v = p[(size_t)i * kAcc + k];
  v += (i + 1 < n_items) ? p[(size_t)(i + 1) * kAcc + k] : 0.0;
  v += (i + 2 < n_items) ? p[(size_t)(i + 2) * kAcc + k] : 0.0;
  v += (i + 3 < n_items) ? p[(size_t)(i + 3) * kAcc + k] : 0.0;
  return v;
}

__global__ void __launch_bounds__(256) k_icp_finalize(const NnJob *__restrict__ jobs)
{
  __shared__ double red[4][kAcc];
  __shared__ double tot[kAcc];
  const double *__restrict__ partials = jobs[blockIdx.x].partials;
  const int split = jobs[blockIdx.x].split, n_items = jobs[blockIdx.x].n_items;
  const int nblocks = (n_items + 3) >> 2;              // in units of four items, whichever kernel wrote them
  IcpState *st = jobs[blockIdx.x].st;
  if (st->done) return;
  double acc[kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; ++k) acc[k] = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += blockDim.x)
#pragma unroll
    for (int k = 0; k < kAcc; ++k) acc[k] += nn_block_partial(partials, b, k, split, n_items);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kAcc; ++k) {
    const double v = wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kAcc) tot[threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
  __syncthreads();
  if (threadIdx.x != 0) return;

  const double cnt = tot[16];
  st->n_corr = (int)cnt;
  if (cnt < 3.0) {   // min_number_correspondences_: "Not enough correspondences" -> not converged, stop
    st->converged = 0;
    st->done = 1;
    return;
  }
  const double inv = 1.0 / cnt;
  double mp[3] = {tot[0] * inv, tot[1] * inv, tot[2] * inv}, mq[3] = {tot[3] * inv, tot[4] * inv, tot[5] * inv};
  double sigma[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) sigma[r * 3 + c] = tot[6 + r * 3 + c] * inv - mq[r] * mp[c];
  double U[9], S[3], V[9];
  svd3_shared(sigma, U, S, V);
  double Sd[3] = {1.0, 1.0, 1.0};
  if (det3_shared(sigma) < 0) Sd[2] = -1.0;
  int rank = 0;
  for (int i = 0; i < 3; ++i)
    if (!(fabs(S[i]) <= fabs(S[0]) * 1e-5)) ++rank;
  if (rank == 2) Sd[2] = (det3_shared(U) * det3_shared(V) > 0) ? 1.0 : -1.0;
  float Ti[16];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double a = 0;
      for (int k = 0; k < 3; ++k) a += U[r * 3 + k] * Sd[k] * V[c * 3 + k];
      Ti[c * 4 + r] = (float)a;
    }
  for (int r = 0; r < 3; ++r) {
    // t = dst_mean - R * src_mean (with the float R, like Eigen's float instantiation)
    const double a = mq[r] - ((double)Ti[0 * 4 + r] * mp[0] + (double)Ti[1 * 4 + r] * mp[1] + (double)Ti[2 * 4 + r] * mp[2]);
    Ti[12 + r] = (float)a;
  }
  Ti[3] = Ti[7] = Ti[11] = 0.0f;
  Ti[15] = 1.0f;
  // final = Tinc * final
  float Tn[16];
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) {
      float a = 0.0f;
      for (int k = 0; k < 4; ++k) a += Ti[k * 4 + r] * st->T[c * 4 + k];
      Tn[c * 4 + r] = a;
    }
  for (int i = 0; i < 16; ++i) { st->T[i] = Tn[i]; st->Tinc[i] = Ti[i]; }
  const int iters = ++st->iters;
  // DefaultConvergenceCriteria::hasConverged
  if (iters >= st->max_iter) { st->converged = 1; st->done = 1; return; }
  const double cos_angle = 0.5 * ((double)Ti[0] + (double)Ti[5] + (double)Ti[10] - 1.0);
  const double translation_sqr = (double)Ti[12] * Ti[12] + (double)Ti[13] * Ti[13] + (double)Ti[14] * Ti[14];
  if (cos_angle >= st->rot_thresh && translation_sqr <= st->trans_thresh) { st->converged = 1; st->done = 1; return; }
  const double mse = tot[15] * inv;
  if (fabs(mse - st->prev_mse) < 1e-12) { st->converged = 1; st->done = 1; return; }
  st->prev_mse = mse;
}

__global__ void __launch_bounds__(256) k_score_finalize(const NnJob *__restrict__ jobs)
{
  __shared__ double red[4][2];
  const double *__restrict__ partials = jobs[blockIdx.x].partials;
  const int split = jobs[blockIdx.x].split, n_items = jobs[blockIdx.x].n_items;
  const int nblocks = (n_items + 3) >> 2;
  double *out = jobs[blockIdx.x].out;
  IcpState *st = jobs[blockIdx.x].st;
  if (st && (!st->done || st->scored)) return;
  double s = 0.0, n = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += blockDim.x) {
    s += nn_block_partial(partials, b, 15, split, n_items);
    n += nn_block_partial(partials, b, 16, split, n_items);
  }
  s = wave_sum(s); n = wave_sum(n);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[wave][0] = s; red[wave][1] = n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    out[1] = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    if (st) st->scored = 1;
  }
}

// the source runs in the cloud's Hilbert order, one compact work item (<= 64 points) per wave (grid.hip)
static const float4 *morton_source(Context *c, const mm3d_cloud *src, int &n)
{
  cloud_hilbert(c, src);
  n = (int)src->n_finite;
  return src->hil_pts.get();
}

static float nn_cell_for(double radius)
{
  float cell = (float)(radius * 0.25);
  if (!(cell > 1e-3f)) cell = 0.25f;
  return cell;
}

// What a search derives from its range: the largest squared distance that is still a correspondence, the radius the
// search has to prove (with the slack that covers its own rounding) and the radius the target's grid is built for.
struct NnRange { float max_d2, rmax; double radius; };
// ICP: max_corr_dist is a distance.  (double)d2 > max_dist_sqr rejects: accept d2 <= largest float not above max_dist_sqr
static NnRange nn_range_icp(double max_corr_dist)
{
  const double max_dist_sqr = max_corr_dist * max_corr_dist;
  float max_d2 = (float)max_dist_sqr;
  if ((double)max_d2 > max_dist_sqr) max_d2 = std::nextafterf(max_d2, -INFINITY);
  return {max_d2, (float)(max_corr_dist * 1.0001 + 1e-5), max_corr_dist};
}
// score: max_range_ is compared with the SQUARED distance (PCL quirk), so the search radius is sqrt(max_distance)
static NnRange nn_range_score(double max_distance)
{
  const double radius = std::sqrt(max_distance > 0 ? max_distance : 0.0);
  float max_d2 = (float)max_distance;
  if ((double)max_d2 > max_distance) max_d2 = std::nextafterf(max_d2, -INFINITY);
  return {max_d2, (float)(radius * 1.0001 + 1e-5), radius};
}
// rings of cells (around a query's own cell) beyond which the distance transform need not tell cells apart
static int nn_max_ring(float rmax, const Grid &g) { return (int)std::ceil(rmax / g.cell) + 1; }

// One work item per block (k_nn_wave's SPLIT 4) when the source has too few items to keep the chip busy with one
// wave each: 256 CUs x 4 SIMDs take 1024 waves before any two share a SIMD.  Measured on MI355X, pairs/s with
// the split off / on: 16 x 100 k points (1.3 k items) 1765 / 1823, 4 x 200 k (2.5 k items) 245 / 257,
// 64 x 50 k (0.6 k items) 4135 / 4925, 16 x 500 k (7.8 k items) 706 / 669.
static bool nn_split_items(int n_items) { return n_items <= 4096; }

// launches k_nn_wave<MODE> over `count` jobs (device array), picking the one-item-per-block variant for small sources
template <int MODE>
static void launch_nn(Context *c, const char *name, double bytes, const NnJob *jobs_dev, int count, unsigned grid_x, bool split, float max_d2,
                      float rmax)
{
  if (split)
    MM3D_LAUNCH(c, name, bytes, (k_nn_wave<MODE, 4>), dim3(grid_x, count), dim3(256), 0, jobs_dev, max_d2, rmax);
  else
    MM3D_LAUNCH(c, name, bytes, (k_nn_wave<MODE, 1>), dim3(grid_x, count), dim3(256), 0, jobs_dev, max_d2, rmax);
}

// ICP from a guess and, if wanted, transformScore of the result -- the tail of every pair estimate -- for a BATCH
// of pairs in lockstep: one launch per step serves every pair of the batch (blockIdx.y = the pair), and the batch
// shares ONE host synchronisation per chunk of iterations.  A guess may already live on the device (SAC-IA's
// winning hypothesis), the score kernel reads the transform straight out of the ICP state, and the states and
// scores come back in one copy.  The score is launched speculatively after each chunk of iterations; a pair's
// score is only kept once its ICP has finished (it nearly always has: the reference's epsilon is loose).
// plane: point-to-plane ICP (icp_plane.hip's icp_plane_step over NnPlaneJobs that carry each target's normals) instead of
// icp_corr_reduce + icp_finalize; everything else -- states, chunks, waits, the speculative point-to-point score -- is shared.
// ndt: NDT (ndt.hip's ndt_step over NdtJobs that carry each target's voxel table) in the ICP's place: no grid of the target is
// read by it, max_corr_dist is not read by it, and its partials are always per block of four work items.
// Correspondence rejection (mm3d_set_icp_rejection): when the jobs carry options (IcpScoreJob::reject, the same for the whole batch),
// the Point and Plane kinds take icp_reject.hip's icp_reject_step in the place of their search + reduction launch -- it leaves the
// same partials for the kept correspondences -- and then their own finalize kernel.  NDT does not read the setting.
// color: coloured ICP (mm3d_set_icp_color): point-to-plane's jobs, partials and finalize kernel, with icp_color.hip's
// icp_color_step over NnColorJobs (the target's gradient records, the source's reference points) as the search + reduction
// launch.  The jobs carry no rejection options (the setters exclude each other).
enum class IcpKind { Point, Plane, Ndt, Color };
static float bits_to_float(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
static void icp_batch(Context *c, IcpScoreJob *jobs, int n_jobs, bool run_icp, double max_corr_dist, int max_iterations, double eps,
                      bool want_score, double score_max_distance, IcpKind kind)
{
  const bool color = kind == IcpKind::Color, plane = kind == IcpKind::Plane || color, ndt = kind == IcpKind::Ndt;
  static_assert(offsetof(IcpState, T) == 0, "the score kernel reads T at the head of the state");
  c->last_icp_iterations = 0;
  c->last_icp_converged = 0;
  // the ICP's and the score's search parameters
  const NnRange icp_range = nn_range_icp(max_corr_dist), score_range = nn_range_score(score_max_distance);
  const double score_radius = score_range.radius;
  const float max_d2 = icp_range.max_d2, rmax = icp_range.rmax;
  const float s_max_d2 = score_range.max_d2, s_rmax = score_range.rmax;

  struct Live { int job; const float4 *sp; int ns, n_items; const Grid *tg, *sg; int max_ring, s_ring; };
  std::vector<Live> live;
  for (int j = 0; j < n_jobs; ++j) {
    IcpScoreJob &J = jobs[j];
    J.out.iterations = 0; J.out.converged = 0; J.out.n_corr = 0; J.out.score = DBL_MAX;
    int ns = 0;
    const float4 *sp = (J.src->n && J.tgt->n) ? morton_source(c, J.src, ns) : nullptr;
    const Grid *tg = (ns && run_icp && !ndt) ? &cloud_grid(c, J.tgt, nn_cell_for(max_corr_dist)) : nullptr;
    const bool ndt_icp = ns && run_icp && ndt;
    const Grid *sg = (ns && want_score) ? &cloud_grid(c, J.tgt, nn_cell_for(score_radius)) : nullptr;
    if (ns == 0 || (tg && tg->n == 0) || (sg && sg->n == 0) || (!tg && !sg && !ndt_icp)) {
      // nothing to search: Identity * guess, and the score of an empty search
      if (J.guess_dev) {
        float *hT = (float *)c->pin(256);
        MM3D_HIP(hipMemcpyAsync(hT, J.guess_dev, 64, hipMemcpyDeviceToHost, c->stream));
        c->sync();
        memcpy(J.out.T, hT, sizeof(J.out.T));
      } else {
        memcpy(J.out.T, J.guess_host, sizeof(J.out.T));
      }
      continue;
    }
    if (plane && tg && (!J.tgt_normals || J.tgt_normals->n != J.tgt->n))
      throw Error(MM3D_EINVAL, "point-to-plane ICP: the target's normals do not match its points");
    if (color && tg && !J.tgt_color) throw Error(MM3D_EINVAL, "coloured ICP: the target has no gradient records");
    if (ndt_icp && !J.tgt_ndt) throw Error(MM3D_EINVAL, "NDT: the target has no voxel table");
    Live L{j, sp, ns, J.src->n_wave_items, tg, sg, 0, 0};
    L.max_ring = tg ? nn_max_ring(rmax, *tg) : 0;
    if (tg) grid_ensure_dt(c, *tg, L.max_ring);
    L.s_ring = sg ? nn_max_ring(s_rmax, *sg) : 0;
    if (sg) grid_ensure_dt(c, *sg, L.s_ring);
    live.push_back(L);
  }
  const int B = (int)live.size();
  if (B == 0) return;
  const mm3d_icp_rejection_options *rej = (run_icp && !ndt && !color) ? jobs[live[0].job].reject : nullptr;
  const double color_lambda = jobs[live[0].job].color_lambda;

  // one work item per block while the whole batch has too few items to fill the chip with one wave each
  // (the finalize kernels add the partials up in one fixed order, so the choice never shows in a result)
  int total_items = 0;
  for (const Live &L : live) total_items += L.n_items;
  // (test hooks: mm3d_debug_icp_rejection_split, mm3d_debug_icp_color_split)
  const int forced_split = rej ? icp_reject_forced_split() : (color && run_icp) ? icp_color_forced_split() : 0;
  const bool split = forced_split ? forced_split == 4 : nn_split_items(total_items);
  size_t part_total = 0;
  unsigned grid_x = 0;
  double icp_bytes = 0.0, score_bytes = 0.0;
  std::vector<unsigned> nb(B);
  // (the ICP partials: kAcc per block, kPlaneAcc for point-to-plane; the score's stay kAcc)
  const int icp_acc = plane ? kPlaneAcc : ndt ? kNdtAcc : kAcc;
  size_t icp_part_total = 0;
  unsigned ndt_grid_x = 0;
  for (int b = 0; b < B; ++b) {
    nb[b] = split ? (unsigned)live[b].n_items : div_up(live[b].n_items, 4);
    part_total += (size_t)nb[b] * kAcc;
    const unsigned icp_nb = ndt ? div_up(live[b].n_items, 4) : nb[b];
    icp_part_total += (size_t)icp_nb * icp_acc;
    grid_x = std::max(grid_x, nb[b]);
    ndt_grid_x = std::max(ndt_grid_x, icp_nb);
    icp_bytes += live[b].ns * (color ? 60.0 : plane ? 28.0 : ndt ? 16.0 + 52.0 * jobs[live[b].job].ndt_neighbours : 12.0);   // (point-to-plane: + the winner's normal; coloured: + its record and the source's reference point; NDT: the point, and an index word and a record per voxel)
    score_bytes += live[b].ns * 12.0 + (live[b].sg ? live[b].sg->n * 12.0 : 0.0);
  }
  DevBuf<double> partials(c, icp_part_total), s_partials(c, want_score ? part_total : 1);
  DevBuf<double> out(c, (size_t)2 * B);
  // (rejection: the pairs' records live behind the states, so that one copy brings both back)
  const size_t rec_bytes = rej ? sizeof(RejRecord) * B : 0;
  DevBuf<IcpState> st(c, B + div_up(rec_bytes, sizeof(IcpState)));
  RejRecord *d_rec = (RejRecord *)(st.get() + B);
  size_t rej_src = 0, rej_tgt = 0;
  unsigned rej_max_src = 0;
  if (rej)
    for (const Live &L : live) {
      rej_src += (size_t)L.ns;
      rej_tgt += rej->one_to_one ? jobs[L.job].tgt->n : 0;
      rej_max_src = std::max(rej_max_src, (unsigned)L.ns);
    }
  DevBuf<NnRejectJob> d_rjobs(c, rej ? (size_t)B : 1);
  DevBuf<int2> rej_corr(c, rej ? rej_src : 1);
  DevBuf<unsigned long long> rej_owner(c, rej_tgt ? rej_tgt : 1);
  DevBuf<unsigned> rej_hist(c, rej ? (size_t)B * 1024 : 1);
  DevBuf<NnJob> d_jobs(c, (size_t)2 * B);                 // [0, B): ICP, [B, 2B): score
  DevBuf<NnPlaneJob> d_pjobs(c, plane ? (size_t)B : 1);   // point-to-plane: the ICP jobs with their normals
  DevBuf<NdtJob> d_njobs(c, ndt ? (size_t)B : 1);         // NDT: the ICP jobs with their voxel tables
  DevBuf<NnColorJob> d_cjobs(c, color ? (size_t)B : 1);   // coloured: the point-to-plane jobs with the records and the source's reference points

  // host images, in the pinned arena: states | ICP jobs | score jobs | scores back | point-to-plane jobs | NDT jobs | rejecting jobs | coloured jobs
  const size_t st_bytes = sizeof(IcpState) * B, job_bytes = sizeof(NnJob) * 2 * B, out_bytes = 16 * (size_t)B;
  const size_t pjob_bytes = plane ? sizeof(NnPlaneJob) * B : 0, njob_bytes = ndt ? sizeof(NdtJob) * B : 0;
  const size_t rjob_bytes = rej ? sizeof(NnRejectJob) * B : 0, st_rec_bytes = st_bytes + rec_bytes;
  const size_t cjob_bytes = color ? sizeof(NnColorJob) * B : 0;
  char *pinned = (char *)c->pin(st_rec_bytes + job_bytes + out_bytes + pjob_bytes + njob_bytes + rjob_bytes + cjob_bytes + 64);
  IcpState *hp = (IcpState *)pinned;
  RejRecord *hr = (RejRecord *)(pinned + st_bytes);
  NnJob *hj = (NnJob *)(pinned + ((st_rec_bytes + 15) & ~(size_t)15));
  double *ho = (double *)((char *)hj + job_bytes);
  NnPlaneJob *hpj = (NnPlaneJob *)((char *)ho + out_bytes);
  NdtJob *hnj = (NdtJob *)((char *)hpj + pjob_bytes);
  NnRejectJob *hrj = (NnRejectJob *)((char *)hnj + njob_bytes);
  NnColorJob *hcj = (NnColorJob *)((char *)hrj + rjob_bytes);
  size_t off = 0, icp_off = 0, rej_src_off = 0, rej_tgt_off = 0;
  for (int b = 0; b < B; ++b) {
    const Live &L = live[b];
    const IcpScoreJob &J = jobs[L.job];
    IcpState h;
    memset(&h, 0, sizeof(h));
    if (!J.guess_dev) memcpy(h.T, J.guess_host, sizeof(h.T));
    h.prev_mse = DBL_MAX;
    h.rot_thresh = 1.0 - eps;
    h.trans_thresh = eps;
    h.max_iter = max_iterations;
    h.done = run_icp ? 0 : 1;
    hp[b] = h;
    NnJob q;
    memset(&q, 0, sizeof(q));
    q.src = L.sp;
    q.items = (const int2 *)J.src->wave_items.get();
    q.n_items = L.n_items;
    q.nblocks = (int)nb[b];
    q.split = split ? 1 : 0;
    q.tgt_ref = (const float4 *)J.tgt->pts.get();
    q.st = st.get() + b;
    q.Tc = nullptr;
    q.out = out.get() + 2 * b;
    if (L.tg) { q.g = L.tg->view(); q.max_ring = L.max_ring; }
    q.partials = partials.get() + icp_off;
    hj[b] = q;
    if (plane) {
      hpj[b].nn = q;
      hpj[b].nrm = L.tg ? (const float4 *)J.tgt_normals->nrm.get() : nullptr;
    }
    if (color) {
      hcj[b].pl = hpj[b];
      hcj[b].rec = L.tg ? J.tgt_color : nullptr;
      hcj[b].src_ref = (const float4 *)J.src->pts.get();
    }
    if (rej) {
      NnRejectJob rj;
      memset(&rj, 0, sizeof(rj));
      rj.nn = q;
      rj.nrm = (plane && L.tg) ? (const float4 *)J.tgt_normals->nrm.get() : nullptr;
      rj.corr = rej_corr.get() + rej_src_off;
      rj.owner = rej->one_to_one ? rej_owner.get() + rej_tgt_off : nullptr;
      rj.hist = rej_hist.get() + (size_t)b * 1024;
      rj.rec = d_rec + b;
      rj.n_src = L.ns;
      hrj[b] = rj;
      memset(&hr[b], 0, sizeof(RejRecord));
      hr[b].cut = 1;
      rej_src_off += (size_t)L.ns;
      rej_tgt_off += rej->one_to_one ? J.tgt->n : 0;
    }
    if (ndt) {
      NdtJob nj;
      memset(&nj, 0, sizeof(nj));
      nj.nn = q;
      nj.nn.split = 0;
      nj.nn.nblocks = (int)div_up(L.n_items, 4);
      if (const NdtTable *t = run_icp ? J.tgt_ndt : nullptr) {
        nj.rec = (const float4 *)t->rec.get();
        nj.index = (const int *)t->index.get();
        nj.inv = t->inv;
        for (int a = 0; a < 3; ++a) { nj.mn[a] = t->mn[a]; nj.dims[a] = t->dims[a]; }
      }
      nj.neighbours = J.ndt_neighbours;
      nj.n_src = L.ns;
      hnj[b] = nj;
    }
    if (L.sg) { q.g = L.sg->view(); q.max_ring = L.s_ring; }
    q.partials = s_partials.get() + (want_score ? off : 0);
    hj[B + b] = q;
    off += (size_t)nb[b] * kAcc;
    icp_off += (size_t)(ndt ? div_up(L.n_items, 4) : nb[b]) * icp_acc;
  }
  MM3D_HIP(hipMemcpyAsync(st.get(), hp, st_rec_bytes, hipMemcpyHostToDevice, c->stream));
  MM3D_HIP(hipMemcpyAsync(d_jobs.get(), hj, job_bytes, hipMemcpyHostToDevice, c->stream));
  if (rej) {
    MM3D_HIP(hipMemcpyAsync(d_rjobs.get(), hrj, rjob_bytes, hipMemcpyHostToDevice, c->stream));
    // (a place of the Hilbert-ordered source that no work item covers holds "no match" for good)
    MM3D_HIP(hipMemsetAsync(rej_corr.get(), 0xff, rej_src * sizeof(int2), c->stream));
  }
  if (plane) MM3D_HIP(hipMemcpyAsync(d_pjobs.get(), hpj, pjob_bytes, hipMemcpyHostToDevice, c->stream));
  if (ndt) MM3D_HIP(hipMemcpyAsync(d_njobs.get(), hnj, njob_bytes, hipMemcpyHostToDevice, c->stream));
  if (color) MM3D_HIP(hipMemcpyAsync(d_cjobs.get(), hcj, cjob_bytes, hipMemcpyHostToDevice, c->stream));
  for (int b = 0; b < B; ++b)
    if (jobs[live[b].job].guess_dev)
      MM3D_HIP(hipMemcpyAsync(st.get() + b, jobs[live[b].job].guess_dev, 64, hipMemcpyDeviceToDevice, c->stream));
  // iterations launched between two looks at the `done` flags: with the reference's loose epsilon 86 % of the pairs
  // converge in one iteration and 95 % in two.  A launch after `done` does nothing, but it is not free on a GPU
  // that runs sixteen streams: its blocks still queue for 20 KB of LDS and 128 registers behind the other streams'
  // kernels before they can find that out.  So the first look comes after ONE iteration (a batch of one or two
  // pairs is then usually finished), later ones after two.
  static const int first_chunk_knob = [] { const char *e = getenv("MM3D_ICP_FIRST_CHUNK"); return e ? atoi(e) : 0; }();   // A/B knob (1 or 2; 0: by batch size)
  const int min_chunk = first_chunk_knob > 0 ? std::min(first_chunk_knob, 2) : (B <= 2 ? 1 : 2);
  for (int round = 0;; ++round) {
    const int chunk = round == 0 ? min_chunk : 2;
    if (run_icp) {
      for (int k = 0; k < chunk; ++k) {
        if (rej) {
          icp_reject_step(c, d_rjobs.get(), B, grid_x, rej_max_src, split, plane, max_d2, rmax, *rej, rej_owner.get(),
                          rej_tgt * sizeof(unsigned long long), icp_bytes + rej_src * 8.0);
          if (plane) icp_plane_finalize(c, d_pjobs.get(), B, icp_part_total * 8.0);
          else MM3D_LAUNCH(c, "icp_finalize", part_total * 8.0, k_icp_finalize, dim3(B), dim3(256), 0, (const NnJob *)d_jobs.get());
          continue;
        }
        if (color) {
          icp_color_step(c, d_cjobs.get(), B, grid_x, split, max_d2, rmax, color_lambda, icp_bytes);
          icp_plane_finalize(c, d_pjobs.get(), B, icp_part_total * 8.0);
          continue;
        }
        if (plane) {
          icp_plane_step(c, d_pjobs.get(), B, grid_x, split, max_d2, rmax, icp_bytes, icp_part_total * 8.0);
          continue;
        }
        if (ndt) {
          ndt_step(c, d_njobs.get(), B, ndt_grid_x, icp_bytes, icp_part_total * 8.0);
          continue;
        }
        launch_nn<0>(c, "icp_corr_reduce", icp_bytes, d_jobs.get(), B, grid_x, split, max_d2, rmax);
        MM3D_LAUNCH(c, "icp_finalize", part_total * 8.0, k_icp_finalize, dim3(B), dim3(256), 0, (const NnJob *)d_jobs.get());
      }
    }
    if (want_score) {
      launch_nn<1>(c, "score_nn_reduce", score_bytes, d_jobs.get() + B, B, grid_x, split, s_max_d2, s_rmax);
      MM3D_LAUNCH(c, "score_finalize", 0, k_score_finalize, dim3(B), dim3(256), 0, (const NnJob *)(d_jobs.get() + B));
      MM3D_HIP(hipMemcpyAsync(ho, out.get(), out_bytes, hipMemcpyDeviceToHost, c->stream));
    }
    MM3D_HIP(hipMemcpyAsync(hp, st.get(), st_rec_bytes, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    bool all_done = true;
    for (int b = 0; b < B; ++b) {
      IcpScoreJob &J = jobs[live[b].job];
      if (hp[b].done && !J.closed) {
        // first chunk after which this pair is finished: its state and score are final
        memcpy(J.out.T, hp[b].T, sizeof(J.out.T));
        J.out.iterations = hp[b].iters;
        J.out.converged = hp[b].converged;
        J.out.n_corr = hp[b].n_corr;
        if (want_score) J.out.score = ho[2 * b + 1] > 0.0 ? ho[2 * b] / ho[2 * b + 1] : DBL_MAX;
        if (rej) {
          const RejRecord &r = hr[b];
          J.reject_stats.matched = r.matched;
          J.reject_stats.after_one_to_one = rej->one_to_one ? r.survivors : r.matched;
          J.reject_stats.kept = r.kept;
          J.reject_stats.threshold_d2 = r.cut == 0 ? bits_to_float(r.tau_bits) : r.cut == 1 ? INFINITY : -1.0f;
          J.reject_stats.iterations = hp[b].iters;
          J.reject_stats.converged = hp[b].converged;
        }
        J.closed = true;
      }
      if (!hp[b].done) all_done = false;
    }
    if (all_done) break;
  }
  const IcpScoreJob &last = jobs[live[B - 1].job];
  c->last_icp_iterations = last.out.iterations;
  c->last_icp_converged = last.out.converged;
}

void icp_score_batch(Context *c, IcpScoreJob *jobs, int n_jobs, bool run_icp, double max_corr_dist, int max_iterations, double eps,
                     bool want_score, double score_max_distance)
{
  icp_batch(c, jobs, n_jobs, run_icp, max_corr_dist, max_iterations, eps, want_score, score_max_distance, IcpKind::Point);
}

void icp_plane_score_batch(Context *c, IcpScoreJob *jobs, int n_jobs, bool run_icp, double max_corr_dist, int max_iterations, double eps,
                           bool want_score, double score_max_distance)
{
  icp_batch(c, jobs, n_jobs, run_icp, max_corr_dist, max_iterations, eps, want_score, score_max_distance, IcpKind::Plane);
}

void icp_color_score_batch(Context *c, IcpScoreJob *jobs, int n_jobs, bool run_icp, double max_corr_dist, int max_iterations, double eps,
                           bool want_score, double score_max_distance)
{
  icp_batch(c, jobs, n_jobs, run_icp, max_corr_dist, max_iterations, eps, want_score, score_max_distance, IcpKind::Color);
}

void ndt_score_batch(Context *c, IcpScoreJob *jobs, int n_jobs, bool run_icp, double max_corr_dist, int max_iterations, double eps,
                     bool want_score, double score_max_distance)
{
  icp_batch(c, jobs, n_jobs, run_icp, max_corr_dist, max_iterations, eps, want_score, score_max_distance, IcpKind::Ndt);
}

PairTail icp_score(Context *c, const mm3d_cloud *src, const mm3d_cloud *tgt, const float *guess_dev, const float guess_host[16],
                   bool run_icp, double max_corr_dist, int max_iterations, double eps, bool want_score, double score_max_distance)
{
  IcpScoreJob J;
  J.src = src; J.tgt = tgt; J.guess_dev = guess_dev;
  if (guess_host) memcpy(J.guess_host, guess_host, sizeof(J.guess_host));
  icp_score_batch(c, &J, 1, run_icp, max_corr_dist, max_iterations, eps, want_score, score_max_distance);
  return J.out;
}

IcpResult icp(Context *c, const mm3d_cloud *src, const mm3d_cloud *tgt, const float guess[16],
              double max_corr_dist, int max_iterations, double eps)
{
  const PairTail t = icp_score(c, src, tgt, nullptr, guess, true, max_corr_dist, max_iterations, eps, false, 0.0);
  IcpResult res;
  memcpy(res.T, t.T, sizeof(res.T));
  res.iterations = t.iterations;
  res.converged = t.converged;
  return res;
}

double transform_score(Context *c, const mm3d_cloud *src, const mm3d_cloud *tgt, const float T[16], double max_distance)
{
  if (src->n == 0 || tgt->n == 0) return DBL_MAX;
  const NnRange range = nn_range_score(max_distance);
  const Grid &tg = cloud_grid(c, tgt, nn_cell_for(range.radius));
  int ns = 0;
  const float4 *sp = morton_source(c, src, ns);
  if (ns == 0 || tg.n == 0) return DBL_MAX;
  const float max_d2 = range.max_d2, rmax = range.rmax;
  const int max_ring = nn_max_ring(rmax, tg);
  grid_ensure_dt(c, tg, max_ring);
  const int n_items = src->n_wave_items;
  const bool split = nn_split_items(n_items);
  const unsigned nblocks = split ? (unsigned)n_items : div_up(n_items, 4);
  DevBuf<double> partials(c, (size_t)nblocks * kAcc);
  DevBuf<float> dT(c, 16);
  DevBuf<double> out(c, 2);
  DevBuf<NnJob> d_job(c, 1);
  char *pinned = (char *)c->pin(512 + sizeof(NnJob));
  float *hT = (float *)pinned;
  double *ho = (double *)(pinned + 128);
  NnJob *hj = (NnJob *)(pinned + 256);
  memcpy(hT, T, 64);
  NnJob q;
  memset(&q, 0, sizeof(q));
  q.src = sp;
  q.items = (const int2 *)src->wave_items.get();
  q.n_items = n_items;
  q.nblocks = (int)nblocks;
  q.split = split ? 1 : 0;
  q.g = tg.view();
  q.tgt_ref = (const float4 *)tgt->pts.get();
  q.Tc = dT.get();
  q.partials = partials.get();
  q.out = out.get();
  q.max_ring = max_ring;
  *hj = q;
  MM3D_HIP(hipMemcpyAsync(dT.get(), hT, 64, hipMemcpyHostToDevice, c->stream));
  MM3D_HIP(hipMemcpyAsync(d_job.get(), hj, sizeof(NnJob), hipMemcpyHostToDevice, c->stream));
  launch_nn<1>(c, "score_nn_reduce", ns * 12.0 + tg.n * 12.0, d_job.get(), 1, nblocks, split, max_d2, rmax);
  MM3D_LAUNCH(c, "score_finalize", 0, k_score_finalize, dim3(1), dim3(256), 0, (const NnJob *)d_job.get());
  MM3D_HIP(hipMemcpyAsync(ho, out.get(), 16, hipMemcpyDeviceToHost, c->stream));
  c->sync();
  return ho[1] > 0.0 ? ho[0] / ho[1] : DBL_MAX;
}

// mm3d_debug_nn_search: range, cell, ring and distance transform as icp_batch (convention 0) or transform_score (1) derive
// them, the source in its Hilbert order and work items as every search takes it, one launch of k_nn_probe with the split forced
static void debug_nn_search(Context *c, const mm3d_cloud *src, const mm3d_cloud *tgt, const float T[16], double range, int convention,
                            int split, int *idx, float *d2, mm3d_nn_search_info *info)
{
  const NnRange r = convention == 0 ? nn_range_icp(range) : nn_range_score(range);
  mm3d_nn_search_info I;
  memset(&I, 0, sizeof(I));
  I.max_d2 = r.max_d2;
  I.rmax = r.rmax;
  std::vector<int> h_idx(src->n, -1);
  std::vector<float> h_d2(src->n, INFINITY);
  int ns = 0;
  const float4 *sp = (src->n && tgt->n) ? morton_source(c, src, ns) : nullptr;
  const Grid *tg = ns ? &cloud_grid(c, tgt, nn_cell_for(r.radius)) : nullptr;
  if (tg && tg->n) {
    const int max_ring = nn_max_ring(r.rmax, *tg);
    grid_ensure_dt(c, *tg, max_ring);
    const int n_items = src->n_wave_items;
    const unsigned nblocks = split == 4 ? (unsigned)n_items : div_up(n_items, 4);
    I.cell = tg->cell;
    I.max_ring = max_ring;
    for (int a = 0; a < 3; ++a) { I.dims[a] = tg->dims[a]; I.origin[a] = tg->mn[a]; }
    I.n_items = n_items;
    DevBuf<int> d_idx(c, src->n);
    DevBuf<float> d_d2(c, src->n), dT(c, 16);
    DevBuf<NnJob> d_job(c, 1);
    char *pinned = (char *)c->pin(256 + sizeof(NnJob));
    float *hT = (float *)pinned;
    NnJob *hj = (NnJob *)(pinned + 256);
    memcpy(hT, T, 64);
    NnJob q;
    memset(&q, 0, sizeof(q));
    q.src = sp;
    q.items = (const int2 *)src->wave_items.get();
    q.n_items = n_items;
    q.nblocks = (int)nblocks;
    q.split = split == 4 ? 1 : 0;
    q.g = tg->view();
    q.tgt_ref = (const float4 *)tgt->pts.get();
    q.Tc = dT.get();
    q.max_ring = max_ring;
    *hj = q;
    // (non-finite source points are in no work item: they keep -1 / +inf)
    MM3D_HIP(hipMemcpyAsync(d_idx.get(), h_idx.data(), src->n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    MM3D_HIP(hipMemcpyAsync(d_d2.get(), h_d2.data(), src->n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    MM3D_HIP(hipMemcpyAsync(dT.get(), hT, 64, hipMemcpyHostToDevice, c->stream));
    MM3D_HIP(hipMemcpyAsync(d_job.get(), hj, sizeof(NnJob), hipMemcpyHostToDevice, c->stream));
    if (split == 4)
      MM3D_LAUNCH(c, "debug_nn_search", ns * 24.0, (k_nn_probe<4>), dim3(nblocks), dim3(256), 0, (const NnJob *)d_job.get(), r.max_d2, r.rmax,
                  d_idx.get(), d_d2.get());
    else
      MM3D_LAUNCH(c, "debug_nn_search", ns * 24.0, (k_nn_probe<1>), dim3(nblocks), dim3(256), 0, (const NnJob *)d_job.get(), r.max_d2, r.rmax,
                  d_idx.get(), d_d2.get());
    MM3D_HIP(hipMemcpyAsync(h_idx.data(), d_idx.get(), src->n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MM3D_HIP(hipMemcpyAsync(h_d2.data(), d_d2.get(), src->n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    c->sync();
  }
  if (src->n) {
    memcpy(idx, h_idx.data(), src->n * sizeof(int));
    memcpy(d2, h_d2.data(), src->n * sizeof(float));
  }
  if (info) *info = I;
}

// mm3d_debug_icp_rejection: range, cell, ring, distance transform, source order and work items as icp_batch derives them, one
// iteration's correspondence stage (icp_reject.hip) at T with the split forced, and every source point's decision
static void debug_icp_rejection(Context *c, const mm3d_cloud *src, const mm3d_cloud *tgt, const float T[16], double max_corr_dist,
                                const mm3d_icp_rejection_options &opt, int split, int *idx, float *d2, unsigned char *kept,
                                mm3d_icp_rejection_stats *stats)
{
  const NnRange r = nn_range_icp(max_corr_dist);
  mm3d_icp_rejection_stats S{0, 0, 0, INFINITY, 0, 0};
  std::vector<int> h_idx(src->n, -1);
  std::vector<float> h_d2(src->n, INFINITY);
  std::vector<unsigned char> h_kept(src->n, 0);
  int ns = 0;
  const float4 *sp = (src->n && tgt->n) ? morton_source(c, src, ns) : nullptr;
  const Grid *tg = ns ? &cloud_grid(c, tgt, nn_cell_for(r.radius)) : nullptr;
  if (tg && tg->n) {
    const int max_ring = nn_max_ring(r.rmax, *tg);
    grid_ensure_dt(c, *tg, max_ring);
    const int n_items = src->n_wave_items;
    const unsigned nblocks = split == 4 ? (unsigned)n_items : div_up(n_items, 4);
    DevBuf<int> d_idx(c, src->n);
    DevBuf<float> d_d2(c, src->n);
    DevBuf<unsigned char> d_kept(c, src->n);
    DevBuf<IcpState> st(c, 2);                       // the state, and the record behind it
    RejRecord *d_rec = (RejRecord *)(st.get() + 1);
    DevBuf<NnRejectJob> d_job(c, 1);
    DevBuf<int2> corr(c, (size_t)ns);
    DevBuf<unsigned long long> owner(c, opt.one_to_one ? tgt->n : 1);
    DevBuf<unsigned> hist(c, 1024);
    char *pinned = (char *)c->pin(2 * sizeof(IcpState) + sizeof(NnRejectJob) + 64);
    IcpState *hs = (IcpState *)pinned;
    RejRecord *hr = (RejRecord *)(hs + 1);
    NnRejectJob *hj = (NnRejectJob *)(pinned + 2 * sizeof(IcpState));
    memset(hs, 0, 2 * sizeof(IcpState));
    memcpy(hs->T, T, 64);
    hr->cut = 1;
    NnRejectJob q;
    memset(&q, 0, sizeof(q));
    q.nn.src = sp;
    q.nn.items = (const int2 *)src->wave_items.get();
    q.nn.n_items = n_items;
    q.nn.nblocks = (int)nblocks;
    q.nn.split = split == 4 ? 1 : 0;
    q.nn.g = tg->view();
    q.nn.tgt_ref = (const float4 *)tgt->pts.get();
    q.nn.st = st.get();
    q.nn.max_ring = max_ring;
    q.corr = corr.get();
    q.owner = opt.one_to_one ? owner.get() : nullptr;
    q.hist = hist.get();
    q.rec = d_rec;
    q.n_src = ns;
    *hj = q;
    // (non-finite source points are in no work item: they keep -1 / +inf / 0)
    MM3D_HIP(hipMemcpyAsync(d_idx.get(), h_idx.data(), src->n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    MM3D_HIP(hipMemcpyAsync(d_d2.get(), h_d2.data(), src->n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    MM3D_HIP(hipMemsetAsync(d_kept.get(), 0, src->n, c->stream));
    MM3D_HIP(hipMemsetAsync(corr.get(), 0xff, (size_t)ns * sizeof(int2), c->stream));
    MM3D_HIP(hipMemcpyAsync(st.get(), hs, 2 * sizeof(IcpState), hipMemcpyHostToDevice, c->stream));
    MM3D_HIP(hipMemcpyAsync(d_job.get(), hj, sizeof(NnRejectJob), hipMemcpyHostToDevice, c->stream));
    icp_reject_debug(c, d_job.get(), nblocks, (unsigned)ns, n_items, split == 4, r.max_d2, r.rmax, opt, owner.get(),
                     opt.one_to_one ? tgt->n * sizeof(unsigned long long) : 0, d_idx.get(), d_d2.get(), d_kept.get());
    MM3D_HIP(hipMemcpyAsync(h_idx.data(), d_idx.get(), src->n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MM3D_HIP(hipMemcpyAsync(h_d2.data(), d_d2.get(), src->n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    MM3D_HIP(hipMemcpyAsync(h_kept.data(), d_kept.get(), src->n, hipMemcpyDeviceToHost, c->stream));
    MM3D_HIP(hipMemcpyAsync(hs, st.get(), 2 * sizeof(IcpState), hipMemcpyDeviceToHost, c->stream));
    c->sync();
    S.matched = hr->matched;
    S.after_one_to_one = opt.one_to_one ? hr->survivors : hr->matched;
    S.kept = hr->kept;
    S.threshold_d2 = hr->cut == 0 ? bits_to_float(hr->tau_bits) : hr->cut == 1 ? INFINITY : -1.0f;
  }
  if (src->n) {
    memcpy(idx, h_idx.data(), src->n * sizeof(int));
    memcpy(d2, h_d2.data(), src->n * sizeof(float));
    memcpy(kept, h_kept.data(), src->n);
  }
  if (stats) *stats = S;
}

#ifdef MM3D_NN_STATS
extern "C" void mm3d_debug_nn_stats(unsigned long long *out, int reset)
{
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_nn_stats), sizeof(unsigned long long) * 64);
  if (reset) { unsigned long long z[64] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_nn_stats), z, sizeof(z)); }
}
#endif

// Everything icp_score() would build lazily on its first use of these clouds: afterwards pair
// estimates only READ the clouds' caches, so one map can serve pairs on several contexts at once.
void prepare_pair_search(Context *c, const mm3d_cloud *points, double max_corr_dist, double score_max_distance)
{
  if (points->n == 0) return;
  int ns = 0;
  (void)morton_source(c, points, ns);
  const NnRange ranges[2] = {nn_range_icp(max_corr_dist), nn_range_score(score_max_distance)};
  for (const NnRange &range : ranges) {
    const Grid &g = cloud_grid(c, points, nn_cell_for(range.radius));
    if (g.n == 0) continue;
    grid_ensure_dt(c, g, nn_max_ring(range.rmax, g));
  }
}

}  // namespace mm3d

// the C entry point of the search probe (include/mm3d.h) lives with its kernel, like fpfh.hip's mm3d_debug_pair_bins: the
// host-only builds of the library link capi.cpp without this file
extern "C" int mm3d_debug_nn_search(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target, const float T[16], double range,
                                    int convention, int split, int *idx, float *d2, mm3d_nn_search_info *info)
{
  if (!source || !target || !T || (convention != 0 && convention != 1) || (split != 1 && split != 4)) return MM3D_EINVAL;
  if (!(range >= 0.0) || !std::isfinite(range)) return MM3D_EINVAL;
  if (source->n && (!idx || !d2)) return MM3D_EINVAL;
  return mm3d::guarded(ctx, [&] { mm3d::debug_nn_search(ctx, source, target, T, range, convention, split, idx, d2, info); });
}

extern "C" int mm3d_debug_icp_rejection(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target, const float T[16],
                                        double max_correspondence_distance, const mm3d_icp_rejection_options *options, int split, int *idx,
                                        float *d2, unsigned char *kept, mm3d_icp_rejection_stats *stats)
{
  if (!source || !target || !T || !options || !mm3d::icp_rejection_options_valid(options) || (split != 1 && split != 4)) return MM3D_EINVAL;
  if (!(max_correspondence_distance >= 0.0) || !std::isfinite(max_correspondence_distance)) return MM3D_EINVAL;
  if (source->n && (!idx || !d2 || !kept)) return MM3D_EINVAL;
  return mm3d::guarded(ctx, [&] {
    mm3d::debug_icp_rejection(ctx, source, target, T, max_correspondence_distance, *options, split, idx, d2, kept, stats);
  });
}

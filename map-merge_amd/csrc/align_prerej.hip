// align_prerej.hip -- prerejective RANSAC initial alignment, the opt-in alternative to the reference's SAC-IA
// (mm3d_set_alignment; include/mm3d.h states the algorithm).
//
// The algorithm of pcl::SampleConsensusPrerejective (Buch et al., "Pose estimation using local structure-specific shape and
// appearance context", ICRA 2013): 3-sample draws among the k nearest descriptors, rejected from their three edge-length
// ratios before a transform is fitted; the survivors are ranked by their inliers.  SAC-IA's hypotheses come from the host's
// rand() replay, one after the other; these come from a counter-based generator, one lane each, so millions are drawn, most
// thrown away for a few dozen flops, and only the survivors scored.
//
//   k_prerej_draw<false>  one lane per draw: the six words, six 16-byte keypoint gathers, three ratio tests; a block's survivor count
//   (exclusive_scan_int)  where each block's survivors start
//   k_prerej_draw<true>   the same draws again, the survivors written behind their block's start in lane order (a wave ballot
//                         gives the rank): the list ascends in h by construction, no atomic arrival order anywhere
//   k_prerej_model        one lane per survivor: Umeyama on its three pairs in double (linalg_shared.hpp), 16 floats
//   k_prerej_score        one block per hypothesis over the source keypoints in their Hilbert order: the float transform, the
//                         exact nearest target keypoint (the merged neighbourhood lists of the target's grid, as SAC-IA's
//                         error kernel reads them), the inlier count and the inliers' d2 sum in double
//   k_prerej_pick         one block: the winner
//   k_prerej_refit        one block: Umeyama in double over the winner's inlier pairs
//   k_prerej_score        the refit, as a hypothesis of its own
//   k_prerej_final        the refit or the winner; the transform and the statistics
//
// Every sum has one order: lane t of a block takes the keypoints t, t + 256, ... in turn, the 64 lanes of a wave are added by
// wave_sum's shuffles, the four waves as (w0 + w1) + (w2 + w3).  Nothing depends on what else is in flight.
#include <cmath>
#include <cstring>

#include "capi_guard.hpp"
#include "drivers.hpp"
#include "device_util.hpp"
#include "linalg_shared.hpp"

namespace mm3d {

// ---------------------------------------------------------------- the draws
// splitmix64's finaliser on ((seed << 32) | h) + (j + 1) * golden gamma: word j of draw h (include/mm3d.h)
__device__ __forceinline__ uint64_t prerej_word(uint64_t base, int j)
{
  uint64_t z = base + (uint64_t)(j + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ int prerej_bounded(uint64_t w, int n) { return (int)(((w >> 32) * (uint64_t)(uint32_t)n) >> 32); }

// squared edge length ((dx dx + dy dy) + dz dz) in double: exact differences of floats, no contraction
__device__ __forceinline__ double prerej_edge2(const float4 a, const float4 b)
{
  const double dx = (double)a.x - (double)b.x, dy = (double)a.y - (double)b.y, dz = (double)a.z - (double)b.z;
  return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}
__device__ __forceinline__ bool prerej_edge_ok(double ds, double dt, double sim2)
{
  const double lo = ds < dt ? ds : dt, hi = ds < dt ? dt : ds;
  return ds > 0.0 && dt > 0.0 && lo >= __dmul_rn(sim2, hi);      // (anything not a number compares false)
}

struct PrerejDraw {
  const float4 *skp, *tkp;     // keypoints in reference order
  const int *nn;               // [ns][kk]: the nearest target descriptors of every source keypoint
  int ns, nt, kk, samples;
  unsigned seed;
  double sim2;
  int *block_count;            // [blocks + 1]: survivors per block, then their exclusive scan
  int4 *surv;                  // [M][2]: (h, i0, i1, i2), (t0, t1, t2, 0)
};

template <bool WRITE>
__global__ void __launch_bounds__(256) k_prerej_draw(PrerejDraw J, const int *__restrict__ block_start)
{
  const unsigned h = blockIdx.x * 256u + threadIdx.x;
  bool ok = h < (unsigned)J.samples;
  int i0 = 0, i1 = 0, i2 = 0, t0 = 0, t1 = 0, t2 = 0;
  if (ok) {
    const uint64_t base = ((uint64_t)J.seed << 32) | (uint64_t)h;
    i0 = prerej_bounded(prerej_word(base, 0), J.ns);
    i1 = prerej_bounded(prerej_word(base, 1), J.ns - 1);
    i1 += i1 >= i0 ? 1 : 0;
    i2 = prerej_bounded(prerej_word(base, 2), J.ns - 2);
    const int lo = min(i0, i1), hi = max(i0, i1);
    i2 += i2 >= lo ? 1 : 0;
    i2 += i2 >= hi ? 1 : 0;
    t0 = J.nn[(size_t)i0 * J.kk + prerej_bounded(prerej_word(base, 3), J.kk)];
    t1 = J.nn[(size_t)i1 * J.kk + prerej_bounded(prerej_word(base, 4), J.kk)];
    t2 = J.nn[(size_t)i2 * J.kk + prerej_bounded(prerej_word(base, 5), J.kk)];
    // (a row of the table is padded with -1 where the search found nothing comparable: descriptors that are not numbers)
    ok = t0 >= 0 && t1 >= 0 && t2 >= 0 && t0 < J.nt && t1 < J.nt && t2 < J.nt && t0 != t1 && t0 != t2 && t1 != t2;
  }
  if (ok) {
    const float4 a0 = J.skp[i0], a1 = J.skp[i1], a2 = J.skp[i2];
    const float4 b0 = J.tkp[t0], b1 = J.tkp[t1], b2 = J.tkp[t2];
    ok = prerej_edge_ok(prerej_edge2(a0, a1), prerej_edge2(b0, b1), J.sim2) &&
         prerej_edge_ok(prerej_edge2(a1, a2), prerej_edge2(b1, b2), J.sim2) &&
         prerej_edge_ok(prerej_edge2(a2, a0), prerej_edge2(b2, b0), J.sim2);
  }
  const unsigned long long mask = ballot(ok);
  __shared__ int s_wave[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_wave[wave] = __popcll(mask);
  __syncthreads();
  if (!WRITE) {
    if (threadIdx.x == 0) J.block_count[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
    return;
  }
  if (!ok) return;
  int pos = block_start[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) pos += s_wave[w];
  J.surv[(size_t)pos * 2] = make_int4((int)h, i0, i1, i2);
  J.surv[(size_t)pos * 2 + 1] = make_int4(t0, t1, t2, 0);
}

// ---------------------------------------------------------------- the hypotheses
// Umeyama without scale over n pairs given their sums: the means, sigma = E[d s^T] - E[d] E[s]^T (double), the SVD core of
// linalg_shared.hpp; T column-major 4x4 in float.  sum_s / sum_d: 3 each; sum_ds[r * 3 + c] = sum of d_r s_c.
__device__ inline void prerej_umeyama(const double *sum_s, const double *sum_d, const double *sum_ds, double n, float *T)
{
  const double inv = 1.0 / n;
  double sm[3], dm[3], sigma[9], R[9], t[3];
  for (int a = 0; a < 3; ++a) { sm[a] = sum_s[a] * inv; dm[a] = sum_d[a] * inv; }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) sigma[r * 3 + c] = sum_ds[r * 3 + c] * inv - dm[r] * sm[c];
  umeyama_core_shared(sigma, sm, dm, 1e-12, R, t);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[c * 4 + r] = (float)R[r * 3 + c];
    T[12 + r] = (float)t[r];
  }
  T[3] = T[7] = T[11] = 0.0f;
  T[15] = 1.0f;
}

__global__ void __launch_bounds__(64)
k_prerej_model(const float4 *__restrict__ skp, const float4 *__restrict__ tkp, const int4 *__restrict__ surv, int M,
               float *__restrict__ T_all)
{
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const int4 a = surv[(size_t)m * 2], b = surv[(size_t)m * 2 + 1];
  const int si[3] = {a.y, a.z, a.w}, ti[3] = {b.x, b.y, b.z};
  // the three pairs about the first source / target point: the sums stay small next to the coordinates
  const float4 s0 = skp[si[0]], d0 = tkp[ti[0]];
  double sum_s[3] = {0, 0, 0}, sum_d[3] = {0, 0, 0}, sum_ds[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 1; i < 3; ++i) {
    const float4 p = skp[si[i]], q = tkp[ti[i]];
    const double s[3] = {(double)p.x - (double)s0.x, (double)p.y - (double)s0.y, (double)p.z - (double)s0.z};
    const double d[3] = {(double)q.x - (double)d0.x, (double)q.y - (double)d0.y, (double)q.z - (double)d0.z};
    for (int r = 0; r < 3; ++r) {
      sum_s[r] += s[r]; sum_d[r] += d[r];
      for (int c = 0; c < 3; ++c) sum_ds[r * 3 + c] += d[r] * s[c];
    }
  }
  float T[16];
  prerej_umeyama(sum_s, sum_d, sum_ds, 3.0, T);
  // back from the shifted frames: x -> R (x - s0) + t' + d0
  const double o[3] = {(double)s0.x, (double)s0.y, (double)s0.z}, e[3] = {(double)d0.x, (double)d0.y, (double)d0.z};
  for (int r = 0; r < 3; ++r)
    T[12 + r] = (float)((double)T[12 + r] + e[r] - ((double)T[r] * o[0] + (double)T[4 + r] * o[1] + (double)T[8 + r] * o[2]));
#pragma unroll
  for (int i = 0; i < 16; ++i) T_all[(size_t)m * 16 + i] = T[i];
}

// ---------------------------------------------------------------- scoring
// The exact float nearest target keypoint of p within `radius`: d2 and the point, INFINITY when there is none.  The scan of
// SAC-IA's error term (registration.hip's sacia_term): ONE contiguous span of the query's cell, the merged list of the 3x3x3
// block around it in ascending distance from the cell centre, left at the first entry that can no longer be nearer than
// what is still worth finding.  The minimum is over exact float distances (first minimum in list order: the list is a
// function of the target alone), so the order of the scan does not show in d2.
__device__ __forceinline__ float prerej_nearest(const GridView &g, const float3 p, float thr2, float radius, float4 &hit)
{
  float best = INFINITY;
  hit = make_float4(0.f, 0.f, 0.f, 0.f);
  const int cx = cell_floor(p.x, g.minx, g.inv), cy = cell_floor(p.y, g.miny, g.inv), cz = cell_floor(p.z, g.minz, g.inv);
  const bool inside = cx >= 0 && cx < g.dx && cy >= 0 && cy < g.dy && cz >= 0 && cz < g.dz;
  if (inside) {
    const size_t c = ((size_t)cz * g.dy + cy) * g.dx + cx;
    const int b = g.nb_start[c], e = g.nb_start[c + 1];
    const float ox = p.x - (g.minx + ((float)cx + 0.5f) * g.cell), oy = p.y - (g.miny + ((float)cy + 0.5f) * g.cell);
    const float oz = p.z - (g.minz + ((float)cz + 0.5f) * g.cell);
    const float slack = sqrtf(ox * ox + oy * oy + oz * oz) + 1e-3f * g.cell;
    float want = thr2;
    for (int j = b; j < e; ++j) {
      const float4 q = g.nb_pts[j];
      const float d = dist2(p.x, p.y, p.z, q.x, q.y, q.z);
      if (d < best) { best = d; hit = q; }
      want = fminf(want, best);
      const float lb = q.w - slack;
      if (lb > 0.0f && lb * lb > want) break;
    }
  } else {
    for_each_candidate(g, p.x, p.y, p.z, radius, [&](const float4 &q) {
      const float d = dist2(p.x, p.y, p.z, q.x, q.y, q.z);
      if (d < best) { best = d; hit = q; }
      return true;
    });
  }
  return best;
}

__device__ __forceinline__ double prerej_block_sum(double v, double *s4)
{
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

// one block per hypothesis: count[m] inliers, sum[m] their d2 in double
__global__ void __launch_bounds__(256)
k_prerej_score(const float4 *__restrict__ skp_q, int ns, GridView g, const float *__restrict__ T_all, float thr2, float radius,
               int *__restrict__ count, double *__restrict__ sum)
{
  const size_t m = blockIdx.x;
  float Tl[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) Tl[k] = T_all[m * 16 + k];
  int cnt = 0;
  double acc = 0.0;
  for (int i = threadIdx.x; i < ns; i += 256) {
    const float4 s = skp_q[i];
    float4 hit;
    const float d = prerej_nearest(g, xform(Tl, s.x, s.y, s.z), thr2, radius, hit);
    if (d <= thr2) { ++cnt; acc += (double)d; }
  }
  __shared__ double s4[4];
  const double tot = prerej_block_sum(acc, s4);
  const double n = prerej_block_sum((double)cnt, s4);       // (integers below 2^53: exact)
  if (threadIdx.x == 0) { count[m] = (int)n; sum[m] = tot; }
}

// ---------------------------------------------------------------- the pick
struct PrerejCtl {
  int winner;          // row of the survivor list, -1: none
  int converged;
  int count;
  int refit_kept;
  double sum;
  long long winner_h;
};

// a is better than b: (converged) the lower mean inlier d2, (not) the higher count; ties to the lower row = the lower h
__device__ __forceinline__ bool prerej_better_mean(double ea, int ma, double eb, int mb)
{
  return mb < 0 || (ma >= 0 && (ea < eb || (ea == eb && ma < mb)));
}
__device__ __forceinline__ bool prerej_better_count(int ca, int ma, int cb, int mb)
{
  return mb < 0 || (ma >= 0 && (ca > cb || (ca == cb && ma < mb)));
}

__global__ void __launch_bounds__(256)
k_prerej_pick(const int *__restrict__ count, const double *__restrict__ sum, const int4 *__restrict__ surv, int M, int ns,
              double inlier_fraction, PrerejCtl *__restrict__ ctl)
{
  const double need = inlier_fraction * (double)ns;
  int am = -1, bm = -1, bc = 0;
  double ae = 0.0;
  for (int m = threadIdx.x; m < M; m += 256) {          // ascending rows: only a strictly better one replaces
    const int c = count[m];
    if (c >= 1 && (double)c >= need) {
      const double e = sum[m] / (double)c;
      if (am < 0 || e < ae) { am = m; ae = e; }
    }
    if (bm < 0 || c > bc) { bm = m; bc = c; }
  }
  __shared__ int s_am[256], s_bm[256], s_bc[256];
  __shared__ double s_ae[256];
  s_am[threadIdx.x] = am; s_ae[threadIdx.x] = ae; s_bm[threadIdx.x] = bm; s_bc[threadIdx.x] = bc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const int t = threadIdx.x, u = t + o;
      if (prerej_better_mean(s_ae[u], s_am[u], s_ae[t], s_am[t])) { s_am[t] = s_am[u]; s_ae[t] = s_ae[u]; }
      if (prerej_better_count(s_bc[u], s_bm[u], s_bc[t], s_bm[t])) { s_bm[t] = s_bm[u]; s_bc[t] = s_bc[u]; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    PrerejCtl c;
    c.converged = s_am[0] >= 0 ? 1 : 0;
    c.winner = c.converged ? s_am[0] : s_bm[0];
    c.count = c.winner >= 0 ? count[c.winner] : 0;
    c.sum = c.winner >= 0 ? sum[c.winner] : 0.0;
    c.refit_kept = 0;
    c.winner_h = c.winner >= 0 ? (long long)(unsigned)surv[(size_t)c.winner * 2].x : -1;
    *ctl = c;
  }
}

// Umeyama in double over the winner's inlier pairs (source keypoint, its nearest target keypoint): 15 sums about the first
// source keypoint / its image, each in the block's fixed order; T_refit receives the fit (the winner itself when it did not
// converge, or with fewer than three inliers: the rescoring then changes nothing).
__global__ void __launch_bounds__(256)
k_prerej_refit(const float4 *__restrict__ skp_q, int ns, GridView g, const float *__restrict__ T_all, float thr2, float radius,
               const PrerejCtl *__restrict__ ctl, float *__restrict__ T_refit)
{
  const PrerejCtl c = *ctl;
  if (c.winner < 0) return;
  float Tl[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) Tl[k] = T_all[(size_t)c.winner * 16 + k];
  if (!c.converged || c.count < 3) {
    if (threadIdx.x < 16) T_refit[threadIdx.x] = Tl[threadIdx.x];
    return;
  }
  const float4 o4 = skp_q[0];
  const float3 e3 = xform(Tl, o4.x, o4.y, o4.z);
  const double o[3] = {(double)o4.x, (double)o4.y, (double)o4.z}, e[3] = {(double)e3.x, (double)e3.y, (double)e3.z};
  double acc[15];
#pragma unroll
  for (int k = 0; k < 15; ++k) acc[k] = 0.0;
  for (int i = threadIdx.x; i < ns; i += 256) {
    const float4 s4 = skp_q[i];
    float4 hit;
    const float d2 = prerej_nearest(g, xform(Tl, s4.x, s4.y, s4.z), thr2, radius, hit);
    if (d2 <= thr2) {
      const double s[3] = {(double)s4.x - o[0], (double)s4.y - o[1], (double)s4.z - o[2]};
      const double d[3] = {(double)hit.x - e[0], (double)hit.y - e[1], (double)hit.z - e[2]};
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        acc[r] += s[r]; acc[3 + r] += d[r];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) acc[6 + r * 3 + cc] += d[r] * s[cc];
      }
    }
  }
  __shared__ double s4w[4];
  double tot[15];
#pragma unroll
  for (int k = 0; k < 15; ++k) tot[k] = prerej_block_sum(acc[k], s4w);
  if (threadIdx.x == 0) {
    float T[16];
    prerej_umeyama(tot, tot + 3, tot + 6, (double)c.count, T);
    for (int r = 0; r < 3; ++r)
      T[12 + r] = (float)((double)T[12 + r] + e[r] - ((double)T[r] * o[0] + (double)T[4 + r] * o[1] + (double)T[8 + r] * o[2]));
    bool finite = true;
    for (int k = 0; k < 16; ++k) finite = finite && (T[k] - T[k] == 0.0f);
    for (int k = 0; k < 16; ++k) T_refit[k] = finite ? T[k] : Tl[k];
  }
}

// the refit when it is not worse (more inliers, or as many and a mean d2 not larger), else the winner: T_out and the verdict
__global__ void __launch_bounds__(64)
k_prerej_final(const float *__restrict__ T_all, const float *__restrict__ T_refit, const int *__restrict__ refit_count,
               const double *__restrict__ refit_sum, PrerejCtl *__restrict__ ctl, float *__restrict__ T_out)
{
  const PrerejCtl c = *ctl;
  if (c.winner < 0) return;
  const int rc = *refit_count;
  const double rs = *refit_sum;
  // (means of equal counts: the sums compare as the means do)
  const bool keep = c.converged && (rc > c.count || (rc == c.count && rs <= c.sum));
  if (threadIdx.x < 16) T_out[threadIdx.x] = keep ? T_refit[threadIdx.x] : T_all[(size_t)c.winner * 16 + threadIdx.x];
  if (threadIdx.x == 0 && keep) { ctl->count = rc; ctl->sum = rs; ctl->refit_kept = 1; }
}

// ---------------------------------------------------------------- host
// the grid of a target's keypoints a radius query reads as one span per cell (cells a hair longer than the radius, merged
// 3x3x3 lists), cached on the cloud like SAC-IA's
static const Grid &prerej_target_grid(Context *c, const mm3d_cloud *tkp, float radius)
{
  const float want = radius * 1.001f;
  const Grid &g = cloud_grid(c, tkp, want > 0.125f ? want : 0.125f);
  grid_ensure_nblists(c, g, 1);
  return g;
}

static bool options_ok(const mm3d_alignment_options *o)
{
  return o && (o->method == MM3D_ALIGN_SAC_IA || o->method == MM3D_ALIGN_PREREJECTIVE) && o->samples >= 1 && o->samples <= (1 << 30) &&
         o->k >= 1 && o->k <= 64 && o->similarity >= 0.0 && o->similarity <= 1.0 && o->inlier_fraction >= 0.0 &&
         o->inlier_fraction <= 1.0;                                                      // (a NaN fails every comparison)
}

// the whole alignment; f as estimate_pair_front leaves it.  rows / counts / cap / n_rows: mm3d_debug_prerejective_survivors.
static void prerej_align(Context *c, const mm3d_alignment_options &o, unsigned seed, const mm3d_cloud *skp, const mm3d_desc *sd,
                         const mm3d_cloud *tkp, const mm3d_desc *td, double inlier_distance, PairFront &f, mm3d_alignment_stats *stats,
                         int *rows = nullptr, int *counts = nullptr, size_t cap = 0, size_t *n_rows = nullptr)
{
  std::memset(f.T0, 0, sizeof(f.T0));
  f.T0[0] = f.T0[5] = f.T0[10] = f.T0[15] = 1.0f;      // SAC-IA's guess, what a failed alignment hands to ICP
  f.on_device = false;
  f.sac_h = 0;
  mm3d_alignment_stats st{o.samples, 0, 0, -1, 0, 0};
  if (stats) *stats = st;
  if (n_rows) *n_rows = 0;
  const int ns = (int)skp->n, nt = (int)tkp->n;
  if (ns < 3 || nt < 3) return;
  MM3D_REQUIRE(sd->n == (size_t)ns && td->n == (size_t)nt, "prerejective alignment: keypoints and descriptors differ in size");
  MM3D_REQUIRE(inlier_distance > 0.0 && inlier_distance < 1e18, "prerejective alignment: the inlier distance must be positive and finite");
  const int kk = std::min(o.k, nt);
  DevBuf<int> nn;
  DevBuf<float> nd;
  desc_knn(c, sd, td, kk, nn, nd);
  const float radius = (float)inlier_distance;
  const float thr2 = (float)(inlier_distance * inlier_distance);
  const Grid &g = prerej_target_grid(c, tkp, radius);
  cloud_hilbert(c, skp);
  const bool permuted = skp->hil_pts.get() && skp->n_finite == skp->n;
  const float4 *skp_q = permuted ? (const float4 *)skp->hil_pts.get() : (const float4 *)skp->pts.get();

  const unsigned blocks = div_up((size_t)o.samples, 256);
  DevBuf<int> block_count(c, (size_t)blocks + 1), block_start(c, (size_t)blocks + 1);
  MM3D_HIP(hipMemsetAsync(block_count.get() + blocks, 0, sizeof(int), c->stream));
  PrerejDraw D;
  D.skp = (const float4 *)skp->pts.get(); D.tkp = (const float4 *)tkp->pts.get(); D.nn = nn.get();
  D.ns = ns; D.nt = nt; D.kk = kk; D.samples = o.samples; D.seed = seed; D.sim2 = o.similarity * o.similarity;
  D.block_count = block_count.get(); D.surv = nullptr;
  MM3D_LAUNCH(c, "prerej_draw", o.samples * 96.0, k_prerej_draw<false>, dim3(blocks), dim3(256), 0, D, (const int *)nullptr);
  exclusive_scan_int(c, block_count.get(), block_start.get(), (size_t)blocks + 1);
  int *hM = (int *)c->pin(64);
  MM3D_HIP(hipMemcpyAsync(hM, block_start.get() + blocks, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  c->sync();
  const int M = hM[0];
  st.survivors = M;
  if (stats) *stats = st;
  if (n_rows) *n_rows = (size_t)M;
  if (M <= 0) return;

  DevBuf<int4> surv(c, (size_t)M * 2);
  D.surv = surv.get();
  MM3D_LAUNCH(c, "prerej_draw", o.samples * 96.0 + M * 32.0, k_prerej_draw<true>, dim3(blocks), dim3(256), 0, D, (const int *)block_start.get());
  DevBuf<float> T_all(c, ((size_t)M + 1) * 16);            // the survivors' models, then the refit
  DevBuf<int> count(c, (size_t)M + 1);
  DevBuf<double> sum(c, (size_t)M + 1);
  DevBuf<PrerejCtl> ctl(c, 1);
  f.dT0 = DevBuf<float>(c, 16);
  MM3D_LAUNCH(c, "prerej_model", M * 256.0, k_prerej_model, dim3(div_up((size_t)M, 64)), dim3(64), 0, D.skp, D.tkp, (const int4 *)surv.get(),
              M, T_all.get());
  const double score_bytes = (double)ns * 16.0;
  MM3D_LAUNCH(c, "prerej_score", score_bytes * M, k_prerej_score, dim3((unsigned)M), dim3(256), 0, skp_q, ns, g.view(),
              (const float *)T_all.get(), thr2, radius, count.get(), sum.get());
  MM3D_LAUNCH(c, "prerej_pick", M * 12.0, k_prerej_pick, dim3(1), dim3(256), 0, (const int *)count.get(), (const double *)sum.get(),
              (const int4 *)surv.get(), M, ns, o.inlier_fraction, ctl.get());
  float *T_refit = T_all.get() + (size_t)M * 16;
  MM3D_LAUNCH(c, "prerej_refit", score_bytes, k_prerej_refit, dim3(1), dim3(256), 0, skp_q, ns, g.view(), (const float *)T_all.get(), thr2,
              radius, (const PrerejCtl *)ctl.get(), T_refit);
  MM3D_LAUNCH(c, "prerej_score", score_bytes, k_prerej_score, dim3(1), dim3(256), 0, skp_q, ns, g.view(), (const float *)T_refit, thr2,
              radius, count.get() + M, sum.get() + M);
  MM3D_LAUNCH(c, "prerej_final", 256.0, k_prerej_final, dim3(1), dim3(64), 0, (const float *)T_all.get(), (const float *)T_refit,
              (const int *)(count.get() + M), (const double *)(sum.get() + M), ctl.get(), f.dT0.get());
  PrerejCtl *hc = (PrerejCtl *)c->pin(sizeof(PrerejCtl));
  MM3D_HIP(hipMemcpyAsync(hc, ctl.get(), sizeof(PrerejCtl), hipMemcpyDeviceToHost, c->stream));
  const size_t n_out = rows ? std::min(cap, (size_t)M) : 0;
  std::vector<int4> hrows;
  if (n_out) {
    hrows.resize(n_out * 2);
    MM3D_HIP(hipMemcpyAsync(hrows.data(), surv.get(), n_out * 2 * sizeof(int4), hipMemcpyDeviceToHost, c->stream));
    if (counts) MM3D_HIP(hipMemcpyAsync(counts, count.get(), n_out * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  }
  c->sync();
  for (size_t r = 0; r < n_out; ++r) {
    const int4 a = hrows[r * 2], b = hrows[r * 2 + 1];
    const int v[7] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z};
    std::memcpy(rows + r * 7, v, sizeof(v));
  }
  f.on_device = true;
  st.hypotheses_scored = (long long)M + (hc->converged && hc->count >= 3 ? 1 : 0);
  st.winner_h = hc->winner_h;
  st.winner_inliers = hc->count;
  st.converged = hc->converged;
  if (stats) *stats = st;
}

namespace {
struct AlignPrerejective final : AlignMethodBase {
  void prepare(Context *c, const mm3d_cloud *kp, double inlier_distance) const override
  {
    if (kp->n == 0 || !(inlier_distance > 0.0 && inlier_distance < 1e18)) return;
    (void)prerej_target_grid(c, kp, (float)inlier_distance);
    cloud_hilbert(c, kp);
  }
  void front(Context *c, const mm3d_alignment_options &o, unsigned seed, const mm3d_cloud *skp, const mm3d_desc *sd, const mm3d_cloud *tkp,
             const mm3d_desc *td, double inlier_distance, PairFront &f, mm3d_alignment_stats *stats) const override
  {
    prerej_align(c, o, seed, skp, sd, tkp, td, inlier_distance, f, stats);
  }
};
const AlignPrerejective g_prerejective;
}  // namespace

}  // namespace mm3d

using namespace mm3d;

extern "C" {

int mm3d_set_alignment(mm3d_ctx *ctx, const mm3d_alignment_options *options)
{
  if (!ctx || !options_ok(options)) return MM3D_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the method changes)
  return select_stage(ctx, Stage::Alignment, [&](StageSelection &s) {
    s.align_options = *options;
    s.align = stage_active(Stage::Alignment, s) ? &g_prerejective : nullptr;
  });
}

int mm3d_get_alignment(const mm3d_ctx *ctx, mm3d_alignment_options *options)
{
  if (!ctx || !options) return MM3D_EINVAL;
  *options = ctx->sel.align_options;
  return MM3D_OK;
}

int mm3d_last_alignment_stats(const mm3d_ctx *ctx, mm3d_alignment_stats *stats)
{
  if (!ctx || !stats) return MM3D_EINVAL;
  *stats = ctx->last_align_stats;
  return MM3D_OK;
}

static int prerej_call(mm3d_ctx *ctx, const mm3d_cloud *skp, const mm3d_desc *sd, const mm3d_cloud *tkp, const mm3d_desc *td,
                       double inlier_distance, const mm3d_alignment_options *options, float T[16], mm3d_alignment_stats *stats, int *rows,
                       int *counts, size_t cap, size_t *n_rows)
{
  if (!ctx || !skp || !sd || !tkp || !td || !options_ok(options)) return MM3D_EINVAL;
  if (!(inlier_distance > 0.0 && inlier_distance < 1e18) || sd->n != skp->n || td->n != tkp->n) {
    ctx->err = "prerejective alignment: the inlier distance must be positive and finite, the descriptors one per keypoint";
    return MM3D_EINVAL;
  }
  return guarded(ctx, [&] {
    PairFront f;
    prerej_align(ctx, *options, ctx->rnd.seed0, skp, sd, tkp, td, inlier_distance, f, stats, rows, counts, cap, n_rows);
    if (!T) return;
    std::memcpy(T, f.T0, sizeof(f.T0));
    if (f.on_device) {
      float *hT = (float *)ctx->pin(64);
      MM3D_HIP(hipMemcpyAsync(hT, f.dT0.get(), sizeof(float) * 16, hipMemcpyDeviceToHost, ctx->stream));
      ctx->sync();
      std::memcpy(T, hT, sizeof(float) * 16);
    }
  });
}

int mm3d_estimate_transform_prerejective(mm3d_ctx *ctx, const mm3d_cloud *skp, const mm3d_desc *sd, const mm3d_cloud *tkp,
                                         const mm3d_desc *td, double inlier_distance, const mm3d_alignment_options *options, float T[16],
                                         mm3d_alignment_stats *stats)
{
  if (!T) return MM3D_EINVAL;
  return prerej_call(ctx, skp, sd, tkp, td, inlier_distance, options, T, stats, nullptr, nullptr, 0, nullptr);
}

int mm3d_debug_prerejective_survivors(mm3d_ctx *ctx, const mm3d_cloud *skp, const mm3d_desc *sd, const mm3d_cloud *tkp, const mm3d_desc *td,
                                      double inlier_distance, const mm3d_alignment_options *options, int *rows, int *counts, size_t cap,
                                      size_t *n_survivors)
{
  if (!n_survivors || (cap && !rows)) return MM3D_EINVAL;
  return prerej_call(ctx, skp, sd, tkp, td, inlier_distance, options, nullptr, nullptr, rows, counts, cap, n_survivors);
}

}  // extern "C"

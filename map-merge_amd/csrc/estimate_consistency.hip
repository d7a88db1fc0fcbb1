// estimate_consistency.hip -- consistency-graph estimation, the opt-in alternative to the RANSAC behind estimation_method =
// MATCHING (mm3d_set_estimator; include/mm3d.h states the rule, step by step).
//
// Two correct correspondences preserve the distance between their points; the graph of pairwise length-compatible
// correspondences holds the inliers as a clique (Leordeanu and Hebert 2005; Chen et al., SC2-PCR, 2022).  Every decision is an
// integer or a comparison of doubles formed in one written order, so nothing depends on what else is in flight.
//
//   k_cons_gather   one lane per correspondence: its two keypoints, the keypoint indices in .w
//   k_cons_graph    a block owns 64 rows (their records in LDS, read as broadcasts) and 256 columns (one per lane, in
//                   registers); a wave's ballot over one row is one 64-bit word of A.  The whole matrix is computed, not the
//                   upper triangle with its mirror (DESIGN.md section 7l says why)
//   k_cons_degree   one wave per row: the popcount sum
//   k_cons_rank     one lane per correspondence and span of 2 048 others: its rank in (deg descending, i ascending) by counting
//   k_cons_seeds    the correspondences of rank below `seeds` into the seed list
//   k_cons_hypotheses  a block per seed: popcount(row_s & row_j) for the set j, a wave per row; the consensus - 1 largest by
//                   repeated block maxima of (S, -j) keys; Umeyama in double over the set in ascending order
//   (ransac_count)  registration.hip's, unchanged: every hypothesis scored in one launch
// One copy back and one wait; the winner and RANSAC's own tail (host_pipeline.cpp::ransac_model_tail) are the host's.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "capi_guard.hpp"
#include "drivers.hpp"
#include "device_util.hpp"
#include "linalg_shared.hpp"

namespace mm3d {

constexpr int kConsMaxCorr = 32768;       // the bit rows of one pair stay at or below 128 MB
constexpr int kConsMaxConsensus = 64;
constexpr int kConsHypBlocks = 256;       // blocks of k_cons_hypotheses: each owns a scratch row of C keys

struct ConsCtl { unsigned long long deg_sum; };      // the sum of the degrees: twice the edges

__global__ void __launch_bounds__(256)
k_cons_gather(const float4 *__restrict__ skp, const float4 *__restrict__ tkp, const int *__restrict__ is, const int *__restrict__ it,
              int C, float4 *__restrict__ P, float4 *__restrict__ Q)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C) return;
  float4 p = skp[is[i]], q = tkp[it[i]];
  p.w = __int_as_float(is[i]);
  q.w = __int_as_float(it[i]);
  P[i] = p;
  Q[i] = q;
}

// squared length ((dx dx + dy dy) + dz dz) in double: exact differences of floats, no contraction
__device__ __forceinline__ double cons_len2(const float4 a, const float4 b)
{
  const double dx = (double)a.x - (double)b.x, dy = (double)a.y - (double)b.y, dz = (double)a.z - (double)b.z;
  return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}
// step 1 of the rule (anything not a number compares false)
__device__ __forceinline__ bool cons_compatible(const float4 pi, const float4 qi, const float4 pj, const float4 qj, double t2)
{
  if (__float_as_int(pi.w) == __float_as_int(pj.w) || __float_as_int(qi.w) == __float_as_int(qj.w)) return false;
  const double da = cons_len2(pi, pj), db = cons_len2(qi, qj);
  const double e = __dsub_rn(__dadd_rn(da, db), t2);
  return da > t2 && db > t2 && __dmul_rn(e, e) <= __dmul_rn(4.0, __dmul_rn(da, db));
}

// grid (ceil(W / 4), ceil(C / 64)): wave w of block (bx, by) makes word bx * 4 + w of the rows by * 64 ... + 63
__global__ void __launch_bounds__(256)
k_cons_graph(const float4 *__restrict__ P, const float4 *__restrict__ Q, int C, int W, double t2, unsigned long long *__restrict__ A)
{
  __shared__ float4 sP[64], sQ[64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.y * 64;
  if (threadIdx.x < 64) {
    const int i = r0 + (int)threadIdx.x;
    sP[threadIdx.x] = i < C ? P[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    sQ[threadIdx.x] = i < C ? Q[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  const int w = blockIdx.x * 4 + wave;
  if (w >= W) return;                                   // (wave-uniform, behind the barrier)
  const int j = w * 64 + lane;
  const bool live = j < C;                              // bits at and beyond C stay zero
  const float4 pj = live ? P[j] : make_float4(0.f, 0.f, 0.f, 0.f), qj = live ? Q[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  const int rows = min(64, C - r0);
  unsigned long long mine = 0ull;
  for (int ii = 0; ii < rows; ++ii) {
    const unsigned long long m = ballot(live && cons_compatible(sP[ii], sQ[ii], pj, qj, t2));
    if (lane == ii) mine = m;
  }
  if (lane < rows) A[(size_t)(r0 + lane) * W + w] = mine;
}

__global__ void __launch_bounds__(256) k_cons_degree(const unsigned long long *__restrict__ A, int C, int W, int *__restrict__ deg)
{
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= C) return;                                 // (wave-uniform)
  int n = 0;
  for (int w = lane; w < W; w += 64) n += __popcll(A[(size_t)row * W + w]);
  n = wave_sum(n);
  if (lane == 0) deg[row] = n;
}

// step 3: correspondence i with deg >= 2 is seed number #{j eligible : deg_j > deg_i, or deg_j == deg_i and j < i}.  With
// key = (deg << 15) | (32767 - i) -- deg < C <= 2^15, i < 2^15 -- that is #{j eligible : key_j > key_i}; 0 = not eligible.
__device__ __forceinline__ unsigned cons_seed_key(int deg, int i) { return deg >= 2 ? ((unsigned)deg << 15) | (unsigned)(32767 - i) : 0u; }
constexpr int kConsRankSpan = 2048;       // the j of one block of k_cons_rank

// grid (ceil(C / 256), ceil(C / kConsRankSpan)): block (bx, by) counts, for its 256 i, the larger keys among its span of j,
// and adds the count to rank[i] (zeroed; integer sums: the order of the atomics does not show)
__global__ void __launch_bounds__(256) k_cons_rank(const int *__restrict__ deg, int C, int *__restrict__ rank)
{
  __shared__ unsigned s_key[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const unsigned ki = i < C ? cons_seed_key(deg[i], i) : 0u;
  const int j_end = min(C, ((int)blockIdx.y + 1) * kConsRankSpan);
  int n = 0;
  for (int j0 = blockIdx.y * kConsRankSpan; j0 < j_end; j0 += 256) {
    const int j = j0 + (int)threadIdx.x;
    s_key[threadIdx.x] = j < j_end ? cons_seed_key(deg[j], j) : 0u;
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < 256; ++k) n += s_key[k] > ki ? 1 : 0;
    __syncthreads();
  }
  if (ki != 0u && n) atomicAdd(&rank[i], n);
}

__global__ void __launch_bounds__(256)
k_cons_seeds(const int *__restrict__ deg, const int *__restrict__ rank, int C, int H, int *__restrict__ seeds, ConsCtl *__restrict__ ctl)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int di = i < C ? deg[i] : 0;
  if (di >= 2 && rank[i] < H) seeds[rank[i]] = i;
  const int dsum = wave_sum(di);                        // (an integer sum: the order of the atomics does not show)
  if ((threadIdx.x & 63) == 0 && dsum) atomicAdd(&ctl->deg_sum, (unsigned long long)dsum);
}

__device__ __forceinline__ unsigned cons_block_max(unsigned v, unsigned *s4)
{
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return max(max(s4[0], s4[1]), max(s4[2], s4[3]));
}

// Umeyama without scale over the n pairs idx[0..n) (ascending), the sums in double about the first pair's points so that they
// stay small next to the coordinates; the formulas of the prerejective refit (align_prerej.hip)
__device__ inline void cons_umeyama(const float4 *__restrict__ P, const float4 *__restrict__ Q, const int *idx, int n, float *T)
{
  const float4 s0 = P[idx[0]], d0 = Q[idx[0]];
  const double o[3] = {(double)s0.x, (double)s0.y, (double)s0.z}, e[3] = {(double)d0.x, (double)d0.y, (double)d0.z};
  double sum_s[3] = {0, 0, 0}, sum_d[3] = {0, 0, 0}, sum_ds[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 1; k < n; ++k) {
    const float4 p = P[idx[k]], q = Q[idx[k]];
    const double s[3] = {(double)p.x - o[0], (double)p.y - o[1], (double)p.z - o[2]};
    const double d[3] = {(double)q.x - e[0], (double)q.y - e[1], (double)q.z - e[2]};
    for (int r = 0; r < 3; ++r) {
      sum_s[r] += s[r]; sum_d[r] += d[r];
      for (int c = 0; c < 3; ++c) sum_ds[r * 3 + c] += d[r] * s[c];
    }
  }
  const double inv = 1.0 / (double)n;
  double sm[3], dm[3], sigma[9], R[9], t[3];
  for (int a = 0; a < 3; ++a) { sm[a] = sum_s[a] * inv; dm[a] = sum_d[a] * inv; }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) sigma[r * 3 + c] = sum_ds[r * 3 + c] * inv - dm[r] * sm[c];
  umeyama_core_shared(sigma, sm, dm, 1e-12, R, t);
  // back from the shifted frames, x -> R (x - s0) + t + d0, and rounded once
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[c * 4 + r] = (float)R[r * 3 + c];
    T[12 + r] = (float)(t[r] + e[r] - (R[r * 3] * o[0] + R[r * 3 + 1] * o[1] + R[r * 3 + 2] * o[2]));
  }
  T[3] = T[7] = T[11] = 0.0f;
  T[15] = 1.0f;
}

// steps 4 and 5.  Block b takes the seeds of rank b, b + gridDim.x, ...; keys: [gridDim.x][C], the block's scratch row.
// A key is (S << 16) | (65535 - j): S <= C <= 2^15 and j < 2^15, so the larger key is the larger S and, among equals, the lower j.
__global__ void __launch_bounds__(256)
k_cons_hypotheses(const unsigned long long *__restrict__ A, const float4 *__restrict__ P, const float4 *__restrict__ Q, int C, int W,
                  const int *__restrict__ seeds, int H, int K, unsigned *__restrict__ keys, int *__restrict__ cons, int *__restrict__ nk,
                  float *__restrict__ T_all)
{
  __shared__ unsigned long long s_row[kConsMaxCorr / 64];
  __shared__ int s_pick[kConsMaxConsensus], s_sorted[kConsMaxConsensus];
  __shared__ unsigned s4[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned *key = keys + (size_t)blockIdx.x * C;
  for (int r = blockIdx.x; r < H; r += gridDim.x) {
    const int s = seeds[r];                             // (block-uniform)
    __syncthreads();                                    // the previous seed's shared arrays have been read
    if (s < 0) {
      if ((int)threadIdx.x < K) cons[(size_t)r * K + threadIdx.x] = -1;
      if (threadIdx.x < 16) T_all[(size_t)r * 16 + threadIdx.x] = 0.0f;
      if (threadIdx.x == 0) nk[r] = 0;
      continue;
    }
    for (int w = threadIdx.x; w < W; w += 256) s_row[w] = A[(size_t)s * W + w];
    __syncthreads();
    // S_sj of the j with A_sj set, a wave per row
    for (int j = wave; j < C; j += 4) {
      unsigned k = 0u;
      if ((s_row[j >> 6] >> (j & 63)) & 1ull) {         // (wave-uniform)
        int n = 0;
        for (int w = lane; w < W; w += 64) n += __popcll(s_row[w] & A[(size_t)j * W + w]);
        n = wave_sum(n);
        if (n >= 1) k = ((unsigned)n << 16) | (unsigned)(65535 - j);
      }
      if (lane == 0) key[j] = k;
    }
    __syncthreads();
    // the K - 1 largest keys, in descending order: each the largest below the one before
    unsigned last = 0xFFFFFFFFu;
    int n_pick = 0;
    for (; n_pick < K - 1; ++n_pick) {
      unsigned m = 0u;
      for (int j = threadIdx.x; j < C; j += 256) {
        const unsigned k = key[j];
        if (k < last && k > m) m = k;
      }
      m = cons_block_max(m, s4);
      if (m == 0u) break;                               // (block-uniform)
      if (threadIdx.x == 0) s_pick[n_pick] = 65535 - (int)(m & 0xFFFFu);
      last = m;
    }
    if (threadIdx.x == 0) s_pick[n_pick] = s;           // (never among the picks: A_ss = 0)
    const int n = n_pick + 1;
    __syncthreads();
    // ascending index order: every element's rank among n distinct ones
    if ((int)threadIdx.x < n) {
      const int e = s_pick[threadIdx.x];
      int rank = 0;
      for (int k = 0; k < n; ++k) rank += s_pick[k] < e ? 1 : 0;
      s_sorted[rank] = e;
    }
    __syncthreads();
    if ((int)threadIdx.x < K) cons[(size_t)r * K + threadIdx.x] = (int)threadIdx.x < n ? s_sorted[threadIdx.x] : -1;
    if (threadIdx.x == 0) {
      float T[16];
      if (n >= 3) cons_umeyama(P, Q, s_sorted, n, T);
      else for (int k = 0; k < 16; ++k) T[k] = 0.0f;
      for (int k = 0; k < 16; ++k) T_all[(size_t)r * 16 + k] = T[k];
      nk[r] = n;
    }
  }
}

// ---------------------------------------------------------------- host
static bool options_ok(const mm3d_estimator_options *o)
{
  return o && (o->method == MM3D_ESTIMATOR_RANSAC || o->method == MM3D_ESTIMATOR_CONSISTENCY) && o->tolerance >= 0.0 &&
         o->seeds >= 1 && o->seeds <= 4096 && o->consensus >= 3 && o->consensus <= kConsMaxConsensus;   // (a NaN fails every comparison)
}

// what mm3d_debug_consistency asks for (null: not wanted)
struct ConsDebug {
  unsigned long long *rows = nullptr;
  int *deg = nullptr, *seeds = nullptr, *consensus = nullptr, *counts = nullptr;
  float *hypotheses = nullptr;
  size_t *n_seeds = nullptr;
};

// the whole rule: T and inliers as ransac_transform leaves them
static size_t consistency_transform(Context *c, const mm3d_estimator_options &o, const mm3d_cloud *skp_, const mm3d_cloud *tkp_,
                                    const mm3d_corr *corr, size_t n_corr_, double inlier_threshold, float T[16],
                                    std::vector<mm3d_corr> &inliers, mm3d_estimator_stats *stats, const ConsDebug *dbg = nullptr)
{
  std::memset(T, 0, sizeof(float) * 16);
  inliers.clear();
  mm3d_estimator_stats st{(long long)n_corr_, 0, 0, 0, -1, -1, 0};
  if (stats) *stats = st;
  if (dbg && dbg->n_seeds) *dbg->n_seeds = 0;
  if (n_corr_ > (size_t)kConsMaxCorr) throw Error(MM3D_EUNSUPPORTED, "consistency estimation: more than 32768 correspondences");
  const int C = (int)n_corr_;
  if (C < 3) return 0;
  const std::vector<float4> &skp = cloud_host(c, skp_);
  const std::vector<float4> &tkp = cloud_host(c, tkp_);
  std::vector<int> is(C), it(C);
  for (int i = 0; i < C; ++i) {
    MM3D_REQUIRE(corr[i].index_query >= 0 && (size_t)corr[i].index_query < skp.size() && corr[i].index_match >= 0 &&
                     (size_t)corr[i].index_match < tkp.size(),
                 "correspondence index out of range");
    is[i] = corr[i].index_query; it[i] = corr[i].index_match;
  }
  const int W = (C + 63) / 64, H = std::min(o.seeds, C), K = o.consensus;
  const double tau = o.tolerance > 0.0 ? o.tolerance : inlier_threshold;
  const double t2 = tau * tau, thr2 = inlier_threshold * inlier_threshold;
  const unsigned hyp_blocks = (unsigned)std::min(H, kConsHypBlocks);

  DevBuf<int> d_is(c, C), d_it(c, C), deg(c, C), rank(c, C), seeds(c, H), cons(c, (size_t)H * K), nk(c, H), counts(c, H);
  DevBuf<float4> P(c, C), Q(c, C);
  DevBuf<unsigned long long> A(c, (size_t)C * W);
  DevBuf<unsigned> keys(c, (size_t)hyp_blocks * C);
  DevBuf<float> T_all(c, (size_t)H * 16);
  DevBuf<ConsCtl> ctl(c, 1);
  MM3D_HIP(hipMemcpyAsync(d_is.get(), is.data(), sizeof(int) * C, hipMemcpyHostToDevice, c->stream));
  MM3D_HIP(hipMemcpyAsync(d_it.get(), it.data(), sizeof(int) * C, hipMemcpyHostToDevice, c->stream));
  MM3D_HIP(hipMemsetAsync(seeds.get(), 0xFF, sizeof(int) * H, c->stream));
  MM3D_HIP(hipMemsetAsync(ctl.get(), 0, sizeof(ConsCtl), c->stream));
  MM3D_HIP(hipMemsetAsync(rank.get(), 0, sizeof(int) * C, c->stream));
  MM3D_LAUNCH(c, "cons_gather", C * 72.0, k_cons_gather, dim3(div_up(C, 256)), dim3(256), 0, (const float4 *)skp_->pts.get(),
              (const float4 *)tkp_->pts.get(), (const int *)d_is.get(), (const int *)d_it.get(), C, P.get(), Q.get());
  MM3D_LAUNCH(c, "cons_graph", (double)C * W * 8.0, k_cons_graph, dim3(div_up(W, 4), div_up(C, 64)), dim3(256), 0,
              (const float4 *)P.get(), (const float4 *)Q.get(), C, W, t2, A.get());
  MM3D_LAUNCH(c, "cons_degree", (double)C * W * 8.0, k_cons_degree, dim3(div_up(C, 4)), dim3(256), 0,
              (const unsigned long long *)A.get(), C, W, deg.get());
  MM3D_LAUNCH(c, "cons_rank", C * 8.0, k_cons_rank, dim3(div_up(C, 256), div_up(C, kConsRankSpan)), dim3(256), 0, (const int *)deg.get(), C,
              rank.get());
  MM3D_LAUNCH(c, "cons_seeds", C * 12.0, k_cons_seeds, dim3(div_up(C, 256)), dim3(256), 0, (const int *)deg.get(), (const int *)rank.get(), C,
              H, seeds.get(), ctl.get());
  MM3D_LAUNCH(c, "cons_hypotheses", 0, k_cons_hypotheses, dim3(hyp_blocks), dim3(256), 0, (const unsigned long long *)A.get(),
              (const float4 *)P.get(), (const float4 *)Q.get(), C, W, (const int *)seeds.get(), H, K, keys.get(), cons.get(), nk.get(),
              T_all.get());
  ransac_count(c, skp_->pts.get(), tkp_->pts.get(), d_is.get(), d_it.get(), C, T_all.get(), H, thr2, counts.get());

  // one copy back, one wait: [ctl | seeds | nk | counts | T_all]
  std::vector<int> h_seeds(H), h_nk(H), h_counts(H);
  std::vector<float> h_T((size_t)H * 16);
  ConsCtl h_ctl{};
  MM3D_HIP(hipMemcpyAsync(&h_ctl, ctl.get(), sizeof(ConsCtl), hipMemcpyDeviceToHost, c->stream));
  MM3D_HIP(hipMemcpyAsync(h_seeds.data(), seeds.get(), sizeof(int) * H, hipMemcpyDeviceToHost, c->stream));
  MM3D_HIP(hipMemcpyAsync(h_nk.data(), nk.get(), sizeof(int) * H, hipMemcpyDeviceToHost, c->stream));
  MM3D_HIP(hipMemcpyAsync(h_counts.data(), counts.get(), sizeof(int) * H, hipMemcpyDeviceToHost, c->stream));
  MM3D_HIP(hipMemcpyAsync(h_T.data(), T_all.get(), sizeof(float) * 16 * H, hipMemcpyDeviceToHost, c->stream));
  if (dbg) {
    if (dbg->rows) MM3D_HIP(hipMemcpyAsync(dbg->rows, A.get(), sizeof(unsigned long long) * (size_t)C * W, hipMemcpyDeviceToHost, c->stream));
    if (dbg->deg) MM3D_HIP(hipMemcpyAsync(dbg->deg, deg.get(), sizeof(int) * C, hipMemcpyDeviceToHost, c->stream));
    if (dbg->consensus) MM3D_HIP(hipMemcpyAsync(dbg->consensus, cons.get(), sizeof(int) * (size_t)H * K, hipMemcpyDeviceToHost, c->stream));
  }
  c->sync();

  // step 7: the first maximum among the seeds with a hypothesis
  int best = -1;
  for (int r = 0; r < H; ++r) {
    if (h_seeds[r] < 0) continue;
    ++st.seeds;
    if (h_nk[r] < 3) { h_counts[r] = -1; continue; }
    ++st.hypotheses;
    if (best < 0 || h_counts[r] > h_counts[best]) best = r;
  }
  for (int r = 0; r < H; ++r)
    if (h_seeds[r] < 0) h_counts[r] = -1;
  st.edges = (long long)(h_ctl.deg_sum / 2);
  if (best >= 0) { st.winner_index = h_seeds[best]; st.winner_rank = best; st.winner_inliers = h_counts[best]; }
  if (stats) *stats = st;
  if (dbg) {
    if (dbg->n_seeds) *dbg->n_seeds = (size_t)st.seeds;
    if (dbg->seeds) std::memcpy(dbg->seeds, h_seeds.data(), sizeof(int) * H);
    if (dbg->counts) std::memcpy(dbg->counts, h_counts.data(), sizeof(int) * H);
    if (dbg->hypotheses) std::memcpy(dbg->hypotheses, h_T.data(), sizeof(float) * 16 * H);
  }
  if (best < 0) return 0;
  return ransac_model_tail(skp, tkp, corr, is, it, &h_T[(size_t)best * 16], thr2, T, inliers);
}

namespace {
struct EstimatorConsistency final : EstimatorMethodBase {
  void front(Context *c, const mm3d_estimator_options &o, const mm3d_cloud *skp, const mm3d_desc *sd, const mm3d_cloud *tkp,
             const mm3d_desc *td, double inlier_threshold, size_t matching_k, PairFront &f, mm3d_estimator_stats *stats) const override
  {
    std::memset(f.T0, 0, sizeof(f.T0));
    f.on_device = false;
    f.counts = PairCounts();
    std::vector<mm3d_corr> corr, inl;
    find_correspondences(c, sd, td, matching_k, corr);
    consistency_transform(c, o, skp, tkp, corr.data(), corr.size(), inlier_threshold, f.T0, inl, stats);
    f.counts.n_correspondences = (int)corr.size();
    f.counts.n_inliers = (int)inl.size();
  }
};
const EstimatorConsistency g_consistency;
}  // namespace

}  // namespace mm3d

using namespace mm3d;

extern "C" {

int mm3d_set_estimator(mm3d_ctx *ctx, const mm3d_estimator_options *options)
{
  if (!ctx || !options_ok(options)) return MM3D_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the method changes)
  return select_stage(ctx, Stage::Estimator, [&](StageSelection &s) {
    s.estimator_options = *options;
    s.estimator = stage_active(Stage::Estimator, s) ? &g_consistency : nullptr;
  });
}

int mm3d_get_estimator(const mm3d_ctx *ctx, mm3d_estimator_options *options)
{
  if (!ctx || !options) return MM3D_EINVAL;
  *options = ctx->sel.estimator_options;
  return MM3D_OK;
}

int mm3d_last_estimator_stats(const mm3d_ctx *ctx, mm3d_estimator_stats *stats)
{
  if (!ctx || !stats) return MM3D_EINVAL;
  *stats = ctx->last_estimator_stats;
  return MM3D_OK;
}

int mm3d_estimate_transform_consistency(mm3d_ctx *ctx, const mm3d_cloud *skp, const mm3d_cloud *tkp, const mm3d_corr *corr, size_t n_corr,
                                        double inlier_threshold, const mm3d_estimator_options *options, float T[16], mm3d_corr *inliers,
                                        size_t cap, size_t *n_inliers, mm3d_estimator_stats *stats)
{
  if (!ctx || !skp || !tkp || (!corr && n_corr) || !T || !options_ok(options)) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    std::vector<mm3d_corr> inl;
    consistency_transform(ctx, *options, skp, tkp, corr, n_corr, inlier_threshold, T, inl, stats);
    if (n_inliers) *n_inliers = inl.size();
    if (inliers) {
      if (cap < inl.size()) throw Error(MM3D_ECAPACITY, "inlier buffer too small");
      std::memcpy(inliers, inl.data(), inl.size() * sizeof(mm3d_corr));
    }
  });
}

int mm3d_debug_consistency(mm3d_ctx *ctx, const mm3d_cloud *skp, const mm3d_cloud *tkp, const mm3d_corr *corr, size_t n_corr,
                           double inlier_threshold, const mm3d_estimator_options *options, unsigned long long *rows, int *deg, int *seeds,
                           size_t *n_seeds, int *consensus, float *hypotheses, int *counts)
{
  if (!ctx || !skp || !tkp || (!corr && n_corr) || !options_ok(options)) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    ConsDebug d;
    d.rows = rows; d.deg = deg; d.seeds = seeds; d.n_seeds = n_seeds; d.consensus = consensus; d.hypotheses = hypotheses; d.counts = counts;
    float T[16];
    std::vector<mm3d_corr> inl;
    consistency_transform(ctx, *options, skp, tkp, corr, n_corr, inlier_threshold, T, inl, nullptr, &d);
  });
}

}  // extern "C"

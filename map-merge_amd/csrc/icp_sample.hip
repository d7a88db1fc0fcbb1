// icp_sample.hip -- ICP source sampling on gfx950: the pair stage's ICP searches a sample of the source map instead of every point
// of it (mm3d_set_icp_sampling, mm3d_sample_icp_source; include/mm3d.h states the rule to the operation).  NORMAL_SPACE keeps
// the same number of points from every direction a surface faces (Rusinkiewicz and Levoy, 3DIM 2001; PCL's NormalSpaceSampling
// is the known implementation, and no parity with it is claimed); STRIDE keeps every k-th valid point.  Not a reference stage
// (DESIGN.md section 7m).
//
// One pass family per cloud, nothing read back but the sample's size:
//   k_smp_bucket   a lane per point: its bucket id (one byte, 0xFF = never sampled), and the block's count per bucket from
//                  per-wave LDS histograms -- plain stores into the block's own row, no global atomics
//   k_smp_levels   ONE block: per bucket the exclusive prefix of the blocks' counts (in place), then n_valid, the budget m, the
//                  water-fill level L by a binary search over the at most 192 counts, and take_b; all of it stays on the device
//   k_smp_select   the geometry of k_smp_bucket again: every point's stable rank inside its bucket -- within a wave a loop over
//                  the distinct keys present (ballot, popcount of the lower lanes), across the block's waves through LDS, across
//                  the blocks through k_smp_levels' prefixes -- and the keep flag floor((r+1) take / c) > floor(r take / c)
//   compact        the library's ordered compaction (grid.hip::cloud_of_kept): the sample cloud, its bounding box, and the one
//                  host wait; a stage call that wants the kept reference indices runs one more fused scan over the flags
// Everything is integer arithmetic or one rounded f32 multiply and a compare, so the sample does not depend on the launch
// geometry, the stream or what else runs.
#include <cmath>
#include <cstring>

#include "capi_guard.hpp"
#include "drivers.hpp"
#include "device_util.hpp"
#include "map_kept.hpp"
#include "nn_core.hpp"
#include "scan_fused.hpp"

namespace mm3d {

namespace {

constexpr int kSmpRounds = 4;                               // a wave takes 4 x 64 consecutive points,
constexpr int kSmpPerWave = kWave * kSmpRounds;
constexpr int kSmpPerBlock = 4 * kSmpPerWave;               // a block of four waves 1024
constexpr int kSmpMaxBuckets = 192;                         // 3 bins^2, bins <= 8
constexpr int kSmpInvalid = 0xFF;
// the control words k_smp_levels leaves: c_b | take_b | n_valid, m, L, non-empty buckets
constexpr int kSmpCtlTake = kSmpMaxBuckets, kSmpCtlStats = 2 * kSmpMaxBuckets, kSmpCtlWords = 2 * kSmpMaxBuckets + 4;

struct SmpRule {
  int method, bins, max_points;
  float inv_bins;                                           // 1.0f / bins, exact: bins is a power of two
  double fraction;
};

// cu of the rule: how many of the edges e_k r, e_k = -1 + 2k / bins, lie at or below q
__device__ __forceinline__ int smp_cell(float q, float r, int bins, float inv_bins)
{
  int cell = 0;
  for (int k = 1; k < bins; ++k) cell += q >= __fmul_rn(__fmul_rn((float)(2 * k - bins), inv_bins), r) ? 1 : 0;
  return cell;
}

__device__ __forceinline__ int smp_bucket(const float4 &p, const float4 *__restrict__ nrm, int i, const SmpRule &rule)
{
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) return kSmpInvalid;
  if (rule.method == MM3D_ICP_SAMPLE_STRIDE) return 0;
  const float4 n = nrm[i];
  if (!(isfinite(n.x) && isfinite(n.y) && isfinite(n.z)) || (n.x == 0.0f && n.y == 0.0f && n.z == 0.0f)) return kSmpInvalid;
  // the face: the largest |component|, ties to the lowest index; s its component, then the two that follow it cyclically
  int a = 0;
  float s = n.x, u = n.y, v = n.z, best = fabsf(n.x);
  if (fabsf(n.y) > best) { a = 1; s = n.y; u = n.z; v = n.x; best = fabsf(n.y); }
  if (fabsf(n.z) > best) { a = 2; s = n.z; u = n.x; v = n.y; best = fabsf(n.z); }
  if (s < 0.0f) { u = -u; v = -v; }                        // antipodes fold
  return (a * rule.bins + smp_cell(u, best, rule.bins, rule.inv_bins)) * rule.bins + smp_cell(v, best, rule.bins, rule.inv_bins);
}

// The stable rank of this lane's key among the wave's points so far, and the wave's running histogram moved past this round.
// A loop over the distinct keys present: the first lane still waiting names the key, a ballot finds its lanes, a lane's rank is
// what the histogram holds plus the lanes below it.  Called by all 64 lanes; hist is the wave's own LDS row.
__device__ __forceinline__ int smp_wave_rank(int key, int lane, int *hist)
{
  unsigned long long todo = ballot(key != kSmpInvalid);
  int rank = 0;
  while (todo) {                                            // (wave-uniform)
    const int leader = __ffsll((long long)todo) - 1;
    const int k = __shfl(key, leader, kWave);
    const unsigned long long same = ballot(key == k);
    const int before = hist[k];                             // one address for the whole wave
    if (key == k) rank = before + __popcll(same & ((1ull << lane) - 1ull));
    wave_lds_fence();
    if (lane == leader) hist[k] = before + __popcll(same);
    wave_lds_fence();
    todo &= ~same;
  }
  return rank;
}

__global__ void __launch_bounds__(256)
k_smp_bucket(const float4 *__restrict__ pts, const float4 *__restrict__ nrm, int n, SmpRule rule, int n_buckets,
             unsigned char *__restrict__ bucket, int *__restrict__ counts /* [blocks][n_buckets] */)
{
  __shared__ int s_hist[4][kSmpMaxBuckets];
  for (int k = threadIdx.x; k < 4 * kSmpMaxBuckets; k += 256) (&s_hist[0][0])[k] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * kSmpPerBlock + wave * kSmpPerWave;
#pragma unroll
  for (int r = 0; r < kSmpRounds; ++r) {
    const long long i = base + r * kWave + lane;
    int key = kSmpInvalid;
    if (i < n) {
      key = smp_bucket(pts[i], nrm, (int)i, rule);
      bucket[i] = (unsigned char)key;
    }
    (void)smp_wave_rank(key, lane, s_hist[wave]);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < n_buckets; b += 256)
    counts[(size_t)blockIdx.x * n_buckets + b] = (s_hist[0][b] + s_hist[1][b]) + (s_hist[2][b] + s_hist[3][b]);
}

__global__ void __launch_bounds__(256)
k_smp_levels(int *__restrict__ counts /* in: [blocks][n_buckets]; out: their exclusive prefixes over the blocks */, int blocks,
             int n_buckets, SmpRule rule, int *__restrict__ ctl)
{
  __shared__ int s_cnt[kSmpMaxBuckets];
  if (threadIdx.x < kSmpMaxBuckets) {
    // (sixteen blocks' counts are loaded before the first prefix is stored: one word at a time, load - store - load, the column
    // of 489 blocks of a 500 k-point cloud took 117 us of memory latency)
    constexpr int kAhead = 16;
    int run = 0;
    if ((int)threadIdx.x < n_buckets)
      for (int b0 = 0; b0 < blocks; b0 += kAhead) {
        int *w = counts + (size_t)b0 * n_buckets + threadIdx.x;
        int c[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) c[u] = b0 + u < blocks ? w[(size_t)u * n_buckets] : 0;
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
          if (b0 + u < blocks) w[(size_t)u * n_buckets] = run;
          run += c[u];
        }
      }
    s_cnt[threadIdx.x] = run;
  }
  __syncthreads();
  if (threadIdx.x >= kWave) return;                         // the rest is the first wave's, all 64 lanes of it
  const int lane = threadIdx.x;
  int c[3], take[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) c[j] = s_cnt[3 * lane + j];   // three consecutive buckets per lane: ascending in (lane, j)
  const int n_valid = wave_sum(c[0] + c[1] + c[2]);
  const int cmax = wave_max_int(max(c[0], max(c[1], c[2])));
  long long m = (long long)(rule.fraction * (double)n_valid);     // floor: the product is >= 0
  if (m > n_valid) m = n_valid;
  if (rule.max_points > 0 && m > rule.max_points) m = rule.max_points;
  if (n_valid > 0 && m < 1) m = 1;
  // the largest L in [0, cmax] with sum min(c_b, L) <= m (the sum never passes n_valid < 2^31)
  int lo = 0, hi = cmax;
  while (lo < hi) {                                         // (wave-uniform)
    const int mid = lo + (hi - lo + 1) / 2;
    const int sum = wave_sum(min(c[0], mid) + min(c[1], mid) + min(c[2], mid));
    if (sum <= m) lo = mid;
    else hi = mid - 1;
  }
  const int L = lo;
#pragma unroll
  for (int j = 0; j < 3; ++j) take[j] = min(c[j], L);
  const int rem = (int)m - wave_sum(take[0] + take[1] + take[2]);
  // what is left goes one each to the buckets with c_b > L, in ascending bucket index
  const int over = (c[0] > L) + (c[1] > L) + (c[2] > L);
  int ahead = wave_scan_incl(over) - over;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (c[j] > L) {
      if (ahead < rem) ++take[j];
      ++ahead;
    }
  const int nonempty = wave_sum((c[0] > 0) + (c[1] > 0) + (c[2] > 0));
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    ctl[3 * lane + j] = c[j];
    ctl[kSmpCtlTake + 3 * lane + j] = take[j];
  }
  if (lane == 0) {
    ctl[kSmpCtlStats + 0] = n_valid;
    ctl[kSmpCtlStats + 1] = (int)m;
    ctl[kSmpCtlStats + 2] = L;
    ctl[kSmpCtlStats + 3] = nonempty;
  }
}

__global__ void __launch_bounds__(256)
k_smp_select(const unsigned char *__restrict__ bucket, int n, int n_buckets, const int *__restrict__ prefix /* [blocks][n_buckets] */,
             const int *__restrict__ ctl, int *__restrict__ flags)
{
  __shared__ int s_hist[4][kSmpMaxBuckets];
  for (int k = threadIdx.x; k < 4 * kSmpMaxBuckets; k += 256) (&s_hist[0][0])[k] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * kSmpPerBlock + wave * kSmpPerWave;
  int key[kSmpRounds], rank[kSmpRounds];
#pragma unroll
  for (int r = 0; r < kSmpRounds; ++r) {
    const long long i = base + r * kWave + lane;
    key[r] = i < n ? (int)bucket[i] : kSmpInvalid;
    rank[r] = smp_wave_rank(key[r], lane, s_hist[wave]);    // among the wave's own points
  }
  __syncthreads();
  // a wave's totals become where its ranks start: the blocks before this one, then the waves before it
  for (int b = threadIdx.x; b < n_buckets; b += 256) {
    int run = prefix[(size_t)blockIdx.x * n_buckets + b];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = s_hist[w][b];
      s_hist[w][b] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSmpRounds; ++r) {
    const long long i = base + r * kWave + lane;
    if (i >= n) continue;
    int keep = 0;
    if (key[r] != kSmpInvalid) {
      const long long rk = (long long)s_hist[wave][key[r]] + rank[r];
      const long long take = ctl[kSmpCtlTake + key[r]], cnt = ctl[key[r]];      // cnt >= 1: the point itself
      keep = ((rk + 1) * take) / cnt > (rk * take) / cnt ? 1 : 0;
    }
    flags[i] = keep;
  }
}

// the kept points' reference indices, in order: the flags' exclusive prefix is a kept point's place
struct SmpFlagLoad {
  const int *flags; size_t n;
  __device__ __forceinline__ int operator()(size_t j) const { return flags[j] ? 1 : 0; }
};
struct SmpIndexStore {
  int *idx;
  __device__ __forceinline__ void operator()(size_t j, int prefix, int v) const { if (v) idx[prefix] = (int)j; }
  __device__ __forceinline__ void done() const {}
};

bool sampling_options_valid(const mm3d_icp_sampling_options *o)
{
  if (o->method != MM3D_ICP_SAMPLE_NONE && o->method != MM3D_ICP_SAMPLE_STRIDE && o->method != MM3D_ICP_SAMPLE_NORMAL_SPACE) return false;
  if (!(o->fraction > 0.0 && o->fraction <= 1.0)) return false;       // (false for NaN)
  if (o->bins != 1 && o->bins != 2 && o->bins != 4 && o->bins != 8) return false;
  return o->max_points >= 0;
}
bool same_options(const mm3d_icp_sampling_options &a, const mm3d_icp_sampling_options &b)
{
  return a.method == b.method && a.fraction == b.fraction && a.max_points == b.max_points && a.bins == b.bins;
}

// The sample of `in` under `o` (STRIDE or NORMAL_SPACE) as a cloud of its own, complete on c's stream after the one wait (its
// size and bounding box).  nrm: one per point under NORMAL_SPACE, not read under STRIDE.  indices (may be null) receives the
// kept points' reference indices on the device.
mm3d_cloud *sample_icp_source(Context *c, const mm3d_cloud *in, const mm3d_normals *nrm, const mm3d_icp_sampling_options &o,
                              mm3d_icp_sampling_stats *stats, DevBuf<int> *indices)
{
  MM3D_REQUIRE(o.method == MM3D_ICP_SAMPLE_STRIDE || o.method == MM3D_ICP_SAMPLE_NORMAL_SPACE, "ICP sampling: no method to sample with");
  MM3D_REQUIRE(in->n < ((size_t)1 << 31), "ICP sampling: more than 2^31 - 1 points");
  const bool by_normals = o.method == MM3D_ICP_SAMPLE_NORMAL_SPACE;
  if (by_normals && (!nrm || nrm->n != in->n)) throw Error(MM3D_EINVAL, "ICP sampling: the normals do not match the points");
  const int n = (int)in->n;
  mm3d_icp_sampling_stats st{n, 0, 0, 0, 0};
  if (n == 0) {
    if (stats) *stats = st;
    if (indices) *indices = DevBuf<int>(c, 0);
    return cloud_from_device(c, DevBuf<float4>(c, 0), 0);
  }
  const SmpRule rule{o.method, o.bins, o.max_points, 1.0f / (float)o.bins, o.fraction};
  const int n_buckets = by_normals ? 3 * o.bins * o.bins : 1;
  const unsigned blocks = div_up((size_t)n, kSmpPerBlock);
  DevBuf<unsigned char> bucket(c, n);
  DevBuf<int> counts(c, (size_t)blocks * n_buckets), ctl(c, kSmpCtlWords), flags(c, n);
  MM3D_LAUNCH(c, "icp_sample_bucket", n * (by_normals ? 33.0 : 17.0), k_smp_bucket, dim3(blocks), dim3(256), 0, in->pts.get(),
              by_normals ? (const float4 *)nrm->nrm.get() : nullptr, n, rule, n_buckets, bucket.get(), counts.get());
  MM3D_LAUNCH(c, "icp_sample_levels", (double)blocks * n_buckets * 8.0, k_smp_levels, dim3(1), dim3(256), 0, counts.get(), (int)blocks,
              n_buckets, rule, ctl.get());
  MM3D_LAUNCH(c, "icp_sample_select", n * 5.0, k_smp_select, dim3(blocks), dim3(256), 0, (const unsigned char *)bucket.get(), n, n_buckets,
              (const int *)counts.get(), (const int *)ctl.get(), flags.get());
  int *h = (int *)c->pin(64);                               // (arrives with the compaction's count: its wait is the one wait)
  MM3D_HIP(hipMemcpyAsync(h, ctl.get() + kSmpCtlStats, 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (indices) {
    *indices = DevBuf<int>(c, n);
    scan_fused(c, "icp_sample_indices", n * 8.0, (size_t)n, SmpFlagLoad{flags.get(), (size_t)n}, SmpIndexStore{indices->get()});
  }
  size_t m = 0;
  std::unique_ptr<mm3d_cloud> res(cloud_of_kept(c, in, flags.get(), false, &m));
  st.valid = h[0]; st.sampled = h[1]; st.level = h[2]; st.buckets = h[3];
  MM3D_REQUIRE(m == (size_t)h[1], "ICP sampling: the kept points are not the budget");
  if (stats) *stats = st;
  return res.release();
}

// the selected sampler: a map's sample lives on the map (map_kept.hpp), fresh only for equal options
struct IcpSampler final : IcpSamplerBase {
  const mm3d_cloud *sample(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p, mm3d_icp_sampling_stats *stats) const override
  {
    const mm3d_icp_sampling_options &o = ctx->sel.sampling_options;
    const IcpSample *s = map_kept(ctx, m, &mm3d_map::icp_sample, [&](const IcpSample &have) { return same_options(have.opt, o); }, [&] {
      const mm3d_normals *nrm = o.method == MM3D_ICP_SAMPLE_NORMAL_SPACE ? map_normals(ctx, m, p) : nullptr;
      std::unique_ptr<IcpSample> made(new IcpSample());
      made->opt = o;
      made->cloud.reset(sample_icp_source(ctx, m->points, nrm, o, &made->stats, nullptr));
      if (made->cloud->n) cloud_hilbert(ctx, made->cloud.get());      // the ICP's query order, before anybody else sees the sample
      return made;
    });
    if (stats) *stats = s->stats;
    return s->cloud.get();
  }
};
const IcpSampler g_sampler;

}  // namespace

}  // namespace mm3d

using namespace mm3d;

extern "C" {

int mm3d_set_icp_sampling(mm3d_ctx *ctx, const mm3d_icp_sampling_options *options)
{
  if (!ctx || !options || !sampling_options_valid(options)) return MM3D_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the selection changes)
  return select_stage(ctx, Stage::Sampling, [&](StageSelection &s) {
    s.sampling_options = *options;
    s.sampler = stage_active(Stage::Sampling, s) ? &g_sampler : nullptr;
  });
}

int mm3d_get_icp_sampling(const mm3d_ctx *ctx, mm3d_icp_sampling_options *options)
{
  if (!ctx || !options) return MM3D_EINVAL;
  *options = ctx->sel.sampling_options;
  return MM3D_OK;
}

int mm3d_last_icp_sampling_stats(const mm3d_ctx *ctx, mm3d_icp_sampling_stats *stats)
{
  if (!ctx || !stats) return MM3D_EINVAL;
  *stats = ctx->last_sampling_stats;
  return MM3D_OK;
}

int mm3d_sample_icp_source(mm3d_ctx *ctx, const mm3d_cloud *points, const mm3d_normals *normals, const mm3d_icp_sampling_options *options,
                           mm3d_cloud **out, int *indices, size_t capacity)
{
  if (!ctx || !points || !options || !out || !sampling_options_valid(options) || options->method == MM3D_ICP_SAMPLE_NONE) return MM3D_EINVAL;
  *out = nullptr;
  if (options->method == MM3D_ICP_SAMPLE_NORMAL_SPACE && !normals) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    DevBuf<int> idx;
    std::unique_ptr<mm3d_cloud> s(sample_icp_source(ctx, points, normals, *options, &ctx->last_sampling_stats, indices ? &idx : nullptr));
    const size_t k = std::min(s->n, capacity);
    if (indices && k) {
      int *h = (int *)ctx->pin(k * sizeof(int));
      MM3D_HIP(hipMemcpyAsync(h, idx.get(), k * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
      ctx->sync();
      std::memcpy(indices, h, k * sizeof(int));
    }
    *out = s.release();
  });
}

int mm3d_estimate_transform_icp_sampled(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_normals *source_normals, const mm3d_cloud *target,
                                        const mm3d_normals *target_normals, const mm3d_icp_sampling_options *options,
                                        const float initial_guess[16], double max_corr_dist, int max_iterations, double eps, float T[16])
{
  if (!ctx || !source || !target || !options || !initial_guess || !T || !sampling_options_valid(options)) return MM3D_EINVAL;
  if (options->method == MM3D_ICP_SAMPLE_NORMAL_SPACE && !source_normals) return MM3D_EINVAL;
  if (target_normals && target_normals->n != target->n) {
    ctx->err = "mm3d_estimate_transform_icp_sampled: the normals do not match the target's points";
    return MM3D_EINVAL;
  }
  return guarded(ctx, [&] {
    // the sample, then the call the caller would have made on it
    std::unique_ptr<mm3d_cloud> s;
    if (options->method != MM3D_ICP_SAMPLE_NONE)
      s.reset(sample_icp_source(ctx, source, source_normals, *options, &ctx->last_sampling_stats, nullptr));
    IcpScoreJob J;
    J.src = s ? s.get() : source; J.tgt = target; J.tgt_normals = target_normals;
    std::memcpy(J.guess_host, initial_guess, sizeof(J.guess_host));
    icp_score_batch(ctx, target_normals ? icp_plane_method() : nullptr, &J, 1, true, max_corr_dist, max_iterations, eps, false, 0.0);
    std::memcpy(T, J.out.T, sizeof(J.out.T));
  });
}

}  // extern "C"

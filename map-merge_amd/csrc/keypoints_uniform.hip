// keypoints_uniform.hip -- uniform keypoints on gfx950: one cloud point per occupied voxel of the global lattice, the point
// nearest its voxel's centre (mm3d_uniform_keypoints, mm3d_set_keypoints; include/mm3d.h states the rule to the operation).
// Not a reference stage: the reference only offers SIFT and Harris.
//
// One pass family per cloud, nothing read back but the keypoint count:
//   k_ukp_range   the voxel index range of the finite points (ordered-uint atomics, one set per block)
//   k_ukp_keys    a lane per point, one coalesced 16-byte load: voxel key relative to the range's minimum, float bits of d2
//   radix sort    (key, input index) pairs, stable: the voxels become runs, in any launch geometry the same runs
//   scan_fused    run heads -> the voxel number of every sorted position
//   k_ukp_winner  a lane per sorted position: segmented wave minimum of float_bits(d2) << 32 | index over the lanes of one
//                 voxel, then ONE 64-bit atomicMin per (wave, voxel) -- a voxel of 10 000 points costs 157 atomics, not a
//                 10 000-step loop of one thread.  Integer minima: the result does not depend on the order they arrive in.
//   k_ukp_mark    a lane per voxel: flag its winner's input index
//   compact       the library's ordered compaction of the flagged records (grid.hip::compact_points), whose count is the
//                 one host wait
// The extent rule (index range product > INT32_MAX: every finite point is a keypoint) is decided on the device from the range
// words, by every lane for itself, so the host never waits for the range.
#include <cmath>
#include <cstring>

#include "capi_guard.hpp"
#include "drivers.hpp"
#include "device_util.hpp"
#include "scan_fused.hpp"

namespace mm3d {

namespace {

constexpr uint32_t kUkpInvalid = 0xFFFFFFFFu;

// the voxel index of one coordinate, as a float: floor of ONE float multiply (filters.hip forms VoxelGrid's keys the same way)
__device__ __forceinline__ float ukp_index(float x, float inv) { return floorf(__fmul_rn(x, inv)); }

// What the range words say: the minimum index per axis, the key multipliers, and the extent rule.  The indices are
// integer-valued floats, so their differences are exact in double wherever the product is small enough to matter.
struct UkpFrame { double mn[3]; unsigned mul1, mul2; bool overflow; };
__device__ __forceinline__ UkpFrame ukp_frame(const unsigned *__restrict__ range)
{
  UkpFrame f;
  double d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    f.mn[a] = (double)ord2f(range[a]);
    d[a] = ((double)ord2f(range[3 + a]) - f.mn[a]) + 1.0;
  }
  f.overflow = !((d[0] * d[1]) * d[2] <= 2147483647.0);      // (an infinite index makes this inf or NaN: the rule applies)
  f.mul1 = f.overflow ? 0u : (unsigned)d[0];
  f.mul2 = f.overflow ? 0u : (unsigned)(d[0] * d[1]);
  return f;
}

__global__ void __launch_bounds__(256)
k_ukp_range(const float4 *__restrict__ pts, int n, float inv, unsigned *__restrict__ range /* min i j k, max i j k (ordered) */)
{
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int cnt = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 p = pts[i];
    if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) continue;
    const float f[3] = {ukp_index(p.x, inv), ukp_index(p.y, inv), ukp_index(p.z, inv)};
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], f[a]); hi[a] = fmaxf(hi[a], f[a]); }
    ++cnt;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) { lo[a] = wave_min_f(lo[a]); hi[a] = wave_max_f(hi[a]); }
  cnt = wave_sum(cnt);
  __shared__ float s_lo[4][3], s_hi[4][3];
  __shared__ int s_cnt[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { s_lo[wave][a] = lo[a]; s_hi[wave][a] = hi[a]; }
    s_cnt[wave] = cnt;                                   // (lane 0 holds the wave's sum)
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3] > 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float l = s_lo[0][a], h = s_hi[0][a];
      for (int w = 1; w < 4; ++w) { l = fminf(l, s_lo[w][a]); h = fmaxf(h, s_hi[w][a]); }
      atomicMin(&range[a], f2ord(l));
      atomicMax(&range[3 + a], f2ord(h));
    }
  }
}

__global__ void __launch_bounds__(256)
k_ukp_keys(const float4 *__restrict__ pts, int n, float inv, float leaf, const unsigned *__restrict__ range, uint32_t *__restrict__ keys,
           uint32_t *__restrict__ vals, uint32_t *__restrict__ d2bits)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  vals[i] = (uint32_t)i;
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) { keys[i] = kUkpInvalid; d2bits[i] = kUkpInvalid; return; }
  const float fi = ukp_index(p.x, inv), fj = ukp_index(p.y, inv), fk = ukp_index(p.z, inv);
  const float dx = __fsub_rn(p.x, __fmul_rn(__fadd_rn(fi, 0.5f), leaf));
  const float dy = __fsub_rn(p.y, __fmul_rn(__fadd_rn(fj, 0.5f), leaf));
  const float dz = __fsub_rn(p.z, __fmul_rn(__fadd_rn(fk, 0.5f), leaf));
  d2bits[i] = __float_as_uint(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));   // >= +0 or +inf: the bits ascend with it
  const UkpFrame f = ukp_frame(range);
  uint32_t key = 0;                                       // (under the extent rule the runs are not read)
  if (!f.overflow)
    key = (uint32_t)((double)fi - f.mn[0]) + (uint32_t)((double)fj - f.mn[1]) * f.mul1 + (uint32_t)((double)fk - f.mn[2]) * f.mul2;
  keys[i] = key;
}

// a voxel starts where the sorted key changes; the non-finite points' key sorts last and starts nothing
struct UkpHeadLoad {
  const uint32_t *keys; int n;
  __device__ __forceinline__ int operator()(size_t j) const
  {
    const uint32_t k = keys[j];
    return (k != kUkpInvalid && (j == 0 || keys[j - 1] != k)) ? 1 : 0;
  }
};
struct UkpVoxelStore {
  int *voxel;
  __device__ __forceinline__ void operator()(size_t j, int prefix, int v) const { voxel[j] = prefix + v - 1; }
  __device__ __forceinline__ void done() const {}
};

__global__ void __launch_bounds__(256)
k_ukp_winner(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ order, const uint32_t *__restrict__ d2bits,
             const int *__restrict__ voxel, int n, const unsigned *__restrict__ range, unsigned long long *__restrict__ best,
             int *__restrict__ flags)
{
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const uint32_t key = j < n ? keys[j] : kUkpInvalid;
  const uint32_t idx = j < n ? order[j] : 0u;
  if (ukp_frame(range).overflow) {                        // (the same for every lane of the grid)
    if (key != kUkpInvalid) flags[idx] = 1;
    return;
  }
  unsigned long long m = key != kUkpInvalid ? ((unsigned long long)d2bits[idx] << 32) | idx : ~0ull;
  // inclusive segmented minimum: equal keys are neighbours, so "the lane o below has my key" means "and so has every lane between"
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const uint32_t k2 = __shfl_up(key, o, kWave);
    const unsigned long long m2 = __shfl_up(m, o, kWave);
    if (lane >= o && k2 == key && m2 < m) m = m2;
  }
  const uint32_t next = __shfl_down(key, 1, kWave);
  if (key != kUkpInvalid && (lane == kWave - 1 || next != key)) atomicMin(&best[voxel[j]], m);
}

__global__ void __launch_bounds__(256)
k_ukp_mark(const unsigned long long *__restrict__ best, int n, int *__restrict__ flags)
{
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const unsigned long long b = best[v];
  if (b != ~0ull) flags[(uint32_t)b] = 1;                 // (the low word is an input index < n)
}

// leaf as the rule reads it: a positive finite float with a finite reciprocal
bool ukp_leaf_ok(double leaf)
{
  if (!(leaf > 0.0) || !std::isfinite(leaf)) return false;
  const float lf = (float)leaf;
  return lf > 0.0f && std::isfinite(lf) && std::isfinite(1.0f / lf);
}

mm3d_cloud *uniform_keypoints(Context *c, const mm3d_cloud *in, double leaf_d)
{
  MM3D_REQUIRE(ukp_leaf_ok(leaf_d), "uniform keypoints: the leaf must be positive and finite, as a float and its reciprocal too");
  MM3D_REQUIRE(in->n < ((size_t)1 << 31), "uniform keypoints: more than 2^31 - 1 points");
  const int n = (int)in->n;
  if (n == 0) return cloud_from_device(c, DevBuf<float4>(c, 0), 0);
  const float leaf = (float)leaf_d, inv = 1.0f / leaf;
  const unsigned blocks = div_up((size_t)n, 256);

  DevBuf<unsigned> range(c, 8);
  unsigned *h = (unsigned *)c->pin(64);
  std::memcpy(h, kBoxInit, sizeof(kBoxInit));             // min words FFFFFFFF, max words 0 (device_util.hpp::f2ord)
  MM3D_HIP(hipMemcpyAsync(range.get(), h, sizeof(kBoxInit), hipMemcpyHostToDevice, c->stream));
  MM3D_LAUNCH(c, "ukp_range", n * 16.0, k_ukp_range, dim3(std::min<unsigned>(div_up((size_t)n, 256 * 8), 512)), dim3(256), 0, in->pts.get(), n,
              inv, range.get());
  DevBuf<uint32_t> keys(c, n), vals(c, n), keys2(c, n), vals2(c, n), d2bits(c, n);
  MM3D_LAUNCH(c, "ukp_keys", n * 28.0, k_ukp_keys, dim3(blocks), dim3(256), 0, in->pts.get(), n, inv, leaf, (const unsigned *)range.get(),
              keys.get(), vals.get(), d2bits.get());
  sort_pairs_u32(c, keys.get(), keys2.get(), vals.get(), vals2.get(), (size_t)n, 32);
  DevBuf<int> voxel(c, n), flags(c, n);
  DevBuf<unsigned long long> best(c, n);                  // (at most one voxel per point)
  scan_fused(c, "ukp_voxels", n * 8.0, (size_t)n, UkpHeadLoad{keys2.get(), n}, UkpVoxelStore{voxel.get()});
  MM3D_HIP(hipMemsetAsync(best.get(), 0xFF, (size_t)n * sizeof(unsigned long long), c->stream));
  MM3D_HIP(hipMemsetAsync(flags.get(), 0, (size_t)n * sizeof(int), c->stream));
  MM3D_LAUNCH(c, "ukp_winner", n * 24.0, k_ukp_winner, dim3(blocks), dim3(256), 0, (const uint32_t *)keys2.get(), (const uint32_t *)vals2.get(),
              (const uint32_t *)d2bits.get(), (const int *)voxel.get(), n, (const unsigned *)range.get(), best.get(), flags.get());
  MM3D_LAUNCH(c, "ukp_mark", n * 12.0, k_ukp_mark, dim3(blocks), dim3(256), 0, (const unsigned long long *)best.get(), n, flags.get());
  DevBuf<float4> out;
  unsigned box[7];
  const size_t m = compact_points(c, in->pts.get(), flags.get(), (size_t)n, out, box);   // the one wait: the count, and the keypoints' box with it
  if ((size_t)n >= ((size_t)1 << 20) && m * 2 < (size_t)n) {     // as in the filters: a large, mostly empty bound-sized buffer is not kept
    DevBuf<float4> fit(c, m);
    if (m) MM3D_HIP(hipMemcpyAsync(fit.get(), out.get(), m * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    c->settle();
    out = std::move(fit);
  }
  mm3d_cloud *res = cloud_from_device(c, std::move(out), m);
  cloud_set_bbox(res, box);
  return res;
}

struct KeypointsUniform final : KeypointSourceBase {
  int source() const override { return MM3D_KEYPOINTS_UNIFORM; }
  mm3d_cloud *keypoints(Context *c, const mm3d_cloud *points, double leaf) const override { return uniform_keypoints(c, points, leaf); }
};
const KeypointsUniform g_uniform;

bool options_ok(const mm3d_keypoint_options *o)
{
  if (!o || (o->source != MM3D_KEYPOINTS_REFERENCE && o->source != MM3D_KEYPOINTS_UNIFORM)) return false;
  return o->leaf == 0.0 || ukp_leaf_ok(o->leaf);
}

}  // namespace

}  // namespace mm3d

using namespace mm3d;

extern "C" {

int mm3d_uniform_keypoints(mm3d_ctx *ctx, const mm3d_cloud *points, double leaf, mm3d_cloud **out)
{
  if (!ctx || !points || !out) return MM3D_EINVAL;
  *out = nullptr;
  return guarded(ctx, [&] { *out = uniform_keypoints(ctx, points, leaf); });
}

int mm3d_set_keypoints(mm3d_ctx *ctx, const mm3d_keypoint_options *options)
{
  if (!ctx || !options_ok(options)) return MM3D_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the source changes)
  // (features travel in the bundles, so device lists carry the option: the peers follow)
  select_stages(ctx, true, [&](StageSelection &s) {
    s.keypoints = options->source == MM3D_KEYPOINTS_UNIFORM ? &g_uniform : nullptr;
    s.keypoint_options = *options;
  });
  return MM3D_OK;
}

int mm3d_get_keypoints(const mm3d_ctx *ctx, mm3d_keypoint_options *options)
{
  if (!ctx || !options) return MM3D_EINVAL;
  *options = ctx->sel.keypoint_options;
  return MM3D_OK;
}

}  // extern "C"

// keypoints_uniform.hip -- uniform keypoints on gfx950: one cloud point per occupied voxel of the global lattice, the point
// nearest its voxel's centre (mm3d_uniform_keypoints, mm3d_set_keypoints; include/mm3d.h states the rule to the operation).
// Not a reference stage: the reference only offers SIFT and Harris.
//
// One pass family per cloud, nothing read back but the keypoint count:
//   ukp_range     the voxel index range of the finite points (lattice.hpp::k_lattice_range, as every stage of the global lattice)
//   k_ukp_keys    a lane per point, one coalesced 16-byte load: voxel key relative to the range's minimum, float bits of d2
//   radix sort    (key, input index) pairs, stable: the voxels become runs, in any launch geometry the same runs
//   scan_fused    run heads (lattice.hpp::LatticeRunHead) -> the voxel number of every sorted position
//   k_ukp_winner  a lane per sorted position: segmented wave minimum of float_bits(d2) << 32 | index over the lanes of one
//                 voxel, then ONE 64-bit atomicMin per (wave, voxel) -- a voxel of 10 000 points costs 157 atomics, not a
//                 10 000-step loop of one thread.  Integer minima: the result does not depend on the order they arrive in.
//   k_ukp_mark    a lane per voxel: flag its winner's input index
//   compact       the library's ordered compaction of the flagged records (grid.hip::cloud_of_kept), whose count is the
//                 one host wait
// The extent rule (index range product > INT32_MAX: every finite point is a keypoint) is decided on the device from the range
// words, by every lane for itself, so the host never waits for the range.
#include "capi_guard.hpp"
#include "drivers.hpp"
#include "lattice.hpp"
#include "scan_fused.hpp"

namespace mm3d {

namespace {

// The extent rule: a box of more than INT32_MAX voxels gets no keys, and every finite point is a keypoint (an infinite index,
// or a range that no point has touched, makes the product inf or NaN: the rule applies)
__device__ __forceinline__ bool ukp_extent_rule(const LatticeFrame<3> &f) { return !(f.cells <= 2147483647.0); }

__global__ void __launch_bounds__(256)
k_ukp_keys(const float4 *__restrict__ pts, int n, float inv, float leaf, const unsigned *__restrict__ range, uint32_t *__restrict__ keys,
           uint32_t *__restrict__ vals, uint32_t *__restrict__ d2bits)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  vals[i] = (uint32_t)i;
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) { keys[i] = kLatticeInvalid; d2bits[i] = kLatticeInvalid; return; }
  const float fi = lattice_index(p.x, inv), fj = lattice_index(p.y, inv), fk = lattice_index(p.z, inv);
  const float dx = __fsub_rn(p.x, __fmul_rn(__fadd_rn(fi, 0.5f), leaf));
  const float dy = __fsub_rn(p.y, __fmul_rn(__fadd_rn(fj, 0.5f), leaf));
  const float dz = __fsub_rn(p.z, __fmul_rn(__fadd_rn(fk, 0.5f), leaf));
  d2bits[i] = __float_as_uint(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));   // >= +0 or +inf: the bits ascend with it
  const LatticeFrame<3> f = lattice_frame<3>(range);
  uint32_t key = 0;                                       // (under the extent rule the runs are not read)
  if (!ukp_extent_rule(f))                                // x fastest: i + j * d0 + k * d0 * d1
    key = (uint32_t)((double)fi - f.mn[0]) + (uint32_t)((double)fj - f.mn[1]) * (unsigned)f.d[0] +
          (uint32_t)((double)fk - f.mn[2]) * (unsigned)(f.d[0] * f.d[1]);
  keys[i] = key;
}

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
  const uint32_t key = j < n ? keys[j] : kLatticeInvalid;
  const uint32_t idx = j < n ? order[j] : 0u;
  if (ukp_extent_rule(lattice_frame<3>(range))) {         // (the same for every lane of the grid)
    if (key != kLatticeInvalid) flags[idx] = 1;
    return;
  }
  unsigned long long m = key != kLatticeInvalid ? ((unsigned long long)d2bits[idx] << 32) | idx : ~0ull;
  // inclusive segmented minimum: equal keys are neighbours, so "the lane o below has my key" means "and so has every lane between"
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const uint32_t k2 = __shfl_up(key, o, kWave);
    const unsigned long long m2 = __shfl_up(m, o, kWave);
    if (lane >= o && k2 == key && m2 < m) m = m2;
  }
  const uint32_t next = __shfl_down(key, 1, kWave);
  if (key != kLatticeInvalid && (lane == kWave - 1 || next != key)) atomicMin(&best[voxel[j]], m);
}

__global__ void __launch_bounds__(256)
k_ukp_mark(const unsigned long long *__restrict__ best, int n, int *__restrict__ flags)
{
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const unsigned long long b = best[v];
  if (b != ~0ull) flags[(uint32_t)b] = 1;                 // (the low word is an input index < n)
}

mm3d_cloud *uniform_keypoints(Context *c, const mm3d_cloud *in, double leaf_d)
{
  MM3D_REQUIRE(lattice_side_ok(leaf_d), "uniform keypoints: the leaf must be positive and finite, as a float and its reciprocal too");
  MM3D_REQUIRE(in->n < ((size_t)1 << 31), "uniform keypoints: more than 2^31 - 1 points");
  const int n = (int)in->n;
  if (n == 0) return cloud_from_device(c, DevBuf<float4>(c, 0), 0);
  const float leaf = (float)leaf_d, inv = 1.0f / leaf;
  const unsigned blocks = div_up((size_t)n, 256);

  DevBuf<unsigned> range(c, 8);
  lattice_range<3>(c, "ukp_range", n * 16.0, in->pts.get(), n, inv, LatticeFinite{}, range.get());
  DevBuf<uint32_t> keys(c, n), vals(c, n), keys2(c, n), vals2(c, n), d2bits(c, n);
  MM3D_LAUNCH(c, "ukp_keys", n * 28.0, k_ukp_keys, dim3(blocks), dim3(256), 0, in->pts.get(), n, inv, leaf, (const unsigned *)range.get(),
              keys.get(), vals.get(), d2bits.get());
  sort_pairs_u32(c, keys.get(), keys2.get(), vals.get(), vals2.get(), (size_t)n, 32);
  DevBuf<int> voxel(c, n), flags(c, n);
  DevBuf<unsigned long long> best(c, n);                  // (at most one voxel per point)
  scan_fused(c, "ukp_voxels", n * 8.0, (size_t)n, LatticeRunHead{keys2.get()}, UkpVoxelStore{voxel.get()});
  MM3D_HIP(hipMemsetAsync(best.get(), 0xFF, (size_t)n * sizeof(unsigned long long), c->stream));
  MM3D_HIP(hipMemsetAsync(flags.get(), 0, (size_t)n * sizeof(int), c->stream));
  MM3D_LAUNCH(c, "ukp_winner", n * 24.0, k_ukp_winner, dim3(blocks), dim3(256), 0, (const uint32_t *)keys2.get(), (const uint32_t *)vals2.get(),
              (const uint32_t *)d2bits.get(), (const int *)voxel.get(), n, (const unsigned *)range.get(), best.get(), flags.get());
  MM3D_LAUNCH(c, "ukp_mark", n * 12.0, k_ukp_mark, dim3(blocks), dim3(256), 0, (const unsigned long long *)best.get(), n, flags.get());
  return cloud_of_kept(c, in, flags.get(), false);       // the one wait: the count, and the keypoints' box with it
}

struct KeypointsUniform final : KeypointSourceBase {
  int source() const override { return MM3D_KEYPOINTS_UNIFORM; }
  mm3d_cloud *keypoints(Context *c, const mm3d_cloud *points, double leaf) const override { return uniform_keypoints(c, points, leaf); }
};
const KeypointsUniform g_uniform;

bool options_ok(const mm3d_keypoint_options *o)
{
  if (!o || (o->source != MM3D_KEYPOINTS_REFERENCE && o->source != MM3D_KEYPOINTS_UNIFORM)) return false;
  return o->leaf == 0.0 || lattice_side_ok(o->leaf);
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
  return select_stage(ctx, Stage::Keypoints, [&](StageSelection &s) {
    s.keypoint_options = *options;
    s.keypoints = stage_active(Stage::Keypoints, s) ? &g_uniform : nullptr;
  });
}

int mm3d_get_keypoints(const mm3d_ctx *ctx, mm3d_keypoint_options *options)
{
  if (!ctx || !options) return MM3D_EINVAL;
  *options = ctx->sel.keypoint_options;
  return MM3D_OK;
}

}  // extern "C"

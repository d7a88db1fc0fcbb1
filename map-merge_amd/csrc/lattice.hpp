// lattice.hpp -- the global lattice of the voxel stages: the cell index of a coordinate is floor(x * inv), the same cells
// whatever the cloud.  Uniform keypoints (keypoints_uniform.hip), the NDT voxel table (ndt.hip) and the correlative signature
// (align_correlative.hip) open alike -- the index range of the counted points, keys relative to its minimum, a radix sort, run
// heads through scan_fused -- and VoxelGrid (filters.hip) and the overlap confidence (confidence_overlap.hip) form the same
// index.  Host and device code; one text for all of them, so that the stages cannot come to disagree about which cell a point
// is in, which range words mean "no point", or what a usable cell side is.
//
// The key of a cell stays with its stage: x fastest for the keypoints, i most significant for NDT (its records' order), the
// class bit for the correlative signature.  So do the sort's buffers, which two of the stages read long after the sort.
#pragma once

#include <algorithm>
#include <cmath>

#include "device_util.hpp"

namespace mm3d {

// the key of a point that is in no cell: it sorts last and starts no run
constexpr uint32_t kLatticeInvalid = 0xFFFFFFFFu;

// the cell index of one coordinate, as a float: floor of ONE float multiply (VoxelGrid's, bit for bit; the tree is built
// without contraction, so the host's product rounds as the device's)
__host__ __device__ __forceinline__ float lattice_index(float x, float inv)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return floorf(__fmul_rn(x, inv));
#else
  return floorf(x * inv);
#endif
}

// a cell side as the stages' rules read it: a positive finite float with a finite reciprocal
inline bool lattice_side_ok(double side)
{
  if (!(side > 0.0) || !std::isfinite(side)) return false;
  const float f = (float)side;
  return f > 0.0f && std::isfinite(f) && std::isfinite(1.0f / f);
}

// What the range words say (minima at [0, AXES), maxima at [AXES, 2 AXES), ordered uints): the minimum index and the extent
// per axis, and the number of cells in the box.  The indices are integer-valued floats, so their differences are exact in
// double wherever the product is small enough to matter; an infinite index, or words that no point has touched, make the
// product inf or NaN, which no stage's limit admits (!(cells <= limit)).
template <int AXES> struct LatticeFrame { double mn[AXES], d[AXES], cells; };
template <int AXES> __host__ __device__ __forceinline__ LatticeFrame<AXES> lattice_frame(const unsigned *range)
{
  LatticeFrame<AXES> f;
#pragma unroll
  for (int a = 0; a < AXES; ++a) {
    f.mn[a] = (double)ord2f(range[a]);
    f.d[a] = ((double)ord2f(range[AXES + a]) - f.mn[a]) + 1.0;
  }
  f.cells = f.d[0];
#pragma unroll
  for (int a = 1; a < AXES; ++a) f.cells *= f.d[a];
  return f;
}

// the points a stage counts when nothing but the point decides: the finite ones
struct LatticeFinite {
  __device__ __forceinline__ bool operator()(int, const float4 &p) const { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }
};

// The index range of the counted points over the first AXES coordinates: ordered-uint atomics, one set per block, and a block
// with no counted point touches nothing (its minima would be +inf).  256 threads, any grid.
template <int AXES, class Counted>
__global__ void __launch_bounds__(256)
k_lattice_range(const float4 *__restrict__ pts, int n, float inv, Counted counted, unsigned *__restrict__ range)
{
  float lo[AXES], hi[AXES];
#pragma unroll
  for (int a = 0; a < AXES; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
  int cnt = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 p = pts[i];
    if (!counted(i, p)) continue;
    const float xyz[3] = {p.x, p.y, p.z};
#pragma unroll
    for (int a = 0; a < AXES; ++a) {
      const float f = lattice_index(xyz[a], inv);
      lo[a] = fminf(lo[a], f);
      hi[a] = fmaxf(hi[a], f);
    }
    ++cnt;
  }
#pragma unroll
  for (int a = 0; a < AXES; ++a) { lo[a] = wave_min_f(lo[a]); hi[a] = wave_max_f(hi[a]); }
  cnt = wave_sum(cnt);
  __shared__ float s_lo[4][AXES], s_hi[4][AXES];
  __shared__ int s_cnt[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < AXES; ++a) { s_lo[wave][a] = lo[a]; s_hi[wave][a] = hi[a]; }
    s_cnt[wave] = cnt;                                   // (lane 0 holds the wave's sum)
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3] > 0) {
#pragma unroll
    for (int a = 0; a < AXES; ++a) {
      float l = s_lo[0][a], h = s_hi[0][a];
      for (int w = 1; w < 4; ++w) { l = fminf(l, s_lo[w][a]); h = fmaxf(h, s_hi[w][a]); }
      atomicMin(&range[a], f2ord(l));
      atomicMax(&range[AXES + a], f2ord(h));
    }
  }
}

// Enqueues the range of pts[0, n) into range[0, 2 AXES) and zeroes the words behind it up to eight, which the stages use for
// their counts.  No wait: whoever needs the range on the host reads the words back with what else it waits for.
template <int AXES, class Counted>
void lattice_range(Context *c, const char *label, double bytes, const float4 *pts, int n, float inv, Counted counted, unsigned *range)
{
  unsigned *h = (unsigned *)c->pin(64);
  for (int w = 0; w < 8; ++w) h[w] = w < AXES ? 0xFFFFFFFFu : 0u;      // (device_util.hpp::f2ord: above every minimum, below every maximum)
  MM3D_HIP(hipMemcpyAsync(range, h, 8 * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
  const auto kernel = &k_lattice_range<AXES, Counted>;
  MM3D_LAUNCH(c, label, bytes, kernel, dim3(std::min<unsigned>(div_up((size_t)n, 256 * 8), 512)), dim3(256), 0, pts, n, inv, counted, range);
}

// a cell starts where the sorted key changes; the key of the points in no cell sorts last and starts nothing
struct LatticeRunHead {
  const uint32_t *keys;
  __device__ __forceinline__ int operator()(size_t j) const
  {
    const uint32_t k = keys[j];
    return (k != kLatticeInvalid && (j == 0 || keys[j - 1] != k)) ? 1 : 0;
  }
};

}  // namespace mm3d

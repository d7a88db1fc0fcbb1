// map_cache.hip -- the device part of the map cache of mm3d_estimate_maps_transforms (map_cache.cpp, mm3d_set_map_cache).
//
// Whether a map is unchanged since an earlier call is decided on the packed records cloud_from_memory just uploaded
// (float4 {x, y, z, rgba-bits}): ONE pass reads them -- together with the cached records the slot held last time, when
// there are as many -- and gives a 128-bit digest (which cached entry to compare with, when that was not the slot's) and
// the exact verdict "every record equal, bit for bit".  A hit always rests on that verdict; the digest only picks the
// candidate.  16 B per point read (32 B with the candidate): HBM-bound, so 256-thread blocks of dwordx4 loads, at most
// 2048 blocks striding over the cloud.
#include <algorithm>

#include "device_util.hpp"

namespace mm3d {

namespace {

constexpr int kDigestBlock = 256;
constexpr unsigned kDigestMaxBlocks = 2048;

__device__ __forceinline__ unsigned long long fmix64(unsigned long long x)
{
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

}  // namespace

// out[0], out[1]: the digest, wrapping sums over the records of two independent mixes of (record bits, index) -- integer
// sums, so the launch order does not matter, and the index in the mix makes a permutation count; out[2] != 0: some record
// differs from `hint`'s (hint != null).  out is zero on entry.
template <bool kDigest>
__global__ __launch_bounds__(kDigestBlock) void k_cloud_digest_compare(const uint4 *__restrict__ a, const uint4 *__restrict__ hint, size_t n,
                                                                      unsigned long long *__restrict__ out)
{
  unsigned long long h0 = 0, h1 = 0;
  bool differ = false;
  const size_t step = (size_t)gridDim.x * kDigestBlock;
  for (size_t i = (size_t)blockIdx.x * kDigestBlock + threadIdx.x; i < n; i += step) {
    const uint4 r = a[i];
    if (kDigest) {
      const unsigned long long lo = (unsigned long long)r.x | ((unsigned long long)r.y << 32);
      const unsigned long long hi = (unsigned long long)r.z | ((unsigned long long)r.w << 32);
      const unsigned long long ix = (unsigned long long)i;
      h0 += fmix64(lo ^ fmix64(hi + ix * 0x9e3779b97f4a7c15ull));
      h1 += fmix64(hi * 0xd6e8feb86659fd93ull ^ fmix64(lo + (ix ^ 0xa0761d6478bd642full) * 0xe7037ed1a0b428dbull));
    }
    if (hint) {
      const uint4 q = hint[i];
      differ |= (r.x != q.x) | (r.y != q.y) | (r.z != q.z) | (r.w != q.w);
    }
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (hint) {                                               // (uniform: every lane of the block gets here)
    const unsigned long long m = __ballot(differ);
    if (m != 0ull && lane == 0) atomicOr(out + 2, 1ull);
  }
  if (kDigest) {
    for (int o = kWave / 2; o > 0; o >>= 1) {
      h0 += __shfl_xor(h0, o, kWave);
      h1 += __shfl_xor(h1, o, kWave);
    }
    // the block's four waves meet in LDS: one 64-bit atomic per block and word (not per wave) on the two words everybody adds to
    __shared__ unsigned long long part[2][kDigestBlock / kWave];
    if (lane == 0) { part[0][wave] = h0; part[1][wave] = h1; }
    __syncthreads();
    if (threadIdx.x < 2) {
      unsigned long long s = 0;
      for (int w = 0; w < kDigestBlock / kWave; ++w) s += part[threadIdx.x][w];
      atomicAdd(out + threadIdx.x, s);
    }
  }
}

CloudDigest cloud_digest_compare(Context *c, const float4 *a, const float4 *hint, size_t n, bool want_digest)
{
  CloudDigest d;
  if (n == 0) return d;
  DevBuf<unsigned long long> res(c, 4);
  MM3D_HIP(hipMemsetAsync(res.get(), 0, 4 * sizeof(unsigned long long), c->stream));
  const unsigned blocks = std::min<unsigned>(div_up(n, kDigestBlock), kDigestMaxBlocks);
  const double bytes = (double)n * 16.0 * (hint ? 2.0 : 1.0);
  if (want_digest)
    MM3D_LAUNCH(c, "cloud_digest_compare", bytes, k_cloud_digest_compare<true>, dim3(blocks), dim3(kDigestBlock), 0, (const uint4 *)a,
                (const uint4 *)hint, n, res.get());
  else
    MM3D_LAUNCH(c, "cloud_digest_compare", bytes, k_cloud_digest_compare<false>, dim3(blocks), dim3(kDigestBlock), 0, (const uint4 *)a,
                (const uint4 *)hint, n, res.get());
  auto *h = (unsigned long long *)c->pin(4 * sizeof(unsigned long long));
  MM3D_HIP(hipMemcpyAsync(h, res.get(), 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  c->sync();
  d.h0 = h[0];
  d.h1 = h[1];
  d.equal = hint != nullptr && h[2] == 0;
  return d;
}

}  // namespace mm3d

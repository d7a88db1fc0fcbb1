// fake_digest.cpp -- TEST INFRASTRUCTURE: a host stand-in for map_cache.hip's cloud_digest_compare (types.hpp), so that the
// map cache (map_cache.cpp) and the drivers that use it (driver_streams.cpp) run under the sanitizers on tests/host_san's fake device
// layer, where "device" memory is host memory.  Nothing here is product code.
#include <cstring>

#include "types.hpp"

namespace mm3d {

static unsigned long long fmix64(unsigned long long x)
{
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}

CloudDigest cloud_digest_compare(Context *c, const float4 *a, const float4 *hint, size_t n, bool want_digest)
{
  // TEST KNOB: a map of exactly this many points makes the cache's device pass fail (a call that throws half-way)
  if (const char *e = getenv("MM3D_FAKE_DIGEST_FAIL_POINTS"))
    if ((size_t)atol(e) == n) throw Error(MM3D_EDEVICE, "fake device failure in cloud_digest_compare");
  CloudDigest d;
  bool differ = false;
  for (size_t i = 0; i < n; ++i) {
    unsigned long long lo, hi;
    std::memcpy(&lo, &a[i].x, 8);
    std::memcpy(&hi, &a[i].z, 8);
    if (want_digest) {
      d.h0 += fmix64(lo ^ fmix64(hi + i * 0x9e3779b97f4a7c15ull));
      d.h1 += fmix64(hi * 0xd6e8feb86659fd93ull ^ fmix64(lo + (i ^ 0xa0761d6478bd642full) * 0xe7037ed1a0b428dbull));
    }
    if (hint && std::memcmp(&a[i], &hint[i], 16) != 0) differ = true;
  }
  d.equal = hint != nullptr && !differ;
  c->sync();
  return d;
}

}  // namespace mm3d

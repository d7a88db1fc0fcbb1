// cache_main.cpp -- TEST INFRASTRUCTURE: drives mm3d_estimate_maps_transforms with the map cache on (mm3d_set_map_cache) on the
// fake device layer of tests/host_san, on 1 and 3 streams, beside a plain context in lock-step: repeats, changed maps, reordered
// maps, eviction, parameter changes, SAC_IA with and without mm3d_srand, and calls that fail half-way -- every call's
// transforms, pair records and map sizes must be the plain context's bits, and the cache's counters exact.  Built with
// -fsanitize=thread or -fsanitize=address,undefined by tests/host_san_cache/build.sh; exit code 0 = every check passed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mm3d.h"

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("CHECK failed at line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

struct Pt { float x, y, z; uint32_t rgba; };
static std::vector<Pt> make_cloud(int n, unsigned seed)
{
  std::vector<Pt> v(n);
  uint32_t s = seed * 2654435761u + 12345u;
  auto u = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; };
  for (int i = 0; i < n; ++i) { v[i] = Pt{u() * 20.f + (float)seed, u() * 20.f, u() * 2.f, 0xff000000u | (s >> 8)}; }
  return v;
}

struct Result {
  int status = 0;
  size_t n_out = 0, n_pairs = 0;
  std::vector<float> T;
  std::vector<mm3d_pair_result> pairs;
  std::vector<size_t> pts, kps;
};

static Result run(mm3d_ctx *c, const std::vector<std::vector<Pt>> &clouds, const mm3d_params &p)
{
  Result r;
  const size_t n = clouds.size();
  std::vector<mm3d_cloud_view> views;
  for (auto &cl : clouds) views.push_back(mm3d_cloud_view{cl.data(), cl.size(), sizeof(Pt), 12});
  r.T.assign(n * 16, 0.f);
  r.pairs.assign(n * (n - 1) / 2 + 1, mm3d_pair_result{});
  std::memset(r.pairs.data(), 0, r.pairs.size() * sizeof(mm3d_pair_result));
  r.status = mm3d_estimate_maps_transforms(c, views.data(), n, &p, r.T.data(), &r.n_out, r.pairs.data(), &r.n_pairs);
  r.pts.assign(n, 0);
  r.kps.assign(n, 0);
  mm3d_last_run_map_sizes(c, r.pts.data(), r.kps.data(), n);
  return r;
}

static bool same(const Result &a, const Result &b)
{
  return a.status == MM3D_OK && b.status == MM3D_OK && a.n_out == b.n_out && a.n_pairs == b.n_pairs &&
         std::memcmp(a.T.data(), b.T.data(), a.n_out * 16 * sizeof(float)) == 0 &&
         std::memcmp(a.pairs.data(), b.pairs.data(), a.n_pairs * sizeof(mm3d_pair_result)) == 0 && a.pts == b.pts && a.kps == b.kps;
}

// one call on both contexts (re-seeded first when seed != 0); the caching one's counters of the call come back in st
static size_t lockstep(mm3d_ctx *cached, mm3d_ctx *plain, const std::vector<std::vector<Pt>> &clouds, const mm3d_params &p, long long st[6],
                       unsigned seed = 0)
{
  if (seed) { mm3d_srand(cached, seed); mm3d_srand(plain, seed); }
  const Result a = run(cached, clouds, p), b = run(plain, clouds, p);
  CHECK(same(a, b));
  CHECK(mm3d_map_cache_stats(cached, st, 1) == MM3D_OK);
  return b.n_pairs;
}

static void expect(const long long st[6], long long hits, long long misses, long long reused, long long computed, int line)
{
  if (st[0] != hits || st[1] != misses || st[2] != reused || st[3] != computed) {
    std::printf("stats at line %d: %lld %lld %lld %lld, expected %lld %lld %lld %lld\n", line, st[0], st[1], st[2], st[3], hits, misses, reused,
                computed);
    ++failures;
  }
}
#define EXPECT(st, h, m, r, c) expect(st, h, m, r, c, __LINE__)

static void sequence(int streams, int method)
{
  const int kMaps = 6, kPts = 2400;
  std::vector<std::vector<Pt>> clouds;
  for (int m = 0; m < kMaps; ++m) clouds.push_back(make_cloud(kPts + 37 * m, (unsigned)m + 1));
  mm3d_ctx *cached = nullptr, *plain = nullptr;
  CHECK(mm3d_create(0, &cached) == MM3D_OK && mm3d_create(0, &plain) == MM3D_OK);
  CHECK(mm3d_set_streams(cached, streams) == MM3D_OK && mm3d_set_streams(plain, streams) == MM3D_OK);
  CHECK(mm3d_set_map_cache(cached, 16) == MM3D_OK && mm3d_get_map_cache(cached) == 16 && mm3d_get_map_cache(plain) == 0);
  mm3d_srand(cached, 1);
  mm3d_srand(plain, 1);
  mm3d_params p;
  mm3d_params_default(&p);
  p.descriptor_type = MM3D_DESC_FPFH;
  p.estimation_method = method;
  const bool reuse = method == MM3D_EST_MATCHING;
  long long st[6];
  // cold, then the same maps again
  size_t P = lockstep(cached, plain, clouds, p, st);
  CHECK(P == 15);
  EXPECT(st, 0, 6, 0, 15);
  CHECK(st[4] == 6 && st[5] > 0);
  P = lockstep(cached, plain, clouds, p, st);
  EXPECT(st, 6, 0, reuse ? 15 : 0, reuse ? 0 : 15);
  // one point of map 2 moved by one ulp
  std::vector<std::vector<Pt>> changed = clouds;
  changed[2][100].y = std::nextafter(changed[2][100].y, 1e9f);
  P = lockstep(cached, plain, changed, p, st);
  EXPECT(st, 5, 1, reuse ? 10 : 0, reuse ? 5 : 15);
  // reversed: every map hits in another slot, every pair is now the other way round
  std::vector<std::vector<Pt>> rev(clouds.rbegin(), clouds.rend());
  P = lockstep(cached, plain, rev, p, st);
  EXPECT(st, 6, 0, 0, 15);
  // a pair-only parameter: features hit, pairs do not; confidence_threshold: nothing misses
  mm3d_params q = p;
  q.max_iterations = 33;
  P = lockstep(cached, plain, clouds, q, st);
  EXPECT(st, 6, 0, 0, 15);
  q = p;
  q.confidence_threshold = 0.5;
  P = lockstep(cached, plain, clouds, q, st);
  EXPECT(st, 6, 0, reuse ? 15 : 0, reuse ? 0 : 15);
  // SAC_IA's pairs come back with the generator state they started from
  if (!reuse) {
    P = lockstep(cached, plain, clouds, p, st, 9);
    P = lockstep(cached, plain, clouds, p, st, 9);
    EXPECT(st, 6, 0, 15, 0);
  }
  // a call whose maps fail to build (an unknown descriptor type), and one that fails half-way through (the fake device pass
  // fails for a map of 1111 points, behind two new maps that were built and staged): both come back with their status, and
  // the cache is what it was
  long long before[6], after[6];
  CHECK(mm3d_map_cache_stats(cached, before, 0) == MM3D_OK);
  q = p;
  q.descriptor_type = 9;
  CHECK(run(cached, clouds, q).status == MM3D_EINVAL);
  std::vector<std::vector<Pt>> bad = {make_cloud(2000, 41), make_cloud(2100, 42), make_cloud(1111, 43), clouds[0]};
  setenv("MM3D_FAKE_DIGEST_FAIL_POINTS", "1111", 1);
  CHECK(run(cached, bad, p).status == MM3D_EDEVICE);
  unsetenv("MM3D_FAKE_DIGEST_FAIL_POINTS");
  {
    // the same call failing one stage later: that map misses, and the (fake) keypoint detector throws while it is built
    mm3d_cloud *raw = nullptr, *down = nullptr;
    CHECK(mm3d_cloud_create(plain, bad[2].data(), bad[2].size(), sizeof(Pt), 12, &raw) == MM3D_OK);
    CHECK(mm3d_downsample(plain, raw, p.resolution, &down) == MM3D_OK);
    setenv("MM3D_FAKE_FAIL_POINTS", std::to_string(mm3d_cloud_size(down)).c_str(), 1);
    mm3d_cloud_free(plain, raw); mm3d_cloud_free(plain, down);
    CHECK(run(cached, bad, p).status == MM3D_EDEVICE);
    unsetenv("MM3D_FAKE_FAIL_POINTS");
  }
  CHECK(mm3d_map_cache_stats(cached, after, 0) == MM3D_OK);
  CHECK(std::memcmp(before, after, sizeof(before)) == 0);
  P = lockstep(cached, plain, clouds, p, st, 1);               // (the first call's generator state again: SAC_IA's pairs too)
  EXPECT(st, 6, 0, 15, 0);
  std::vector<std::vector<Pt>> two(bad.begin(), bad.begin() + 2);
  P = lockstep(cached, plain, two, p, st);                   // (the failed call's maps were not kept)
  EXPECT(st, 0, 2, 0, 1);
  // room for three maps: the call's last three stay, and the results stay exact
  CHECK(mm3d_set_map_cache(cached, 3) == MM3D_OK && mm3d_get_map_cache(cached) == 3);
  CHECK(mm3d_map_cache_stats(cached, st, 1) == MM3D_OK && st[4] <= 3);
  for (int rep = 0; rep < 3; ++rep) {
    P = lockstep(cached, plain, clouds, p, st);
    CHECK(st[4] <= 3);
  }
  EXPECT(st, 3, 3, reuse ? 3 : 0, reuse ? 12 : 15);
  // streams come and go under the cache; clearing empties it; 0 turns it off
  CHECK(mm3d_set_streams(cached, streams == 1 ? 3 : 1) == MM3D_OK && mm3d_set_streams(plain, streams == 1 ? 3 : 1) == MM3D_OK);
  P = lockstep(cached, plain, clouds, p, st);
  EXPECT(st, 3, 3, reuse ? 3 : 0, reuse ? 12 : 15);
  mm3d_map_cache_clear(cached);
  CHECK(mm3d_map_cache_stats(cached, st, 1) == MM3D_OK && st[4] == 0 && st[5] == 0);
  P = lockstep(cached, plain, clouds, p, st);
  EXPECT(st, 0, 6, 0, 15);
  CHECK(mm3d_set_map_cache(cached, 0) == MM3D_OK && mm3d_get_map_cache(cached) == 0);
  CHECK(mm3d_map_cache_stats(cached, st, 0) == MM3D_OK && st[4] == 0);
  CHECK(mm3d_set_map_cache(cached, 5) == MM3D_OK);             // (on again: mm3d_destroy frees it)
  P = lockstep(cached, plain, clouds, p, st);
  mm3d_destroy(cached);
  mm3d_destroy(plain);
}

int main()
{
  long long st[6];
  CHECK(mm3d_set_map_cache(nullptr, 4) == MM3D_EINVAL && mm3d_get_map_cache(nullptr) == 0 && mm3d_map_cache_stats(nullptr, st, 0) == MM3D_EINVAL);
  mm3d_map_cache_clear(nullptr);
  mm3d_ctx *c = nullptr;
  CHECK(mm3d_create(0, &c) == MM3D_OK);
  CHECK(mm3d_set_map_cache(c, -1) == MM3D_EINVAL && mm3d_map_cache_stats(c, nullptr, 0) == MM3D_EINVAL);
  CHECK(mm3d_map_cache_stats(c, st, 0) == MM3D_OK && st[0] == 0 && st[4] == 0);
  mm3d_destroy(c);
  for (int streams : {1, 3})
    for (int method : {MM3D_EST_MATCHING, MM3D_EST_SAC_IA}) sequence(streams, method);
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("map cache host driver ok\n");
  return 0;
}

// driver_shard.cpp -- mm3d_estimate_maps_transforms in shardable pieces, one process per device (mm3d_shard_*, include/mm3d.h).
#include <algorithm>
#include <atomic>

#include "device_util.hpp"
#include "capi_guard.hpp"
#include "drivers.hpp"

using namespace mm3d;

// ---------------------------------------------------------------- the same job on N processes (one per GPU)
// The N > 1 driver, inside the library like the N = 1 one (estimate_maps_streams): the caller (bench.py,
// one process per GPU) only moves bytes between ranks -- one all-gather of the maps' feature bundles, one
// all-gather of the pair records.  A rank extracts the features of the maps it owns (on its streams),
// receives the other maps' bundles, and estimates the pairs whose TARGET it owns, so each rank builds
// target-side search structures (grids, distance transforms, k-NN operands) for n / world maps only.
// Owners zig-zag over the ranks (0 1 .. w-1 w-1 .. 1 0 0 1 ..): target j has j pairs, and j and its mirror
// image share a rank, which evens the pair counts out.
// (struct mm3d_shard: drivers.hpp)

// (no lock, no device selection: the callers -- mm3d_shard_begin under guarded(), estimate_maps_devices on a device's own thread -- did both)
mm3d_shard *mm3d::shard_begin_impl(mm3d_ctx *ctx, const mm3d_cloud_view *clouds, size_t n, const mm3d_params *params, int rank, int world)
{
  std::unique_ptr<mm3d_shard> sh(new mm3d_shard());
  sh->ctx = ctx; sh->rank = rank; sh->world = world; sh->n = n; sh->params = *params;
  sh->maps.assign(n, nullptr);
  std::vector<size_t> mine;
  for (size_t i = 0; i < n; ++i)
    if (mm3d_shard_map_owner(i, world) == rank) mine.push_back(i);
  std::atomic<size_t> next{0};
  on_streams(ctx, [&](size_t, mm3d_ctx *c, const std::atomic<bool> &failed) {
    for (;;) {
      const size_t k = next.fetch_add(1);
      if (k >= mine.size() || failed.load()) break;
      const size_t i = mine[k];
      std::unique_ptr<mm3d_cloud> raw = cloud_from_view(c, clouds[i]);
      // this rank is the map's target-side owner; nobody else sees the map before on_streams has drained every stream
      sh->maps[i] = build_private_map(c, raw.get(), params).release();   // (distinct slots: no lock needed; the shard owns it from here)
    }
  });
  return sh.release();
}

extern "C" {

int mm3d_shard_map_owner(size_t map, int world)
{
  if (world <= 1) return 0;
  const size_t j = map % (2 * (size_t)world);
  return (int)(j < (size_t)world ? j : 2 * (size_t)world - 1 - j);
}

int mm3d_shard_begin(mm3d_ctx *ctx, const mm3d_cloud_view *clouds, size_t n, const mm3d_params *params, int rank, int world,
                     mm3d_shard **out)
{
  if (!ctx || !params || !out || (n && !clouds) || world < 1 || rank < 0 || rank >= world) return MM3D_EINVAL;
  *out = nullptr;
  return guarded(ctx, [&] {
    if (const StageRule *r = first_stage_left_home(ctx->sel)) throw Error(MM3D_EUNSUPPORTED, std::string("mm3d_shard_begin: ") + r->stays_home);
    *out = shard_begin_impl(ctx, clouds, n, params, rank, world);
  });
}

int mm3d_shard_bundle_sizes(const mm3d_shard *sh, uint64_t *n_points, uint64_t *n_keypoints)
{
  if (!sh || !n_points || !n_keypoints) return MM3D_EINVAL;
  for (size_t i = 0; i < sh->n; ++i) {
    const bool own = sh->maps[i] && mm3d_shard_map_owner(i, sh->world) == sh->rank;
    n_points[i] = own ? sh->maps[i]->points->n : 0;
    n_keypoints[i] = own ? sh->maps[i]->keypoints->n : 0;
  }
  return MM3D_OK;
}

// A map's bundle (round 5: the source-side structures travel with it).  What a rank does with another rank's map is the SOURCE
// role: ICP / score / SAC-IA scoring read the cloud in its Hilbert query order through its work items, the rand() replay reads
// the keypoints on the host.  Until round 5 a rank rebuilt those orders from the points it had received (two Hilbert sorts and a
// wait per map: 2.3 ms per rank and step at N = 8, with fourteen foreign maps); now the owner -- who has them -- sends them:
//   header (256 B) | points 16 B x P | keypoints 16 B x K | descriptors 4 B x dim x K |
//   points in Hilbert order 16 B x P | their work items 8 B x (P / 64 + 16 386) | the same two for the keypoints
// Every part starts 16-byte aligned and is as large as P and K allow (the sizes are all a receiver knows before the exchange);
// the header says how much of the Hilbert parts is meant, and carries the bounding boxes.  The order a pair's reductions run in
// is then the owner's, i.e. the one-process run's, by construction.
namespace {
struct BundleHeader {
  uint64_t magic, n_points, n_keypoints;
  uint64_t p_finite, p_items, k_finite, k_items;
  uint32_t p_have, k_have;                   // bounding box + Hilbert copy + items are in the bundle
  float p_bmin[3], p_bmax[3], k_bmin[3], k_bmax[3];
  unsigned char pad[256 - 7 * 8 - 2 * 4 - 12 * 4];
};
static_assert(sizeof(BundleHeader) == 256, "bundle header");
constexpr uint64_t kBundleMagic = 0x6d6d33642d623032ull;          // "mm3d-b02"
// A stack object (a bundle header) is the source / destination of an asynchronous copy: nothing may unwind the frame while
// that copy can still be in flight.  Armed until the function's own wait.
struct DrainOnUnwind {
  Context *c;
  bool armed = true;
  ~DrainOnUnwind() { if (armed) (void)stream_wait(c->stream); }
};
struct BundleLayout {
  size_t pts, kp, desc, p_hil, p_items, k_hil, k_items, total, p_item_cap, k_item_cap;
};
size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
BundleLayout bundle_layout(uint64_t P, uint64_t K, int dim)
{
  BundleLayout L;
  L.p_item_cap = (size_t)P / 64 + 16384 + 2;                        // cloud_hilbert's bound (grid.hip)
  L.k_item_cap = (size_t)K / 64 + 16384 + 2;
  L.pts = sizeof(BundleHeader);
  L.kp = L.pts + (size_t)P * 16;
  L.desc = L.kp + (size_t)K * 16;
  L.p_hil = up16(L.desc + (size_t)K * (size_t)(dim > 0 ? dim : 0) * 4);
  L.p_items = L.p_hil + (size_t)P * 16;
  L.k_hil = up16(L.p_items + L.p_item_cap * sizeof(int2));
  L.k_items = L.k_hil + (size_t)K * 16;
  L.total = up16(L.k_items + L.k_item_cap * sizeof(int2));
  return L;
}
}  // namespace

size_t mm3d_shard_bundle_bytes(uint64_t n_points, uint64_t n_keypoints, int descriptor_type)
{
  return bundle_layout(n_points, n_keypoints, mm3d_descriptor_dim(descriptor_type)).total;
}

int mm3d_shard_pack(mm3d_shard *sh, size_t map, void *dst)
{
  if (!sh || map >= sh->n || !sh->maps[map] || !dst) return MM3D_EINVAL;
  mm3d_ctx *ctx = sh->ctx;
  return guarded(ctx, [&] {
    const mm3d_map *m = sh->maps[map];
    char *d = static_cast<char *>(dst);
    const BundleLayout L = bundle_layout(m->points->n, m->keypoints->n, m->desc->dim);
    // the query orders exist on the owner as soon as it has played the source role once; a map that has not is ordered now
    if (m->points->n) cloud_hilbert(ctx, m->points);
    if (m->keypoints->n) cloud_hilbert(ctx, m->keypoints);
    // (ordinary memory: the pinned arena may wrap under the copies below, and 256 bytes need no pinning)
    BundleHeader header;
    BundleHeader *h = &header;
    std::memset(h, 0, sizeof(*h));
    h->magic = kBundleMagic; h->n_points = m->points->n; h->n_keypoints = m->keypoints->n;
    auto side = [&](const mm3d_cloud *cl, uint64_t &fin, uint64_t &items, uint32_t &have, float *bmin, float *bmax, size_t off_hil,
                    size_t off_items, size_t item_cap) {
      have = (cl->n && cl->have_bbox && cl->hil_pts.get() && (size_t)cl->n_wave_items <= item_cap) ? 1u : 0u;
      if (!have) return;
      fin = cl->n_finite; items = (uint64_t)cl->n_wave_items;
      for (int a = 0; a < 3; ++a) { bmin[a] = cl->bmin[a]; bmax[a] = cl->bmax[a]; }
      if (cl->n_finite) MM3D_HIP(hipMemcpyAsync(d + off_hil, cl->hil_pts.get(), cl->n_finite * 16, hipMemcpyDefault, ctx->stream));
      if (cl->n_wave_items)
        MM3D_HIP(hipMemcpyAsync(d + off_items, cl->wave_items.get(), (size_t)cl->n_wave_items * sizeof(int2), hipMemcpyDefault, ctx->stream));
    };
    DrainOnUnwind drain{ctx};                 // (`header` is read by the copy queued below)
    side(m->points, h->p_finite, h->p_items, h->p_have, h->p_bmin, h->p_bmax, L.p_hil, L.p_items, L.p_item_cap);
    side(m->keypoints, h->k_finite, h->k_items, h->k_have, h->k_bmin, h->k_bmax, L.k_hil, L.k_items, L.k_item_cap);
    MM3D_HIP(hipMemcpyAsync(d, h, sizeof(*h), hipMemcpyDefault, ctx->stream));
    if (m->points->n) MM3D_HIP(hipMemcpyAsync(d + L.pts, m->points->pts.get(), m->points->n * 16, hipMemcpyDefault, ctx->stream));
    if (m->keypoints->n) MM3D_HIP(hipMemcpyAsync(d + L.kp, m->keypoints->pts.get(), m->keypoints->n * 16, hipMemcpyDefault, ctx->stream));
    if (m->desc->n) MM3D_HIP(hipMemcpyAsync(d + L.desc, m->desc->data.get(), m->desc->n * (size_t)m->desc->dim * 4, hipMemcpyDefault, ctx->stream));
    ctx->sync();
    drain.armed = false;
  });
}

// one received bundle -> a map in the source role, on context c (copies, a short wait for the 256-byte header and ONE for the rest; no kernel unless the owner sent no orders)
static std::unique_ptr<mm3d_map> map_from_bundle(mm3d_ctx *c, const void *src, uint64_t n_points, uint64_t n_keypoints, int descriptor_type)
{
  const char *s = static_cast<const char *>(src);
  const int dim = mm3d_descriptor_dim(descriptor_type);
  const BundleLayout L = bundle_layout(n_points, n_keypoints, dim);
  // (into ordinary memory: the pinned arena may wrap under cloud_host() below, and 256 bytes need no pinning)
  BundleHeader header;
  BundleHeader *h = &header;
  std::memset(h, 0, sizeof(*h));
  // the header first, blocking (256 bytes), and checked BEFORE the large copies are queued at sizes the caller supplied
  if (s) {
    MM3D_HIP(hipMemcpyAsync(h, s, sizeof(*h), hipMemcpyDefault, c->stream));
    DrainOnUnwind drain{c};
    c->sync();
    drain.armed = false;
    if (h->magic != kBundleMagic || h->n_points != n_points || h->n_keypoints != n_keypoints)
      throw Error(MM3D_EINVAL, "mm3d_shard_unpack: not a bundle of this library version, or the sizes do not match it");
  }
  std::unique_ptr<mm3d_cloud> pts(cloud_from_memory(c, n_points ? s + L.pts : nullptr, n_points, 16, 12));
  std::unique_ptr<mm3d_cloud> kp(cloud_from_memory(c, n_keypoints ? s + L.kp : nullptr, n_keypoints, 16, 12));
  std::unique_ptr<mm3d_desc> desc(desc_from_memory(c, reinterpret_cast<const float *>(s ? s + L.desc : nullptr), n_keypoints, descriptor_type));
  // the Hilbert parts at their full size (how much of them is meant is in the header, which arrives with the same wait)
  struct Side { DevBuf<float4> hil; DevBuf<int2> items; };
  auto grab = [&](uint64_t n, size_t off_hil, size_t off_items, size_t item_cap) {
    Side sd;
    if (!n || !s) return sd;
    sd.hil = DevBuf<float4>(c, n);
    sd.items = DevBuf<int2>(c, item_cap);
    MM3D_HIP(hipMemcpyAsync(sd.hil.get(), s + off_hil, (size_t)n * 16, hipMemcpyDefault, c->stream));
    MM3D_HIP(hipMemcpyAsync(sd.items.get(), s + off_items, item_cap * sizeof(int2), hipMemcpyDefault, c->stream));
    return sd;
  };
  Side ps = grab(n_points, L.p_hil, L.p_items, L.p_item_cap), ks = grab(n_keypoints, L.k_hil, L.k_items, L.k_item_cap);
  (void)cloud_host(c, kp.get());                      // (the host copy of the keypoints: this is the wait)
  c->sync();
  auto adopt = [&](mm3d_cloud *cl, Side &sd, uint32_t have, uint64_t fin, uint64_t items, const float *bmin, const float *bmax, size_t item_cap) {
    if (!have || !cl->n || fin > cl->n || items > item_cap) return;
    std::lock_guard<std::recursive_mutex> lk(cl->cache_mu);
    cl->have_bbox = true;
    cl->n_finite = (size_t)fin;
    for (int a = 0; a < 3; ++a) { cl->bmin[a] = bmin[a]; cl->bmax[a] = bmax[a]; }
    cl->hil_pts = std::move(sd.hil);
    cl->wave_items = std::move(sd.items);
    cl->n_wave_items = (int)items;
  };
  adopt(pts.get(), ps, h->p_have, h->p_finite, h->p_items, h->p_bmin, h->p_bmax, L.p_item_cap);
  adopt(kp.get(), ks, h->k_have, h->k_finite, h->k_items, h->k_bmin, h->k_bmax, L.k_item_cap);
  // (an owner that sent no orders -- an empty or all-NaN cloud -- leaves them to be built here, as before round 5)
  if (pts->n) cloud_hilbert(c, pts.get());
  if (kp->n) cloud_hilbert(c, kp.get());
  c->sync();
  return make_map(std::move(pts), std::move(kp), std::move(desc));
}

int mm3d_shard_unpack(mm3d_shard *sh, size_t map, const void *src, uint64_t n_points, uint64_t n_keypoints)
{
  if (!sh || map >= sh->n || (!src && (n_points || n_keypoints))) return MM3D_EINVAL;
  if (sh->maps[map]) return MM3D_OK;               // an owned map is already here
  mm3d_ctx *ctx = sh->ctx;
  return guarded(ctx, [&] {
    // source role only: the query orders of ICP / score and of SAC-IA's scoring, and the host copy of the
    // keypoints that the rand() replay reads; target-side structures are the owner's business
    sh->maps[map] = map_from_bundle(ctx, src, n_points, n_keypoints, sh->params.descriptor_type).release();
  });
}

// every map another rank owns, on the context's streams (at 8 ranks that is 14 of 16 maps per rank)
int mm3d_shard_unpack_many(mm3d_shard *sh, size_t count, const size_t *maps, const void *const *srcs, const uint64_t *n_points,
                           const uint64_t *n_keypoints)
{
  if (!sh || (count && (!maps || !srcs || !n_points || !n_keypoints))) return MM3D_EINVAL;
  mm3d_ctx *ctx = sh->ctx;
  return guarded(ctx, [&] {
    for (size_t k = 0; k < count; ++k)
      if (maps[k] >= sh->n || (!srcs[k] && (n_points[k] || n_keypoints[k]))) throw Error(MM3D_EINVAL, "mm3d_shard_unpack_many: bad item");
    std::atomic<size_t> next{0};
    on_streams(ctx, [&](size_t, mm3d_ctx *c, const std::atomic<bool> &failed) {
      for (;;) {
        const size_t k = next.fetch_add(1);
        if (k >= count || failed.load()) break;
        const size_t i = maps[k];
        if (sh->maps[i]) continue;                    // an owned map is already here
        PrivateObjects priv(c);                       // nobody sees the map before this worker's waits
        sh->maps[i] = map_from_bundle(c, srcs[k], n_points[k], n_keypoints[k], sh->params.descriptor_type).release();   // source role only, as in mm3d_shard_unpack; distinct slots
      }
    });
  });
}

}  // extern "C"

void mm3d::shard_pairs_impl(mm3d_shard *sh, mm3d_pair_result *pairs, unsigned char *mine, size_t capacity, size_t *n_pairs)
{
  mm3d_ctx *ctx = sh->ctx;
  for (size_t i = 0; i < sh->n; ++i)
    if (!sh->maps[i]) throw Error(MM3D_EINVAL, "mm3d_shard_pairs: a map has neither been computed here nor unpacked");
  const mm3d_params *params = &sh->params;
  // the live pairs in the reference's order, and the generator state before each of them (the draws of a pair
  // depend on its source keypoints only: every rank replays the whole stream on the host, ~30 us per pair)
  std::vector<std::pair<size_t, size_t>> live;
  for (const auto &ij : all_pairs(sh->n))
    if (is_pair(sh->maps[ij.first], sh->maps[ij.second])) live.push_back(ij);
  const size_t P = live.size();
  *n_pairs = P;
  if (P > capacity) throw Error(MM3D_ECAPACITY, "mm3d_shard_pairs: room for every live pair is needed");
  // state_at[q] = the generator before pair q, advanced on demand (under rng_mu) as far as a worker needs it:
  // the first pairs start at once, the table's tail (~30 us of host work per pair) is filled in while they run
  std::vector<GlibcRand> state_at(P + 1, ctx->rnd);
  size_t known_upto = 0;
  std::mutex rng_mu;
  std::vector<const std::vector<float4> *> src_kp(sh->n, nullptr);
  for (size_t i = 0; i < sh->n; ++i) src_kp[i] = &cloud_host(ctx, sh->maps[i]->keypoints);   // (cached at prepare / unpack time)
  auto advance_states = [&](size_t upto) {
    std::lock_guard<std::mutex> lk(rng_mu);
    while (known_upto < upto) {
      GlibcRand r = state_at[known_upto];
      // (not pair_replay_draws: mm3d_set_alignment can still reach a shard's context after mm3d_shard_begin has looked, and this
      // replay has never asked the context)
      pair_rand_replay(r, params->estimation_method, *src_kp[live[known_upto].first], params->inlier_threshold, params->max_iterations);
      state_at[++known_upto] = r;
    }
  };
  std::vector<size_t> todo;
  for (size_t q = 0; q < P; ++q) {
    pair_record_init(&pairs[q], live[q].first, live[q].second);
    mine[q] = mm3d_shard_map_owner(live[q].second, sh->world) == sh->rank ? 1 : 0;
    if (mine[q]) todo.push_back(q);
  }
  // batches of pairs with the same target (pairs_estimate_batch), at most kPairBatch of them and not so many that
  // a stream runs dry: every map exists already, so the whole list can be cut up front
  const size_t S = ctx->helpers.size() + 1;
  const size_t take = pair_batch_take(todo.size(), S);
  std::stable_sort(todo.begin(), todo.end(), [&](size_t a, size_t b) { return live[a].second < live[b].second; });
  std::vector<std::pair<size_t, size_t>> batches;           // [first, last) into todo
  for (size_t a = 0; a < todo.size();) {
    size_t b = a + 1;
    while (b < todo.size() && b - a < take && live[todo[b]].second == live[todo[a]].second) ++b;
    batches.emplace_back(a, b);
    a = b;
  }
  std::atomic<size_t> next{0};
  on_streams(ctx, [&](size_t, mm3d_ctx *c, const std::atomic<bool> &failed) {
    std::vector<PairWork> work;
    for (;;) {
      const size_t k = next.fetch_add(1);
      if (k >= batches.size() || failed.load()) break;
      work.clear();
      for (size_t e = batches[k].first; e < batches[k].second; ++e) {
        const size_t q = todo[e];
        advance_states(q);
        work.push_back(PairWork{sh->maps[live[q].first], sh->maps[live[q].second], &pairs[q], state_at[q]});
      }
      pairs_estimate_batch(c, work.data(), work.size(), params);
    }
  });
  advance_states(P);
  ctx->rnd = state_at[P];                       // where the reference's sequential loop leaves the generator
}

extern "C" {

int mm3d_shard_pairs(mm3d_shard *sh, mm3d_pair_result *pairs, unsigned char *mine, size_t capacity, size_t *n_pairs)
{
  if (!sh || !n_pairs || !pairs || !mine) return MM3D_EINVAL;
  return guarded(sh->ctx, [&] { shard_pairs_impl(sh, pairs, mine, capacity, n_pairs); });
}

void mm3d_shard_end(mm3d_shard *sh)
{
  if (!sh) return;
  mm3d_ctx *ctx = sh->ctx;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)stream_wait(ctx->stream);
    for (mm3d_ctx *h : ctx->helpers) (void)stream_wait(h->stream);
  }
  delete sh;
}

}  // extern "C"

// driver_streams.cpp -- mm3d_estimate_maps_transforms on one device: over the context's streams, or on one stream.
#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <exception>
#include <thread>

#include "device_util.hpp"
#include "capi_guard.hpp"
#include "drivers.hpp"

using namespace mm3d;

// estimateMapsTransforms over the context's streams (mm3d_set_streams).  The reference's two loops
// (map_merging.cpp:212-242 per cloud, :256-269 per pair) are dealt to S workers, one context (HIP
// stream + memory pool) and one host thread each: about 3/4 of them extract features, every worker
// then claims pairs in the reference's order and waits until both maps of its pair exist.  A map is
// prepared (map_prepare_impl) before it is published, so pairs only read it.  The reference's single
// rand() stream is kept by replay: every worker starts from the caller's generator state and replays
// the draws of the pairs it does not execute (execute = false, host only), so each pair sees exactly
// the state the sequential loop would give it; worker 0 (the caller's own context) replays to the
// end, which leaves the caller's generator where the sequential loop would.
void mm3d::estimate_maps_streams(mm3d_ctx *ctx, const mm3d_cloud_view *clouds, size_t n, const mm3d_params *params, float *out_T,
                                 size_t *n_out, mm3d_pair_result *pairs_out, size_t *n_pairs_out)
{
  std::vector<mm3d_ctx *> cs{ctx};
  cs.insert(cs.end(), ctx->helpers.begin(), ctx->helpers.end());
  const size_t S = cs.size();
  // many small maps (at least two per worker): every worker extracts features first, and the pairs then start in
  // batches; otherwise (few large maps) 3/4 of the workers do, and the others begin with the pairs of the first maps
  // (measured on 16 x 500 k points with 16 workers, map pairs/s at 6 / 8 / 10 / 12 / 16 feature workers:
  // 740 / 741 / 736 / 765 / 741;
  // and three quarters of the maps with 8 x 2 M points: 93.0 pairs/s with 6 feature workers, 91.2 with 12 = all 8 maps at
  // once; the dense indoor variant 59.0 / 53.9)
  size_t F = (S <= 4 || n >= 2 * S) ? S : std::max<size_t>(4, std::min(S * 3 / 4, (n * 3 + 3) / 4));
  if (const char *e = std::getenv("MM3D_FEATURE_WORKERS")) {     // tuning knob: how many workers start on features
    const long v = std::atol(e);
    if (v >= 1) F = std::min<size_t>(S, (size_t)v);
  }
  const std::vector<std::pair<size_t, size_t>> all = all_pairs(n);
  std::vector<const mm3d_map *> maps(n, nullptr);
  // mm3d_set_map_cache: maps[i] is the cache's (a hit, or a miss handed over once built) where borrowed[i] is set
  MapCacheBase *const cache = ctx->map_cache;
  std::vector<char> borrowed(n, 0);
  struct MapsGuard {                                    // the maps go when the call ends, whichever way
    std::vector<const mm3d_map *> &m;
    const std::vector<char> &borrowed;
    ~MapsGuard()
    {
      for (size_t i = 0; i < m.size(); ++i)
        if (!borrowed[i]) delete m[i];
    }
  } maps_guard{maps, borrowed};
  std::vector<mm3d_pair_result> rec(all.size());
  std::vector<char> ready(n, 0), done(all.size(), 0);
  std::mutex mu;
  std::condition_variable cv;
  size_t next_map = 0;
  bool abort = false;
  std::exception_ptr first_error;
  const GlibcRand rnd0 = ctx->rnd;
  const RunClock clock;
  ctx->last_points.assign(n, 0);
  ctx->last_keypoints.assign(n, 0);
  ctx->last_features_s = ctx->last_total_s = 0.0;

  // The reference's single rand() stream, without serialising the pairs on it: the draws a pair consumes
  // depend on its SOURCE keypoints only (pair_rand_replay), given that its target has a keypoint at all.
  // state_at[q] = the generator before pair q; it is advanced pair by pair (once, under rng_mu) as far as
  // a worker needs it, taking "is pair q live" from the maps that exist and ASSUMING a target that is
  // still being computed will have keypoints.  A pair can therefore start as soon as its own two maps
  // and the sources of the rows before it exist -- not only after the last map.  Every assumption is
  // checked once all maps exist; a wrong one (a map without keypoints, e.g. an untextured cloud) makes
  // the call redo the pair loop sequentially, which is the reference's loop.
  const size_t P = all.size();
  std::vector<GlibcRand> state_at(P + 1, rnd0);
  std::vector<char> assumed_live(P, 0), claimed(P, 0);
  size_t known_upto = 0;                                // state_at[0 .. known_upto] are final
  std::mutex rng_mu;
  auto wait_ready = [&](size_t i) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return abort || ready[i]; });
    if (abort) throw Error(MM3D_EDEVICE, "aborted");
  };
  auto is_ready = [&](size_t i) { std::lock_guard<std::mutex> lk(mu); return ready[i] != 0; };
  auto advance_states = [&](size_t p) {                 // make state_at[p] final
    std::lock_guard<std::mutex> rl(rng_mu);
    while (known_upto < p) {
      const size_t q = known_upto, a = all[q].first, b = all[q].second;
      wait_ready(a);
      bool live = maps[a]->keypoints->n > 0;
      if (live) {
        if (is_ready(b)) live = maps[b]->keypoints->n > 0;
        else assumed_live[q] = 1;
      }
      GlibcRand r = state_at[q];
      if (live) pair_replay_draws(r, ctx, params, cloud_host(cs[0], maps[a]->keypoints));
      state_at[q + 1] = r;
      known_upto = q + 1;
    }
  };
  // the next pairs to work on: the first unclaimed ones, in the reference's order, whose two maps and all
  // earlier sources exist (maps finish roughly in index order, so that is rarely a restriction).  A worker takes
  // its share of what can start right now, up to kPairBatch pairs: their ICP / score tails then run as one batch
  // (many small maps: thousands of pairs are ready at once and a launch per pair leaves the chip idle), while a
  // job whose pairs trickle in behind the feature stage keeps dealing them out one by one.
  auto claim_pairs = [&](std::vector<size_t> &out) -> bool {
    out.clear();
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      if (abort) return false;
      bool any_left = false;
      size_t prefix = 0, avail = 0;
      while (prefix < n && ready[prefix]) ++prefix;      // maps [0, prefix) exist
      for (size_t q = 0; q < P; ++q) {
        if (claimed[q]) continue;
        any_left = true;
        if (all[q].first < prefix && ready[all[q].second]) ++avail;
      }
      if (!any_left) return false;
      if (avail) {
        // a batch shares its TARGET (the pairs (i, t) of one t): one descriptor search for the sampled rows of all
        // its sources, and one target grid under every search of the batch
        const size_t take = pair_batch_take(avail, S);
        size_t target = n;
        for (size_t q = 0; q < P && out.size() < take; ++q)
          if (!claimed[q] && all[q].first < prefix && ready[all[q].second] && (target == n || all[q].second == target)) {
            target = all[q].second;
            claimed[q] = 1;
            out.push_back(q);
          }
        return true;
      }
      cv.wait(lk);
    }
  };
  auto worker = [&](size_t w) {
    mm3d_ctx *c = cs[w];
    try {
      if (hipSetDevice(c->device) != hipSuccess) throw Error(MM3D_EDEVICE, "hipSetDevice failed");
      while (w < F) {
        size_t i;
        {
          std::lock_guard<std::mutex> lk(mu);
          if (abort || next_map >= n) break;
          i = next_map++;
        }
        std::unique_ptr<mm3d_cloud> raw = cloud_from_view(c, clouds[i]);
        if (cache && raw->n > 0) {
          // an unchanged map: its bundle is published at once, nothing else runs on the device for it
          if (const mm3d_map *hit = cache->lookup(c, i, raw.get())) {
            raw.reset();
            {
              std::lock_guard<std::mutex> lk(mu);
              maps[i] = hit;
              borrowed[i] = 1;
              ready[i] = 1;
              record_map_sizes(ctx, i, hit);
              ctx->last_features_s = std::max(ctx->last_features_s, clock.since_start());
            }
            cv.notify_all();
            continue;
          }
        }
        std::unique_ptr<mm3d_map> held = build_private_map(c, raw.get(), params);   // this worker's alone until it is published
        const bool keep = cache && raw->n > 0;
        {
          std::lock_guard<std::mutex> lk(mu);
          mm3d_map *m = held.release();
          maps[i] = m;
          if (keep) {
            cache->insert(i, std::move(raw), m);         // (the cache owns the map and its raw points from here on)
            borrowed[i] = 1;
          }
          ready[i] = 1;
          record_map_sizes(ctx, i, m);
          ctx->last_features_s = std::max(ctx->last_features_s, clock.since_start());
        }
        raw.reset();
        cv.notify_all();
      }
      std::vector<size_t> mine, work_q;
      std::vector<PairWork> work;
      while (claim_pairs(mine)) {
        work.clear();
        work_q.clear();
        for (size_t p : mine) {
          const mm3d_map *ms = maps[all[p].first], *mt = maps[all[p].second];
          if (is_pair(ms, mt)) {
            advance_states(p);                          // (a reused pair's draws are replayed all the same)
            rec[p].source_idx = all[p].first;
            rec[p].target_idx = all[p].second;
            if (cache && cache->pair_lookup(all[p].first, all[p].second, state_at[p], &rec[p])) continue;
            work.push_back(PairWork{ms, mt, &rec[p], state_at[p]});
            work_q.push_back(p);
          }
        }
        if (!work.empty()) pairs_estimate_batch(c, work.data(), work.size(), params);
        if (cache)
          for (size_t k = 0; k < work.size(); ++k) cache->pair_insert(all[work_q[k]].first, all[work_q[k]].second, work[k].rnd, *work[k].out);
        for (size_t p : mine)
          if (is_pair(maps[all[p].first], maps[all[p].second])) done[p] = 1;
      }
      // (every map and every batch of pairs ended in a wait that brought its results to the host: nothing is in flight here
      // unless a kernel left an error flag to be looked at)
      if (!c->deferred.empty()) c->sync();
    } catch (...) {
      std::lock_guard<std::mutex> lk(mu);
      if (!first_error) first_error = std::current_exception();
      abort = true;
      cv.notify_all();
    }
  };
  std::vector<std::thread> threads;
  for (size_t w = 1; w < S; ++w) threads.emplace_back(worker, w);
  worker(0);
  for (auto &t : threads) t.join();
  // every stream has been synchronised by its worker (or the run was aborted): the maps can go
  for (size_t w = 0; w < S; ++w) (void)stream_wait(cs[w]->stream);
  if (first_error) std::rethrow_exception(first_error);
  // all maps exist now: finish the generator states and check what was assumed about late targets
  advance_states(P);
  bool assumptions_hold = true;
  for (size_t q = 0; q < P; ++q)
    if (assumed_live[q] && maps[all[q].second]->keypoints->n == 0) assumptions_hold = false;
  if (assumptions_hold) {
    ctx->rnd = state_at[P];                             // where the sequential loop leaves the generator
  } else {
    // a target turned out to have no keypoints: the states after that pair were positioned wrongly.
    // Redo the pair loop the reference's way, on the caller's stream.  (The map cache is left out of it: the records it took
    // above are still right for the states they name.)
    ctx->rnd = rnd0;
    std::fill(done.begin(), done.end(), 0);
    for (size_t q = 0; q < P; ++q) {
      const mm3d_map *ms = maps[all[q].first], *mt = maps[all[q].second];
      if (!is_pair(ms, mt)) continue;
      pair_estimate_impl(ctx, ms, mt, params, true, &rec[q]);
      rec[q].source_idx = all[q].first;
      rec[q].target_idx = all[q].second;
      done[q] = 1;
    }
    ctx->sync();
  }
  std::vector<mm3d_pair_result> pairs;
  for (size_t p = 0; p < all.size(); ++p)
    if (done[p]) pairs.push_back(rec[p]);
  finish_run(pairs.data(), pairs.size(), params, n, out_T, n_out, pairs_out, n_pairs_out);
  ctx->last_total_s = clock.since_start();
}

// the reference's two loops on ONE stream, in the reference's order (mm3d_set_streams(ctx, 1), the default)
void mm3d::estimate_maps_sequential(mm3d_ctx *ctx, const mm3d_cloud_view *clouds, size_t n, const mm3d_params *params, float *out_T,
                                    size_t *n_out, mm3d_pair_result *pairs_out, size_t *n_pairs_out)
{
  const RunClock clock;
  ctx->last_points.assign(n, 0);
  ctx->last_keypoints.assign(n, 0);
  std::vector<const mm3d_map *> maps(n, nullptr);       // every map of the call; those the map cache does not hold
  std::vector<std::unique_ptr<mm3d_map>> owned(n);      // (mm3d_set_map_cache) are `owned`, and go when the call ends
  MapCacheBase *const cache = ctx->map_cache;
  for (size_t i = 0; i < n; ++i) {
    std::unique_ptr<mm3d_cloud> raw = cloud_from_view(ctx, clouds[i]);
    maps[i] = cache && raw->n > 0 ? cache->lookup(ctx, i, raw.get()) : nullptr;
    if (!maps[i]) {
      owned[i] = map_features_impl(ctx, raw.get(), params);
      map_prepare_impl(ctx, owned[i].get(), params);      // search structures and k-NN target operands, once per map
      maps[i] = owned[i].get();
      if (cache && raw->n > 0) {                          // built from the same upload: the cache takes it and the map
        cache->insert(i, std::move(raw), owned[i].get());
        (void)owned[i].release();
      }
    }
    record_map_sizes(ctx, i, maps[i]);
  }
  ctx->last_features_s = clock.since_start();
  std::vector<mm3d_pair_result> pairs;
  for (size_t i = 0; i + 1 < n; ++i)
    for (size_t j = i + 1; j < n; ++j)
      if (is_pair(maps[i], maps[j])) {
        mm3d_pair_result r;
        pair_record_init(&r, i, j);
        pairs.push_back(r);
      }
  for (auto &r : pairs) {
    const mm3d_map *ms = maps[r.source_idx], *mt = maps[r.target_idx];
    if (cache && cache->pair_lookup(r.source_idx, r.target_idx, ctx->rnd, &r)) {
      // reused: the generator still moves on by the draws the pair would have taken
      pair_replay_draws(ctx->rnd, ctx, params, cloud_host(ctx, ms->keypoints));
      continue;
    }
    const GlibcRand r0 = ctx->rnd;
    pair_estimate_impl(ctx, ms, mt, params, true, &r);
    if (cache) cache->pair_insert(r.source_idx, r.target_idx, r0, r);
  }
  finish_run(pairs.data(), pairs.size(), params, n, out_T, n_out, pairs_out, n_pairs_out);
  ctx->last_total_s = clock.since_start();
}

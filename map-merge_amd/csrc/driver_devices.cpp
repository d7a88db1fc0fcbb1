// driver_devices.cpp -- mm3d_estimate_maps_transforms on a device list in one process (mm3d_create_devices).
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <exception>
#include <thread>

#include "device_util.hpp"
#include "capi_guard.hpp"
#include "drivers.hpp"

using namespace mm3d;

// ---------------------------------------------------------------- the same job on N devices of ONE process
// estimateMapsTransforms behind the reference's own entry point on a device list (mm3d_create_devices): the reference's
// caller is one process -- a ROS timer callback, R/src/map_merge_node.cpp:133-153 -- and cannot be relaunched under torchrun.
// One host thread per device drives that device's root context and its streams through the mm3d_shard_* scheme:
//   1. features of the maps the device owns (zig-zag ownership, shard_begin_impl) incl. their target-side structures;
//   2. when every device is done, each PULLS the other maps' bundles and source-side structures from their owners with
//      hipMemcpyPeerAsync (devices.cpp::cloud_clone_from_peer), dealt to its streams -- xGMI is point to point, every
//      device reads from up to seven peers at once; nothing is recomputed (the multi-process form re-builds the Hilbert
//      orders from the bundles: 2.3 ms per rank at N = 8);
//   3. the pairs whose TARGET the device owns (shard_pairs_impl), every device replaying the reference's single rand() stream;
//   4. ONE RCCL all-gather of the 104-byte pair records (devices.cpp::gather_pair_records), then the pose graph on the host.
// Same bits as one device: the ownership only decides where a map or a pair is computed.
// (extern "C": devices_debug and drain_devices have been in the library's symbol table under these names since they were
// written inside capi.cpp's extern "C" block; that table does not change with the files)
extern "C" {
namespace {
bool devices_debug()
{
  static const bool dbg = [] { const char *e = getenv("MM3D_DEVICES_DEBUG"); return e && atoi(e); }();
  return dbg;
}
// after a failed run: every stream of every device is drained before the shards (and their maps) go
void drain_devices(const std::vector<mm3d_ctx *> &roots, int restore_device)
{
  for (mm3d_ctx *r : roots) {
    (void)hipSetDevice(r->device);
    (void)stream_wait(r->stream);
    for (mm3d_ctx *h : r->helpers) (void)stream_wait(h->stream);
  }
  (void)hipSetDevice(restore_device);
}
// a barrier the device threads can leave through a failure: whoever throws releases the others, who then throw too
struct FailBarrier {
  std::mutex mu;
  std::condition_variable cv;
  size_t n, waiting = 0, generation = 0;
  bool failed = false;
  explicit FailBarrier(size_t n_) : n(n_) {}
  void wait()
  {
    std::unique_lock<std::mutex> lk(mu);
    if (failed) throw Error(MM3D_EDEVICE, "another device failed");
    const size_t gen = generation;
    if (++waiting == n) { waiting = 0; ++generation; cv.notify_all(); return; }
    cv.wait(lk, [&] { return failed || generation != gen; });
    if (failed) throw Error(MM3D_EDEVICE, "another device failed");
  }
  void fail()
  {
    std::lock_guard<std::mutex> lk(mu);
    failed = true;
    cv.notify_all();
  }
};
}  // namespace
}  // extern "C"

// ---- one process, several devices --------------------------------------------------------------------------------------
// What every device of a run shares on the host (one process: one address space).
struct DevicesRun {
  std::vector<mm3d_ctx *> roots;
  size_t D = 0, n = 0;
  std::vector<std::unique_ptr<mm3d_shard>> sh;            // per device: its own maps and its copies of the others'
  std::vector<std::vector<mm3d_pair_result>> rec;         // per device, by live-pair number
  std::vector<std::vector<unsigned char>> mine;
  std::vector<size_t> np;
  std::vector<double> t_feat, t_exch, t_pairs;
  RunClock clock;
};

// Round 5's form: three lock-step stages -- every device's features, barrier, every device pulls every other map, every
// device replays the WHOLE rand() stream for itself and runs its pairs, barrier.  Kept as the fallback of the pipelined form
// below (a map without keypoints falsifies its assumptions) and as its A/B (MM3D_DEVICES_STAGED=1).
static void devices_run_staged(mm3d_ctx *ctx, DevicesRun &R, const mm3d_cloud_view *clouds, const mm3d_params *params, size_t max_pairs)
{
  std::vector<mm3d_ctx *> &roots = R.roots;
  const size_t D = R.D, n = R.n;
  FailBarrier bar(D);
  std::mutex err_mu;
  std::exception_ptr first_error;
  for (size_t d = 1; d < D; ++d) roots[d]->rnd = ctx->rnd;        // every device replays the one rand() stream from the caller's state
  auto body = [&](size_t d) {
    mm3d_ctx *root = roots[d];
    // (the peers are reached only through this call, which holds the first context's lock: theirs is taken for the helpers'
    // sake of invariants only -- nothing else can be using them)
    std::unique_lock<std::mutex> peer_lock;
    if (d > 0) peer_lock = std::unique_lock<std::mutex>(root->mu);
    try {
      if (hipSetDevice(root->device) != hipSuccess) throw Error(MM3D_EDEVICE, "hipSetDevice failed");
      R.sh[d].reset(shard_begin_impl(root, clouds, n, params, (int)d, (int)D));
      R.t_feat[d] = R.clock.since_start();
      bar.wait();                                         // every owner's maps exist and its streams are drained
      // the other devices' maps: bundle + source-side structures straight from the owner's memory, dealt to this device's streams
      std::vector<size_t> theirs;
      for (size_t i = 0; i < n; ++i)
        if (!R.sh[d]->maps[i]) theirs.push_back(i);
      std::atomic<size_t> next{0};
      on_streams(root, [&](size_t, mm3d_ctx *c, const std::atomic<bool> &failed) {
        for (;;) {
          const size_t k = next.fetch_add(1);
          if (k >= theirs.size() || failed.load()) break;
          const size_t i = theirs[k];
          const size_t o = (size_t)mm3d_shard_map_owner(i, (int)D);
          // distinct slots; nobody reads another device's non-owned slots
          R.sh[d]->maps[i] = pull_map_from_peer(c, R.sh[o]->maps[i], roots[o]->device).release();
        }
      });
      R.t_exch[d] = R.clock.since_start();
      shard_pairs_impl(R.sh[d].get(), R.rec[d].data(), R.mine[d].data(), max_pairs, &R.np[d]);
      R.t_pairs[d] = R.clock.since_start();
      if (devices_debug()) fprintf(stderr, "mm3d devices (staged): dev%zu features %.2f ms, pulls done %.2f ms, pairs done %.2f ms (its own replay of every pair inside)\n", d,
                                   1e3 * R.t_feat[d], 1e3 * R.t_exch[d], 1e3 * R.t_pairs[d]);
      // an owner's maps are read by its peers' pulls: nobody leaves (and nothing is freed) before everybody has pulled
      bar.wait();
    } catch (...) {
      bar.fail();
      std::lock_guard<std::mutex> lk(err_mu);
      if (!first_error) first_error = std::current_exception();
    }
  };
  {
    std::vector<std::thread> threads;
    for (size_t d = 1; d < D; ++d) threads.emplace_back(body, d);
    body(0);
    for (auto &t : threads) t.join();
  }
  (void)hipSetDevice(ctx->device);
  if (first_error) {
    drain_devices(roots, ctx->device);
    std::rethrow_exception(first_error);
  }
}

// Round 6: the same split -- features by owner, pairs by target owner, peer copies in between -- WITHOUT the lock-step and
// WITHOUT D private replays of the rand() stream:
//   * ONE table of generator states (state_at[q] = the state before pair q of the reference's loop), filled once by one host
//     thread as the sources' keypoints appear (the draws of a pair depend on its source keypoints only) and read by every
//     device.  Before, each device replayed all n (n - 1) / 2 pairs itself: 8.5 us x 2 016 pairs = 17 ms of serial host work
//     per device on 64 x 50 k maps, the size of a device's whole pair stage at N = 8 ("host RNG replay dominates").
//   * per-map readiness: a map is published (a flag under the run's mutex, behind its owner's full stream wait) the moment its
//     owner has finished it; any device pulls it then (hipMemcpyPeerAsync on its own stream) and starts a pair as soon as the
//     pair's two maps are on the device and the pair's state is in the table.  Only the end of the call waits for everybody
//     (an owner's maps are read by its peers' pulls until then).
// The table assumes that a target which does not exist yet will have keypoints (as estimate_maps_streams does); the
// assumptions are checked when every map exists.  Returns false when one was wrong: the caller runs the staged form.
static bool devices_run_pipelined(mm3d_ctx *ctx, DevicesRun &R, const mm3d_cloud_view *clouds, const mm3d_params *params)
{
  std::vector<mm3d_ctx *> &roots = R.roots;
  const size_t D = R.D, n = R.n;
  const std::vector<std::pair<size_t, size_t>> all = all_pairs(n);
  const size_t P = all.size();
  for (size_t d = 0; d < D; ++d) {
    R.sh[d].reset(new mm3d_shard());
    R.sh[d]->ctx = roots[d]; R.sh[d]->rank = (int)d; R.sh[d]->world = (int)D; R.sh[d]->n = n; R.sh[d]->params = *params;
    R.sh[d]->maps.assign(n, nullptr);
  }
  std::mutex mu;                                          // guards everything below but the table
  std::condition_variable cv;
  std::vector<char> ready(n, 0);                          // map i is published by its owner
  std::vector<std::vector<char>> pull_claimed(D, std::vector<char>(n, 0)), have(D, std::vector<char>(n, 0));
  std::vector<char> claimed(P, 0);
  std::vector<std::vector<size_t>> own_maps(D), todo(D);  // per device: the maps it owns; the pairs whose target it owns
  std::vector<size_t> next_own(D, 0);
  for (size_t i = 0; i < n; ++i) own_maps[(size_t)mm3d_shard_map_owner(i, (int)D)].push_back(i);
  for (size_t q = 0; q < P; ++q) todo[(size_t)mm3d_shard_map_owner(all[q].second, (int)D)].push_back(q);
  bool abort = false;
  std::exception_ptr first_error;
  std::vector<mm3d_pair_result> rec_all(P);
  std::vector<char> done(P, 0);
  // the table
  std::vector<GlibcRand> state_at(P + 1, ctx->rnd);
  std::vector<char> assumed_live(P, 0);
  std::atomic<size_t> known_upto{0};                      // state_at[0 .. known_upto] are final
  double fill_busy_s = 0.0, fill_done_s = 0.0;            // (the filler thread's alone until it is joined)
  auto fill_table = [&] {
    try {
      for (size_t q = 0; q < P; ++q) {
        const size_t a = all[q].first, b = all[q].second;
        const mm3d_map *ma = nullptr;
        bool live = false;
        {
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [&] { return abort || ready[a]; });
          if (abort) return;
          ma = R.sh[(size_t)mm3d_shard_map_owner(a, (int)D)]->maps[a];
          live = ma->keypoints->n > 0;
          if (live) {
            if (ready[b]) live = R.sh[(size_t)mm3d_shard_map_owner(b, (int)D)]->maps[b]->keypoints->n > 0;
            else assumed_live[q] = 1;
          }
        }
        GlibcRand r = state_at[q];
        const auto tb = std::chrono::steady_clock::now();
        // (the host copy of an owner's keypoints was made when the map was prepared: no device is touched here)
        if (live) pair_replay_draws(r, ctx, params, cloud_host(roots[(size_t)mm3d_shard_map_owner(a, (int)D)], ma->keypoints));
        fill_busy_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - tb).count();
        fill_done_s = R.clock.since_start();
        state_at[q + 1] = r;
        known_upto.store(q + 1, std::memory_order_release);
        if ((q & 7) == 7 || q + 1 == P) { std::lock_guard<std::mutex> lk(mu); cv.notify_all(); }
      }
    } catch (...) {
      std::lock_guard<std::mutex> lk(mu);
      if (!first_error) first_error = std::current_exception();
      abort = true;
      cv.notify_all();
    }
  };
  auto device_body = [&](size_t d) {
    mm3d_ctx *root = roots[d];
    std::unique_lock<std::mutex> peer_lock;
    if (d > 0) peer_lock = std::unique_lock<std::mutex>(root->mu);
    const size_t S = root->helpers.size() + 1;
    try {
      if (hipSetDevice(root->device) != hipSuccess) throw Error(MM3D_EDEVICE, "hipSetDevice failed");
      on_streams(root, [&](size_t, mm3d_ctx *c, const std::atomic<bool> &failed) {
        // 1. this device's own maps, in index order
        for (;;) {
          size_t i;
          {
            std::lock_guard<std::mutex> lk(mu);
            if (abort || failed.load() || next_own[d] >= own_maps[d].size()) break;
            i = own_maps[d][next_own[d]++];
          }
          std::unique_ptr<mm3d_cloud> raw = cloud_from_view(c, clouds[i]);
          // this device is the map's target-side owner; the build ends in a full wait: the map is complete in this device's
          // memory BEFORE anybody is told
          std::unique_ptr<mm3d_map> held = build_private_map(c, raw.get(), params);
          raw.reset();
          {
            std::lock_guard<std::mutex> lk(mu);
            R.sh[d]->maps[i] = held.release();
            have[d][i] = 1;
            ready[i] = 1;
            R.t_feat[d] = std::max(R.t_feat[d], R.clock.since_start());
          }
          cv.notify_all();
        }
        // 2. pulls and pairs, whatever can start
        std::vector<size_t> batch;
        std::vector<PairWork> work;
        for (;;) {
          size_t pull = n;
          batch.clear();
          {
            std::unique_lock<std::mutex> lk(mu);
            for (;;) {
              if (abort || failed.load()) return;
              // a published map this device does not hold yet: first, it unlocks pairs
              for (size_t i = 0; i < n && pull == n; ++i)
                if (ready[i] && !have[d][i] && !pull_claimed[d][i]) pull = i;
              if (pull != n) { pull_claimed[d][pull] = 1; break; }
              // pairs of this device whose two maps are here and whose state is in the table: a batch shares its target
              const size_t known = known_upto.load(std::memory_order_acquire);
              size_t avail = 0, left = 0;
              for (size_t q : todo[d]) {
                if (claimed[q]) continue;
                ++left;
                if (q <= known && have[d][all[q].first] && have[d][all[q].second]) ++avail;
              }
              if (avail) {
                const size_t take = pair_batch_take(avail, S);
                size_t target = n;
                for (size_t q : todo[d]) {
                  if (batch.size() >= take) break;
                  if (claimed[q] || q > known || !have[d][all[q].first] || !have[d][all[q].second]) continue;
                  if (target != n && all[q].second != target) continue;
                  target = all[q].second;
                  claimed[q] = 1;
                  batch.push_back(q);
                }
                break;
              }
              bool pulls_left = false;
              for (size_t i = 0; i < n; ++i) pulls_left = pulls_left || (!have[d][i] && !pull_claimed[d][i]);
              if (!left && !pulls_left) return;           // nothing more for this worker, ever
              cv.wait(lk);
            }
          }
          if (pull != n) {
            const size_t o = (size_t)mm3d_shard_map_owner(pull, (int)D);
            // (the owner's copy is published: complete, and not freed before every thread has joined)
            std::unique_ptr<mm3d_map> m = pull_map_from_peer(c, R.sh[o]->maps[pull], roots[o]->device);
            {
              std::lock_guard<std::mutex> lk(mu);
              R.sh[d]->maps[pull] = m.release();
              have[d][pull] = 1;
              R.t_exch[d] = std::max(R.t_exch[d], R.clock.since_start());
            }
            cv.notify_all();
            continue;
          }
          work.clear();
          for (size_t q : batch) {
            const mm3d_map *ms = R.sh[d]->maps[all[q].first], *mt = R.sh[d]->maps[all[q].second];
            if (is_pair(ms, mt)) {
              rec_all[q].source_idx = all[q].first;
              rec_all[q].target_idx = all[q].second;
              work.push_back(PairWork{ms, mt, &rec_all[q], state_at[q]});
              done[q] = 1;                                // (distinct q per worker; read after the joins)
            }
          }
          if (!work.empty()) pairs_estimate_batch(c, work.data(), work.size(), params);
          { std::lock_guard<std::mutex> lk(mu); R.t_pairs[d] = std::max(R.t_pairs[d], R.clock.since_start()); }
        }
      });
    } catch (...) {
      std::lock_guard<std::mutex> lk(mu);
      if (!first_error) first_error = std::current_exception();
      abort = true;
      cv.notify_all();
    }
  };
  {
    std::thread filler(fill_table);
    std::vector<std::thread> threads;
    for (size_t d = 1; d < D; ++d) threads.emplace_back(device_body, d);
    device_body(0);
    for (auto &t : threads) t.join();
    { std::lock_guard<std::mutex> lk(mu); if (first_error) abort = true; }
    cv.notify_all();
    filler.join();
  }
  (void)hipSetDevice(ctx->device);
  if (first_error) {
    drain_devices(roots, ctx->device);
    std::rethrow_exception(first_error);
  }
  if (devices_debug()) {
    fprintf(stderr, "mm3d devices (pipelined): %zu devices, %zu maps, %zu pairs; ONE rand() table: %.2f ms of replay on one host thread, complete %.2f ms into the call "
            "(0 ms of replay on the devices' threads);", D, n, P, 1e3 * fill_busy_s, 1e3 * fill_done_s);
    for (size_t d = 0; d < D; ++d) fprintf(stderr, " dev%zu last map %.2f last pull %.2f last pair %.2f ms;", d, 1e3 * R.t_feat[d], 1e3 * R.t_exch[d], 1e3 * R.t_pairs[d]);
    fprintf(stderr, "\n");
  }
  // every map exists: were the table's assumptions right?
  for (size_t q = 0; q < P; ++q)
    if (assumed_live[q] && R.sh[0]->maps[all[q].second]->keypoints->n == 0) return false;
  ctx->rnd = state_at[P];                                 // where the reference's sequential loop leaves the generator
  // the live pairs in the reference's order, per executing device (what the gather sends)
  size_t nl = 0;
  for (size_t q = 0; q < P; ++q) {
    if (!done[q]) continue;
    const size_t d = (size_t)mm3d_shard_map_owner(all[q].second, (int)D);
    for (size_t e = 0; e < D; ++e) {
      pair_record_init(&R.rec[e][nl], all[q].first, all[q].second);
      R.mine[e][nl] = e == d ? 1 : 0;
    }
    R.rec[d][nl] = rec_all[q];
    ++nl;
  }
  for (size_t d = 0; d < D; ++d) R.np[d] = nl;
  return true;
}

void mm3d::estimate_maps_devices(mm3d_ctx *ctx, const mm3d_cloud_view *clouds, size_t n, const mm3d_params *params, float *out_T,
                                 size_t *n_out, mm3d_pair_result *pairs_out, size_t *n_pairs_out)
{
  std::vector<mm3d_ctx *> roots{ctx};
  roots.insert(roots.end(), ctx->peers.begin(), ctx->peers.end());
  const size_t D = roots.size();
  const size_t max_pairs = n * (n - 1) / 2;
  if (D == 1) {
    // a list of one device: nothing to shard, so the job runs as on a plain context (pipelined over the streams, not in
    // barriered stages) -- and its pair records still travel through the communicator's all-gather (a world of one), so that
    // the collective of the path is exercised wherever a device list is used
    std::vector<mm3d_pair_result> local(std::max<size_t>(max_pairs, 1));
    size_t np = 0;
    if (!ctx->helpers.empty()) estimate_maps_streams(ctx, clouds, n, params, out_T, n_out, local.data(), &np);
    else estimate_maps_sequential(ctx, clouds, n, params, out_T, n_out, local.data(), &np);
    const double t_before = ctx->last_total_s;
    std::vector<std::vector<mm3d_pair_result>> send(1);
    send[0].assign(local.begin(), local.begin() + (ptrdiff_t)np);
    std::vector<mm3d_pair_result> gathered;
    ctx->last_gather_s = gather_pair_records(ctx->device_set, roots, send, np, gathered);
    ctx->last_exchange_s = ctx->last_features_s;
    ctx->last_pairs_s = t_before;
    finish_run(gathered.data(), np, params, n, out_T, n_out, pairs_out, n_pairs_out);   // (from what the gather delivered)
    ctx->last_total_s = t_before + ctx->last_gather_s;
    return;
  }
  DevicesRun R;
  R.roots = roots; R.D = D; R.n = n;
  R.sh.resize(D);
  R.rec.assign(D, std::vector<mm3d_pair_result>(max_pairs));
  R.mine.assign(D, std::vector<unsigned char>(max_pairs, 0));
  R.np.assign(D, 0);
  R.t_feat.assign(D, 0.0); R.t_exch.assign(D, 0.0); R.t_pairs.assign(D, 0.0);
  R.clock = RunClock();
  static const bool staged_only = [] { const char *e = getenv("MM3D_DEVICES_STAGED"); return e && atoi(e); }();
  const GlibcRand rnd0 = ctx->rnd;
  bool ran = false;
  if (!staged_only) {
    ran = devices_run_pipelined(ctx, R, clouds, params);
    if (!ran) {                                           // a map without keypoints: the table was positioned wrongly after it
      for (size_t d = 0; d < D; ++d) { (void)hipSetDevice(roots[d]->device); R.sh[d].reset(); }
      (void)hipSetDevice(ctx->device);
      ctx->rnd = rnd0;
    }
  }
  if (!ran) devices_run_staged(ctx, R, clouds, params, max_pairs);
  ctx->last_points.assign(n, 0);
  ctx->last_keypoints.assign(n, 0);
  for (size_t i = 0; i < n; ++i) record_map_sizes(ctx, i, R.sh[0]->maps[i]);
  ctx->last_features_s = *std::max_element(R.t_feat.begin(), R.t_feat.end());
  ctx->last_exchange_s = *std::max_element(R.t_exch.begin(), R.t_exch.end());
  ctx->last_pairs_s = *std::max_element(R.t_pairs.begin(), R.t_pairs.end());
  // the gather: rank d sends the records of its own pairs, in pair order, padded to the largest rank's count
  const size_t P = R.np[0];
  for (size_t d = 1; d < D; ++d)
    if (R.np[d] != P) throw Error(MM3D_EDEVICE, "estimate_maps_devices: the devices disagree on the live pairs");
  std::vector<std::vector<mm3d_pair_result>> send(D);
  std::vector<std::vector<size_t>> which(D);
  for (size_t d = 0; d < D; ++d)
    for (size_t q = 0; q < P; ++q)
      if (R.mine[d][q]) { send[d].push_back(R.rec[d][q]); which[d].push_back(q); }
  size_t slots = 0;
  for (size_t d = 0; d < D; ++d) slots = std::max(slots, send[d].size());
  std::vector<mm3d_pair_result> gathered;
  ctx->last_gather_s = gather_pair_records(ctx->device_set, roots, send, slots, gathered);
  std::vector<mm3d_pair_result> pairs(P);
  std::vector<char> seen(P, 0);
  for (size_t d = 0; d < D; ++d)
    for (size_t k = 0; k < which[d].size(); ++k) {
      pairs[which[d][k]] = gathered[d * slots + k];
      seen[which[d][k]] = 1;
    }
  for (size_t q = 0; q < P; ++q)
    if (!seen[q]) throw Error(MM3D_EDEVICE, "estimate_maps_devices: a pair has no owner");
  // the shards (maps on every device) go now; every stream was drained by its device's thread
  for (size_t d = 0; d < D; ++d) {
    (void)hipSetDevice(roots[d]->device);
    R.sh[d].reset();
  }
  (void)hipSetDevice(ctx->device);
  finish_run(pairs.data(), pairs.size(), params, n, out_T, n_out, pairs_out, n_pairs_out);
  ctx->last_total_s = R.clock.since_start();
}

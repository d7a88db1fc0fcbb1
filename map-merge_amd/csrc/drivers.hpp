// drivers.hpp -- what the host files behind the extern "C" boundary share: capi.cpp (the boundary itself), pair_estimate.cpp
// (the map builders and the pair estimator) and the N-map drivers of mm3d_estimate_maps_transforms (driver_streams.cpp: one
// device; driver_shard.cpp: one process per device; driver_devices.cpp: a device list in one process).  Host code only: a
// kernel file includes this for its setter's sake (select_stage, stage_rules.hpp) and nothing else.  Everything declared between the
// visibility pragmas stays inside libmm3d.so.
#pragma once

#include <atomic>
#include <chrono>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "stage_rules.hpp"
#include "types.hpp"

// one rank's (or one device's) share of a job: the maps it owns and its copies of the others' (driver_shard.cpp)
struct mm3d_shard {
  mm3d_ctx *ctx = nullptr;
  int rank = 0, world = 1;
  size_t n = 0;
  mm3d_params params{};
  std::vector<mm3d_map *> maps;
  ~mm3d_shard()
  {
    for (mm3d_map *x : maps) delete x;
  }
};

// one pair of a batch: its two maps, where its record goes, and the generator state it starts from
struct PairWork { const mm3d_map *s, *t; mm3d_pair_result *out; mm3d::GlibcRand rnd; };

// Context::private_objects for a scope: what is built inside is the context's alone until the builder has drained the stream
// itself, so no waits for other contexts' sake while it is built (Context::settle)
namespace {
struct PrivateObjects {
  mm3d_ctx *c;
  explicit PrivateObjects(mm3d_ctx *c_) : c(c_) { c->private_objects = true; }
  PrivateObjects(const PrivateObjects &) = delete;
  ~PrivateObjects() { c->private_objects = false; }
};
}  // namespace

#pragma GCC visibility push(hidden)
namespace mm3d {

// (the one way a context's stage selection changes -- the seventeen setters, in their kernel files -- is stage_rules.hpp's select_stage)

// ---- pair_estimate.cpp: the map builders
std::unique_ptr<mm3d_cloud> cloud_from_view(mm3d_ctx *c, const mm3d_cloud_view &v);
std::unique_ptr<mm3d_map> make_map(std::unique_ptr<mm3d_cloud> points, std::unique_ptr<mm3d_cloud> keypoints, std::unique_ptr<mm3d_desc> desc);
mm3d_desc *desc_from_memory(mm3d_ctx *ctx, const float *data, size_t n, int descriptor_type);
// wait = false: the caller goes on in the same stream (map_prepare_impl) and waits once, there
std::unique_ptr<mm3d_map> map_features_impl(mm3d_ctx *ctx, const mm3d_cloud *raw, const mm3d_params *p, bool wait = true);
void map_prepare_impl(mm3d_ctx *ctx, mm3d_map *m, const mm3d_params *p);
std::unique_ptr<mm3d_map> build_private_map(mm3d_ctx *c, const mm3d_cloud *raw, const mm3d_params *p);
std::unique_ptr<mm3d_map> pull_map_from_peer(mm3d_ctx *c, const mm3d_map *src, int src_device);

// ---- pair_estimate.cpp: the pair estimator
void pair_estimate_impl(mm3d_ctx *ctx, const mm3d_map *s, const mm3d_map *t, const mm3d_params *p, bool execute, mm3d_pair_result *out);
void pairs_estimate_batch(mm3d_ctx *ctx, PairWork *w, size_t n, const mm3d_params *p);
size_t pair_batch_take(size_t avail, size_t S);
std::vector<std::pair<size_t, size_t>> all_pairs(size_t n);
// the draws one live pair takes from the reference's single rand() stream: they depend on its source keypoints (their host
// copy) only, and there are none under a prerejective alignment (replay_method)
void pair_replay_draws(GlibcRand &rnd, const mm3d_ctx *ctx, const mm3d_params *p, const std::vector<float4> &skp_host);
// an empty record of the pair (source, target)
void pair_record_init(mm3d_pair_result *r, size_t source, size_t target);
// the end of every driver: the pair records go out, and computeGlobalTransforms runs over them
void finish_run(const mm3d_pair_result *pairs, size_t n_pairs, const mm3d_params *params, size_t n, float *out_T, size_t *n_out,
                mm3d_pair_result *pairs_out, size_t *n_pairs_out);

// the reference's loop skips a pair unless both maps have keypoints (map_merging.cpp:250)
inline bool is_pair(const mm3d_map *s, const mm3d_map *t) { return s->keypoints->n > 0 && t->keypoints->n > 0; }
// what a run reports of map i (mm3d_last_run_map_sizes)
inline void record_map_sizes(mm3d_ctx *ctx, size_t i, const mm3d_map *m)
{
  ctx->last_points[i] = m->points->n;
  ctx->last_keypoints[i] = m->keypoints->n;
}
// seconds since the run began
struct RunClock {
  std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
  double since_start() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); }
};

// ---- the drivers
void estimate_maps_streams(mm3d_ctx *ctx, const mm3d_cloud_view *clouds, size_t n, const mm3d_params *params, float *out_T,
                           size_t *n_out, mm3d_pair_result *pairs_out, size_t *n_pairs_out);
void estimate_maps_sequential(mm3d_ctx *ctx, const mm3d_cloud_view *clouds, size_t n, const mm3d_params *params, float *out_T,
                              size_t *n_out, mm3d_pair_result *pairs_out, size_t *n_pairs_out);
void estimate_maps_devices(mm3d_ctx *ctx, const mm3d_cloud_view *clouds, size_t n, const mm3d_params *params, float *out_T,
                           size_t *n_out, mm3d_pair_result *pairs_out, size_t *n_pairs_out);
// driver_shard.cpp, for the device-list driver
mm3d_shard *shard_begin_impl(mm3d_ctx *ctx, const mm3d_cloud_view *clouds, size_t n, const mm3d_params *params, int rank, int world);
void shard_pairs_impl(mm3d_shard *sh, mm3d_pair_result *pairs, unsigned char *mine, size_t capacity, size_t *n_pairs);

}  // namespace mm3d
#pragma GCC visibility pop

// run fn(worker index, context, failed) on the context's streams (the caller's thread is worker 0); the first
// exception is rethrown.  `failed` is set when any worker has thrown: the others stop taking work.
template <class Fn>
static void on_streams(mm3d_ctx *ctx, Fn &&fn)
{
  std::vector<mm3d_ctx *> cs{ctx};
  cs.insert(cs.end(), ctx->helpers.begin(), ctx->helpers.end());
  std::mutex mu;
  std::exception_ptr first_error;
  std::atomic<bool> failed{false};
  auto body = [&](size_t w) {
    try {
      if (hipSetDevice(cs[w]->device) != hipSuccess) throw mm3d::Error(MM3D_EDEVICE, "hipSetDevice failed");
      fn(w, cs[w], failed);
      cs[w]->sync();
    } catch (...) {
      failed.store(true);
      std::lock_guard<std::mutex> lk(mu);
      if (!first_error) first_error = std::current_exception();
    }
  };
  std::vector<std::thread> threads;
  for (size_t w = 1; w < cs.size(); ++w) threads.emplace_back(body, w);
  body(0);
  for (auto &t : threads) t.join();
  for (mm3d_ctx *c : cs) (void)mm3d::stream_wait(c->stream);
  if (first_error) std::rethrow_exception(first_error);
}

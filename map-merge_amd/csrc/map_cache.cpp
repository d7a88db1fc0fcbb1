// map_cache.cpp -- the feature / pair cache of mm3d_estimate_maps_transforms (include/mm3d.h, mm3d_set_map_cache).
//
// The reference's caller runs estimateMapsTransforms on a timer with every robot's latest map (R/src/map_merge_node.cpp:
// 133-153), and most maps are the same from one tick to the next.  What a call computes is a pure function of inputs
// the library can compare exactly:
//   - a map's bundle (filtered points, keypoints, descriptor rows, the search structures map_prepare_impl builds) of the
//     cloud's packed 16-byte records and the parameters map_features_impl / map_prepare_impl read;
//   - a pair record of its two bundles and the parameters the pair stage reads -- and, under SAC_IA, of the glibc rand()
//     state it starts from (MATCHING's RANSAC seeds its own mt19937 per call).
// So a reused bundle or record is the bits the call would have computed.  Identity is content: a cached entry keeps its
// packed records on the device, and a map hits only when k_cloud_digest_compare (map_cache.hip) finds every record equal;
// the 128-bit digest only says which entry to compare with.  Entries are evicted least recently used; evicting a map
// drops the pair records that name it.  What a call adds is staged and committed only when the call succeeds.
#include <algorithm>
#include <atomic>
#include <unordered_map>

#include "types.hpp"

namespace mm3d {

namespace {

// the parameters a field at a time, doubles as their bits (mm3d_params has padding between its int and double members: it is
// never compared as memory)
struct KeyBuilder {
  std::string s;
  KeyBuilder &u64(uint64_t v) { s.append((const char *)&v, sizeof(v)); return *this; }
  KeyBuilder &i32(int v) { return u64((uint64_t)(uint32_t)v); }
  KeyBuilder &f64(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u64(u); }
};

// what map_features_impl and map_prepare_impl read
std::string feature_key(const mm3d_params *p, const StageSelection &sel)
{
  const mm3d_keypoint_options &kp = sel.keypoint_options;
  KeyBuilder k;
  k.f64(p->resolution).f64(p->descriptor_radius).i32(p->outliers_min_neighbours).f64(p->normal_radius).i32(p->keypoint_type)
      .f64(p->keypoint_threshold).i32(p->descriptor_type).f64(p->max_correspondence_distance).i32(p->estimation_method);
  // where the keypoints come from (mm3d_set_keypoints): a bundle of the reference's detectors is never a uniform one's, nor
  // one of another leaf (0 = the default, a function of descriptor_radius above; not read under the reference's detectors)
  k.i32(kp.source).f64(kp.source == MM3D_KEYPOINTS_UNIFORM ? kp.leaf : 0.0);
  // what filters the down-sampled cloud (mm3d_set_outlier_filter): a radius-filtered bundle is never a statistical one's, nor
  // one of other options (which the radius filter does not read: whatever they are, its bundles are shared)
  const mm3d_outlier_options &ol = sel.outlier_options;
  const bool stat = ol.method == MM3D_OUTLIERS_STATISTICAL;
  k.i32(stat ? ol.method : 0).i32(stat ? ol.mean_k : 0).f64(stat ? ol.stddev_mult : 0.0);
  // what drops the small clusters of the filtered cloud (mm3d_set_cluster_filter): zeros while it is off, whatever the other
  // two fields are; LARGEST does not read min_size
  const mm3d_cluster_options &cf = sel.cluster_options;
  const bool on = cf.method != MM3D_CLUSTERS_OFF;
  k.i32(on ? cf.method : 0).i32(cf.method == MM3D_CLUSTERS_MIN_SIZE ? cf.min_size : 0).f64(on ? cf.tolerance : 0.0);
  // what smooths the filtered cloud before the normals (mm3d_set_smoothing): zeros unless the method is MLS and the maps ask it
  // (the composed map is no bundle's business)
  const mm3d_smooth_options &sm = sel.smooth_options;
  const bool mls = sm.method == MM3D_SMOOTH_MLS && (sm.where & MM3D_SMOOTH_MAPS);
  k.i32(mls ? sm.method : 0).i32(mls ? sm.order : 0).i32(mls ? sm.min_neighbours : 0).f64(mls ? sm.radius : 0.0);
  // what takes the planes out of the filtered cloud (mm3d_set_planes): all nine fields, zeros while it is off
  const mm3d_plane_options &pl = sel.plane_options;
  const bool pon = pl.method != MM3D_PLANES_OFF;
  k.i32(pon ? pl.method : 0).i32(pon ? pl.max_planes : 0).i32(pon ? pl.samples : 0).i32(pon ? pl.refit : 0).i32(pon ? (int)pl.seed : 0);
  k.f64(pon ? pl.distance : 0.0).f64(pon ? pl.min_fraction : 0.0);
  for (int a = 0; a < 3; ++a) k.f64(pon ? pl.axis[a] : 0.0);
  k.f64(pon ? pl.max_angle_deg : 0.0);
  return k.s;
}

// what the pair stage reads (pair_estimate_impl / pairs_estimate_batch), and the ICP method (mm3d_set_icp_method): a
// point-to-point record is never one of point-to-plane's.  (The map key needs no method: the normals point-to-plane keeps are
// a function of the points and normal_radius.)
std::string pair_params_key(const mm3d_params *p, const StageSelection &sel)
{
  const mm3d_alignment_options &align = sel.align_options;
  const mm3d_refine_options &refine = sel.refine_options;
  const mm3d_coarse_options &coarse = sel.coarse_options;
  const mm3d_confidence_options &conf = sel.confidence_options;
  KeyBuilder k;
  k.i32(p->estimation_method).i32(p->refine_transform).f64(p->inlier_threshold).f64(p->max_correspondence_distance)
      .i32(p->max_iterations).u64(p->matching_k).f64(p->transform_epsilon).i32(sel.icp_method());
  // the alignment (mm3d_set_alignment): a SAC-IA record is never a prerejective one's, nor one of other options
  k.i32(align.method).i32(align.samples).i32(align.k).f64(align.similarity).f64(align.inlier_fraction);
  // the refinement (mm3d_set_refinement): an ICP record is never an NDT one's, nor an NDT one that of other options (which the
  // ICP does not read: whatever they are, its records are shared)
  const bool ndt = refine.method == MM3D_REFINE_NDT;
  k.i32(refine.method).f64(ndt ? refine.resolution : 0.0).i32(ndt ? refine.neighbours : 0).i32(ndt ? refine.min_points : 0)
      .f64(ndt ? refine.regularisation : 0.0);
  // the coarse alignment (mm3d_set_coarse_alignment): a correlative record is never one of the descriptor estimates, nor one of
  // other options (which nothing else reads: whatever they are, the other records are shared)
  const bool corr = coarse.method == MM3D_COARSE_CORRELATIVE;
  k.i32(coarse.method).f64(corr ? coarse.cell : 0.0).i32(corr ? coarse.cell_factor : 0).i32(corr ? coarse.yaw_steps : 0)
      .i32(corr ? coarse.yaw_factor : 0).i32(corr ? coarse.candidates : 0).f64(corr ? coarse.wall_nz : 0.0)
      .f64(corr ? coarse.ground_nz : 0.0).i32(corr ? coarse.min_points : 0).f64(corr ? coarse.accept_fraction : 0.0);
  // the confidence (mm3d_set_confidence): a record with the reference's confidence is never one with the overlap confidence,
  // nor an overlap one that of other options (which the reference's does not read: whatever they are, its records are shared)
  const bool ovl = conf.method == MM3D_CONFIDENCE_OVERLAP;
  k.i32(conf.method).f64(ovl ? conf.voxel : 0.0).i32(ovl ? conf.min_points : 0).f64(ovl ? conf.min_overlap : 0.0)
      .i32(ovl ? conf.view_margin : 0);
  // the ICP's correspondence rejection (mm3d_set_icp_rejection): the five options while the selection is active, zeros
  // otherwise (an inactive selection's other values are read by nothing: whatever they are, its records are shared)
  const mm3d_icp_rejection_options &rej = sel.reject_options;
  const bool rejecting = sel.rejecting();
  k.i32(rejecting ? rej.one_to_one : 0).i32(rejecting ? rej.distance : 0).f64(rejecting ? rej.overlap_ratio : 0.0)
      .i32(rejecting ? rej.min_correspondences : 0).f64(rejecting ? rej.median_factor : 0.0);
  // the geometric rejectors (mm3d_set_icp_geometry_rejection): the six options while the selection is active, zeros otherwise
  const mm3d_icp_geometry_options &geo = sel.geometry_options;
  const bool geometric = sel.geometric();
  k.i32(geometric ? geo.boundary : 0).f64(geometric ? geo.boundary_radius : 0.0).f64(geometric ? geo.boundary_angle_deg : 0.0)
      .i32(geometric ? geo.boundary_min_neighbours : 0).i32(geometric ? geo.normals : 0).f64(geometric ? geo.normal_angle_deg : 0.0);
  // coloured ICP (mm3d_set_icp_color): the four options while enabled, zeros otherwise (a disabled selection's other values
  // are read by nothing: whatever they are, its records are shared)
  const mm3d_icp_color_options &col = sel.color_options;
  const bool colored = col.enabled != 0;
  k.i32(colored ? col.enabled : 0).f64(colored ? col.lambda_geometric : 0.0).f64(colored ? col.gradient_radius : 0.0)
      .i32(colored ? col.min_neighbours : 0);
  // generalized ICP (mm3d_set_icp_generalized): (enabled, epsilon) while enabled, zeros otherwise
  const mm3d_icp_generalized_options &gen = sel.generalized_options;
  const bool generalized = gen.enabled != 0;
  k.i32(generalized ? gen.enabled : 0).f64(generalized ? gen.epsilon : 0.0);
  // the estimator under MATCHING (mm3d_set_estimator): a RANSAC record is never a consistency one's, nor a consistency one
  // that of other options (which RANSAC does not read: whatever they are, its records are shared)
  const mm3d_estimator_options &est = sel.estimator_options;
  const bool cons = est.method == MM3D_ESTIMATOR_CONSISTENCY;
  k.i32(cons ? est.method : 0).f64(cons ? est.tolerance : 0.0).i32(cons ? est.seeds : 0).i32(cons ? est.consensus : 0);
  // the ICP's source sampling (mm3d_set_icp_sampling): the four options while a method is set, zeros otherwise (nothing reads
  // the other values under NONE: whatever they are, its records are shared)
  const mm3d_icp_sampling_options &smp = sel.sampling_options;
  const bool sampling = smp.method != MM3D_ICP_SAMPLE_NONE;
  k.i32(sampling ? smp.method : 0).f64(sampling ? smp.fraction : 0.0).i32(sampling ? smp.max_points : 0).i32(sampling ? smp.bins : 0);
  // the ICP's robust kernel (mm3d_set_icp_robust): the five options while a kernel is selected, zeros otherwise (nothing reads the
  // other values under OFF: whatever they are, its records are shared)
  const mm3d_icp_robust_options &rob = sel.robust_options;
  const bool robust = sel.robust();
  k.i32(robust ? rob.kernel : 0).f64(robust ? rob.scale : 0.0).f64(robust ? rob.scale_start : 0.0).f64(robust ? rob.anneal : 0.0)
      .f64(robust ? rob.tuning : 0.0);
  return k.s;
}

size_t cloud_bytes(const mm3d_cloud *c)
{
  std::lock_guard<std::recursive_mutex> lk(const_cast<mm3d_cloud *>(c)->cache_mu);
  size_t b = c->pts.size() * 16 + c->hil_pts.size() * 16 + c->hil_keys.size() * 4 + c->wave_items.size() * 8;
  for (const auto &g : c->grids)
    b += g.second->cell_start.size() * 4 + g.second->sorted.size() * 16 + g.second->dt.size() + g.second->nb_start.size() * 4 +
         g.second->nb_pts.size() * 16;
  return b;
}

size_t desc_bytes(const mm3d_desc *d)
{
  return (d->data.size() + d->knn_colsum.size() + d->knn_Bp.size() + d->rf.size()) * 4 + (d->knn_nsort.size() + d->knn_nperm.size()) * 4;
}

struct Entry {
  uint64_t id = 0;
  std::string fkey;                      // feature_key of the parameters it was built with
  size_t n = 0;
  unsigned long long h0 = 0, h1 = 0;     // digest of the packed records
  std::unique_ptr<mm3d_cloud> raw;       // the packed records themselves (16 B per point), for the exact compare
  mm3d_map *map = nullptr;
  uint64_t tick = 0;                     // last call that used it (least recently used goes first)
  Entry() = default;
  Entry(const Entry &) = delete;
  Entry &operator=(const Entry &) = delete;
  ~Entry() { delete map; }
  size_t bytes() const
  {
    return raw->pts.size() * 16 + cloud_bytes(map->points) + cloud_bytes(map->keypoints) + desc_bytes(map->desc) +
           (map->normals ? map->normals->nrm.size() * 16 : 0) +   // (normals: point-to-plane ICP only)
           (map->ndt ? map->ndt->rec.size() * 16 + map->ndt->index.size() * 4 : 0) +   // (voxel table: NDT only)
           (map->coarse ? (map->coarse->scells.size() + map->coarse->gcells.size()) * 16 + map->coarse->ccells.size() * 8 +
                              map->coarse->dil.size() + map->coarse->gh.size() * 4 : 0) +   // (signature: correlative alignment only)
           (map->overlap ? map->overlap->near.size() * 8 + map->overlap->view.size() : 0) +   // (table: overlap confidence only)
           (map->color ? map->color->rec.size() * 16 : 0) +   // (gradient records: coloured ICP only)
           (map->icp_sample ? cloud_bytes(map->icp_sample->cloud.get()) : 0) +   // (the source sample: ICP sampling only)
           (map->boundary ? map->boundary->flags.size() : 0);   // (boundary flags: the boundary rejector only)
  }
};

struct PairRecord {
  mm3d_pair_result rec;
  uint64_t src = 0, tgt = 0;             // entry ids
  uint64_t tick = 0;
};

class MapCache final : public MapCacheBase {
 public:
  explicit MapCache(int max_maps) : max_maps_(max_maps) {}

  int max_maps() const { return max_maps_.load(); }
  void set_max_maps(int m)
  {
    std::lock_guard<std::mutex> lk(mu_);
    max_maps_ = m;
    evict_locked();
    bytes_ = held_bytes_locked();
  }
  void clear()
  {
    std::lock_guard<std::mutex> lk(mu_);
    pairs_.clear();
    entries_.clear();
    slot_hint_.clear();
    bytes_ = 0;
  }
  void stats(long long out[6], bool reset)
  {
    std::lock_guard<std::mutex> lk(mu_);
    for (int i = 0; i < 4; ++i) out[i] = counters_[i];
    out[4] = (long long)entries_.size();
    out[5] = (long long)bytes_;
    if (reset)
      for (long long &c : counters_) c = 0;
  }

  void begin(size_t n_maps, const mm3d_params *p, const StageSelection &sel) override
  {
    std::lock_guard<std::mutex> lk(mu_);
    reset_call_locked();
    fkey_ = feature_key(p, sel);
    pkey_ = pair_params_key(p, sel);
    // (the correlative alignment reads neither the generator nor its seed: no state in its pairs' keys)
    sac_ia_ = p->estimation_method == MM3D_EST_SAC_IA && sel.coarse_options.method != MM3D_COARSE_CORRELATIVE;
    prerej_ = sac_ia_ && sel.align_options.method == MM3D_ALIGN_PREREJECTIVE;
    slot_entry_.assign(n_maps, 0);
    slot_digest_.assign(n_maps, {0ull, 0ull});
    staged_.reserve(n_maps);             // (insert never reallocates: it cannot fail once it owns a map)
  }

  const mm3d_map *lookup(Context *c, size_t slot, const mm3d_cloud *raw) override
  {
    // the committed entries do not change while a call runs (they are only added or evicted by commit / abort / clear, under
    // the context's lock like the call itself): their records can be read without holding mu_
    const Entry *hint = nullptr;
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (slot < slot_hint_.size()) {
        auto it = entries_.find(slot_hint_[slot]);
        if (it != entries_.end() && it->second->n == raw->n && it->second->fkey == fkey_) hint = it->second.get();
      }
    }
    const CloudDigest d = cloud_digest_compare(c, raw->pts.get(), hint ? hint->raw->pts.get() : nullptr, raw->n, true);
    const Entry *found = d.equal ? hint : nullptr;
    if (!found) {
      // a map that moved to another slot (reordered, a new robot in front of it): the digest names the candidate, and the
      // exact compare still decides
      std::vector<const Entry *> cand;
      {
        std::lock_guard<std::mutex> lk(mu_);
        for (const auto &e : entries_)
          if (e.second.get() != hint && e.second->n == raw->n && e.second->h0 == d.h0 && e.second->h1 == d.h1 && e.second->fkey == fkey_)
            cand.push_back(e.second.get());
      }
      for (const Entry *e : cand)
        if (cloud_digest_compare(c, raw->pts.get(), e->raw->pts.get(), raw->n, false).equal) { found = e; break; }
    }
    std::lock_guard<std::mutex> lk(mu_);
    if (slot < slot_digest_.size()) slot_digest_[slot] = {d.h0, d.h1};
    if (!found) {
      ++call_[1];
      return nullptr;
    }
    ++call_[0];
    slot_entry_[slot] = found->id;
    return found->map;
  }

  void insert(size_t slot, std::unique_ptr<mm3d_cloud> raw, mm3d_map *m) override
  {
    auto e = std::make_unique<Entry>();
    e->fkey = fkey_;
    e->n = raw->n;
    std::lock_guard<std::mutex> lk(mu_);
    const std::pair<unsigned long long, unsigned long long> dg = slot < slot_digest_.size() ? slot_digest_[slot] : std::make_pair(0ull, 0ull);
    e->h0 = dg.first;
    e->h1 = dg.second;
    e->id = next_id_++;
    e->raw = std::move(raw);
    slot_entry_[slot] = e->id;
    e->map = m;                          // owned from here on (nothing below throws: staged_ has its room)
    staged_.push_back(std::move(e));
  }

  bool pair_lookup(size_t s, size_t t, const GlibcRand &rnd, mm3d_pair_result *out) override
  {
    std::lock_guard<std::mutex> lk(mu_);
    if (s >= slot_entry_.size() || t >= slot_entry_.size() || !slot_entry_[s] || !slot_entry_[t]) return false;
    const std::string key = pair_key(slot_entry_[s], slot_entry_[t], rnd);
    const PairRecord *r = nullptr;
    auto it = pairs_.find(key);
    if (it != pairs_.end()) {
      r = &it->second;
      touched_.push_back(key);
    } else {
      auto st = staged_pairs_.find(key);
      if (st != staged_pairs_.end()) r = &st->second;
    }
    if (!r) return false;
    *out = r->rec;
    out->source_idx = s;
    out->target_idx = t;
    ++call_[2];
    return true;
  }

  void pair_insert(size_t s, size_t t, const GlibcRand &rnd, const mm3d_pair_result &rec) override
  {
    std::lock_guard<std::mutex> lk(mu_);
    if (s >= slot_entry_.size() || t >= slot_entry_.size() || !slot_entry_[s] || !slot_entry_[t]) return;
    PairRecord r;
    r.rec = rec;
    r.src = slot_entry_[s];
    r.tgt = slot_entry_[t];
    staged_pairs_[pair_key(r.src, r.tgt, rnd)] = r;
    ++call_[3];
  }

  void commit() override
  {
    std::lock_guard<std::mutex> lk(mu_);
    for (auto &e : staged_) {
      const uint64_t id = e->id;
      entries_.emplace(id, std::move(e));
    }
    staged_.clear();
    // recency in slot order: with more maps than room, the call's last maps stay
    for (uint64_t id : slot_entry_) {
      auto it = entries_.find(id);
      if (it != entries_.end()) it->second->tick = ++tick_;
    }
    slot_hint_ = slot_entry_;
    for (const std::string &k : touched_) {
      auto it = pairs_.find(k);
      if (it != pairs_.end()) it->second.tick = ++tick_;
    }
    for (auto &kv : staged_pairs_) {
      kv.second.tick = ++tick_;
      pairs_[kv.first] = kv.second;
    }
    for (int i = 0; i < 4; ++i) counters_[i] += call_[i];
    evict_locked();
    bytes_ = held_bytes_locked();
    reset_call_locked();
  }

  void abort() noexcept override
  {
    std::lock_guard<std::mutex> lk(mu_);
    reset_call_locked();
  }

 private:
  std::string pair_key(uint64_t src, uint64_t tgt, const GlibcRand &rnd) const
  {
    KeyBuilder k;
    k.s = pkey_;
    k.u64(src).u64(tgt);
    if (prerej_) {                       // prerejective alignment (mm3d_set_alignment) reads the seed and draws nothing from rand()
      k.i32((int)rnd.seed0);
    } else if (sac_ia_) {                // the whole generator state the pair starts from
      for (uint32_t w : rnd.ring) k.i32((int)w);
      k.i32(rnd.f).i32(rnd.b);
    }
    return k.s;
  }

  void reset_call_locked() noexcept
  {
    staged_.clear();                     // (a failed call's bundles: their buffers go back to the pools that made them)
    staged_pairs_.clear();
    touched_.clear();
    slot_entry_.clear();
    for (long long &c : call_) c = 0;
    slot_digest_.clear();
  }

  void evict_locked()
  {
    // pair records first: they live as long as both their maps, and at most 4 * max_maps^2 of them stay (parameters and
    // generator states that do not come back would otherwise pile up)
    while ((int)entries_.size() > max_maps_) {
      auto victim = std::min_element(entries_.begin(), entries_.end(), [](const auto &a, const auto &b) { return a.second->tick < b.second->tick; });
      const uint64_t id = victim->first;
      for (auto it = pairs_.begin(); it != pairs_.end();)
        it = (it->second.src == id || it->second.tgt == id) ? pairs_.erase(it) : std::next(it);
      entries_.erase(victim);
    }
    const size_t cap = 4 * (size_t)max_maps_ * (size_t)max_maps_;
    if (pairs_.size() > cap) {
      std::vector<uint64_t> ticks;
      ticks.reserve(pairs_.size());
      for (const auto &kv : pairs_) ticks.push_back(kv.second.tick);
      std::nth_element(ticks.begin(), ticks.begin() + (pairs_.size() - cap), ticks.end());
      const uint64_t keep_from = ticks[pairs_.size() - cap];       // ticks are distinct: exactly `cap` are >= it
      for (auto it = pairs_.begin(); it != pairs_.end();) it = it->second.tick < keep_from ? pairs_.erase(it) : std::next(it);
    }
  }

  size_t held_bytes_locked() const
  {
    size_t b = 0;
    for (const auto &e : entries_) b += e.second->bytes();
    return b;
  }

  std::mutex mu_;
  std::atomic<int> max_maps_;
  std::map<uint64_t, std::unique_ptr<Entry>> entries_;             // committed, by id
  std::unordered_map<std::string, PairRecord> pairs_;              // committed, by pair key
  std::vector<uint64_t> slot_hint_;                                // the entry each input slot had in the last committed call
  uint64_t next_id_ = 1, tick_ = 0;
  long long counters_[4] = {0, 0, 0, 0};                           // map hits, misses, pairs reused, pairs computed
  size_t bytes_ = 0;
  // the running call
  std::string fkey_, pkey_;
  bool sac_ia_ = false;
  bool prerej_ = false;
  std::vector<uint64_t> slot_entry_;                               // 0: none (not yet looked up, or not cached)
  std::vector<std::pair<unsigned long long, unsigned long long>> slot_digest_;
  std::vector<std::unique_ptr<Entry>> staged_;
  std::unordered_map<std::string, PairRecord> staged_pairs_;
  std::vector<std::string> touched_;
  long long call_[4] = {0, 0, 0, 0};
};

}  // namespace

}  // namespace mm3d

using mm3d::MapCache;

extern "C" {

int mm3d_set_map_cache(mm3d_ctx *ctx, int max_maps)
{
  if (!ctx || max_maps < 0) return MM3D_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the cache changes)
  if (ctx->device_set) {
    ctx->err = "mm3d_set_map_cache: not available on a device-list context";
    return MM3D_EUNSUPPORTED;
  }
  try {
    if (max_maps == 0) {
      delete ctx->map_cache;
      ctx->map_cache = nullptr;
    } else if (ctx->map_cache) {
      static_cast<MapCache *>(ctx->map_cache)->set_max_maps(max_maps);
    } else {
      ctx->map_cache = new MapCache(max_maps);
    }
  } catch (const std::bad_alloc &) {
    ctx->err = "out of host memory";
    return MM3D_ENOMEM;
  }
  return MM3D_OK;
}

int mm3d_get_map_cache(const mm3d_ctx *ctx) { return ctx && ctx->map_cache ? static_cast<const MapCache *>(ctx->map_cache)->max_maps() : 0; }

void mm3d_map_cache_clear(mm3d_ctx *ctx)
{
  if (!ctx) return;
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (ctx->map_cache) static_cast<MapCache *>(ctx->map_cache)->clear();
}

int mm3d_map_cache_stats(const mm3d_ctx *ctx, long long out[6], int reset)
{
  if (!ctx || !out) return MM3D_EINVAL;
  if (!ctx->map_cache) {
    for (int i = 0; i < 6; ++i) out[i] = 0;
    return MM3D_OK;
  }
  static_cast<MapCache *>(ctx->map_cache)->stats(out, reset != 0);
  return MM3D_OK;
}

}  // extern "C"

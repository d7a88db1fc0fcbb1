// pair_estimate.cpp -- what every driver of mm3d_estimate_maps_transforms is made of: a map built and prepared from a caller's
// cloud (or pulled from a peer device), and the estimate of one pair or of a batch of pairs.  Nothing here is exported; the
// extern "C" calls over it are in capi.cpp.
#include <algorithm>
#include <cfloat>
#include <cstdlib>

#include "device_util.hpp"
#include "capi_guard.hpp"
#include "drivers.hpp"

using namespace mm3d;

// mm3d_set_keypoints with leaf = 0: the leaf is descriptor_radius over this (DESIGN.md section 7d has the measurement)
static constexpr double kUniformLeafDivisor = 2.0;
// a caller's view of a map, uploaded; a null / empty map (robot subscribed but no message yet) counts as "no keypoints"
std::unique_ptr<mm3d_cloud> mm3d::cloud_from_view(mm3d_ctx *c, const mm3d_cloud_view &v)
{
  return std::unique_ptr<mm3d_cloud>(cloud_from_memory(c, v.points, v.points ? v.n : 0, v.stride ? v.stride : 16, v.stride ? v.rgba_offset : 12));
}
std::unique_ptr<mm3d_map> mm3d::make_map(std::unique_ptr<mm3d_cloud> points, std::unique_ptr<mm3d_cloud> keypoints, std::unique_ptr<mm3d_desc> desc)
{
  std::unique_ptr<mm3d_map> m(new mm3d_map());
  m->points = points.release(); m->keypoints = keypoints.release(); m->desc = desc.release();
  return m;
}
mm3d_desc *mm3d::desc_from_memory(mm3d_ctx *ctx, const float *data, size_t n, int descriptor_type)
{
  const int dim = mm3d_descriptor_dim(descriptor_type);
  if (dim < 0) throw Error(MM3D_EINVAL, "unknown descriptor type");
  std::unique_ptr<mm3d_desc> r(new mm3d_desc());
  r->n = n; r->dim = dim; r->type = descriptor_type;
  r->data = DevBuf<float>(ctx, n * dim);
  if (n) {
    MM3D_HIP(hipMemcpyAsync(r->data.get(), data, n * dim * sizeof(float), hipMemcpyDefault, ctx->stream));
    ctx->sync();
  }
  return r.release();
}
// wait = false: the caller goes on in the same stream (map_prepare_impl) and waits once, there
std::unique_ptr<mm3d_map> mm3d::map_features_impl(mm3d_ctx *ctx, const mm3d_cloud *raw, const mm3d_params *p, bool wait)
{
  if (p->keypoint_type != MM3D_KP_SIFT && p->keypoint_type != MM3D_KP_HARRIS) throw Error(MM3D_EINVAL, "invalid keypoint type");
  if (p->descriptor_type < 0 || p->descriptor_type >= 6) throw Error(MM3D_EINVAL, "unknown descriptor type");   // dispatch_descriptors.h:63
  std::unique_ptr<mm3d_cloud> down(downsample(ctx, raw, p->resolution));
  // NB: the outlier radius is the DESCRIPTOR radius (map_merging.cpp:219-220)
  // (mm3d_set_outlier_filter: the statistical rule in its place; outliers_min_neighbours is then not read)
  std::unique_ptr<mm3d_cloud> filt(ctx->sel.outliers ? ctx->sel.outliers->filter(ctx, down.get(), ctx->sel.outlier_options, &ctx->last_outlier_stats)
                                                     : remove_outliers(ctx, down.get(), p->descriptor_radius, p->outliers_min_neighbours));
  down.reset();
  // (mm3d_set_planes: the dominant planes leave, or are set aside while the cluster filter looks at the rest; the stage calls the
  // cluster filter itself, so that what stands on a floor is a cluster of its own when the filter sees it)
  if (ctx->sel.planes) {
    mm3d_cloud *res = ctx->sel.planes->filter(ctx, filt.get(), ctx->sel.plane_options, p->resolution, ctx->sel.clusters, ctx->sel.cluster_options,
                                              &ctx->last_plane_stats, ctx->last_planes, &ctx->last_cluster_stats);
    if (res != filt.get()) filt.reset(res);
  }
  // (mm3d_set_cluster_filter: the connected components too small to be structure leave before anything looks at the cloud)
  else if (ctx->sel.clusters) filt.reset(ctx->sel.clusters->filter(ctx, filt.get(), ctx->sel.cluster_options, p->resolution, &ctx->last_cluster_stats));
  // (mm3d_set_smoothing with MM3D_SMOOTH_MAPS: after the filters -- a stray blob would pull the surface towards itself -- and
  // before everything that reads the points; the new cloud's voxel_leaf is 0)
  if (ctx->sel.smoother && (ctx->sel.smooth_options.where & MM3D_SMOOTH_MAPS))
    filt.reset(ctx->sel.smoother->smooth(ctx, filt.get(), ctx->sel.smooth_options, p->resolution, &ctx->last_smooth_stats));
  // computeSurfaceNormals, then detectKeypoints(points, normals, type, keypoint_threshold, normal_radius, resolution)
  // (map_merging.cpp:225-233).  SIFT does not read the normals, and its first octave builds every point's sorted
  // neighbour list over a ball that contains the normals': the two stages share that launch (sift.hip), same bits.
  std::unique_ptr<mm3d_normals> nrm;
  std::unique_ptr<mm3d_cloud> kp;
  if (ctx->sel.keypoints) {
    // mm3d_set_keypoints: no detector runs (keypoint_type and keypoint_threshold are not read); the normals come from their
    // stand-alone launch, since SIFT's fused first octave does not run
    nrm.reset(compute_normals(ctx, filt.get(), p->normal_radius));
    const double leaf = ctx->sel.keypoint_options.leaf > 0.0 ? ctx->sel.keypoint_options.leaf : p->descriptor_radius / kUniformLeafDivisor;
    kp.reset(ctx->sel.keypoints->keypoints(ctx, filt.get(), leaf));
  } else if (p->keypoint_type == MM3D_KP_HARRIS) {
    nrm.reset(compute_normals(ctx, filt.get(), p->normal_radius));
    kp.reset(detect_keypoints_harris(ctx, filt.get(), nrm.get(), p->keypoint_threshold, p->normal_radius));
  } else {
    mm3d_normals *n_out = nullptr;
    static const bool share_grid = [] { const char *e = getenv("MM3D_SIFT_NO_SHARED_GRID"); return !(e && atoi(e)); }();   // A/B knob
    // (every descriptor searches `filt` on a grid of descriptor_radius / 2 cells: the first octave uses that one too)
    kp.reset(detect_keypoints_sift(ctx, filt.get(), p->resolution, 3, 3, p->keypoint_threshold, p->normal_radius, &n_out,
                                   share_grid ? (float)(p->descriptor_radius * 0.5) : 0.0f));
    nrm.reset(n_out);
  }
  std::unique_ptr<mm3d_desc> desc(p->descriptor_type == MM3D_DESC_PFH    ? compute_pfh(ctx, filt.get(), nrm.get(), kp.get(), p->descriptor_radius)
                                  : p->descriptor_type == MM3D_DESC_SC3D ? compute_sc3d(ctx, filt.get(), nrm.get(), kp.get(), p->descriptor_radius)
                                  : p->descriptor_type == MM3D_DESC_RSD ? compute_rsd(ctx, filt.get(), nrm.get(), kp.get(), p->descriptor_radius)
                                  : p->descriptor_type == MM3D_DESC_PFHRGB ? compute_pfhrgb(ctx, filt.get(), nrm.get(), kp.get(), p->descriptor_radius)
                                  : p->descriptor_type == MM3D_DESC_SHOT ? compute_shot(ctx, filt.get(), nrm.get(), kp.get(), p->descriptor_radius)
                                                                         : compute_fpfh(ctx, filt.get(), nrm.get(), kp.get(), p->descriptor_radius));
  if (wait) ctx->sync();
  std::unique_ptr<mm3d_map> m = make_map(std::move(filt), std::move(kp), std::move(desc));
  // point-to-plane, coloured and generalized ICP read them (mm3d_set_icp_method, mm3d_set_icp_color, mm3d_set_icp_generalized),
  // the correlative signature, normal-space sampling (mm3d_set_icp_sampling), and the geometric rejectors: the boundary flags are
  // made from them, the normal test reads them (mm3d_set_icp_geometry_rejection)
  const bool normal_space = ctx->sel.sampler && ctx->sel.sampling_options.method == MM3D_ICP_SAMPLE_NORMAL_SPACE;
  if (ctx->sel.icp || ctx->sel.coarse || ctx->sel.color || ctx->sel.generalized || normal_space || ctx->sel.geometry_options.normals == 1 ||
      ctx->sel.geometry_options.boundary == 1)
    m->normals = std::move(nrm);
  return m;
}

void mm3d::map_prepare_impl(mm3d_ctx *ctx, mm3d_map *m, const mm3d_params *p)
{
  const StageSelection &sel = ctx->sel;
  if (sel.icp) sel.icp->prepare_target(ctx, m, p, nullptr);            // the normals (mm3d_set_icp_method): no wait when the map has them
  if (sel.refine) sel.refine->prepare_target(ctx, m, p, nullptr);      // NDT's voxel table (mm3d_set_refinement)
  if (sel.color) sel.color->prepare_target(ctx, m, p, nullptr);        // the normals and the gradient records (mm3d_set_icp_color)
  if (sel.generalized) sel.generalized->prepare_target(ctx, m, p, nullptr);   // the normals, for either role (mm3d_set_icp_generalized)
  if (sel.coarse) sel.coarse->prepare(ctx, m, p);                      // the correlative signature (mm3d_set_coarse_alignment)
  if (sel.confidence) sel.confidence->prepare(ctx, m, p);              // the overlap table (mm3d_set_confidence)
  if (sel.sampler && p->refine_transform) (void)sel.sampler->sample(ctx, m, p, nullptr);   // the ICP's source sample (mm3d_set_icp_sampling)
  if (sel.geometry && p->refine_transform) sel.geometry->prepare(ctx, m, p);   // the normals and the boundary flags (mm3d_set_icp_geometry_rejection)
  prepare_pair_search(ctx, m->points, p->max_correspondence_distance, p->max_correspondence_distance);
  if (p->estimation_method == MM3D_EST_SAC_IA && sel.align) sel.align->prepare(ctx, m->keypoints, p->max_correspondence_distance);
  else if (p->estimation_method == MM3D_EST_SAC_IA) prepare_sacia_target(ctx, m->keypoints, (float)p->max_correspondence_distance);
  desc_knn_prepare_target(ctx, m->desc);
  (void)cloud_host(ctx, m->keypoints, false);       // (the keypoints' host copy rides on the wait below)
  ctx->sync();                                       // everything complete, the error flags the kernels left looked at
}

// A map built and prepared on one worker's context, for a driver that publishes it afterwards: nobody else sees it before
// map_prepare_impl's full wait -- which also looks at the error flags the kernels left -- and a throw strands nothing.
std::unique_ptr<mm3d_map> mm3d::build_private_map(mm3d_ctx *c, const mm3d_cloud *raw, const mm3d_params *p)
{
  PrivateObjects priv(c);
  std::unique_ptr<mm3d_map> m = map_features_impl(c, raw, p, false);
  map_prepare_impl(c, m.get(), p);                     // (ends in that wait)
  return m;
}

// A map another device owns, for the SOURCE role on context c (as mm3d_shard_unpack): bundle and source-side structures
// straight from the owner's memory, then whatever of the query orders / host copy did not come with the clone
std::unique_ptr<mm3d_map> mm3d::pull_map_from_peer(mm3d_ctx *c, const mm3d_map *src, int src_device)
{
  PrivateObjects priv(c);                              // (nobody sees the copy before the wait below)
  std::unique_ptr<mm3d_cloud> pts(cloud_clone_from_peer(c, src->points, src_device));
  std::unique_ptr<mm3d_cloud> kp(cloud_clone_from_peer(c, src->keypoints, src_device));
  std::unique_ptr<mm3d_desc> desc(desc_clone_from_peer(c, src->desc, src_device));
  if (pts->n) cloud_hilbert(c, pts.get());
  if (kp->n) cloud_hilbert(c, kp.get());
  (void)cloud_host(c, kp.get());
  c->sync();
  return make_map(std::move(pts), std::move(kp), std::move(desc));
}

void mm3d::pair_replay_draws(GlibcRand &rnd, const mm3d_ctx *ctx, const mm3d_params *p, const std::vector<float4> &skp_host)
{
  pair_rand_replay(rnd, ctx->sel.replay_method(p), skp_host, p->inlier_threshold, p->max_iterations);
}

// what an estimate fills in, cleared; source_idx / target_idx are the caller's
static void clear_estimate(mm3d_pair_result *out)
{
  std::memset(out->transform, 0, sizeof(out->transform));
  out->confidence = 0.0;
  out->icp_iterations = 0;
  out->n_correspondences = out->n_inliers = out->icp_correspondences = 0;
}
void mm3d::pair_record_init(mm3d_pair_result *r, size_t source, size_t target)
{
  std::memset(r, 0, sizeof(*r));
  r->source_idx = source;
  r->target_idx = target;
}

void mm3d::pair_estimate_impl(mm3d_ctx *ctx, const mm3d_map *s, const mm3d_map *t, const mm3d_params *p, bool execute,
                             mm3d_pair_result *out)
{
  if (execute && ctx->sel.batch_only(p)) {
    // a batch of one, from (and advancing) the context's generator
    PairWork w{s, t, out, ctx->rnd};
    pairs_estimate_batch(ctx, &w, 1, p);
    return;
  }
  clear_estimate(out);
  if (ctx->sel.coarse || ctx->sel.prerejective(p)) return;   // not executed, and nothing to replay (mm3d_set_alignment, mm3d_set_coarse_alignment)
  // estimateTransform and transformScore of its result (R/src/map_merging.cpp:91-107) as one device
  // pipeline: the transform never visits the host in between
  double score = DBL_MAX;
  PairCounts counts;
  const int iters = estimate_pair(ctx, s->points, s->keypoints, s->desc, t->points, t->keypoints, t->desc,
                                  p->estimation_method, p->refine_transform, p->inlier_threshold,
                                  p->max_correspondence_distance, p->max_iterations, (size_t)p->matching_k,
                                  p->transform_epsilon, out->transform, execute, true, p->max_correspondence_distance, &score, &counts);
  if (!execute) return;
  out->icp_iterations = iters;
  out->n_correspondences = counts.n_correspondences;
  out->n_inliers = counts.n_inliers;
  out->icp_correspondences = counts.icp_correspondences;
  out->confidence = 1.0 / score;
}

constexpr size_t kPairBatch = 16;     // pairs whose tails and scoring share launches
// the two experiment knobs of the pair batches, validated once (a share <= 0 or not a number would divide by zero and cast
// inf to size_t; a batch cap of 0 would never claim a pair and leave the scheduler waiting for ever)
static double pair_share_knob()
{
  static const double v = [] {
    const char *e = getenv("MM3D_PAIR_SHARE");
    double s = e ? atof(e) : 0.25;
    if (!(s >= 1.0 / 64.0)) s = 1.0 / 64.0;           // (also catches NaN)
    return std::min(s, 64.0);
  }();
  return v;
}
static size_t pair_batch_knob()
{
  static const size_t v = [] {
    const char *e = getenv("MM3D_PAIR_BATCH");
    const long b = e ? atol(e) : (long)kPairBatch;
    return (size_t)std::min<long>(std::max<long>(b, 1), 32);      // (32: the largest batch ever run)
  }();
  return v;
}
// How large a batch, of `avail` pairs that can start now on S streams: round 4 measured take = avail / (share * S) on the headline
// (16 streams, 120 pairs trickling in behind the feature stage): share 4 / 2 / 1 / 0.5 / 0.25 / 0.125 -> 989 / 990 / 1004 / 1013 /
// 1021 / 1022 map-pairs/s.  The pair stage's kernels are latency-bound and only four run at a time (hardware queues), so a launch
// that serves four pairs costs little more queue time than one that serves one; with share 2 most batches were a single pair.
// (The cap is an experiment knob: 8 / 16 / 32 the same.)
size_t mm3d::pair_batch_take(size_t avail, size_t S)
{
  return std::min(pair_batch_knob(), std::max<size_t>(1, (size_t)((double)avail / (pair_share_knob() * (double)S))));
}
// every pair of n maps, in the order of the reference's loop (map_merging.cpp:256-269)
std::vector<std::pair<size_t, size_t>> mm3d::all_pairs(size_t n)
{
  std::vector<std::pair<size_t, size_t>> all;
  for (size_t i = 0; i + 1 < n; ++i)
    for (size_t j = i + 1; j < n; ++j) all.emplace_back(i, j);
  return all;
}

// Several pairs on one context: the initial estimates one after the other (each from its own generator state),
// then every pair's ICP + score tail in lockstep, one launch per step for the whole batch (icp_score_batch).
void mm3d::pairs_estimate_batch(mm3d_ctx *ctx, PairWork *w, size_t n, const mm3d_params *p)
{
  std::vector<PairFront> fronts(n);
  std::vector<IcpScoreJob> jobs(n);
  std::vector<SacPrepared> prepared;
  const StageSelection &sel = ctx->sel;
  for (size_t i = 0; i < n; ++i) {
    mm3d_pair_result *out = w[i].out;
    clear_estimate(out);
    ctx->rnd = w[i].rnd;
    if (sel.coarse) {
      // no keypoints, no descriptors, nothing of the generator: the two maps' signatures
      sel.coarse->front(ctx, w[i].s, w[i].t, p, fronts[i], &ctx->last_coarse_stats);
    } else if (sel.prerejective(p)) {
      // the same inputs, max_correspondence_distance as the inlier distance; the generator's seed, none of its draws
      sel.align->front(ctx, sel.align_options, w[i].rnd.seed0, w[i].s->keypoints, w[i].s->desc, w[i].t->keypoints, w[i].t->desc,
                       p->max_correspondence_distance, fronts[i], &ctx->last_align_stats);
    } else if (sel.consistency(p)) {
      // the same correspondences, the consistency graph in RANSAC's place (mm3d_set_estimator); nothing of the generator
      sel.estimator->front(ctx, sel.estimator_options, w[i].s->keypoints, w[i].s->desc, w[i].t->keypoints, w[i].t->desc,
                           p->inlier_threshold, (size_t)p->matching_k, fronts[i], &ctx->last_estimator_stats);
    } else if (p->estimation_method == MM3D_EST_SAC_IA) {
      // argument mapping of matching.cpp:243-246: min_sample_distance := inlier_threshold
      sac_ia_replay(ctx, w[i].s->keypoints, w[i].s->desc, w[i].t->keypoints, w[i].t->desc, p->inlier_threshold, p->max_iterations, true,
                    fronts[i]);
      prepared.push_back(SacPrepared{w[i].s->keypoints, w[i].t->keypoints, w[i].s->desc, w[i].t->desc, &fronts[i]});
    } else {
      estimate_pair_front(ctx, w[i].s->keypoints, w[i].s->desc, w[i].t->keypoints, w[i].t->desc, p->estimation_method,
                          p->inlier_threshold, p->max_correspondence_distance, p->max_iterations, (size_t)p->matching_k, true, fronts[i]);
    }
  }
  if (!prepared.empty()) {
    // the sampled rows of every pair with the same target go through one descriptor search, and the hypotheses of
    // all the batch's pairs are scored by the same five launches
    std::stable_sort(prepared.begin(), prepared.end(), [](const SacPrepared &a, const SacPrepared &b) { return a.td < b.td; });
    std::vector<DevBuf<int>> nn_owners;
    std::vector<DevBuf<float>> nd_owners;
    for (size_t a = 0; a < prepared.size();) {
      size_t b = a;
      while (b < prepared.size() && prepared[b].td == prepared[a].td) ++b;
      nn_owners.emplace_back();
      nd_owners.emplace_back();
      sac_ia_knn(ctx, &prepared[a], (int)(b - a), nn_owners.back(), nd_owners.back());
      a = b;
    }
    sac_ia_finish(ctx, prepared.data(), (int)prepared.size(), p->max_correspondence_distance);
  }
  for (size_t i = 0; i < n; ++i) {
    jobs[i].src = w[i].s->points;
    jobs[i].tgt = w[i].t->points;
    jobs[i].guess_dev = fronts[i].on_device ? fronts[i].dT0.get() : nullptr;
    std::memcpy(jobs[i].guess_host, fronts[i].T0, sizeof(fronts[i].T0));
    // (mm3d_set_icp_rejection; NDT does not read it.  An active mm3d_set_icp_geometry_rejection takes the rejecting step too.)
    if (sel.rejecting() || sel.geometric()) jobs[i].reject = &sel.reject_options;
    if (sel.geometry && p->refine_transform && !sel.refine) sel.geometry->bind(ctx, w[i].s, w[i].t, p, &jobs[i]);
    if (sel.robust()) jobs[i].robust = &sel.robust_options;            // (mm3d_set_icp_robust; point-to-point and point-to-plane read it)
    // (mm3d_set_icp_sampling: the ICP searches with the source map's sample, the score stays over the map)
    if (sel.sampler && p->refine_transform) jobs[i].icp_src = sel.sampler->sample(ctx, w[i].s, p, &ctx->last_sampling_stats);
  }
  // estimateTransform's ICP and transformScore of its result (R/src/map_merging.cpp:91-107), max_distance = max_correspondence_distance
  // (under mm3d_set_confidence nobody reads that score: it is not launched, and the ICP's states come back as they would have)
  const bool want_score = !sel.confidence;
  // NDT in the ICP's place (mm3d_set_refinement), else coloured ICP (mm3d_set_icp_color), else generalized ICP
  // (mm3d_set_icp_generalized), else point-to-plane (mm3d_set_icp_method), else the reference's ICP; a method binds what it keeps
  // on the targets (voxel tables, normals, gradient records) and on the sources (generalized ICP's normals) to the jobs first
  const IcpMethodBase *tail = sel.refine ? sel.refine : sel.color ? sel.color : sel.generalized ? sel.generalized : sel.icp;
  if (tail && p->refine_transform)
    for (size_t i = 0; i < n; ++i) {
      tail->prepare_target(ctx, w[i].t, p, &jobs[i]);
      tail->prepare_source(ctx, w[i].s, p, &jobs[i]);
    }
  icp_score_batch(ctx, tail, jobs.data(), (int)n, p->refine_transform != 0, p->max_correspondence_distance, p->max_iterations,
                  p->transform_epsilon, want_score, p->max_correspondence_distance);
  for (size_t i = 0; i < n; ++i) {
    mm3d_pair_result *out = w[i].out;
    std::memcpy(out->transform, jobs[i].out.T, sizeof(out->transform));
    out->icp_iterations = jobs[i].out.iterations;
    out->n_correspondences = fronts[i].counts.n_correspondences;
    out->n_inliers = fronts[i].counts.n_inliers;
    out->icp_correspondences = jobs[i].out.n_corr;
    out->confidence = 1.0 / jobs[i].out.score;
  }
  if ((sel.rejecting() || sel.geometric()) && !sel.refine && p->refine_transform && n) ctx->last_reject_stats = jobs[n - 1].reject_stats;
  if (sel.geometric() && !sel.refine && p->refine_transform && n) ctx->last_geometry_stats = jobs[n - 1].geometry_stats;
  if (sel.robust() && p->refine_transform && n) ctx->last_robust_stats = jobs[n - 1].robust_stats;
  if (sel.confidence) {
    // the transforms are on the host: both maps' tables (made on first use), one launch and one wait for the whole batch
    std::vector<ConfidencePair> cp(n);
    for (size_t i = 0; i < n; ++i) cp[i] = ConfidencePair{w[i].s, w[i].t, w[i].out->transform, 0.0};
    sel.confidence->score(ctx, cp.data(), n, p, &ctx->last_confidence_stats);
    for (size_t i = 0; i < n; ++i) w[i].out->confidence = cp[i].confidence;
  }
}

void mm3d::finish_run(const mm3d_pair_result *pairs, size_t n_pairs, const mm3d_params *params, size_t n, float *out_T, size_t *n_out,
                      mm3d_pair_result *pairs_out, size_t *n_pairs_out)
{
  if (pairs_out && n_pairs) std::memcpy(pairs_out, pairs, n_pairs * sizeof(mm3d_pair_result));
  if (n_pairs_out) *n_pairs_out = n_pairs;
  const int st = global_transforms(pairs, n_pairs, params->confidence_threshold, n, out_T, n_out);
  if (st != MM3D_OK) throw Error(st, "computeGlobalTransforms failed");
}

// nn.hip -- ICP and transformScore: exact 1-NN of every (transformed) source point in the target
// grid, fused with the reduction the caller needs (K12/K13 in SURVEY 2.2).
//
// estimateTransformICP  R/src/matching.cpp:196-221 -> pcl::IterativeClosestPoint (point-to-point,
//                       TransformationEstimationSVD/Umeyama, DefaultConvergenceCriteria)
// transformScore        R/src/matching.cpp:259-268 -> TransformationValidationEuclidean
//
// Wave-cooperative search.  A wave owns one work item of the source's Hilbert order (<= 64 points
// forming a compact patch), so the cells its queries can touch form a small box of the target grid.  The wave
//   1. reads one distance-transform byte per lane (how many cells to the nearest occupied cell;
//      out of range -> that lane is done),
//   2. takes the bounding box of its lanes' cells, grows it by the largest radius any lane needs,
//   3. streams the box's rows (contiguous spans of the cell-sorted target) through LDS with
//      coalesced 16-byte loads, 512 points per tile,
//   4. every lane scans the tile out of LDS (same address for all lanes = broadcast reads; the tile is
//      kept per component, so four candidates are one 16-byte read and their distances pack),
//   5. a lane is finished when its best distance is within what the box provably covers; otherwise
//      the box grows once more to the radius that lane needs.
// Candidate traffic is therefore LDS traffic; HBM sees the source once (16 B/point) and each target
// span once per wave.  The ICP iteration stays two launches and no host round trip:
// icp_corr_reduce (this search + 17 double partial sums per block through wave shuffles) and
// icp_finalize (Umeyama by 3x3 Jacobi SVD, accumulate, PCL's convergence tests, all on the device).
// Algorithmic traffic: 12 B per source point per iteration.
#include "capi_guard.hpp"
#include "icp_tail.hpp"
#include "nn_core.hpp"

namespace mm3d {

// MODE 0: ICP (transform from the device state, accumulate Umeyama moments)
// MODE 1: transformScore (transform from Tc, accumulate sum d2 / count for d2 <= max_d2)
// SPLIT 1: one work item per wave, four items per block.
// SPLIT 4: one work item per BLOCK: its four waves hold the same 64 points and the same box, each stages and
//          scans a quarter of the box's candidates, and the four minima meet in LDS after every pass.  Same
//          result, a quarter of the time per item: for a source of a few hundred items (a 50 k point map) the
//          chip is mostly idle and the kernel's duration IS one wave's scan.
template <int MODE, int SPLIT>
__global__ void __launch_bounds__(256) MM3D_NN_ATTR
k_nn_wave(const NnJob *__restrict__ jobs, float max_d2, float rmax)
{
  const NnJob &job = jobs[blockIdx.y];
  if ((int)blockIdx.x >= job.nblocks) return;            // the grid is as wide as the batch's largest job
  const float4 *__restrict__ src = job.src;
  const int2 *__restrict__ items = job.items;
  const int n_items = job.n_items;
  const GridView g = job.g;
  const float4 *__restrict__ tgt_ref = job.tgt_ref;
  const IcpState *__restrict__ st = job.st;
  const float *__restrict__ Tc = job.Tc ? job.Tc : job.st->T;
  double *__restrict__ partials = job.partials;
  const int max_ring = job.max_ring;
  __shared__ float Ts[16];
  __shared__ double red[4][kAcc];
  // staged candidates, one array per component: four candidates' x (y, z, index) are ONE 16-byte
  // broadcast read, and the distance arithmetic of candidate pairs packs into v_pk_* instructions
  __shared__ __attribute__((aligned(16))) float s_cx[4][kTile], s_cy[4][kTile], s_cz[4][kTile];
  __shared__ __attribute__((aligned(16))) unsigned s_cw[4][kTile];
  __shared__ int s_off[4][kRows];
  __shared__ int s_beg[4][kRows];
  __shared__ unsigned long long s_merge[SPLIT == 4 ? 4 : 1][64];
  if (MODE == 0 && st->done) return;
  // the score of a pair's ICP result: once, in the first round after its ICP has finished
  if (MODE == 1 && st && (!st->done || st->scored)) return;
  if (threadIdx.x < 16) Ts[threadIdx.x] = (MODE == 0) ? st->T[threadIdx.x] : Tc[threadIdx.x];
  __syncthreads();
#include "nn_search_body.hpp"
  if (SPLIT == 4 && wave != 0) return;     // the four waves hold the same result
  double acc[kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; ++k) acc[k] = 0.0;
  if (valid && best <= max_d2) {   // false for INFINITY / NaN
    if (MODE == 0) {
      const float4 bq = tgt_ref[(unsigned)(bkey & 0xffffffffull)];
      const float bqx = bq.x, bqy = bq.y, bqz = bq.z;
      acc[0] = p.x; acc[1] = p.y; acc[2] = p.z;
      acc[3] = bqx; acc[4] = bqy; acc[5] = bqz;
      acc[6] = (double)bqx * p.x; acc[7] = (double)bqx * p.y; acc[8] = (double)bqx * p.z;
      acc[9] = (double)bqy * p.x; acc[10] = (double)bqy * p.y; acc[11] = (double)bqy * p.z;
      acc[12] = (double)bqz * p.x; acc[13] = (double)bqz * p.y; acc[14] = (double)bqz * p.z;
    }
    acc[15] = best;
    acc[16] = 1.0;
  }
  // A wave none of whose points found a neighbour in range adds seventeen zeros: it writes them without the seventeen
  // reductions (each six shuffle steps on a double).  With the headline's initial poses that is a good part of the waves.
  const bool any_corr = ballot(valid && best <= max_d2) != 0ull;       // wave-uniform
  if (SPLIT == 4) {
#pragma unroll
    for (int k = 0; k < kAcc; ++k) {
      const double v = ((MODE == 0 || k >= 15) && any_corr) ? wave_sum(acc[k]) : 0.0;
      if (lane == 0) partials[(size_t)bid * kAcc + k] = v;
    }
    return;
  }
#pragma unroll
  for (int k = (MODE == 0 ? 0 : 15); k < kAcc; ++k) {
    const double v = any_corr ? wave_sum(acc[k]) : 0.0;
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kAcc) {
    const int k = threadIdx.x;
    double v = 0.0;
    if (MODE == 0 || k >= 15) v = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    partials[(size_t)bid * kAcc + k] = v;
  }
}

// The search alone, per point (test hook mm3d_debug_nn_search): nn_search_body.hpp's keyed search (MODE 0) for one job, and
// each valid lane's result -- the winner's original index and the d2 the lane holds, or -1 / +inf -- stored at the source
// point's ORIGINAL index (src[i].w).  A third compile of the shared body (the same tokens, its own machine code); the
// tests tie k_nn_wave's sums to what it returns.
template <int SPLIT>
__global__ void __launch_bounds__(256) MM3D_NN_ATTR
k_nn_probe(const NnJob *__restrict__ jobs, float max_d2, float rmax, int *__restrict__ out_idx, float *__restrict__ out_d2)
{
  constexpr int MODE = 0;
  const NnJob &job = jobs[0];
  if ((int)blockIdx.x >= job.nblocks) return;
  const float4 *__restrict__ src = job.src;
  const int2 *__restrict__ items = job.items;
  const int n_items = job.n_items;
  const GridView g = job.g;
  const float *__restrict__ Tc = job.Tc;
  const int max_ring = job.max_ring;
  __shared__ float Ts[16];
  __shared__ __attribute__((aligned(16))) float s_cx[4][kTile], s_cy[4][kTile], s_cz[4][kTile];
  __shared__ __attribute__((aligned(16))) unsigned s_cw[4][kTile];
  __shared__ int s_off[4][kRows];
  __shared__ int s_beg[4][kRows];
  __shared__ unsigned long long s_merge[SPLIT == 4 ? 4 : 1][64];
  if (threadIdx.x < 16) Ts[threadIdx.x] = Tc[threadIdx.x];
  __syncthreads();
#include "nn_search_body.hpp"
  if (SPLIT == 4 && wave != 0) return;     // the four waves hold the same result
  if (valid) {
    const int o = __float_as_int(src[i].w);
    const bool found = (unsigned)bkey != 0xffffffffu;
    out_idx[o] = found ? (int)(unsigned)bkey : -1;
    out_d2[o] = found ? best : INFINITY;
  }
}

// one block: reduce partials, Umeyama, accumulate, convergence (DefaultConvergenceCriteria) -- icp_tail.hpp's pieces
__global__ void __launch_bounds__(256) k_icp_finalize(const NnJob *__restrict__ jobs)
{
  __shared__ double red[4][kAcc];
  __shared__ double tot[kAcc];
  const NnJob &job = jobs[blockIdx.x];
  IcpState *st = job.st;
  if (st->done) return;
  icp_totals<kAcc>(job, red, tot);
  if (threadIdx.x != 0) return;

  const double cnt = tot[16];
  st->n_corr = (int)cnt;
  if (cnt < 3.0) return icp_stop_unconverged(st);   // min_number_correspondences_: "Not enough correspondences"
  const double inv = 1.0 / cnt;
  float Ti[16];
  icp_umeyama(tot, inv, Ti);
  icp_advance(st, Ti, true, tot[15] * inv);
}

__global__ void __launch_bounds__(256) k_score_finalize(const NnJob *__restrict__ jobs)
{
  __shared__ double red[4][2];
  const double *__restrict__ partials = jobs[blockIdx.x].partials;
  const int split = jobs[blockIdx.x].split, n_items = jobs[blockIdx.x].n_items;
  const int nblocks = (n_items + 3) >> 2;
  double *out = jobs[blockIdx.x].out;
  IcpState *st = jobs[blockIdx.x].st;
  if (st && (!st->done || st->scored)) return;
  double s = 0.0, n = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += blockDim.x) {
    s += nn_block_partial_n<kAcc>(partials, b, 15, split, n_items);
    n += nn_block_partial_n<kAcc>(partials, b, 16, split, n_items);
  }
  s = wave_sum(s); n = wave_sum(n);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[wave][0] = s; red[wave][1] = n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    out[1] = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    if (st) st->scored = 1;
  }
}

static float nn_cell_for(double radius)
{
  float cell = (float)(radius * 0.25);
  if (!(cell > 1e-3f)) cell = 0.25f;
  return cell;
}

// ICP: max_corr_dist is a distance.  (double)d2 > max_dist_sqr rejects: accept d2 <= largest float not above max_dist_sqr
NnRange nn_range_icp(double max_corr_dist)
{
  const double max_dist_sqr = max_corr_dist * max_corr_dist;
  float max_d2 = (float)max_dist_sqr;
  if ((double)max_d2 > max_dist_sqr) max_d2 = std::nextafterf(max_d2, -INFINITY);
  return {max_d2, (float)(max_corr_dist * 1.0001 + 1e-5), max_corr_dist};
}
// score: max_range_ is compared with the SQUARED distance (PCL quirk), so the search radius is sqrt(max_distance)
NnRange nn_range_score(double max_distance)
{
  const double radius = std::sqrt(max_distance > 0 ? max_distance : 0.0);
  float max_d2 = (float)max_distance;
  if ((double)max_d2 > max_distance) max_d2 = std::nextafterf(max_d2, -INFINITY);
  return {max_d2, (float)(radius * 1.0001 + 1e-5), radius};
}
// rings of cells (around a query's own cell) beyond which the distance transform need not tell cells apart
static int nn_max_ring(float rmax, const Grid &g) { return (int)std::ceil(rmax / g.cell) + 1; }

// One work item per block (k_nn_wave's SPLIT 4) when the source has too few items to keep the chip busy with one
// wave each: 256 CUs x 4 SIMDs take 1024 waves before any two share a SIMD.  Measured on MI355X, pairs/s with
// the split off / on: 16 x 100 k points (1.3 k items) 1765 / 1823, 4 x 200 k (2.5 k items) 245 / 257,
// 64 x 50 k (0.6 k items) 4135 / 4925, 16 x 500 k (7.8 k items) 706 / 669.
bool nn_split_items(int n_items) { return n_items <= 4096; }

// the source runs in the cloud's Hilbert order, one compact work item (<= 64 points) per wave (grid.hip); the target's grid has
// cells of a quarter of the radius and a distance transform out to the ring the radius needs
NnSearch nn_search(Context *c, const mm3d_cloud *src, const mm3d_cloud *tgt, const NnRange *range)
{
  NnSearch s;
  if (src->n == 0 || tgt->n == 0) return s;
  cloud_hilbert(c, src);
  if (src->n_finite == 0) return s;
  s.src = src->hil_pts.get();
  s.items = (const int2 *)src->wave_items.get();
  s.ns = (int)src->n_finite;
  s.n_items = src->n_wave_items;
  s.tgt_ref = (const float4 *)tgt->pts.get();
  if (!range) return s;
  const Grid &g = cloud_grid(c, tgt, nn_cell_for(range->radius));
  if (g.n == 0) return s;
  s.grid = &g;
  s.max_ring = nn_max_ring(range->rmax, g);
  grid_ensure_dt(c, g, s.max_ring);
  return s;
}

NnJob nn_job(const NnSearch &s, bool split, unsigned nblocks, IcpState *st, const float *Tc, double *partials, double *out)
{
  NnJob q;
  memset(&q, 0, sizeof(q));
  q.src = s.src;
  q.items = s.items;
  q.n_items = s.n_items;
  q.nblocks = (int)nblocks;
  q.split = split ? 1 : 0;
  if (s.grid) { q.g = s.grid->view(); q.max_ring = s.max_ring; }
  q.tgt_ref = s.tgt_ref;
  q.st = st;
  q.Tc = Tc;
  q.partials = partials;
  q.out = out;
  return q;
}

// launches k_nn_wave<MODE> over `count` jobs (device array), picking the one-item-per-block variant for small sources
template <int MODE>
static void launch_nn(Context *c, const char *name, double bytes, const NnJob *jobs_dev, int count, unsigned grid_x, bool split, float max_d2,
                      float rmax)
{
  if (split)
    MM3D_LAUNCH(c, name, bytes, (k_nn_wave<MODE, 4>), dim3(grid_x, count), dim3(256), 0, jobs_dev, max_d2, rmax);
  else
    MM3D_LAUNCH(c, name, bytes, (k_nn_wave<MODE, 1>), dim3(grid_x, count), dim3(256), 0, jobs_dev, max_d2, rmax);
}

void icp_point_finalize(Context *c, const NnJob *jobs_dev, int count, double bytes)
{
  MM3D_LAUNCH(c, "icp_finalize", bytes, k_icp_finalize, dim3(count), dim3(256), 0, jobs_dev);
}

namespace {
// the reference's point-to-point ICP: the batch's own NnJobs are all it needs
struct PointStep final : IcpStep {
  double bytes_per_point(const IcpScoreJob &) const override { return 12.0; }
  void iterate(Context *c, const IcpLaunch &L) override
  {
    launch_nn<0>(c, "icp_corr_reduce", L.bytes, L.jobs_dev, L.count, L.grid_x, L.split, L.max_d2, L.rmax);
    icp_point_finalize(c, L.jobs_dev, L.count, L.finalize_bytes);
  }
};
}  // namespace

// ICP from a guess and, if wanted, transformScore of the result -- the tail of every pair estimate -- for a BATCH
// of pairs in lockstep: one launch per step serves every pair of the batch (blockIdx.y = the pair), and the batch
// shares ONE host synchronisation per chunk of iterations.  A guess may already live on the device (SAC-IA's
// winning hypothesis), the score kernel reads the transform straight out of the ICP state, and the states and
// scores come back in one copy.  The score is launched speculatively after each chunk of iterations; a pair's
// score is only kept once its ICP has finished (it nearly always has: the reference's epsilon is loose).
// Which ICP runs is the step's business (IcpStep, nn_core.hpp): everything here -- states, chunks, waits, the speculative
// point-to-point score -- is shared by all of them.
static void icp_batch(Context *c, IcpStep &step, IcpScoreJob *jobs, int n_jobs, bool run_icp, double max_corr_dist, int max_iterations,
                      double eps, bool want_score, double score_max_distance)
{
  static_assert(offsetof(IcpState, T) == 0, "the score kernel reads T at the head of the state");
  c->last_icp_iterations = 0;
  c->last_icp_converged = 0;
  // the ICP's and the score's search parameters
  const NnRange icp_range = nn_range_icp(max_corr_dist), score_range = nn_range_score(score_max_distance);
  const bool icp_grid = run_icp && step.searches;

  struct Live { NnSearch icp, score; };
  std::vector<Live> live;
  std::vector<IcpScoreJob *> live_jobs;
  for (int j = 0; j < n_jobs; ++j) {
    IcpScoreJob &J = jobs[j];
    J.out.iterations = 0; J.out.converged = 0; J.out.n_corr = 0; J.out.score = DBL_MAX;
    // (the ICP searches with its own source -- a sample under mm3d_set_icp_sampling --, the score with the pair's)
    const NnSearch si = nn_search(c, J.icp_source(), J.tgt, icp_grid ? &icp_range : nullptr);
    const NnSearch ss = want_score ? nn_search(c, J.src, J.tgt, &score_range) : NnSearch();
    if (!si.src || (icp_grid && !si.grid) || (want_score && !ss.grid) || (!run_icp && !want_score)) {
      // nothing to search: Identity * guess, and the score of an empty search
      if (J.guess_dev) {
        float *hT = (float *)c->pin(256);
        MM3D_HIP(hipMemcpyAsync(hT, J.guess_dev, 64, hipMemcpyDeviceToHost, c->stream));
        c->sync();
        memcpy(J.out.T, hT, sizeof(J.out.T));
      } else {
        memcpy(J.out.T, J.guess_host, sizeof(J.out.T));
      }
      continue;
    }
    if (run_icp) step.check(J);
    live.push_back(Live{si, ss});
    live_jobs.push_back(&J);
  }
  const int B = (int)live.size();
  if (B == 0) return;

  // one work item per block while the whole batch has too few items to fill the chip with one wave each
  // (the finalize kernels add the partials up in one fixed order, so the choice never shows in a result)
  // Each of the two searches from its own items: they are the same items unless the ICP's source is a sample.
  int total_items = 0, score_items = 0;
  for (const Live &L : live) { total_items += L.icp.n_items; score_items += want_score ? L.score.n_items : L.icp.n_items; }
  const int forced_split = run_icp ? step.forced_split : 0;
  const bool split = forced_split ? forced_split == 4 : nn_split_items(score_items);
  // (a step that does not search keeps four items per block whatever the batch does)
  const bool icp_split = (forced_split ? forced_split == 4 : nn_split_items(total_items)) && step.searches;
  size_t part_total = 0, icp_part_total = 0;
  unsigned grid_x = 0, icp_grid_x = 0;
  double icp_bytes = 0.0, score_bytes = 0.0;
  std::vector<unsigned> nb(B), icp_nb(B);
  for (int b = 0; b < B; ++b) {
    nb[b] = nn_blocks(want_score ? live[b].score.n_items : live[b].icp.n_items, split);
    icp_nb[b] = nn_blocks(live[b].icp.n_items, icp_split);
    part_total += (size_t)nb[b] * kAcc;
    icp_part_total += (size_t)icp_nb[b] * step.acc;
    grid_x = std::max(grid_x, nb[b]);
    icp_grid_x = std::max(icp_grid_x, icp_nb[b]);
    icp_bytes += live[b].icp.ns * step.bytes_per_point(*live_jobs[b]);
    score_bytes += (want_score ? live[b].score.ns : live[b].icp.ns) * 12.0 + (live[b].score.grid ? live[b].score.grid->n * 12.0 : 0.0);
  }
  DevBuf<double> partials(c, icp_part_total), s_partials(c, want_score ? part_total : 1);
  DevBuf<double> out(c, (size_t)2 * B);
  // (what a step keeps per pair beside the state lives behind the states, so that one copy brings both back)
  const size_t rec_bytes = step.record_bytes(B);
  DevBuf<IcpState> st(c, B + div_up(rec_bytes, sizeof(IcpState)));
  DevBuf<NnJob> d_jobs(c, (size_t)2 * B);                 // [0, B): ICP, [B, 2B): score

  // host images, in the pinned arena: states | the step's records | ICP jobs | score jobs | scores back | the step's jobs.
  // ONE request: a later pin() may replace the arena under the pointers of an earlier one.
  const size_t st_bytes = sizeof(IcpState) * B, job_bytes = sizeof(NnJob) * 2 * B, out_bytes = 16 * (size_t)B;
  const size_t st_rec_bytes = st_bytes + rec_bytes;
  char *pinned = (char *)c->pin(st_rec_bytes + job_bytes + out_bytes + step.pinned_bytes(B) + 64);
  IcpState *hp = (IcpState *)pinned;
  NnJob *hj = (NnJob *)(pinned + ((st_rec_bytes + 15) & ~(size_t)15));
  double *ho = (double *)((char *)hj + job_bytes);
  step.begin(c, live_jobs.data(), B, (char *)ho + out_bytes, pinned + st_bytes, st.get() + B);
  size_t off = 0, icp_off = 0;
  for (int b = 0; b < B; ++b) {
    const IcpScoreJob &J = *live_jobs[b];
    IcpState h;
    memset(&h, 0, sizeof(h));
    if (!J.guess_dev) memcpy(h.T, J.guess_host, sizeof(h.T));
    h.prev_mse = DBL_MAX;
    h.rot_thresh = 1.0 - eps;
    h.trans_thresh = eps;
    h.max_iter = max_iterations;
    h.done = run_icp ? 0 : 1;
    hp[b] = h;
    hj[b] = nn_job(live[b].icp, icp_split, icp_nb[b], st.get() + b, nullptr, partials.get() + icp_off, out.get() + 2 * b);
    step.bind(b, hj[b], J);
    hj[B + b] = nn_job(live[b].score, split, nb[b], st.get() + b, nullptr, s_partials.get() + (want_score ? off : 0), out.get() + 2 * b);
    off += (size_t)nb[b] * kAcc;
    icp_off += (size_t)icp_nb[b] * step.acc;
  }
  MM3D_HIP(hipMemcpyAsync(st.get(), hp, st_rec_bytes, hipMemcpyHostToDevice, c->stream));
  MM3D_HIP(hipMemcpyAsync(d_jobs.get(), hj, job_bytes, hipMemcpyHostToDevice, c->stream));
  step.upload(c);
  for (int b = 0; b < B; ++b)
    if (live_jobs[b]->guess_dev)
      MM3D_HIP(hipMemcpyAsync(st.get() + b, live_jobs[b]->guess_dev, 64, hipMemcpyDeviceToDevice, c->stream));
  // iterations launched between two looks at the `done` flags: with the reference's loose epsilon 86 % of the pairs
  // converge in one iteration and 95 % in two.  A launch after `done` does nothing, but it is not free on a GPU
  // that runs sixteen streams: its blocks still queue for 20 KB of LDS and 128 registers behind the other streams'
  // kernels before they can find that out.  So the first look comes after ONE iteration (a batch of one or two
  // pairs is then usually finished), later ones after two.
  static const int first_chunk_knob = [] { const char *e = getenv("MM3D_ICP_FIRST_CHUNK"); return e ? atoi(e) : 0; }();   // A/B knob (1 or 2; 0: by batch size)
  const int min_chunk = first_chunk_knob > 0 ? std::min(first_chunk_knob, 2) : (B <= 2 ? 1 : 2);
  const IcpLaunch launch{d_jobs.get(), B, icp_grid_x, icp_split, icp_range.max_d2, icp_range.rmax, icp_bytes, icp_part_total * 8.0};
  for (int round = 0;; ++round) {
    const int chunk = round == 0 ? min_chunk : 2;
    if (run_icp)
      for (int k = 0; k < chunk; ++k) step.iterate(c, launch);
    if (want_score) {
      launch_nn<1>(c, "score_nn_reduce", score_bytes, d_jobs.get() + B, B, grid_x, split, score_range.max_d2, score_range.rmax);
      MM3D_LAUNCH(c, "score_finalize", 0, k_score_finalize, dim3(B), dim3(256), 0, (const NnJob *)(d_jobs.get() + B));
      MM3D_HIP(hipMemcpyAsync(ho, out.get(), out_bytes, hipMemcpyDeviceToHost, c->stream));
    }
    MM3D_HIP(hipMemcpyAsync(hp, st.get(), st_rec_bytes, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    bool all_done = true;
    for (int b = 0; b < B; ++b) {
      IcpScoreJob &J = *live_jobs[b];
      if (hp[b].done && !J.closed) {
        // first chunk after which this pair is finished: its state and score are final
        memcpy(J.out.T, hp[b].T, sizeof(J.out.T));
        J.out.iterations = hp[b].iters;
        J.out.converged = hp[b].converged;
        J.out.n_corr = hp[b].n_corr;
        if (want_score) J.out.score = ho[2 * b + 1] > 0.0 ? ho[2 * b] / ho[2 * b + 1] : DBL_MAX;
        step.close(b, hp[b], J);
        J.closed = true;
      }
      if (!hp[b].done) all_done = false;
    }
    if (all_done) break;
  }
  const IcpScoreJob &last = *live_jobs[B - 1];
  c->last_icp_iterations = last.out.iterations;
  c->last_icp_converged = last.out.converged;
}

// Where the step is chosen: the method's (null: the reference's point-to-point ICP), and a method that can reject correspondences
// makes the rejecting step when the jobs carry options (IcpScoreJob::reject, the same for the whole batch) and the ICP runs.
void icp_score_batch(Context *c, const IcpMethodBase *method, IcpScoreJob *jobs, int n_jobs, bool run_icp, double max_corr_dist,
                     int max_iterations, double eps, bool want_score, double score_max_distance)
{
  const mm3d_icp_rejection_options *reject = (run_icp && n_jobs) ? jobs[0].reject : nullptr;
  // (a robust kernel, IcpScoreJob::robust, likewise: point-to-point's and point-to-plane's ICP then run icp_robust.hip's step)
  const mm3d_icp_robust_options *robust = (run_icp && n_jobs) ? jobs[0].robust : nullptr;
  const bool plain = !method || method == icp_plane_method();      // (the setters keep the other methods and a kernel apart)
  // (step 1b of the rejecting step, IcpScoreJob::geometry, rides on the rejection options: mm3d_set_icp_geometry_rejection)
  const mm3d_icp_geometry_options *geometry = (reject && plain) ? jobs[0].geometry : nullptr;
  const std::unique_ptr<IcpStep> step = robust && plain ? icp_robust_step(*robust, method != nullptr, max_iterations)
                                        : geometry      ? icp_reject_step(*reject, method != nullptr, geometry)
                                        : method        ? method->step(reject)
                                        : reject        ? icp_reject_step(*reject, false)
                                                        : std::unique_ptr<IcpStep>(new PointStep());
  icp_batch(c, *step, jobs, n_jobs, run_icp, max_corr_dist, max_iterations, eps, want_score, score_max_distance);
}

PairTail icp_score(Context *c, const mm3d_cloud *src, const mm3d_cloud *tgt, const float *guess_dev, const float guess_host[16],
                   bool run_icp, double max_corr_dist, int max_iterations, double eps, bool want_score, double score_max_distance)
{
  IcpScoreJob J;
  J.src = src; J.tgt = tgt; J.guess_dev = guess_dev;
  if (guess_host) memcpy(J.guess_host, guess_host, sizeof(J.guess_host));
  icp_score_batch(c, nullptr, &J, 1, run_icp, max_corr_dist, max_iterations, eps, want_score, score_max_distance);
  return J.out;
}

IcpResult icp(Context *c, const mm3d_cloud *src, const mm3d_cloud *tgt, const float guess[16],
              double max_corr_dist, int max_iterations, double eps)
{
  const PairTail t = icp_score(c, src, tgt, nullptr, guess, true, max_corr_dist, max_iterations, eps, false, 0.0);
  IcpResult res;
  memcpy(res.T, t.T, sizeof(res.T));
  res.iterations = t.iterations;
  res.converged = t.converged;
  return res;
}

double transform_score(Context *c, const mm3d_cloud *src, const mm3d_cloud *tgt, const float T[16], double max_distance)
{
  const NnRange range = nn_range_score(max_distance);
  const NnSearch s = nn_search(c, src, tgt, &range);
  if (!s.grid) return DBL_MAX;
  const bool split = nn_split_items(s.n_items);
  const unsigned nblocks = nn_blocks(s.n_items, split);
  DevBuf<double> partials(c, (size_t)nblocks * kAcc);
  DevBuf<float> dT(c, 16);
  DevBuf<double> out(c, 2);
  DevBuf<NnJob> d_job(c, 1);
  char *pinned = (char *)c->pin(512 + sizeof(NnJob));
  float *hT = (float *)pinned;
  double *ho = (double *)(pinned + 128);
  NnJob *hj = (NnJob *)(pinned + 256);
  memcpy(hT, T, 64);
  *hj = nn_job(s, split, nblocks, nullptr, dT.get(), partials.get(), out.get());
  MM3D_HIP(hipMemcpyAsync(dT.get(), hT, 64, hipMemcpyHostToDevice, c->stream));
  MM3D_HIP(hipMemcpyAsync(d_job.get(), hj, sizeof(NnJob), hipMemcpyHostToDevice, c->stream));
  launch_nn<1>(c, "score_nn_reduce", s.ns * 12.0 + s.grid->n * 12.0, d_job.get(), 1, nblocks, split, range.max_d2, range.rmax);
  MM3D_LAUNCH(c, "score_finalize", 0, k_score_finalize, dim3(1), dim3(256), 0, (const NnJob *)d_job.get());
  MM3D_HIP(hipMemcpyAsync(ho, out.get(), 16, hipMemcpyDeviceToHost, c->stream));
  c->sync();
  return ho[1] > 0.0 ? ho[0] / ho[1] : DBL_MAX;
}

// mm3d_debug_nn_search: the search set-up as icp_batch (convention 0) or transform_score (1) derive it, one launch of
// k_nn_probe with the split forced
static void debug_nn_search(Context *c, const mm3d_cloud *src, const mm3d_cloud *tgt, const float T[16], double range, int convention,
                            int split, int *idx, float *d2, mm3d_nn_search_info *info)
{
  const NnRange r = convention == 0 ? nn_range_icp(range) : nn_range_score(range);
  mm3d_nn_search_info I;
  memset(&I, 0, sizeof(I));
  I.max_d2 = r.max_d2;
  I.rmax = r.rmax;
  std::vector<int> h_idx(src->n, -1);
  std::vector<float> h_d2(src->n, INFINITY);
  const NnSearch s = nn_search(c, src, tgt, &r);
  if (s.grid) {
    const unsigned nblocks = nn_blocks(s.n_items, split == 4);
    I.cell = s.grid->cell;
    I.max_ring = s.max_ring;
    for (int a = 0; a < 3; ++a) { I.dims[a] = s.grid->dims[a]; I.origin[a] = s.grid->mn[a]; }
    I.n_items = s.n_items;
    DevBuf<int> d_idx(c, src->n);
    DevBuf<float> d_d2(c, src->n), dT(c, 16);
    DevBuf<NnJob> d_job(c, 1);
    char *pinned = (char *)c->pin(256 + sizeof(NnJob));
    float *hT = (float *)pinned;
    NnJob *hj = (NnJob *)(pinned + 256);
    memcpy(hT, T, 64);
    *hj = nn_job(s, split == 4, nblocks, nullptr, dT.get(), nullptr, nullptr);
    // (non-finite source points are in no work item: they keep -1 / +inf)
    MM3D_HIP(hipMemcpyAsync(d_idx.get(), h_idx.data(), src->n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    MM3D_HIP(hipMemcpyAsync(d_d2.get(), h_d2.data(), src->n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    MM3D_HIP(hipMemcpyAsync(dT.get(), hT, 64, hipMemcpyHostToDevice, c->stream));
    MM3D_HIP(hipMemcpyAsync(d_job.get(), hj, sizeof(NnJob), hipMemcpyHostToDevice, c->stream));
    if (split == 4)
      MM3D_LAUNCH(c, "debug_nn_search", s.ns * 24.0, (k_nn_probe<4>), dim3(nblocks), dim3(256), 0, (const NnJob *)d_job.get(), r.max_d2, r.rmax,
                  d_idx.get(), d_d2.get());
    else
      MM3D_LAUNCH(c, "debug_nn_search", s.ns * 24.0, (k_nn_probe<1>), dim3(nblocks), dim3(256), 0, (const NnJob *)d_job.get(), r.max_d2, r.rmax,
                  d_idx.get(), d_d2.get());
    MM3D_HIP(hipMemcpyAsync(h_idx.data(), d_idx.get(), src->n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MM3D_HIP(hipMemcpyAsync(h_d2.data(), d_d2.get(), src->n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    c->sync();
  }
  if (src->n) {
    memcpy(idx, h_idx.data(), src->n * sizeof(int));
    memcpy(d2, h_d2.data(), src->n * sizeof(float));
  }
  if (info) *info = I;
}

#ifdef MM3D_NN_STATS
extern "C" void mm3d_debug_nn_stats(unsigned long long *out, int reset)
{
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_nn_stats), sizeof(unsigned long long) * 64);
  if (reset) { unsigned long long z[64] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_nn_stats), z, sizeof(z)); }
}
#endif

// Everything icp_score() would build lazily on its first use of these clouds: afterwards pair
// estimates only READ the clouds' caches, so one map can serve pairs on several contexts at once.
void prepare_pair_search(Context *c, const mm3d_cloud *points, double max_corr_dist, double score_max_distance)
{
  const NnRange ranges[2] = {nn_range_icp(max_corr_dist), nn_range_score(score_max_distance)};
  for (const NnRange &range : ranges) (void)nn_search(c, points, points, &range);
}

}  // namespace mm3d

// the C entry point of the search probe (include/mm3d.h) lives with its kernel, like fpfh.hip's mm3d_debug_pair_bins: the
// host-only builds of the library link capi.cpp without this file
extern "C" int mm3d_debug_nn_search(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target, const float T[16], double range,
                                    int convention, int split, int *idx, float *d2, mm3d_nn_search_info *info)
{
  if (!source || !target || !T || (convention != 0 && convention != 1) || (split != 1 && split != 4)) return MM3D_EINVAL;
  if (!(range >= 0.0) || !std::isfinite(range)) return MM3D_EINVAL;
  if (source->n && (!idx || !d2)) return MM3D_EINVAL;
  return mm3d::guarded(ctx, [&] { mm3d::debug_nn_search(ctx, source, target, T, range, convention, split, idx, d2, info); });
}

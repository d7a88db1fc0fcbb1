// icp_robust.hip -- a robust loss for the pair stage's ICP, opt-in (mm3d_set_icp_robust): every matched correspondence enters the
// point-to-point or point-to-plane estimate with an M-estimator weight of its Euclidean d2 (L2, Huber, Cauchy, Tukey,
// Geman-McClure) at a scale that is fixed BEFORE the iteration runs.  include/mm3d.h states the rule.
//
// The rejectors of icp_reject.hip need an order statistic of the iteration's own d2, so their iteration is a correspondence
// stage of eight launches.  A weight at a known scale needs nothing but the lane's own match, so here the iteration keeps the
// default ICP's two launches:
//   k_rob_wave      nn_search_body.hpp's wave-cooperative search (the same include as k_nn_wave<0> and k_icp_plane_wave); the
//                   scale sigma_k from the batch's table at the pair's st->iters; the lane's weight in double (one divide for u2,
//                   one more for the reciprocal of Huber, Cauchy and Geman-McClure); the default kernels' terms, each times w,
//                   through wave_sum and the block step into partials of the step's own width: the default layout plus
//                   `matched` and `weighted` (19 doubles, or 32 with normals), in the default kernels' order.
//   k_rob_finalize  one block per pair: the partials in k_icp_finalize's fixed order, Umeyama or the 6x6 solve on totals that
//                   sum w normalises, Tinc, and the convergence step behind the final_k gate.  These are the functions of
//                   icp_tail.hpp that k_icp_finalize and k_icp_plane_finalize call (-ffp-contract=off: inlined twice, they round
//                   the same way), so with L2 (w = 1.0, x * 1.0 = x) the state holds the default ICP's bits.
// No correspondence array, no histogram, no select; per batch one table of doubles, per pair one 32-byte record.
#include <atomic>
#include <climits>
#include <cmath>

#include "capi_guard.hpp"
#include "drivers.hpp"
#include "icp_tail.hpp"
#include "nn_core.hpp"

namespace mm3d {

constexpr int kRobAcc = kAcc + 2;             // k_nn_wave<0>'s 17 (the count slot holds sum w) | matched | weighted
constexpr int kRobPlaneAcc = kPlaneAcc + 2;   // k_icp_plane_wave's 30 (28: sum w, 29: rows with w > 0) | matched | weighted

// What one pair's last iteration leaves behind, on the device beside the pair's IcpState and back on the host in the copy that
// brings the states
struct RobRecord {
  double weight_sum, sigma;
  long long matched, weighted;
};
// the search job plus what the robust step reads and writes beside it; nn.partials: [nblocks][kRobAcc], or [nblocks][kRobPlaneAcc]
struct NnRobustJob {
  NnJob nn;
  const float4 *nrm;          // point-to-plane: the target's normals (tgt_ref's order); null: point-to-point
  RobRecord *rec;
  // mm3d_debug_icp_robust: every valid lane's match and weight, stored at the source point's ORIGINAL index; null otherwise
  int *out_idx;
  float *out_d2;
  double *out_w;
};
// the options as the kernels take them: the kernel, its tuning constant resolved, the scale the run ends on, and the table
struct RobOpts {
  int kernel;
  double tuning, scale;
  const double *sigma;        // [n_sigma]: sigma_k for k < n_sigma, and sigma_{n_sigma - 1} from there on
  int n_sigma;
};

__device__ __forceinline__ double rob_sigma(const RobOpts &o, int k) { return o.sigma[k < o.n_sigma ? k : o.n_sigma - 1]; }

// step 3 of the rule.  h2 = (sigma_k tuning)^2.  Two divides stand in the code: u2's and the reciprocal's.
__device__ __forceinline__ double rob_weight(int kernel, double d2, double h2)
{
  if (kernel == MM3D_ROBUST_L2) return 1.0;
  const double u2 = d2 / h2;
  if (kernel == MM3D_ROBUST_TUKEY) {
    const double a = 1.0 - u2;
    return u2 < 1.0 ? a * a : 0.0;
  }
  if (kernel == MM3D_ROBUST_HUBER && u2 <= 1.0) return 1.0;
  const double b = 1.0 + u2;
  const double den = kernel == MM3D_ROBUST_HUBER ? sqrt(u2) : kernel == MM3D_ROBUST_CAUCHY ? b : b * b;
  return 1.0 / den;
}

template <int SPLIT, bool PLANE>
__global__ void __launch_bounds__(256) MM3D_NN_ATTR
k_rob_wave(const NnRobustJob *__restrict__ rjobs, RobOpts o, float max_d2, float rmax)
{
  constexpr int MODE = 0;                                // (nn_search_body.hpp: the keyed search, with the winner's index)
  constexpr int NACC = PLANE ? kRobPlaneAcc : kRobAcc;
  const NnRobustJob &rj = rjobs[blockIdx.y];
  const NnJob &job = rj.nn;
  if ((int)blockIdx.x >= job.nblocks) return;            // the grid is as wide as the batch's largest job
  const float4 *__restrict__ src = job.src;
  const int2 *__restrict__ items = job.items;
  const int n_items = job.n_items;
  const GridView g = job.g;
  const float4 *__restrict__ tgt_ref = job.tgt_ref;
  const float4 *__restrict__ nrm = rj.nrm;
  const IcpState *__restrict__ st = job.st;
  double *__restrict__ partials = job.partials;
  const int max_ring = job.max_ring;
  __shared__ float Ts[16];
  __shared__ double red[4][NACC];
  __shared__ __attribute__((aligned(16))) float s_cx[4][kTile], s_cy[4][kTile], s_cz[4][kTile];
  __shared__ __attribute__((aligned(16))) unsigned s_cw[4][kTile];
  __shared__ int s_off[4][kRows];
  __shared__ int s_beg[4][kRows];
  __shared__ unsigned long long s_merge[SPLIT == 4 ? 4 : 1][64];
  if (st->done) return;
  if (threadIdx.x < 16) Ts[threadIdx.x] = st->T[threadIdx.x];
  __syncthreads();
#include "nn_search_body.hpp"
  if (SPLIT == 4 && wave != 0) return;     // the four waves hold the same result
  const bool corr = valid && best <= max_d2;   // false for INFINITY / NaN
  // the iteration's scale (block-uniform: the state is written by the finalize launch only)
  const double h = rob_sigma(o, st->iters) * o.tuning, h2 = h * h;
  const unsigned widx = (unsigned)(bkey & 0xffffffffull);
  const double w = corr ? rob_weight(o.kernel, (double)best, h2) : 0.0;
  const bool pos = w > 0.0;
  if (rj.out_idx && valid) {
    const int orig = __float_as_int(src[i].w);
    rj.out_idx[orig] = corr ? (int)widx : -1;
    rj.out_d2[orig] = corr ? best : INFINITY;
    rj.out_w[orig] = w;
  }
  // one term at a time (icp_store_partials): the weight's divides share the registers the search has left
  float bqx = 0.f, bqy = 0.f, bqz = 0.f;
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double r = 0.0, has_row = 0.0;
  if (corr) {
    if (!PLANE) {
      const float4 bq = tgt_ref[widx];
      bqx = bq.x; bqy = bq.y; bqz = bq.z;
    } else if (icp_plane_row(p, nrm[widx], tgt_ref[widx], v, r)) {
      has_row = pos ? 1.0 : 0.0;
    }
  }
  auto term = [&](int k) -> double {
    if (k == NACC - 2) return corr ? 1.0 : 0.0;
    if (k == NACC - 1) return pos ? 1.0 : 0.0;
    if (!PLANE) {
      // k_nn_wave<0>'s terms, times w
      const float pc = (k % 3 == 0) ? p.x : (k % 3 == 1) ? p.y : p.z;
      if (k < 3) return w * (double)pc;
      if (k < 6) return w * (double)(k == 3 ? bqx : k == 4 ? bqy : bqz);
      if (k < 15) return w * ((double)(k < 9 ? bqx : k < 12 ? bqy : bqz) * pc);
      if (k == 15) return corr ? w * (double)best : 0.0;      // (best is +inf without a match)
      return w;
    }
    // point-to-plane's terms, times w
    if (k < 27) return w * icp_plane_term(k, v, r, corr, best, has_row);
    if (k == 27) return corr ? w * (double)best : 0.0;
    if (k == 28) return w;
    return has_row;
  };
  // a wave none of whose points found a neighbour in range adds zeros without the reductions (as k_nn_wave does)
  const bool any_corr = ballot(corr) != 0ull;       // wave-uniform
  icp_store_partials<NACC, SPLIT>(term, any_corr, red, partials, bid);
}

// mm3d_debug_icp_robust: the totals the finalize kernel would read
template <int NACC>
__global__ void __launch_bounds__(256) k_rob_totals(const NnRobustJob *__restrict__ rjobs, double *__restrict__ out)
{
  __shared__ double red[4][NACC];
  __shared__ double tot[NACC];
  icp_totals<NACC>(rjobs[0].nn, red, tot);
  if (threadIdx.x < NACC) out[threadIdx.x] = tot[threadIdx.x];
}

template <bool PLANE>
__global__ void __launch_bounds__(256) k_rob_finalize(const NnRobustJob *__restrict__ rjobs, RobOpts o)
{
  constexpr int NACC = PLANE ? kRobPlaneAcc : kRobAcc;
  __shared__ double red[4][NACC];
  __shared__ double tot[NACC];
  const NnRobustJob &rj = rjobs[blockIdx.x];
  IcpState *st = rj.nn.st;
  if (st->done) return;
  icp_totals<NACC>(rj.nn, red, tot);
  if (threadIdx.x != 0) return;

  const double sigma = rob_sigma(o, st->iters);
  const bool final_k = sigma == o.scale;      // (an annealing run does not stop on a scale it is about to leave)
  const double wsum = tot[PLANE ? 28 : 16], weighted = tot[NACC - 1];
  *rj.rec = RobRecord{wsum, sigma, (long long)tot[NACC - 2], (long long)weighted};
  st->n_corr = (int)weighted;
  if (weighted < 3.0) return icp_stop_unconverged(st);   // min_number_correspondences_: "Not enough correspondences"
  float Ti[16];
  double mse;
  if (!PLANE) {
    // Umeyama on the moments that sum w normalises
    const double inv = 1.0 / wsum;
    icp_umeyama(tot, inv, Ti);
    mse = tot[15] * inv;
  } else {
    // the 6x6 system (a system scaled by sum w has the same solution: nothing is normalised); degenerate with fewer than six
    // weighted rows, or a plane / line that leaves a direction free: stop, not converged, T unchanged
    if (tot[29] < 6.0 || !icp_solve6_transform(tot, Ti)) return icp_stop_unconverged(st);
    mse = tot[27] / wsum;
  }
  icp_advance(st, Ti, final_k, mse);
}

static double rob_tuning(const mm3d_icp_robust_options &o)
{
  if (o.tuning != 0.0) return o.tuning;
  return o.kernel == MM3D_ROBUST_HUBER ? 1.345 : o.kernel == MM3D_ROBUST_CAUCHY ? 2.385 : o.kernel == MM3D_ROBUST_TUKEY ? 4.685 : 1.0;
}

// Step 2 of the rule: sigma_k = max(scale, s_k), s_0 = scale_start, s_{k+1} = s_k * anneal, for k < max_iterations -- cut where the
// rest is constant (sigma_k has reached `scale`, or s_k no longer moves): the kernels read the last entry from there on.
static std::vector<double> rob_table(const mm3d_icp_robust_options &o, int max_iterations)
{
  const bool scaled = o.kernel != MM3D_ROBUST_OFF && o.kernel != MM3D_ROBUST_L2;      // (L2 reads no scale: every iteration is final)
  std::vector<double> t;
  double s = scaled ? o.scale_start : 0.0;
  for (int k = 0; k < std::max(max_iterations, 1); ++k) {
    const double sigma = std::max(o.scale, s);
    t.push_back(sigma);
    const double next = s * o.anneal;
    if (sigma == o.scale || next == s) break;
    s = next;
  }
  return t;
}

static bool icp_robust_options_valid(const mm3d_icp_robust_options *o)
{
  if (o->kernel < MM3D_ROBUST_OFF || o->kernel > MM3D_ROBUST_GEMAN_MCCLURE) return false;
  if (!(o->scale > 0.0) || !std::isfinite(o->scale)) return false;
  if (!(o->scale_start == 0.0 || (o->scale_start >= o->scale && std::isfinite(o->scale_start)))) return false;
  if (!(o->anneal > 0.0 && o->anneal <= 1.0)) return false;
  if (!(o->tuning >= 0.0) || !std::isfinite(o->tuning)) return false;
  // (h * h must be a positive finite double at both ends of the schedule: u2 = d2 / (h * h))
  const double t = rob_tuning(*o), h0 = o->scale * t, h1 = std::max(o->scale, o->scale_start) * t;
  return h0 * h0 > 0.0 && std::isfinite(h1 * h1);
}

static mm3d_icp_robust_stats rob_stats(const RobRecord &r, int iterations, int converged)
{
  return mm3d_icp_robust_stats{r.matched, r.weighted, r.weight_sum, r.sigma, iterations, converged};
}

static void launch_rob_wave(Context *c, const NnRobustJob *jobs_dev, const RobOpts &o, bool plane, int count, unsigned grid_x, bool split,
                            float max_d2, float rmax, double bytes)
{
  const dim3 grid(grid_x, count);
  if (split && plane) MM3D_LAUNCH(c, "icp_robust_corr_reduce", bytes, (k_rob_wave<4, true>), grid, dim3(256), 0, jobs_dev, o, max_d2, rmax);
  else if (split) MM3D_LAUNCH(c, "icp_robust_corr_reduce", bytes, (k_rob_wave<4, false>), grid, dim3(256), 0, jobs_dev, o, max_d2, rmax);
  else if (plane) MM3D_LAUNCH(c, "icp_robust_corr_reduce", bytes, (k_rob_wave<1, true>), grid, dim3(256), 0, jobs_dev, o, max_d2, rmax);
  else MM3D_LAUNCH(c, "icp_robust_corr_reduce", bytes, (k_rob_wave<1, false>), grid, dim3(256), 0, jobs_dev, o, max_d2, rmax);
}

static std::atomic<int> g_forced_split{0};      // mm3d_debug_icp_robust_split: 0 (by size), 1 or 4

namespace {
// One iteration: the fused search / weight / reduce launch over the batch's NnRobustJobs and the robust finalize.  The pairs'
// records ride behind the states; the table of scales sits behind the jobs in the pinned block and is uploaded with them.
struct RobustStep final : IcpStep {
  const mm3d_icp_robust_options opt;
  const bool plane;
  const std::vector<double> table;
  StepJobs<NnRobustJob> jobs;
  DevBuf<double> sigma;
  double *sigma_host = nullptr;
  RobRecord *rec_host = nullptr, *rec_dev = nullptr;
  RobustStep(const mm3d_icp_robust_options &o, bool normals, int max_iterations) : opt(o), plane(normals), table(rob_table(o, max_iterations))
  {
    acc = plane ? kRobPlaneAcc : kRobAcc;
    forced_split = g_forced_split.load();
  }
  RobOpts opts() const
  {
    return RobOpts{opt.kernel == MM3D_ROBUST_OFF ? (int)MM3D_ROBUST_L2 : opt.kernel, rob_tuning(opt), opt.scale, sigma.get(), (int)table.size()};
  }
  double bytes_per_point(const IcpScoreJob &) const override { return plane ? 28.0 : 12.0; }
  void check(const IcpScoreJob &J) const override { if (plane) icp_plane_check(J); }
  size_t pinned_bytes(int B) const override { return jobs.bytes(B) + ((table.size() * sizeof(double) + 15) & ~(size_t)15); }
  size_t record_bytes(int B) const override { return sizeof(RobRecord) * B; }
  void begin(Context *c, const IcpScoreJob *const *, int B, char *pinned, void *rh, void *rd) override
  {
    sigma_host = (double *)jobs.begin(c, B, pinned);
    std::memcpy(sigma_host, table.data(), table.size() * sizeof(double));
    sigma = DevBuf<double>(c, table.size());
    rec_host = (RobRecord *)rh;
    rec_dev = (RobRecord *)rd;
  }
  void bind(int b, const NnJob &q, const IcpScoreJob &J) override
  {
    jobs.host[b] = NnRobustJob{q, plane ? (const float4 *)J.tgt_normals->nrm.get() : nullptr, rec_dev + b, nullptr, nullptr, nullptr};
    rec_host[b] = RobRecord{0.0, 0.0, 0, 0};
  }
  void upload(Context *c) override
  {
    jobs.upload(c);
    MM3D_HIP(hipMemcpyAsync(sigma.get(), sigma_host, table.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  void iterate(Context *c, const IcpLaunch &L) override
  {
    const RobOpts o = opts();
    launch_rob_wave(c, jobs.dev.get(), o, plane, L.count, L.grid_x, L.split, L.max_d2, L.rmax, L.bytes);
    if (plane) MM3D_LAUNCH(c, "icp_robust_finalize", L.finalize_bytes, k_rob_finalize<true>, dim3(L.count), dim3(256), 0, (const NnRobustJob *)jobs.dev.get(), o);
    else MM3D_LAUNCH(c, "icp_robust_finalize", L.finalize_bytes, k_rob_finalize<false>, dim3(L.count), dim3(256), 0, (const NnRobustJob *)jobs.dev.get(), o);
  }
  void close(int b, const IcpState &h, IcpScoreJob &J) override { J.robust_stats = rob_stats(rec_host[b], h.iters, h.converged); }
};
}  // namespace

std::unique_ptr<IcpStep> icp_robust_step(const mm3d_icp_robust_options &opt, bool normals, int max_iterations)
{
  return std::unique_ptr<IcpStep>(new RobustStep(opt, normals, max_iterations));
}

// mm3d_debug_icp_robust: the search set-up as icp_batch derives it, iteration k's k_rob_wave at T with the split forced, every
// source point's match and weight at its original index, and the totals as the finalize would read them
static void debug_icp_robust(Context *c, const mm3d_cloud *src, const mm3d_cloud *tgt, const mm3d_normals *nrm, const float T[16],
                             double max_corr_dist, const mm3d_icp_robust_options &opt, int k, int split, int *idx, float *d2, double *weight,
                             double *sums, mm3d_icp_robust_stats *stats)
{
  const NnRange r = nn_range_icp(max_corr_dist);
  const bool plane = nrm != nullptr;
  const int nacc = plane ? kRobPlaneAcc : kRobAcc;
  const std::vector<double> table = rob_table(opt, k < INT_MAX ? k + 1 : k);
  const double sigma_k = table[std::min((size_t)k, table.size() - 1)];
  mm3d_icp_robust_stats S{0, 0, 0.0, sigma_k, 0, 0};
  std::vector<int> h_idx(src->n, -1);
  std::vector<float> h_d2(src->n, INFINITY);
  std::vector<double> h_w(src->n, 0.0), h_sums(nacc, 0.0);
  const NnSearch s = nn_search(c, src, tgt, &r);
  if (s.grid) {
    const unsigned nblocks = nn_blocks(s.n_items, split == 4);
    DevBuf<int> d_idx(c, src->n);
    DevBuf<float> d_d2(c, src->n);
    DevBuf<double> d_w(c, src->n), d_sums(c, nacc), d_sigma(c, table.size()), partials(c, (size_t)nblocks * nacc);
    DevBuf<IcpState> st(c, 1);
    DevBuf<NnRobustJob> d_job(c, 1);
    const size_t table_bytes = table.size() * sizeof(double);
    char *pinned = (char *)c->pin(sizeof(IcpState) + sizeof(NnRobustJob) + table_bytes + (size_t)nacc * sizeof(double) + 64);
    IcpState *hs = (IcpState *)pinned;
    NnRobustJob *hj = (NnRobustJob *)(hs + 1);
    double *ht = (double *)(hj + 1), *hsum = ht + table.size();
    std::memset(hs, 0, sizeof(IcpState));
    std::memcpy(hs->T, T, 64);
    hs->iters = k;
    std::memcpy(ht, table.data(), table_bytes);
    *hj = NnRobustJob{nn_job(s, split == 4, nblocks, st.get(), nullptr, partials.get(), nullptr), plane ? (const float4 *)nrm->nrm.get() : nullptr,
                      nullptr, d_idx.get(), d_d2.get(), d_w.get()};
    // (non-finite source points are in no work item: they keep -1 / +inf / 0)
    MM3D_HIP(hipMemcpyAsync(d_idx.get(), h_idx.data(), src->n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    MM3D_HIP(hipMemcpyAsync(d_d2.get(), h_d2.data(), src->n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    MM3D_HIP(hipMemsetAsync(d_w.get(), 0, src->n * sizeof(double), c->stream));
    MM3D_HIP(hipMemcpyAsync(st.get(), hs, sizeof(IcpState), hipMemcpyHostToDevice, c->stream));
    MM3D_HIP(hipMemcpyAsync(d_job.get(), hj, sizeof(NnRobustJob), hipMemcpyHostToDevice, c->stream));
    MM3D_HIP(hipMemcpyAsync(d_sigma.get(), ht, table_bytes, hipMemcpyHostToDevice, c->stream));
    const RobOpts o{opt.kernel == MM3D_ROBUST_OFF ? (int)MM3D_ROBUST_L2 : opt.kernel, rob_tuning(opt), opt.scale, d_sigma.get(), (int)table.size()};
    launch_rob_wave(c, d_job.get(), o, plane, 1, nblocks, split == 4, r.max_d2, r.rmax, s.ns * 36.0);
    if (plane) MM3D_LAUNCH(c, "icp_robust_totals", nblocks * nacc * 8.0, k_rob_totals<kRobPlaneAcc>, dim3(1), dim3(256), 0, (const NnRobustJob *)d_job.get(), d_sums.get());
    else MM3D_LAUNCH(c, "icp_robust_totals", nblocks * nacc * 8.0, k_rob_totals<kRobAcc>, dim3(1), dim3(256), 0, (const NnRobustJob *)d_job.get(), d_sums.get());
    MM3D_HIP(hipMemcpyAsync(h_idx.data(), d_idx.get(), src->n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MM3D_HIP(hipMemcpyAsync(h_d2.data(), d_d2.get(), src->n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    MM3D_HIP(hipMemcpyAsync(h_w.data(), d_w.get(), src->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    MM3D_HIP(hipMemcpyAsync(hsum, d_sums.get(), (size_t)nacc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    c->sync();
    std::memcpy(h_sums.data(), hsum, (size_t)nacc * sizeof(double));
    S.matched = (long long)h_sums[nacc - 2];
    S.weighted = (long long)h_sums[nacc - 1];
    S.weight_sum = h_sums[plane ? 28 : 16];
  }
  if (src->n) {
    std::memcpy(idx, h_idx.data(), src->n * sizeof(int));
    std::memcpy(d2, h_d2.data(), src->n * sizeof(float));
    std::memcpy(weight, h_w.data(), src->n * sizeof(double));
  }
  if (sums) std::memcpy(sums, h_sums.data(), (size_t)nacc * sizeof(double));
  if (stats) *stats = S;
}

}  // namespace mm3d

using namespace mm3d;

extern "C" {

int mm3d_set_icp_robust(mm3d_ctx *ctx, const mm3d_icp_robust_options *options)
{
  if (!ctx || !options || !icp_robust_options_valid(options)) return MM3D_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the selection changes)
  return select_stage(ctx, Stage::Robust, [&](StageSelection &s) { s.robust_options = *options; });
}

int mm3d_get_icp_robust(const mm3d_ctx *ctx, mm3d_icp_robust_options *options)
{
  if (!ctx || !options) return MM3D_EINVAL;
  *options = ctx->sel.robust_options;
  return MM3D_OK;
}

int mm3d_last_icp_robust_stats(const mm3d_ctx *ctx, mm3d_icp_robust_stats *stats)
{
  if (!ctx || !stats) return MM3D_EINVAL;
  *stats = ctx->last_robust_stats;
  return MM3D_OK;
}

int mm3d_estimate_transform_icp_robust(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target, const mm3d_normals *target_normals,
                                       const float initial_guess[16], double max_corr_dist, const mm3d_icp_robust_options *options,
                                       int max_iterations, double eps, float T[16], mm3d_icp_robust_stats *stats)
{
  if (!source || !target || !initial_guess || !options || !T || !icp_robust_options_valid(options)) return MM3D_EINVAL;
  if (target_normals && target_normals->n != target->n) {
    if (ctx) ctx->err = "mm3d_estimate_transform_icp_robust: the normals do not match the target's points";
    return MM3D_EINVAL;
  }
  return guarded(ctx, [&] {
    IcpScoreJob J;
    J.src = source; J.tgt = target; J.tgt_normals = target_normals;
    J.robust = options;
    std::memcpy(J.guess_host, initial_guess, sizeof(J.guess_host));
    icp_score_batch(ctx, target_normals ? icp_plane_method() : nullptr, &J, 1, true, max_corr_dist, max_iterations, eps, false, 0.0);
    std::memcpy(T, J.out.T, sizeof(J.out.T));
    // (a pair with nothing to search ran no iteration: its record is the empty one)
    J.robust_stats.iterations = J.out.iterations;
    J.robust_stats.converged = J.out.converged;
    ctx->last_robust_stats = J.robust_stats;
    if (stats) *stats = J.robust_stats;
  });
}

int mm3d_debug_icp_robust_split(int split)
{
  if (split == 0 || split == 1 || split == 4) g_forced_split.store(split);
  return g_forced_split.load();
}

int mm3d_debug_icp_robust(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target, const mm3d_normals *target_normals,
                          const float T[16], double max_correspondence_distance, const mm3d_icp_robust_options *options, int k, int split,
                          int *idx, float *d2, double *weight, double *sums, mm3d_icp_robust_stats *stats)
{
  if (!source || !target || !T || !options || !icp_robust_options_valid(options) || (split != 1 && split != 4) || k < 0) return MM3D_EINVAL;
  if (!(max_correspondence_distance >= 0.0) || !std::isfinite(max_correspondence_distance)) return MM3D_EINVAL;
  if (source->n && (!idx || !d2 || !weight)) return MM3D_EINVAL;
  if (target_normals && target_normals->n != target->n) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    debug_icp_robust(ctx, source, target, target_normals, T, max_correspondence_distance, *options, k, split, idx, d2, weight, sums, stats);
  });
}

}  // extern "C"

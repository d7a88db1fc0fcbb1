// icp_generalized.hip -- generalized ICP, opt-in (mm3d_set_icp_generalized): plane-to-plane refinement (Segal, Haehnel, Thrun,
// "Generalized-ICP", RSS 2009).  include/mm3d.h states the rule.
//
// Every other ICP here models the target's surface alone, so a correspondence is as good as its nearest neighbour: two maps
// sampled differently pull a point-to-point estimate along the surfaces, and a source point near an edge that matches the
// neighbouring face pulls a point-to-plane one.  Generalized ICP weights the correspondence's residual e = q - s by the inverse
// of the sum of BOTH surfaces' covariances, each the disc I - (1 - eps) n n^T of its normal (PCL's R diag(1, 1, eps) R^T): an
// in-plane slide then costs nothing, and a match across two faces counts only along their common edge.  The covariances follow
// from the normals the maps already keep: no per-map kernel and no per-map bytes.  A correspondence adds J^T W J and J^T W e
// (J = [-[s]x | I], three rows) to the same 6x6 system, so the 30 partial sums of k_icp_plane_wave stay the layout, and
// k_icp_plane_finalize runs unchanged behind this file's search kernel.
//   k_icp_generalized_wave   k_icp_plane_wave with the source's normals: nn_search_body.hpp once more, then three 16-byte loads
//                            per matched lane (the target's normal and point, the source's normal at the lane's original
//                            index), W = (C_t + R C_s R^T)^-1 by the adjugate in double on the lane, and the 30 terms formed
//                            from W (6), s (3) and W e (3), each wave-summed and stored one at a time into partials[block][kPlaneAcc].
#include <atomic>
#include <cmath>

#include "capi_guard.hpp"
#include "drivers.hpp"
#include "map_kept.hpp"
#include "icp_tail.hpp"
#include "nn_core.hpp"

namespace mm3d {

// the point-to-plane job plus the source's normals, in the source's reference order (nn.src's .w indexes them), and epsilon.
// pl.nn.partials: [nblocks][kPlaneAcc], read by k_icp_plane_finalize over the NnPlaneJobs.
struct NnGeneralizedJob {
  NnPlaneJob pl;
  const float4 *src_nrm;
  double epsilon;
};

// n / |n| in double; ok is false (and the vector zero) unless the three components are finite and n.n > 0
struct GicpUnit { double x, y, z; bool ok; };
__device__ __forceinline__ GicpUnit gicp_unit(const float4 n)
{
  GicpUnit u{0.0, 0.0, 0.0, false};
  if (!(isfinite(n.x) && isfinite(n.y) && isfinite(n.z))) return u;
  const double x = n.x, y = n.y, z = n.z;
  const double nn = (x * x + y * y) + z * z;
  if (!(nn > 0.0)) return u;
  const double len = sqrt(nn);
  u.x = x / len; u.y = y / len; u.z = z / len;
  u.ok = true;
  return u;
}

// The 27 terms of one correspondence from W (6), s (3) and We (3).  With C = [s]x: J^T W J = | C W C^T   C W |
//                                                                                         | W C^T     W   |
// and J^T W e = (s x We, We).  B(i, j) = (C W)(i, j) = (s x W's column j)(i); A(i, j) = (C W C^T)(i, j) = (s x B's row i)(j).
// The members are scalars and every index is a constant once the term loop is unrolled, so a term is its own few products on
// registers: nothing is indexed at run time, and nothing but the twelve doubles is held between two terms.
struct GicpLane {
  double w00, w01, w02, w11, w12, w22, sx, sy, sz, u0, u1, u2;
  __device__ __forceinline__ double w(int i, int j) const
  {
    const int a = i < j ? i : j, b = i < j ? j : i;
    if (a == 0) return b == 0 ? w00 : b == 1 ? w01 : w02;
    if (a == 1) return b == 1 ? w11 : w12;
    return w22;
  }
  __device__ __forceinline__ double B(int i, int j) const
  {
    if (i == 0) return sy * w(2, j) - sz * w(1, j);
    if (i == 1) return sz * w(0, j) - sx * w(2, j);
    return sx * w(1, j) - sy * w(0, j);
  }
  __device__ __forceinline__ double A(int i, int j) const
  {
    if (j == 0) return sy * B(i, 2) - sz * B(i, 1);
    if (j == 1) return sz * B(i, 0) - sx * B(i, 2);
    return sx * B(i, 1) - sy * B(i, 0);
  }
  __device__ __forceinline__ double ata(int i, int j) const      // i <= j, both in [0, 6)
  {
    if (j < 3) return A(i, j);
    if (i < 3) return B(i, j - 3);
    return w(i - 3, j - 3);
  }
  __device__ __forceinline__ double atr(int i) const
  {
    if (i == 0) return sy * u2 - sz * u1;
    if (i == 1) return sz * u0 - sx * u2;
    if (i == 2) return sx * u1 - sy * u0;
    return i == 3 ? u0 : i == 4 ? u1 : u2;
  }
};

template <int SPLIT>
__global__ void __launch_bounds__(256) MM3D_NN_ATTR
k_icp_generalized_wave(const NnGeneralizedJob *__restrict__ gjobs, float max_d2, float rmax)
{
  constexpr int MODE = 0;                                // (nn_search_body.hpp: the keyed search, with the winner's index)
  const NnJob &job = gjobs[blockIdx.y].pl.nn;
  if ((int)blockIdx.x >= job.nblocks) return;            // the grid is as wide as the batch's largest job
  const float4 *__restrict__ src = job.src;
  const int2 *__restrict__ items = job.items;
  const int n_items = job.n_items;
  const GridView g = job.g;
  const float4 *__restrict__ tgt_ref = job.tgt_ref;
  const float4 *__restrict__ nrm = gjobs[blockIdx.y].pl.nrm;
  const float4 *__restrict__ src_nrm = gjobs[blockIdx.y].src_nrm;
  const double k1e = 1.0 - gjobs[blockIdx.y].epsilon;
  const IcpState *__restrict__ st = job.st;
  double *__restrict__ partials = job.partials;
  const int max_ring = job.max_ring;
  __shared__ float Ts[16];
  __shared__ double red[4][kPlaneAcc];
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
  // the lane's W, s and W e (zero where it has no correspondence, or where either normal is unusable: such a correspondence
  // still counts, and its d2 goes into the MSE of the convergence test)
  GicpLane L{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double rows = 0.0;
  if (corr) {
    const unsigned w = (unsigned)(bkey & 0xffffffffull);
    const GicpUnit nt = gicp_unit(nrm[w]), ns = gicp_unit(src_nrm[__float_as_uint(src[i].w)]);
    if (nt.ok && ns.ok) {
      const float4 d = tgt_ref[w];
      // m = R n_s, R the 3x3 of T (column-major in Ts) in double; not renormalised
      const double mx = ((double)Ts[0] * ns.x + (double)Ts[4] * ns.y) + (double)Ts[8] * ns.z;
      const double my = ((double)Ts[1] * ns.x + (double)Ts[5] * ns.y) + (double)Ts[9] * ns.z;
      const double mz = ((double)Ts[2] * ns.x + (double)Ts[6] * ns.y) + (double)Ts[10] * ns.z;
      // Sigma = 2 I - (1 - eps) (n_t n_t^T + m m^T), symmetric: xx xy xz yy yz zz
      const double a = 2.0 - k1e * (nt.x * nt.x + mx * mx), b = -(k1e * (nt.x * nt.y + mx * my)), c = -(k1e * (nt.x * nt.z + mx * mz));
      const double dd = 2.0 - k1e * (nt.y * nt.y + my * my), e = -(k1e * (nt.y * nt.z + my * mz)), f = 2.0 - k1e * (nt.z * nt.z + mz * mz);
      // W = adj(Sigma) / det(Sigma)
      const double c00 = dd * f - e * e, c01 = c * e - b * f, c02 = b * e - c * dd;
      const double det = (a * c00 + b * c01) + c * c02;
      L.w00 = c00 / det; L.w01 = c01 / det; L.w02 = c02 / det;
      L.w11 = (a * f - c * c) / det; L.w12 = (b * c - a * e) / det; L.w22 = (a * dd - b * b) / det;
      L.sx = p.x; L.sy = p.y; L.sz = p.z;
      const double ex = (double)d.x - L.sx, ey = (double)d.y - L.sy, ez = (double)d.z - L.sz;
      L.u0 = (L.w00 * ex + L.w01 * ey) + L.w02 * ez;
      L.u1 = (L.w01 * ex + L.w11 * ey) + L.w12 * ez;
      L.u2 = (L.w02 * ex + L.w12 * ey) + L.w22 * ez;
      rows = 3.0;
    }
  }
  // one term at a time (icp_store_partials)
  auto term = [&](int k) -> double {
    if (k < 21) return L.ata(kUi[k], kUj[k]);
    if (k < 27) return L.atr(k - 21);
    if (k == 27) return corr ? (double)best : 0.0;
    if (k == 28) return corr ? 1.0 : 0.0;
    return rows;
  };
  // a wave none of whose points found a neighbour in range adds zeros without the reductions (as k_nn_wave does)
  const bool any_corr = ballot(corr) != 0ull;       // wave-uniform
  icp_store_partials<kPlaneAcc, SPLIT>(term, any_corr, red, partials, bid);
}

static std::atomic<int> g_generalized_forced_split{0};      // mm3d_debug_icp_generalized_split: 0 (by size), 1 or 4

namespace {
// point-to-plane's jobs, partials and finalize kernel behind this file's search + reduction launch
struct GeneralizedStep final : IcpStep {
  StepJobs<NnPlaneJob> plane;
  StepJobs<NnGeneralizedJob> jobs;
  GeneralizedStep() { acc = kPlaneAcc; forced_split = g_generalized_forced_split.load(); }
  double bytes_per_point(const IcpScoreJob &) const override { return 60.0; }      // (+ the winner's normal and point, the source's normal)
  void check(const IcpScoreJob &J) const override
  {
    icp_plane_check(J);
    if (!J.src_normals || J.src_normals->n != J.src->n)
      throw Error(MM3D_EINVAL, "generalized ICP: the source's normals do not match its points");
  }
  size_t pinned_bytes(int B) const override { return plane.bytes(B) + jobs.bytes(B); }
  void begin(Context *c, const IcpScoreJob *const *, int B, char *pinned, void *, void *) override { jobs.begin(c, B, plane.begin(c, B, pinned)); }
  void bind(int b, const NnJob &q, const IcpScoreJob &J) override
  {
    plane.host[b] = icp_plane_job(q, J);
    jobs.host[b] = NnGeneralizedJob{plane.host[b], J.src_normals ? (const float4 *)J.src_normals->nrm.get() : nullptr, J.generalized_epsilon};
  }
  void upload(Context *c) override { plane.upload(c); jobs.upload(c); }
  void iterate(Context *c, const IcpLaunch &L) override
  {
    if (L.split)
      MM3D_LAUNCH(c, "icp_generalized_corr_reduce", L.bytes, k_icp_generalized_wave<4>, dim3(L.grid_x, L.count), dim3(256), 0,
                  (const NnGeneralizedJob *)jobs.dev.get(), L.max_d2, L.rmax);
    else
      MM3D_LAUNCH(c, "icp_generalized_corr_reduce", L.bytes, k_icp_generalized_wave<1>, dim3(L.grid_x, L.count), dim3(256), 0,
                  (const NnGeneralizedJob *)jobs.dev.get(), L.max_d2, L.rmax);
    icp_plane_finalize(c, plane.dev.get(), L.count, L.finalize_bytes);
  }
};
}  // namespace

static bool icp_generalized_options_valid(const mm3d_icp_generalized_options *o)
{
  if (o->enabled != 0 && o->enabled != 1) return false;
  return o->epsilon > 0.0 && o->epsilon <= 1.0;       // (false for NaN)
}

namespace {
struct IcpGeneralized final : IcpMethodBase {
  int method() const override { return MM3D_ICP_POINT_TO_PLANE; }     // (not read: mm3d_get_icp_method answers StageSelection::icp's)
  std::unique_ptr<IcpStep> step(const mm3d_icp_rejection_options *) const override { return std::unique_ptr<IcpStep>(new GeneralizedStep()); }
  void prepare_target(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p, IcpScoreJob *job) const override
  {
    const mm3d_normals *n = map_normals(ctx, m, p);
    if (job) {
      job->tgt_normals = n;
      job->generalized_epsilon = ctx->sel.generalized_options.epsilon;
    }
  }
  void prepare_source(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p, IcpScoreJob *job) const override
  {
    const mm3d_normals *n = map_normals(ctx, m, p);
    if (job) job->src_normals = n;
  }
};
const IcpGeneralized g_generalized;
}  // namespace

}  // namespace mm3d

using namespace mm3d;

extern "C" {

int mm3d_set_icp_generalized(mm3d_ctx *ctx, const mm3d_icp_generalized_options *options)
{
  if (!ctx || !options || !icp_generalized_options_valid(options)) return MM3D_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the selection changes)
  return select_stage(ctx, Stage::Generalized, [&](StageSelection &s) {
    s.generalized_options = *options;
    s.generalized = stage_active(Stage::Generalized, s) ? &g_generalized : nullptr;
  });
}

int mm3d_get_icp_generalized(const mm3d_ctx *ctx, mm3d_icp_generalized_options *options)
{
  if (!ctx || !options) return MM3D_EINVAL;
  *options = ctx->sel.generalized_options;
  return MM3D_OK;
}

int mm3d_estimate_transform_icp_generalized(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_normals *source_normals,
                                            const mm3d_cloud *target, const mm3d_normals *target_normals, const float initial_guess[16],
                                            double max_corr_dist, const mm3d_icp_generalized_options *options, int max_iterations,
                                            double eps, float T[16])
{
  if (!source || !source_normals || !target || !target_normals || !initial_guess || !options || !T || !icp_generalized_options_valid(options))
    return MM3D_EINVAL;
  if (source_normals->n != source->n) {
    if (ctx) ctx->err = "mm3d_estimate_transform_icp_generalized: the normals do not match the source's points";
    return MM3D_EINVAL;
  }
  if (target_normals->n != target->n) {
    if (ctx) ctx->err = "mm3d_estimate_transform_icp_generalized: the normals do not match the target's points";
    return MM3D_EINVAL;
  }
  return guarded(ctx, [&] {
    IcpScoreJob J;
    J.src = source; J.tgt = target; J.src_normals = source_normals; J.tgt_normals = target_normals;
    J.generalized_epsilon = options->epsilon;
    std::memcpy(J.guess_host, initial_guess, sizeof(J.guess_host));
    icp_score_batch(ctx, &g_generalized, &J, 1, true, max_corr_dist, max_iterations, eps, false, 0.0);
    std::memcpy(T, J.out.T, sizeof(J.out.T));
  });
}

int mm3d_debug_icp_generalized_split(int split)
{
  if (split == 0 || split == 1 || split == 4) g_generalized_forced_split.store(split);
  return g_generalized_forced_split.load();
}

}  // extern "C"

// icp_plane.hip -- point-to-plane ICP, the opt-in alternative to the reference's point-to-point ICP (mm3d_set_icp_method).
//
// PCL's IterativeClosestPoint with TransformationEstimationPointToPlaneLLS and DefaultConvergenceCriteria: the loop of nn.hip's
// ICP (float transform of the source, exact float nearest neighbour accepted at d2 <= max_d2, T <- Tinc * T in float, the
// convergence tests on the same IcpState: icp_tail.hpp's icp_advance) with a different transform estimate.  For each correspondence
// (s = source point after the current transform, d = target point, n = its normal, finite):
//   row  = [a, b, c, nx, ny, nz],  a = nz sy - ny sz,  b = nx sz - nz sx,  c = ny sx - nx sy
//   r    = n.d - n.s
// and, in double, the 21 sums of the upper triangle of AtA and the 6 of Atr; x = (alpha, beta, gamma, tx, ty, tz) solves
// AtA x = Atr (an unpivoted LDLt in double), and Tinc = [Rz(gamma) Ry(beta) Rx(alpha) | t] (PCL's constructTransformationMatrix).
// Both sums are invariant under n -> -n, so the normals' orientation does not matter.
//
// Two launches per iteration, like icp_corr_reduce / icp_finalize; the row, its terms, the estimate and the convergence step are
// icp_tail.hpp's, shared with the other variants:
//   k_icp_plane_wave      nn_search_body.hpp's wave-cooperative search (the same include as k_nn_wave), then the winner's normal
//                         (one 16-byte load per lane) and the 30 terms (the 27 above, d2, the correspondence, the row) in
//                         double, reduced one term at a time through wave shuffles -> LDS -> partials[block][kPlaneAcc] in
//                         k_nn_wave's fixed order (so the result does not depend on the batch or on the split either);
//   k_icp_plane_finalize  one block per pair: the partials in a fixed order, the 6x6 solve on one lane, Tinc, the convergence step.
//                         Coloured ICP, generalized ICP and the rejecting step with normals end an iteration with it too.
#include <cmath>

#include "capi_guard.hpp"
#include "drivers.hpp"
#include "map_kept.hpp"
#include "icp_tail.hpp"
#include "nn_core.hpp"

namespace mm3d {

template <int SPLIT>
__global__ void __launch_bounds__(256) MM3D_NN_ATTR
k_icp_plane_wave(const NnPlaneJob *__restrict__ pjobs, float max_d2, float rmax)
{
  constexpr int MODE = 0;                                // (nn_search_body.hpp: the keyed search, with the winner's index)
  const NnJob &job = pjobs[blockIdx.y].nn;
  if ((int)blockIdx.x >= job.nblocks) return;            // the grid is as wide as the batch's largest job
  const float4 *__restrict__ src = job.src;
  const int2 *__restrict__ items = job.items;
  const int n_items = job.n_items;
  const GridView g = job.g;
  const float4 *__restrict__ tgt_ref = job.tgt_ref;
  const float4 *__restrict__ nrm = pjobs[blockIdx.y].nrm;
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
  // the lane's row (zero where it has none, or where the target normal is not finite)
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double r = 0.0, has_row = 0.0;
  if (corr) {
    const unsigned w = (unsigned)(bkey & 0xffffffffull);
    if (icp_plane_row(p, nrm[w], tgt_ref[w], v, r)) has_row = 1.0;
  }
  auto term = [&](int k) -> double { return icp_plane_term(k, v, r, corr, best, has_row); };
  // a wave none of whose points found a neighbour in range adds zeros without the reductions (as k_nn_wave does)
  const bool any_corr = ballot(corr) != 0ull;       // wave-uniform
  icp_store_partials<kPlaneAcc, SPLIT>(term, any_corr, red, partials, bid);
}

__global__ void __launch_bounds__(256) k_icp_plane_finalize(const NnPlaneJob *__restrict__ pjobs)
{
  __shared__ double red[4][kPlaneAcc];
  __shared__ double tot[kPlaneAcc];
  const NnJob &job = pjobs[blockIdx.x].nn;
  IcpState *st = job.st;
  if (st->done) return;
  icp_totals<kPlaneAcc>(job, red, tot);
  if (threadIdx.x != 0) return;

  const double cnt = tot[28];
  st->n_corr = (int)cnt;
  if (cnt < 3.0) return icp_stop_unconverged(st);   // min_number_correspondences_: "Not enough correspondences"
  float Ti[16];
  // degenerate (fewer than six rows, or a plane / line that leaves a direction free): stop, not converged, T unchanged
  if (tot[29] < 6.0 || !icp_solve6_transform(tot, Ti)) return icp_stop_unconverged(st);
  icp_advance(st, Ti, true, tot[27] / cnt);
}

// (alone after the search of icp_color.hip and after the rejecting correspondence stage of icp_reject.hip, which write the
// partials this reads)
void icp_plane_finalize(Context *c, const NnPlaneJob *jobs_dev, int count, double finalize_bytes)
{
  MM3D_LAUNCH(c, "icp_plane_finalize", finalize_bytes, k_icp_plane_finalize, dim3(count), dim3(256), 0, jobs_dev);
}

namespace {
// icp_corr_reduce's and icp_finalize's counterparts over the ICP jobs with their normals
struct PlaneStep final : IcpStep {
  StepJobs<NnPlaneJob> jobs;
  PlaneStep() { acc = kPlaneAcc; }
  double bytes_per_point(const IcpScoreJob &) const override { return 28.0; }      // (+ the winner's normal)
  void check(const IcpScoreJob &J) const override { icp_plane_check(J); }
  size_t pinned_bytes(int B) const override { return jobs.bytes(B); }
  void begin(Context *c, const IcpScoreJob *const *, int B, char *pinned, void *, void *) override { jobs.begin(c, B, pinned); }
  void bind(int b, const NnJob &q, const IcpScoreJob &J) override { jobs.host[b] = icp_plane_job(q, J); }
  void upload(Context *c) override { jobs.upload(c); }
  void iterate(Context *c, const IcpLaunch &L) override
  {
    if (L.split)
      MM3D_LAUNCH(c, "icp_plane_corr_reduce", L.bytes, k_icp_plane_wave<4>, dim3(L.grid_x, L.count), dim3(256), 0, (const NnPlaneJob *)jobs.dev.get(),
                  L.max_d2, L.rmax);
    else
      MM3D_LAUNCH(c, "icp_plane_corr_reduce", L.bytes, k_icp_plane_wave<1>, dim3(L.grid_x, L.count), dim3(256), 0, (const NnPlaneJob *)jobs.dev.get(),
                  L.max_d2, L.rmax);
    icp_plane_finalize(c, jobs.dev.get(), L.count, L.finalize_bytes);
  }
};

struct IcpPointToPlane final : IcpMethodBase {
  int method() const override { return MM3D_ICP_POINT_TO_PLANE; }
  std::unique_ptr<IcpStep> step(const mm3d_icp_rejection_options *reject) const override
  {
    return reject ? icp_reject_step(*reject, true) : std::unique_ptr<IcpStep>(new PlaneStep());
  }
  void prepare_target(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p, IcpScoreJob *job) const override
  {
    const mm3d_normals *n = map_normals(ctx, m, p);
    if (job) job->tgt_normals = n;
  }
};
const IcpPointToPlane g_point_to_plane;
}  // namespace
const IcpMethodBase *icp_plane_method() { return &g_point_to_plane; }

}  // namespace mm3d

using namespace mm3d;

extern "C" {

int mm3d_set_icp_method(mm3d_ctx *ctx, int method)
{
  if (!ctx || (method != MM3D_ICP_POINT_TO_POINT && method != MM3D_ICP_POINT_TO_PLANE)) return MM3D_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the method changes)
  // deliberate compatibility: a device-list context refuses every call of this setter, MM3D_ICP_POINT_TO_POINT included,
  // where every other setter accepts an inactive selection
  if (ctx->device_set) return refuse_device_list(ctx, Stage::IcpMethod);
  return select_stage(ctx, Stage::IcpMethod, [&](StageSelection &s) { s.icp = method == MM3D_ICP_POINT_TO_PLANE ? &g_point_to_plane : nullptr; });
}

int mm3d_get_icp_method(const mm3d_ctx *ctx)
{
  if (!ctx) return MM3D_EINVAL;
  return ctx->sel.icp_method();
}

int mm3d_estimate_transform_icp_plane(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target, const mm3d_normals *target_normals,
                                      const float initial_guess[16], double max_corr_dist, int max_iterations, double eps, float T[16])
{
  if (!source || !target || !target_normals || !initial_guess || !T) return MM3D_EINVAL;
  if (target_normals->n != target->n) {
    if (ctx) ctx->err = "mm3d_estimate_transform_icp_plane: the normals do not match the target's points";
    return MM3D_EINVAL;
  }
  return guarded(ctx, [&] {
    IcpScoreJob J;
    J.src = source; J.tgt = target; J.tgt_normals = target_normals;
    std::memcpy(J.guess_host, initial_guess, sizeof(J.guess_host));
    icp_score_batch(ctx, &g_point_to_plane, &J, 1, true, max_corr_dist, max_iterations, eps, false, 0.0);
    std::memcpy(T, J.out.T, sizeof(J.out.T));
  });
}

}  // extern "C"

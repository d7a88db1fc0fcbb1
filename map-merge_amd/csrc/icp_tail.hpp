// icp_tail.hpp -- how every ICP refinement ends an iteration, once: the pieces that the wave kernels and the one-block finalize
// kernels of nn.hip, icp_plane.hip, icp_color.hip, icp_generalized.hip, icp_reject.hip, icp_robust.hip and ndt.hip are made of.
//   wave kernels      icp_plane_row / icp_plane_term   the point-to-plane row of one correspondence and its 30 terms
//                     icp_store_partials               "one term at a time": formed, summed over the wave, stored per item
//                                                      (SPLIT 4) or through red[wave][k] and the four-way add per block
//   finalize kernels  icp_totals                       the partials in one fixed order -> tot[NACC]
//                     icp_umeyama / icp_solve6_transform   the totals -> Tinc (3x3 Jacobi SVD; 6x6 LDLt and Rz Ry Rx)
//                     icp_advance / icp_stop_unconverged   T <- Tinc * T, the count, PCL's DefaultConvergenceCriteria
// A caller keeps what is its own: the mse expression, the count checks, the records.  Device inline functions only; with
// -ffp-contract=off an inlined expression rounds as the same text pasted into the kernel would, which is what the bit-for-bit
// ties between the variants (robust L2 = default, nothing rejected = default, colour at lambda 1 = plane) rest on.
#pragma once
#include "icp_solve6.hpp"
#include "nn_core.hpp"

namespace mm3d {

// ---- wave kernels ----

// The row of one correspondence (s = source point after the current transform, d = target point, n = its normal):
//   v = [nz sy - ny sz, nx sz - nz sx, ny sx - nx sy, nx, ny, nz],  r = n.d - n.s
// false, and v and r untouched (the caller's zeros), where the normal is not finite: such a correspondence still counts, and
// its d2 goes into the MSE of the convergence test.  d is read only behind that test (pass tgt_ref[w] itself).
__device__ __forceinline__ bool icp_plane_row(const float3 p, const float4 n, const float4 &d, double v[6], double &r)
{
  if (!(isfinite(n.x) && isfinite(n.y) && isfinite(n.z))) return false;
  const double sx = p.x, sy = p.y, sz = p.z, nx = n.x, ny = n.y, nz = n.z;
  v[0] = nz * sy - ny * sz;
  v[1] = nx * sz - nz * sx;
  v[2] = ny * sx - nx * sy;
  v[3] = nx; v[4] = ny; v[5] = nz;
  r = (nx * (double)d.x + ny * (double)d.y + nz * (double)d.z) - (nx * sx + ny * sy + nz * sz);
  return true;
}

// term k of kPlaneAcc: AtA's upper triangle (21) | Atr (6) | d2 | the correspondence | the row
__device__ __forceinline__ double icp_plane_term(int k, const double v[6], double r, bool corr, float best, double has_row)
{
  if (k < 21) return v[kUi[k]] * v[kUj[k]];
  if (k < 27) return v[k - 21] * r;
  if (k == 27) return corr ? (double)best : 0.0;
  if (k == 28) return corr ? 1.0 : 0.0;
  return has_row;
}

// One term at a time (formed, summed over the wave, stored): NACC doubles held at once would cost 2 NACC VGPRs on top of the
// search.  The loop is unrolled: k is a constant in every term(k).  A wave with `any` false (wave-uniform: none of its lanes
// has anything to add) writes zeros without the reductions.  SPLIT 4: the calling wave's sums are item bid's partials;
// SPLIT 1: by all four waves of the block, whose sums meet in red and are added in the order icp_totals adds four items'.
template <int NACC, int SPLIT, class Term>
__device__ __forceinline__ void icp_store_partials(Term &&term, bool any, double (*red)[NACC], double *__restrict__ partials, unsigned bid)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NACC; ++k) {
    const double s = any ? wave_sum(term(k)) : 0.0;
    if (lane == 0) {
      if (SPLIT == 4) partials[(size_t)bid * NACC + k] = s;
      else red[wave][k] = s;
    }
  }
  if (SPLIT == 4) return;
  __syncthreads();
  if (threadIdx.x < NACC) {
    const int k = threadIdx.x;
    partials[(size_t)bid * NACC + k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
  }
}

// ---- finalize kernels (one block of 256 threads per pair) ----

// The pair's totals in one fixed order: a thread's blocks b = t, t + 256, ... (nn_block_partial_n: four items make a block
// under `split`), the wave, the four waves.  By all 256 threads; tot is valid for every thread afterwards.
template <int NACC>
__device__ __forceinline__ void icp_totals(const double *__restrict__ partials, int nblocks, int split, int n_items, double (*red)[NACC],
                                           double *tot)
{
  double acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += blockDim.x)
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] += nn_block_partial_n<NACC>(partials, b, k, split, n_items);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NACC; ++k) {
    const double v = wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < NACC) tot[threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
  __syncthreads();
}
// ... of a search job, whichever kernel variant wrote its partials: in units of four items
template <int NACC>
__device__ __forceinline__ void icp_totals(const NnJob &job, double (*red)[NACC], double *tot)
{
  icp_totals<NACC>(job.partials, (job.n_items + 3) >> 2, job.split, job.n_items, red, tot);
}

// The rest is one thread's.

// "Not enough correspondences", or a degenerate system: stop, not converged, T as it was before the iteration
__device__ __forceinline__ void icp_stop_unconverged(IcpState *st)
{
  st->converged = 0;
  st->done = 1;
}

// Umeyama (linalg_shared.hpp's core, Eigen's float precision) from the moments tot[0..14] = sum p | sum q | sum q p^T and
// inv = 1 / their weight: Tinc's rotation and translation
__device__ __forceinline__ void icp_umeyama(const double *tot, double inv, float Ti[16])
{
  double mp[3] = {tot[0] * inv, tot[1] * inv, tot[2] * inv}, mq[3] = {tot[3] * inv, tot[4] * inv, tot[5] * inv};
  double sigma[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) sigma[r * 3 + c] = tot[6 + r * 3 + c] * inv - mq[r] * mp[c];
  double R[9], t[3];
  umeyama_core_shared(sigma, mp, mq, 1e-5, R, t);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Ti[c * 4 + r] = (float)R[r * 3 + c];
  for (int r = 0; r < 3; ++r) {
    // t = dst_mean - R * src_mean (with the float R, like Eigen's float instantiation: not the core's t)
    const double a = mq[r] - ((double)Ti[0 * 4 + r] * mp[0] + (double)Ti[1 * 4 + r] * mp[1] + (double)Ti[2 * 4 + r] * mp[2]);
    Ti[12 + r] = (float)a;
  }
}

// The six-parameter estimate from tot[0..26] = AtA's upper triangle | Atr: x = (alpha, beta, gamma, tx, ty, tz) by solve6_ldlt,
// Tinc's rotation and translation by PCL's constructTransformationMatrix.  false (Ti untouched) where a pivot is at or below
// kPlanePivotTau * trace / 6: a plane or a line that leaves a direction free.  The row-count gate is the caller's.
__device__ __forceinline__ bool icp_solve6_transform(const double *tot, float Ti[16])
{
  double A[36], b[6], x[6];
  for (int k = 0; k < 21; ++k) A[kUi[k] * 6 + kUj[k]] = A[kUj[k] * 6 + kUi[k]] = tot[k];
  for (int i = 0; i < 6; ++i) b[i] = tot[21 + i];
  const double trace = A[0] + A[7] + A[14] + A[21] + A[28] + A[35];
  if (!solve6_ldlt(A, b, kPlanePivotTau * trace / 6.0, x)) return false;
  // constructTransformationMatrix(alpha, beta, gamma, tx, ty, tz) = [Rz(gamma) Ry(beta) Rx(alpha) | t]:
  //   | cg cb   -sg ca + cg sb sa    sg sa + cg sb ca |
  //   | sg cb    cg ca + sg sb sa   -cg sa + sg sb ca |
  //   | -sb      cb sa               cb ca            |
  const double sa = sin(x[0]), ca = cos(x[0]), sb = sin(x[1]), cb = cos(x[1]), sg = sin(x[2]), cg = cos(x[2]);
  const double R[9] = {cg * cb, -sg * ca + cg * sb * sa, sg * sa + cg * sb * ca,
                       sg * cb, cg * ca + sg * sb * sa, -cg * sa + sg * sb * ca,
                       -sb, cb * sa, cb * ca};
  for (int rr = 0; rr < 3; ++rr)
    for (int c = 0; c < 3; ++c) Ti[c * 4 + rr] = (float)R[rr * 3 + c];
  Ti[12] = (float)x[3]; Ti[13] = (float)x[4]; Ti[14] = (float)x[5];
  return true;
}

// final = Tinc * final, the iteration count, and DefaultConvergenceCriteria::hasConverged on Tinc and mse (the caller's
// measure: st->prev_mse holds the last one).  Completes Ti's last row.  test_convergence false: only max_iter can stop the
// loop (a robust run does not stop on a scale it is about to leave).
__device__ __forceinline__ void icp_advance(IcpState *st, float Ti[16], bool test_convergence, double mse)
{
  Ti[3] = Ti[7] = Ti[11] = 0.0f;
  Ti[15] = 1.0f;
  float Tn[16];
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) {
      float a = 0.0f;
      for (int k = 0; k < 4; ++k) a += Ti[k * 4 + r] * st->T[c * 4 + k];
      Tn[c * 4 + r] = a;
    }
  for (int i = 0; i < 16; ++i) { st->T[i] = Tn[i]; st->Tinc[i] = Ti[i]; }
  const int iters = ++st->iters;
  if (iters >= st->max_iter) { st->converged = 1; st->done = 1; return; }
  if (!test_convergence) return;
  const double cos_angle = 0.5 * ((double)Ti[0] + (double)Ti[5] + (double)Ti[10] - 1.0);
  const double translation_sqr = (double)Ti[12] * Ti[12] + (double)Ti[13] * Ti[13] + (double)Ti[14] * Ti[14];
  if (cos_angle >= st->rot_thresh && translation_sqr <= st->trans_thresh) { st->converged = 1; st->done = 1; return; }
  if (fabs(mse - st->prev_mse) < 1e-12) { st->converged = 1; st->done = 1; return; }
  st->prev_mse = mse;
}

}  // namespace mm3d

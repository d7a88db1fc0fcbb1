// ndt.hip -- NDT refinement, the opt-in alternative to the pair stage's ICP (mm3d_set_refinement; include/mm3d.h states the
// rule to the operation).  A Gauss-Newton form of the point-to-distribution Normal Distributions Transform (Biber & Strasser
// 2003, Magnusson 2009): the target is one Gaussian per voxel of the global lattice, and a source point finds its terms by
// computing an index -- no search.  Not a reference stage, and no parity with pcl::NormalDistributionsTransform is claimed
// (audit row 16b).
//
// The table of a target, built once per map (ndt_build_table), one host wait -- the one that sizes it:
//   ndt_range      the voxel index range of the finite points (lattice.hpp::k_lattice_range, as every stage of the global lattice)
//   k_ndt_keys     a lane per point: voxel key relative to the range's minimum, i most significant, so that ascending keys
//                  are ascending (i, j, k)
//   radix sort     (key, input index) pairs, stable: a voxel becomes a run in ascending input index
//   scan_fused     run heads (lattice.hpp::LatticeRunHead) -> the start of every voxel's run, their number and the number of finite points
//   (the wait: range and counts; the records and the dense index are allocated)
//   k_ndt_voxels   a wave per voxel: mean, covariance (two passes), regularisation and the closed-form inverse in double.
//                  Lane l takes the run's positions l, l + 64, ... in ascending order and the 64 lane sums meet in wave_sum's
//                  fixed butterfly: one order, whatever the launch.  Lane 0 rounds to float once, stores the 48-byte record
//                  and the voxel's word of the dense index.
// One iteration of a batch (NdtStep), two launches like icp_corr_reduce / icp_finalize:
//   k_ndt_wave      a lane per source point over the source's Hilbert order and work items (k_nn_wave's: neighbouring lanes
//                   hit neighbouring voxels), blockIdx.y = the pair.  1 or 7 index loads, three 16-byte loads per valid
//                   voxel, the terms in double; per lane sum_w P (6), sum_w P q (3), sum w and the term count, from which the
//                   30 sums are formed and reduced one at a time: wave shuffles -> LDS -> partials[block][kNdtAcc], four
//                   work items per block whatever the batch, so the result depends on neither batch nor stream count.
//   k_ndt_finalize  one block per pair: the partials in a fixed order, the 6x6 solve on one lane, Tinc, the convergence step
//                   on the same IcpState, with the mean weight in the place of the mean d2 -- icp_tail.hpp's pieces, the ones
//                   every ICP's finalize is made of.
#include <cmath>
#include <cstring>

#include "capi_guard.hpp"
#include "drivers.hpp"
#include "map_kept.hpp"
#include "icp_tail.hpp"
#include "lattice.hpp"
#include "nn_core.hpp"
#include "scan_fused.hpp"

namespace mm3d {

// The job's source side and state (nn.g, nn.tgt_ref and nn.max_ring are not read; nn.split is 0: always four work items per
// block, so nn.partials is [ceil(n_items / 4)][kNdtAcc] whatever the batch), and the target's voxel table
struct NdtJob {
  NnJob nn;
  const float4 *rec;          // NdtTable::rec
  const int *index;           // NdtTable::index
  float inv, mn[3];
  int dims[3];
  int neighbours;             // 1 or 7
  int n_src;                  // finite source points: the divisor of the convergence test's mean weight
};
// H upper triangle (21) | g (6) | sum w | terms | points with at least one term
constexpr int kNdtAcc = 30;

namespace {

// the dense index holds one int32 per cell of the voxel bounding box: at most 2^26 cells (256 MiB) -- include/mm3d.h and
// INTEGRATION.md "Size limits" state it
constexpr double kNdtMaxCells = 67108864.0;
// mm3d_set_refinement with resolution = 0: the voxel side is params.resolution times this (DESIGN.md section 7e has the measurement)
constexpr double kNdtDefaultMultiple = 10.0;

// the box of the range words is within the index limit (false for the inf or NaN of an infinite index or an untouched range)
__host__ __device__ inline bool ndt_fits(const LatticeFrame<3> &f) { return f.cells <= kNdtMaxCells; }

__global__ void __launch_bounds__(256)
k_ndt_keys(const float4 *__restrict__ pts, int n, float inv, const unsigned *__restrict__ range, uint32_t *__restrict__ keys,
           uint32_t *__restrict__ vals)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  vals[i] = (uint32_t)i;
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) { keys[i] = kLatticeInvalid; return; }
  const LatticeFrame<3> f = lattice_frame<3>(range);
  uint32_t key = 0;                                       // (a box beyond the limit: the host refuses it, the runs are not read)
  if (ndt_fits(f)) {
    const uint32_t ri = (uint32_t)((double)lattice_index(p.x, inv) - f.mn[0]), rj = (uint32_t)((double)lattice_index(p.y, inv) - f.mn[1]),
                   rk = (uint32_t)((double)lattice_index(p.z, inv) - f.mn[2]);
    key = (ri * (uint32_t)f.d[1] + rj) * (uint32_t)f.d[2] + rk;     // < 2^26
  }
  keys[i] = key;
}

// starts[v] = the sorted position at which voxel v's run begins; info[0] = voxels, info[1] = finite points (where the last run ends)
struct NdtStartStore {
  const uint32_t *keys; size_t n; int *starts; unsigned *info;
  __device__ __forceinline__ void operator()(size_t j, int prefix, int v) const
  {
    if (v) starts[prefix] = (int)j;
    if (j == n - 1) info[0] = (unsigned)(prefix + v);
    if (keys[j] != kLatticeInvalid && (j == n - 1 || keys[j + 1] == kLatticeInvalid)) info[1] = (unsigned)(j + 1);
  }
  __device__ __forceinline__ void done() const {}
};

__global__ void __launch_bounds__(256)
k_ndt_voxels(const float4 *__restrict__ pts, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ order,
             const int *__restrict__ starts, int n_voxels, int n_finite, int min_points, double kappa, float4 *__restrict__ rec,
             int *__restrict__ index)
{
  const int lane = threadIdx.x & 63;
  const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (v >= n_voxels) return;                             // (wave-uniform)
  const int b = starts[v], e = v + 1 < n_voxels ? starts[v + 1] : n_finite;
  const int cnt = e - b;
  double s[3] = {0.0, 0.0, 0.0};
  for (int j = b + lane; j < e; j += kWave) {
    const float4 p = pts[order[j]];
    s[0] += (double)p.x; s[1] += (double)p.y; s[2] += (double)p.z;
  }
  double mu[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) mu[a] = __shfl(wave_sum(s[a]), 0, kWave) / (double)cnt;
  double cv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};        // xx xy xz yy yz zz
  for (int j = b + lane; j < e; j += kWave) {
    const float4 p = pts[order[j]];
    const double dx = (double)p.x - mu[0], dy = (double)p.y - mu[1], dz = (double)p.z - mu[2];
    cv[0] += dx * dx; cv[1] += dx * dy; cv[2] += dx * dz; cv[3] += dy * dy; cv[4] += dy * dz; cv[5] += dz * dz;
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) cv[a] = wave_sum(cv[a]);
  if (lane != 0) return;
  float4 r0 = make_float4((float)mu[0], (float)mu[1], (float)mu[2], 0.0f);
  float4 r1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r2 = make_float4(0.0f, 0.0f, __int_as_float(cnt), 0.0f);
  if (cnt >= min_points) {
    const double inv_n1 = 1.0 / (double)(cnt - 1);
    double xx = cv[0] * inv_n1, xy = cv[1] * inv_n1, xz = cv[2] * inv_n1, yy = cv[3] * inv_n1, yz = cv[4] * inv_n1, zz = cv[5] * inv_n1;
    const double trace = xx + yy + zz;
    const double reg = kappa * (trace / 3.0);
    xx += reg; yy += reg; zz += reg;
    // the inverse by the adjugate
    const double a00 = yy * zz - yz * yz, a01 = xz * yz - xy * zz, a02 = xy * yz - xz * yy;
    const double a11 = xx * zz - xz * xz, a12 = xy * xz - xx * yz, a22 = xx * yy - xy * xy;
    const double det = xx * a00 + xy * a01 + xz * a02;
    const float P[6] = {(float)(a00 / det), (float)(a01 / det), (float)(a02 / det), (float)(a11 / det), (float)(a12 / det), (float)(a22 / det)};
    bool ok = trace > 0.0 && isfinite(r0.x) && isfinite(r0.y) && isfinite(r0.z);
#pragma unroll
    for (int a = 0; a < 6; ++a) ok = ok && isfinite(P[a]);
    if (ok) {
      r0.w = 1.0f;
      r1 = make_float4(P[0], P[1], P[2], P[3]);
      r2.x = P[4]; r2.y = P[5];
    }
  }
  rec[(size_t)v * 3] = r0;
  rec[(size_t)v * 3 + 1] = r1;
  rec[(size_t)v * 3 + 2] = r2;
  index[keys[b]] = v;                                    // (a key is a cell of the dense index, below its size)
}

// column j of J = [-[s]x | I] for the point s: the first three are e_j x s
__device__ __forceinline__ void ndt_jcol(int j, double sx, double sy, double sz, double c[3])
{
  c[0] = j == 1 ? sz : j == 2 ? -sy : j == 3 ? 1.0 : 0.0;
  c[1] = j == 0 ? -sz : j == 2 ? sx : j == 4 ? 1.0 : 0.0;
  c[2] = j == 0 ? sy : j == 1 ? -sx : j == 5 ? 1.0 : 0.0;
}

__global__ void __launch_bounds__(256)
k_ndt_wave(const NdtJob *__restrict__ jobs)
{
  const NdtJob &job = jobs[blockIdx.y];
  if ((int)blockIdx.x >= job.nn.nblocks) return;         // the grid is as wide as the batch's largest job
  const IcpState *__restrict__ st = job.nn.st;
  double *__restrict__ partials = job.nn.partials;
  __shared__ float Ts[16];
  __shared__ double red[4][kNdtAcc];
  if (st->done) return;
  if (threadIdx.x < 16) Ts[threadIdx.x] = st->T[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int item = (int)blockIdx.x * 4 + wave;           // one work item (<= 64 points of one coarse block) per wave
  const int2 it = item < job.nn.n_items ? job.nn.items[item] : make_int2(0, 0);
  // per lane: sum w P (xx xy xz yy yz zz), sum w P q, sum w, the terms -- every voxel of one point shares its J
  double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, bq[3] = {0.0, 0.0, 0.0}, wsum = 0.0;
  int terms = 0;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  if (lane < it.y) {
    const float4 sp = job.nn.src[it.x + lane];
    const float3 p = xform(Ts, sp.x, sp.y, sp.z);
    sx = p.x; sy = p.y; sz = p.z;
    // the point's voxel relative to the table's minimum, as floats: integer-valued, or inf / NaN, which fail every test below
    const float rx = lattice_index(p.x, job.inv) - job.mn[0], ry = lattice_index(p.y, job.inv) - job.mn[1], rz = lattice_index(p.z, job.inv) - job.mn[2];
    const float dx = (float)job.dims[0], dy = (float)job.dims[1], dz = (float)job.dims[2];
#pragma unroll
    for (int nb = 0; nb < 7; ++nb) {
      if (nb >= job.neighbours) break;
      // itself, then -x +x -y +y -z +z
      const float ox = nb == 1 ? -1.0f : nb == 2 ? 1.0f : 0.0f, oy = nb == 3 ? -1.0f : nb == 4 ? 1.0f : 0.0f, oz = nb == 5 ? -1.0f : nb == 6 ? 1.0f : 0.0f;
      const float cx = rx + ox, cy = ry + oy, cz = rz + oz;
      if (!(cx >= 0.0f && cx < dx && cy >= 0.0f && cy < dy && cz >= 0.0f && cz < dz)) continue;
      const int v = job.index[((size_t)(int)cx * job.dims[1] + (int)cy) * job.dims[2] + (int)cz];
      if (v < 0) continue;
      const float4 r0 = job.rec[(size_t)v * 3];
      if (r0.w == 0.0f) continue;                        // no Gaussian: too few points, or a degenerate one
      const float4 r1 = job.rec[(size_t)v * 3 + 1], r2 = job.rec[(size_t)v * 3 + 2];
      const double qx = sx - (double)r0.x, qy = sy - (double)r0.y, qz = sz - (double)r0.z;
      const double pxx = r1.x, pxy = r1.y, pxz = r1.z, pyy = r1.w, pyz = r2.x, pzz = r2.y;
      const double ux = pxx * qx + pxy * qy + pxz * qz, uy = pxy * qx + pyy * qy + pyz * qz, uz = pxz * qx + pyz * qy + pzz * qz;
      const double m = qx * ux + qy * uy + qz * uz;
      if (!isfinite(m)) continue;
      const double w = exp(-0.5 * m);
      A[0] += w * pxx; A[1] += w * pxy; A[2] += w * pxz; A[3] += w * pyy; A[4] += w * pyz; A[5] += w * pzz;
      bq[0] += w * ux; bq[1] += w * uy; bq[2] += w * uz;
      wsum += w;
      ++terms;
    }
  }
  // one sum at a time (icp_store_partials): H_ij = J_i . (A J_j), g_i = -J_i . bq
  auto term = [&](int k) -> double {
    if (k < 21) {
      double ci[3], cj[3];
      ndt_jcol(kUi[k], sx, sy, sz, ci);
      ndt_jcol(kUj[k], sx, sy, sz, cj);
      const double ax = A[0] * cj[0] + A[1] * cj[1] + A[2] * cj[2], ay = A[1] * cj[0] + A[3] * cj[1] + A[4] * cj[2],
                   az = A[2] * cj[0] + A[4] * cj[1] + A[5] * cj[2];
      return ci[0] * ax + ci[1] * ay + ci[2] * az;
    }
    if (k < 27) {
      double ci[3];
      ndt_jcol(k - 21, sx, sy, sz, ci);
      return -(ci[0] * bq[0] + ci[1] * bq[1] + ci[2] * bq[2]);
    }
    if (k == 27) return wsum;
    if (k == 28) return (double)terms;
    return terms > 0 ? 1.0 : 0.0;
  };
  // a wave none of whose points has a term adds zeros without the reductions (as k_nn_wave does)
  const bool any_term = ballot(terms > 0) != 0ull;       // wave-uniform
  icp_store_partials<kNdtAcc, 1>(term, any_term, red, partials, blockIdx.x);
}

__global__ void __launch_bounds__(256) k_ndt_finalize(const NdtJob *__restrict__ jobs)
{
  __shared__ double red[4][kNdtAcc];
  __shared__ double tot[kNdtAcc];
  const NdtJob &job = jobs[blockIdx.x];
  IcpState *st = job.nn.st;
  if (st->done) return;
  icp_totals<kNdtAcc>(job.nn.partials, job.nn.nblocks, 0, job.nn.n_items, red, tot);
  if (threadIdx.x != 0) return;

  st->n_corr = (int)tot[29];
  float Ti[16];
  // degenerate (fewer than six terms, or a pivot at or below the threshold): stop, not converged, T unchanged
  if (tot[28] < 6.0 || !icp_solve6_transform(tot, Ti)) return icp_stop_unconverged(st);
  // DefaultConvergenceCriteria::hasConverged, the mean weight F in the place of the mean d2
  icp_advance(st, Ti, true, tot[27] / (double)job.n_src);
}

// everything but the resolution's "0 = default", which only mm3d_set_refinement admits
bool ndt_options_ok(const mm3d_refine_options *o)
{
  if (!o || (o->method != MM3D_REFINE_ICP && o->method != MM3D_REFINE_NDT)) return false;
  if (o->neighbours != 1 && o->neighbours != 7) return false;
  if (o->min_points < 4) return false;
  return o->regularisation > 0.0 && o->regularisation <= 1.0;      // (false for NaN)
}

// The table of `tgt` at the given voxel side: complete on c's stream on return (the caller waits before anybody else reads it)
std::unique_ptr<NdtTable> ndt_build_table(Context *c, const mm3d_cloud *tgt, double resolution, int min_points, double kappa)
{
  MM3D_REQUIRE(lattice_side_ok(resolution), "NDT: the resolution must be positive and finite, as a float and its reciprocal too");
  MM3D_REQUIRE(tgt->n < ((size_t)1 << 31), "NDT: more than 2^31 - 1 target points");
  std::unique_ptr<NdtTable> t(new NdtTable());
  t->resolution = resolution; t->min_points = min_points; t->regularisation = kappa;
  t->inv = 1.0f / (float)resolution;
  const int n = (int)tgt->n;
  if (n == 0) return t;
  const unsigned blocks = div_up((size_t)n, 256);
  DevBuf<unsigned> range(c, 8);                           // min i j k, max i j k | voxels, finite points
  lattice_range<3>(c, "ndt_range", n * 16.0, tgt->pts.get(), n, t->inv, LatticeFinite{}, range.get());
  DevBuf<uint32_t> keys(c, n), vals(c, n), keys2(c, n), vals2(c, n);
  MM3D_LAUNCH(c, "ndt_keys", n * 24.0, k_ndt_keys, dim3(blocks), dim3(256), 0, tgt->pts.get(), n, t->inv, (const unsigned *)range.get(),
              keys.get(), vals.get());
  sort_pairs_u32(c, keys.get(), keys2.get(), vals.get(), vals2.get(), (size_t)n, 32);
  DevBuf<int> starts(c, n);                               // (at most one voxel per point)
  scan_fused(c, "ndt_runs", n * 8.0, (size_t)n, LatticeRunHead{keys2.get()}, NdtStartStore{keys2.get(), (size_t)n, starts.get(), range.get() + 6});
  unsigned *hr = (unsigned *)c->pin(64);
  MM3D_HIP(hipMemcpyAsync(hr, range.get(), 32, hipMemcpyDeviceToHost, c->stream));
  c->sync();                                              // the one wait: what sizes the table
  const int n_voxels = (int)hr[6], n_finite = (int)hr[7];
  if (n_voxels == 0) return t;                            // no finite point
  const LatticeFrame<3> f = lattice_frame<3>(hr);
  if (!ndt_fits(f))
    throw Error(MM3D_EUNSUPPORTED, "NDT: the target's voxel bounding box needs more than 2^26 index cells at this resolution");
  for (int a = 0; a < 3; ++a) { t->mn[a] = (float)f.mn[a]; t->dims[a] = (int)f.d[a]; }
  t->n_voxels = n_voxels;
  const size_t cells = (size_t)t->dims[0] * t->dims[1] * t->dims[2];
  t->rec = DevBuf<float4>(c, (size_t)n_voxels * 3);
  t->index = DevBuf<int>(c, cells);
  MM3D_HIP(hipMemsetAsync(t->index.get(), 0xFF, cells * sizeof(int), c->stream));
  MM3D_LAUNCH(c, "ndt_voxels", n_finite * 40.0 + n_voxels * 52.0, k_ndt_voxels, dim3(div_up((size_t)n_voxels, 4)), dim3(256), 0, tgt->pts.get(),
              (const uint32_t *)keys2.get(), (const uint32_t *)vals2.get(), (const int *)starts.get(), n_voxels, n_finite, min_points, kappa,
              t->rec.get(), t->index.get());
  c->settle();                                            // (the sort's buffers go back to the pool)
  return t;
}

// the lookup + reduction launch, then the solve / accumulate / convergence launch, on the IcpState protocol of the ICP's.  No
// grid of the target is read and max_corr_dist is not read.
struct NdtStep final : IcpStep {
  StepJobs<NdtJob> jobs;
  NdtStep() { acc = kNdtAcc; searches = false; }
  double bytes_per_point(const IcpScoreJob &J) const override { return 16.0 + 52.0 * J.ndt_neighbours; }      // (the point, and an index word and a record per voxel)
  void check(const IcpScoreJob &J) const override
  {
    if (!J.tgt_ndt) throw Error(MM3D_EINVAL, "NDT: the target has no voxel table");
  }
  size_t pinned_bytes(int B) const override { return jobs.bytes(B); }
  void begin(Context *c, const IcpScoreJob *const *, int B, char *pinned, void *, void *) override { jobs.begin(c, B, pinned); }
  void bind(int b, const NnJob &q, const IcpScoreJob &J) override
  {
    NdtJob nj;
    std::memset(&nj, 0, sizeof(nj));
    nj.nn = q;
    if (const NdtTable *t = J.tgt_ndt) {
      nj.rec = (const float4 *)t->rec.get();
      nj.index = (const int *)t->index.get();
      nj.inv = t->inv;
      for (int a = 0; a < 3; ++a) { nj.mn[a] = t->mn[a]; nj.dims[a] = t->dims[a]; }
    }
    nj.neighbours = J.ndt_neighbours;
    nj.n_src = (int)J.src->n_finite;
    jobs.host[b] = nj;
  }
  void upload(Context *c) override { jobs.upload(c); }
  void iterate(Context *c, const IcpLaunch &L) override
  {
    MM3D_LAUNCH(c, "ndt_wave", L.bytes, k_ndt_wave, dim3(L.grid_x, L.count), dim3(256), 0, (const NdtJob *)jobs.dev.get());
    MM3D_LAUNCH(c, "ndt_finalize", L.finalize_bytes, k_ndt_finalize, dim3(L.count), dim3(256), 0, (const NdtJob *)jobs.dev.get());
  }
};

struct RefineNdt final : IcpMethodBase {
  int method() const override { return MM3D_REFINE_NDT; }
  std::unique_ptr<IcpStep> step(const mm3d_icp_rejection_options *) const override { return std::unique_ptr<IcpStep>(new NdtStep()); }
  // the map's table at the context's options (map_kept.hpp)
  void prepare_target(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p, IcpScoreJob *job) const override
  {
    const mm3d_refine_options &o = ctx->sel.refine_options;
    const double res = o.resolution > 0.0 ? o.resolution : kNdtDefaultMultiple * p->resolution;
    const NdtTable *t = map_kept(
        ctx, m, &mm3d_map::ndt,
        [&](const NdtTable &h) { return h.resolution == res && h.min_points == o.min_points && h.regularisation == o.regularisation; },
        [&] { return ndt_build_table(ctx, m->points, res, o.min_points, o.regularisation); });
    if (job) { job->tgt_ndt = t; job->ndt_neighbours = o.neighbours; }
  }
};
const RefineNdt g_ndt;

}  // namespace

}  // namespace mm3d

using namespace mm3d;

extern "C" {

int mm3d_set_refinement(mm3d_ctx *ctx, const mm3d_refine_options *options)
{
  if (!ctx || !ndt_options_ok(options)) return MM3D_EINVAL;
  if (options->resolution != 0.0 && !lattice_side_ok(options->resolution)) return MM3D_EINVAL;     // (also catches NaN)
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the method changes)
  return select_stage(ctx, Stage::Refinement, [&](StageSelection &s) {
    s.refine_options = *options;
    s.refine = stage_active(Stage::Refinement, s) ? &g_ndt : nullptr;
  });
}

int mm3d_get_refinement(const mm3d_ctx *ctx, mm3d_refine_options *options)
{
  if (!ctx || !options) return MM3D_EINVAL;
  *options = ctx->sel.refine_options;
  return MM3D_OK;
}

int mm3d_estimate_transform_ndt(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target, const float initial_guess[16],
                                const mm3d_refine_options *options, int max_iterations, double eps, float T[16])
{
  if (!ctx || !source || !target || !initial_guess || !T || !ndt_options_ok(options)) return MM3D_EINVAL;
  if (!lattice_side_ok(options->resolution)) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    std::unique_ptr<NdtTable> t = ndt_build_table(ctx, target, options->resolution, options->min_points, options->regularisation);
    IcpScoreJob J;
    J.src = source; J.tgt = target; J.tgt_ndt = t.get(); J.ndt_neighbours = options->neighbours;
    std::memcpy(J.guess_host, initial_guess, sizeof(J.guess_host));
    icp_score_batch(ctx, &g_ndt, &J, 1, true, 0.0, max_iterations, eps, false, 0.0);
    std::memcpy(T, J.out.T, sizeof(J.out.T));
  });
}

int mm3d_debug_ndt_voxels(mm3d_ctx *ctx, const mm3d_cloud *target, const mm3d_refine_options *options, int *ijk, int *count, float *mean,
                          float *icov, unsigned char *valid, size_t cap, size_t *n_voxels)
{
  if (!ctx || !target || !n_voxels || !ndt_options_ok(options) || !lattice_side_ok(options->resolution)) return MM3D_EINVAL;
  if (cap && (!ijk || !count || !mean || !icov || !valid)) return MM3D_EINVAL;
  *n_voxels = 0;
  return guarded(ctx, [&] {
    std::unique_ptr<NdtTable> t = ndt_build_table(ctx, target, options->resolution, options->min_points, options->regularisation);
    const size_t nv = (size_t)t->n_voxels, cells = t->index.size();
    std::vector<float4> rec(nv * 3);
    std::vector<int> index(cells);
    if (nv) {
      MM3D_HIP(hipMemcpyAsync(rec.data(), t->rec.get(), nv * 48, hipMemcpyDeviceToHost, ctx->stream));
      MM3D_HIP(hipMemcpyAsync(index.data(), t->index.get(), cells * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    }
    ctx->sync();
    *n_voxels = nv;
    // the records are in ascending cell order, which is ascending (i, j, k)
    for (size_t cell = 0; cell < cells; ++cell) {
      const int v = index[cell];
      if (v < 0 || (size_t)v >= cap) continue;
      const int ck = (int)(cell % (size_t)t->dims[2]), cj = (int)(cell / (size_t)t->dims[2] % (size_t)t->dims[1]),
                ci = (int)(cell / ((size_t)t->dims[2] * t->dims[1]));
      ijk[3 * v] = (int)t->mn[0] + ci; ijk[3 * v + 1] = (int)t->mn[1] + cj; ijk[3 * v + 2] = (int)t->mn[2] + ck;
      const float4 r0 = rec[3 * (size_t)v], r1 = rec[3 * (size_t)v + 1], r2 = rec[3 * (size_t)v + 2];
      std::memcpy(&count[v], &r2.z, sizeof(int));
      mean[3 * v] = r0.x; mean[3 * v + 1] = r0.y; mean[3 * v + 2] = r0.z;
      const float P[6] = {r1.x, r1.y, r1.z, r1.w, r2.x, r2.y};
      std::memcpy(&icov[6 * (size_t)v], P, sizeof(P));
      valid[v] = r0.w != 0.0f ? 1 : 0;
    }
  });
}

}  // extern "C"

// icp_color.hip -- coloured ICP, opt-in (mm3d_set_icp_color): a photometric term beside point-to-plane's (Park, Zhou, Koltun,
// "Colored Point Cloud Registration Revisited", ICCV 2017).  include/mm3d.h states the rule.
//
// Point-to-plane ICP leaves every direction open that the target's planes leave open (a corridor's axis, a floor's two); what
// such surfaces do have is texture.  A colour gradient on the target's tangent plane, one per target point, turns the intensity
// mismatch of a correspondence into a second residual, and a correspondence adds TWO rows to the same 6x6 system.  So the 30
// partial sums of k_icp_plane_wave stay the layout, and k_icp_plane_finalize runs unchanged behind this file's search kernel.
//   k_color_intensity   every point's record (0, 0, 0, I): what a point keeps that no work item covers (a non-finite one)
//   k_color_gradient    once per map and option set.  A wave takes one Hilbert work item (<= 64 points of one patch), one lane
//                       per point.  The rows of cells of the patch's box grown by the radius are streamed through LDS, 64
//                       candidates at a time (their intensities gathered while they are staged), and every lane adds the
//                       candidates within its radius into its OWN 6 + 3 double sums, in staging order: no cross-lane sum, so
//                       the order is a function of the cloud and the radius alone, and no neighbourhood is too large.
//                       Then the 3x3 LDLt on the lane, and the float4 (gx, gy, gz, I) at the point's original index.
//   k_icp_color_wave    k_icp_plane_wave with the record and the source's own colour: nn_search_body.hpp once more, then three
//                       16-byte loads per matched lane, and the 30 terms formed, wave-summed and stored one at a time into
//                       partials[block][kPlaneAcc].  lambda == 1 is decided per launch (a kernel argument: wave-uniform), and
//                       its terms are then the ones k_icp_plane_wave forms (icp_tail.hpp's row and terms): the same bits.
#include <atomic>
#include <cmath>

#include "capi_guard.hpp"
#include "drivers.hpp"
#include "map_kept.hpp"
#include "icp_tail.hpp"
#include "nn_core.hpp"

namespace mm3d {

// the point-to-plane job plus the target's gradient records and the source's reference points (their rgba).
// pl.nn.partials: [nblocks][kPlaneAcc], read by k_icp_plane_finalize over the NnPlaneJobs.
struct NnColorJob {
  NnPlaneJob pl;
  const float4 *rec;          // the target's records (gx, gy, gz, I), in tgt_ref's order
  const float4 *src_ref;      // the source's points in reference order (nn.src's .w indexes them)
};

// I = (299 r + 587 g + 114 b) / 255000 in [0, 1]: SIFT's integer numerator (sift.hip's intensity_of), divided in double
__device__ __forceinline__ float color_intensity(float w)
{
  const unsigned c = __float_as_uint(w);
  const int r = (int)((c >> 16) & 255u), g = (int)((c >> 8) & 255u), b = (int)(c & 255u);
  return (float)((double)(299 * r + 587 * g + 114 * b) / 255000.0);
}

__global__ void __launch_bounds__(256) k_color_intensity(const float4 *__restrict__ pts, int n, float4 *__restrict__ rec)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) rec[i] = make_float4(0.0f, 0.0f, 0.0f, color_intensity(pts[i].w));
}

// a 3 x 3 symmetric system by the unpivoted LDLt of icp_solve6.hpp, its pivot rule against `floor` (the correlative plane
// fit's solve, align_correlative.hip)
__device__ static bool color_solve3_ldlt(const double A[9], const double b[3], double floor, double x[3])
{
  double L[9], D[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double d = A[j * 3 + j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j * 3 + k] * L[j * 3 + k] * D[k];
    if (!(d > floor)) return false;
    D[j] = d;
#pragma unroll
    for (int i = j + 1; i < 3; ++i) {
      double s = A[i * 3 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i * 3 + k] * L[j * 3 + k] * D[k];
      L[i * 3 + j] = s / d;
    }
  }
  double y[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i * 3 + k] * y[k];
    y[i] = s;
  }
#pragma unroll
  for (int i = 2; i >= 0; --i) {
    double s = y[i] / D[i];
#pragma unroll
    for (int k = i + 1; k < 3; ++k) s -= L[k * 3 + i] * x[k];
    x[i] = s;
  }
  return true;
}

__global__ void __launch_bounds__(256)
k_color_gradient(const float4 *__restrict__ hil, const int2 *__restrict__ items, int n_items, GridView g, const float4 *__restrict__ ref,
                 const float4 *__restrict__ nrm, float radius, float thr, int min_nb, float4 *__restrict__ rec)
{
  __shared__ float4 s_p[4][kWave];         // a staged candidate: x, y, z, intensity
  __shared__ int s_w[4][kWave];            // its original index
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int item = (int)xcd_remap(blockIdx.x, gridDim.x) * 4 + wave;
  if (item >= n_items) return;             // (wave-uniform; the waves of a block never meet at a barrier)
  const int2 it = items[item];
  const bool valid = lane < it.y;
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 n = make_float4(0.f, 0.f, 0.f, 0.f);
  int orig = -1;
  float qi = 0.0f;
  if (valid) {
    q = hil[it.x + lane];
    orig = __float_as_int(q.w);
    qi = color_intensity(ref[orig].w);
    n = nrm[orig];
  }
  // the cells the patch's box grown by the radius reaches (for_each_candidate's conservative range), clamped to the grid
  const float ri = radius * 1.0001f + 1e-4f;
  const float lx = wave_min_f(valid ? q.x : INFINITY), hx = wave_max_f(valid ? q.x : -INFINITY);
  const float ly = wave_min_f(valid ? q.y : INFINITY), hy = wave_max_f(valid ? q.y : -INFINITY);
  const float lz = wave_min_f(valid ? q.z : INFINITY), hz = wave_max_f(valid ? q.z : -INFINITY);
  const int x0 = clampi(cell_floor(lx - ri, g.minx, g.inv), 0, g.dx - 1), x1 = clampi(cell_floor(hx + ri, g.minx, g.inv), 0, g.dx - 1);
  const int y0 = clampi(cell_floor(ly - ri, g.miny, g.inv), 0, g.dy - 1), y1 = clampi(cell_floor(hy + ri, g.miny, g.inv), 0, g.dy - 1);
  const int z0 = clampi(cell_floor(lz - ri, g.minz, g.inv), 0, g.dz - 1), z1 = clampi(cell_floor(hz + ri, g.minz, g.inv), 0, g.dz - 1);
  const bool want = valid && isfinite(n.x) && isfinite(n.y) && isfinite(n.z);
  const double nx = n.x, ny = n.y, nz = n.z;
  double m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
  int count = 0;
  for (int z = z0; z <= z1; ++z)
    for (int y = y0; y <= y1; ++y) {
      const int row = (z * g.dy + y) * g.dx;
      const int beg = g.cell_start[row + x0], end = g.cell_start[row + x1 + 1];     // (wave-uniform)
      for (int t = beg; t < end; t += kWave) {
        const int cnt = min(kWave, end - t);
        if (lane < cnt) {
          const float4 c = g.pts[t + lane];
          const int ci = __float_as_int(c.w);
          s_p[wave][lane] = make_float4(c.x, c.y, c.z, color_intensity(ref[ci].w));
          s_w[wave][lane] = ci;
        }
        wave_lds_sync();
        if (want) {
          for (int k = 0; k < cnt; ++k) {
            const float4 c = s_p[wave][k];                    // (one address for the wave: a broadcast)
            const float d2 = dist2(c.x, c.y, c.z, q.x, q.y, q.z);
            if (d2 <= thr && s_w[wave][k] != orig) {
              const double ex = (double)c.x - (double)q.x, ey = (double)c.y - (double)q.y, ez = (double)c.z - (double)q.z;
              const double en = (ex * nx + ey * ny) + ez * nz;
              const double ux = ex - en * nx, uy = ey - en * ny, uz = ez - en * nz;
              const double w = (double)c.w - (double)qi;
              m00 += ux * ux; m01 += ux * uy; m02 += ux * uz; m11 += uy * uy; m12 += uy * uz; m22 += uz * uz;
              b0 += ux * w; b1 += uy * w; b2 += uz * w;
              ++count;
            }
          }
        }
        wave_lds_sync();                   // the chunk's readers are done before the next one is stored
      }
    }
  if (!valid) return;
  float gx = 0.0f, gy = 0.0f, gz = 0.0f;
  if (want && count >= min_nb) {
    // the soft constraint g.n = 0, weighted by the square of the neighbour count
    const double k2 = (double)count * (double)count;
    const double A[9] = {m00 + k2 * nx * nx, m01 + k2 * nx * ny, m02 + k2 * nx * nz,
                         m01 + k2 * nx * ny, m11 + k2 * ny * ny, m12 + k2 * ny * nz,
                         m02 + k2 * nx * nz, m12 + k2 * ny * nz, m22 + k2 * nz * nz};
    const double rhs[3] = {b0, b1, b2};
    double x[3];
    if (color_solve3_ldlt(A, rhs, kPlanePivotTau * (A[0] + A[4] + A[8]) / 3.0, x)) {
      gx = (float)x[0]; gy = (float)x[1]; gz = (float)x[2];
    }
  }
  rec[orig] = make_float4(gx, gy, gz, qi);
}

template <int SPLIT>
__global__ void __launch_bounds__(256) MM3D_NN_ATTR
k_icp_color_wave(const NnColorJob *__restrict__ cjobs, float max_d2, float rmax, double lam, double mu)
{
  constexpr int MODE = 0;                                // (nn_search_body.hpp: the keyed search, with the winner's index)
  const NnJob &job = cjobs[blockIdx.y].pl.nn;
  if ((int)blockIdx.x >= job.nblocks) return;            // the grid is as wide as the batch's largest job
  const float4 *__restrict__ src = job.src;
  const int2 *__restrict__ items = job.items;
  const int n_items = job.n_items;
  const GridView g = job.g;
  const float4 *__restrict__ tgt_ref = job.tgt_ref;
  const float4 *__restrict__ nrm = cjobs[blockIdx.y].pl.nrm;
  const float4 *__restrict__ grad = cjobs[blockIdx.y].rec;
  const float4 *__restrict__ src_ref = cjobs[blockIdx.y].src_ref;
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
  const bool colored = lam < 1.0;              // (a kernel argument: the same in every lane of every wave)
  // the lane's two rows (zero where it has none, or where the target normal is not finite: such a correspondence still counts,
  // and its d2 goes into the MSE of the convergence test); a zero gradient leaves a zero colour row
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, vc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double r = 0.0, rc = 0.0, has_row = 0.0;
  if (corr) {
    const unsigned w = (unsigned)(bkey & 0xffffffffull);
    const float4 n = nrm[w];
    if (icp_plane_row(p, n, tgt_ref[w], v, r)) {
      has_row = 1.0;
      if (colored) {
        const float4 d = tgt_ref[w];
        const double sx = p.x, sy = p.y, sz = p.z, nx = n.x, ny = n.y, nz = n.z;
        const float4 G = grad[w];
        const double is = color_intensity(src_ref[__float_as_uint(src[i].w)].w);
        const double gx = G.x, gy = G.y, gz = G.z;
        const double ex = sx - (double)d.x, ey = sy - (double)d.y, ez = sz - (double)d.z;
        const double h = (ex * nx + ey * ny) + ez * nz, gn = (gx * nx + gy * ny) + gz * nz;
        const double mx = gx - gn * nx, my = gy - gn * ny, mz = gz - gn * nz;
        const double pred = (double)G.w + ((gx * (ex - h * nx) + gy * (ey - h * ny)) + gz * (ez - h * nz));
        rc = is - pred;
        vc[0] = mz * sy - my * sz;
        vc[1] = mx * sz - mz * sx;
        vc[2] = my * sx - mx * sy;
        vc[3] = mx; vc[4] = my; vc[5] = mz;
      }
    }
  }
  // point-to-plane's terms (icp_plane_term), the 27 of the system weighted with the colour rows' when there are any
  auto term = [&](int k) -> double {
    const double geo = icp_plane_term(k, v, r, corr, best, has_row);
    return colored && k < 27 ? lam * geo + mu * icp_plane_term(k, vc, rc, corr, best, has_row) : geo;
  };
  // a wave none of whose points found a neighbour in range adds zeros without the reductions (as k_nn_wave does)
  const bool any_corr = ballot(corr) != 0ull;       // wave-uniform
  icp_store_partials<kPlaneAcc, SPLIT>(term, any_corr, red, partials, bid);
}

static std::atomic<int> g_color_forced_split{0};      // mm3d_debug_icp_color_split: 0 (by size), 1 or 4

namespace {
// point-to-plane's jobs, partials and finalize kernel behind this file's search + reduction launch
struct ColorStep final : IcpStep {
  StepJobs<NnPlaneJob> plane;
  StepJobs<NnColorJob> jobs;
  double lambda = 1.0;       // the weight of the geometric rows (the photometric ones get 1 - lambda; 1: point-to-plane's terms, bit for bit)
  ColorStep() { acc = kPlaneAcc; forced_split = g_color_forced_split.load(); }
  double bytes_per_point(const IcpScoreJob &) const override { return 60.0; }      // (+ the winner's normal and record, the source's reference point)
  void check(const IcpScoreJob &J) const override
  {
    icp_plane_check(J);
    if (!J.tgt_color) throw Error(MM3D_EINVAL, "coloured ICP: the target has no gradient records");
  }
  size_t pinned_bytes(int B) const override { return plane.bytes(B) + jobs.bytes(B); }
  void begin(Context *c, const IcpScoreJob *const *live, int B, char *pinned, void *, void *) override
  {
    jobs.begin(c, B, plane.begin(c, B, pinned));
    lambda = live[0]->color_lambda;      // (the same for every job of a batch)
  }
  void bind(int b, const NnJob &q, const IcpScoreJob &J) override
  {
    plane.host[b] = icp_plane_job(q, J);
    jobs.host[b] = NnColorJob{plane.host[b], J.tgt_color, (const float4 *)J.src->pts.get()};
  }
  void upload(Context *c) override { plane.upload(c); jobs.upload(c); }
  void iterate(Context *c, const IcpLaunch &L) override
  {
    const double mu = 1.0 - lambda;
    if (L.split)
      MM3D_LAUNCH(c, "icp_color_corr_reduce", L.bytes, k_icp_color_wave<4>, dim3(L.grid_x, L.count), dim3(256), 0, (const NnColorJob *)jobs.dev.get(),
                  L.max_d2, L.rmax, lambda, mu);
    else
      MM3D_LAUNCH(c, "icp_color_corr_reduce", L.bytes, k_icp_color_wave<1>, dim3(L.grid_x, L.count), dim3(256), 0, (const NnColorJob *)jobs.dev.get(),
                  L.max_d2, L.rmax, lambda, mu);
    icp_plane_finalize(c, plane.dev.get(), L.count, L.finalize_bytes);
  }
};
}  // namespace

static bool icp_color_options_valid(const mm3d_icp_color_options *o)
{
  if (o->enabled != 0 && o->enabled != 1) return false;
  if (!(o->lambda_geometric > 0.0 && o->lambda_geometric <= 1.0)) return false;
  if (!(o->gradient_radius >= 0.0) || !std::isfinite(o->gradient_radius)) return false;
  return o->min_neighbours >= 4;
}

// the records of `points` with `normals` (in the points' order): 16 B per point, complete on c's stream (no wait)
static std::unique_ptr<ColorGradients> color_gradients(Context *c, const mm3d_cloud *points, const mm3d_normals *normals, double radius,
                                                       int min_neighbours)
{
  if (normals->n != points->n) throw Error(MM3D_EINVAL, "coloured ICP: the normals do not match the points");
  auto out = std::make_unique<ColorGradients>();
  out->radius = radius;
  out->min_neighbours = min_neighbours;
  out->n = points->n;
  out->rec = DevBuf<float4>(c, points->n ? points->n : 1);
  if (points->n == 0) return out;
  MM3D_LAUNCH(c, "color_intensity", points->n * 32.0, k_color_intensity, dim3(div_up(points->n, 256)), dim3(256), 0, points->pts.get(),
              (int)points->n, out->rec.get());
  cloud_hilbert(c, points);
  if (points->n_finite == 0 || points->n_wave_items == 0) return out;
  const Grid &g = cloud_grid(c, points, (float)(radius * 0.5));
  if (g.n == 0) return out;
  // largest float whose double value does not exceed r * r, as the outlier filter's radius test
  const double r2 = radius * radius;
  float thr = (float)r2;
  if ((double)thr > r2) thr = std::nextafterf(thr, -INFINITY);
  MM3D_LAUNCH(c, "color_gradient", points->n_finite * 64.0, k_color_gradient, dim3(div_up(points->n_wave_items, 4)), dim3(256), 0,
              (const float4 *)points->hil_pts.get(), (const int2 *)points->wave_items.get(), points->n_wave_items, g.view(),
              (const float4 *)points->pts.get(), (const float4 *)normals->nrm.get(), (float)radius, thr, min_neighbours, out->rec.get());
  return out;
}

static double color_radius(const mm3d_icp_color_options &o, const mm3d_params *p) { return o.gradient_radius > 0.0 ? o.gradient_radius : p->normal_radius; }

// the map's records at the context's options (and the normals they are made from), made when missing or stale
static const ColorGradients *map_color(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p)
{
  const mm3d_icp_color_options &o = ctx->sel.color_options;
  const double radius = color_radius(o, p);
  if (!(radius > 0.0) || !std::isfinite(radius)) throw Error(MM3D_EINVAL, "coloured ICP: the gradient radius must be positive");
  return map_kept(ctx, m, &mm3d_map::color,
                  [&](const ColorGradients &have) { return have.radius == radius && have.min_neighbours == o.min_neighbours && have.n == m->points->n; },
                  [&] { return color_gradients(ctx, m->points, map_normals(ctx, m, p), radius, o.min_neighbours); });
}

namespace {
struct IcpColoured final : IcpMethodBase {
  int method() const override { return MM3D_ICP_POINT_TO_PLANE; }     // (not read: mm3d_get_icp_method answers StageSelection::icp's)
  std::unique_ptr<IcpStep> step(const mm3d_icp_rejection_options *) const override { return std::unique_ptr<IcpStep>(new ColorStep()); }
  void prepare_target(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p, IcpScoreJob *job) const override
  {
    const mm3d_normals *n = map_normals(ctx, m, p);
    const ColorGradients *g = map_color(ctx, m, p);
    if (job) {
      job->tgt_normals = n;
      job->tgt_color = g->rec.get();
      job->color_lambda = ctx->sel.color_options.lambda_geometric;
    }
  }
};
const IcpColoured g_coloured;
}  // namespace

}  // namespace mm3d

using namespace mm3d;

extern "C" {

int mm3d_set_icp_color(mm3d_ctx *ctx, const mm3d_icp_color_options *options)
{
  if (!ctx || !options || !icp_color_options_valid(options)) return MM3D_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the selection changes)
  return select_stage(ctx, Stage::Color, [&](StageSelection &s) {
    s.color_options = *options;
    s.color = stage_active(Stage::Color, s) ? &g_coloured : nullptr;
  });
}

int mm3d_get_icp_color(const mm3d_ctx *ctx, mm3d_icp_color_options *options)
{
  if (!ctx || !options) return MM3D_EINVAL;
  *options = ctx->sel.color_options;
  return MM3D_OK;
}

int mm3d_estimate_transform_icp_color(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target, const mm3d_normals *target_normals,
                                      const float initial_guess[16], double max_corr_dist, const mm3d_icp_color_options *options,
                                      int max_iterations, double eps, float T[16])
{
  if (!source || !target || !target_normals || !initial_guess || !options || !T || !icp_color_options_valid(options)) return MM3D_EINVAL;
  if (!(options->gradient_radius > 0.0)) {
    if (ctx) ctx->err = "mm3d_estimate_transform_icp_color: gradient_radius must be positive here (there are no parameters to take it from)";
    return MM3D_EINVAL;
  }
  if (target_normals->n != target->n) {
    if (ctx) ctx->err = "mm3d_estimate_transform_icp_color: the normals do not match the target's points";
    return MM3D_EINVAL;
  }
  return guarded(ctx, [&] {
    const std::unique_ptr<ColorGradients> grad = color_gradients(ctx, target, target_normals, options->gradient_radius, options->min_neighbours);
    IcpScoreJob J;
    J.src = source; J.tgt = target; J.tgt_normals = target_normals;
    J.tgt_color = grad->rec.get();
    J.color_lambda = options->lambda_geometric;
    std::memcpy(J.guess_host, initial_guess, sizeof(J.guess_host));
    icp_score_batch(ctx, &g_coloured, &J, 1, true, max_corr_dist, max_iterations, eps, false, 0.0);
    std::memcpy(T, J.out.T, sizeof(J.out.T));
  });
}

int mm3d_debug_color_gradients(mm3d_ctx *ctx, const mm3d_cloud *points, const mm3d_normals *normals, const mm3d_icp_color_options *options,
                               float *out)
{
  if (!points || !normals || !options || !icp_color_options_valid(options) || !(options->gradient_radius > 0.0)) return MM3D_EINVAL;
  if (normals->n != points->n || (points->n && !out)) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    const std::unique_ptr<ColorGradients> grad = color_gradients(ctx, points, normals, options->gradient_radius, options->min_neighbours);
    if (points->n) MM3D_HIP(hipMemcpyAsync(out, grad->rec.get(), points->n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
  });
}

int mm3d_debug_icp_color_split(int split)
{
  if (split == 0 || split == 1 || split == 4) g_color_forced_split.store(split);
  return g_color_forced_split.load();
}

}  // extern "C"

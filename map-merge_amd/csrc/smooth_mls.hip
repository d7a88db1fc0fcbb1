// smooth_mls.hip -- moving-least-squares smoothing on gfx950: every point is moved onto the Gaussian-weighted plane, or the
// quadratic over that plane, fitted to its neighbours within a radius (mm3d_smooth_displacements, mm3d_smooth_cloud,
// mm3d_set_smoothing; include/mm3d.h states the rule to the operation).  Not a reference stage.
//
// One pass family per cloud, one host wait (the counts'):
//   cloud_grid    the library's cell-sorted grid at a cell just above the radius (radius_grid.hpp: radius_cell), so that a point's neighbours lie in
//                 its 3 x 3 x 3 cells; where the cell had to grow, in as many cells as cover the radius (radius_reach)
//   k_mls_fit     a wave per cell-sorted query.  The lanes stride the candidates of the box's rows of cells, each row one span
//                 of the cell-sorted points, 64 at a time, and test them against the radius; the neighbours among them -- a
//                 third of a box's candidates on a surface -- go through the wave's ring in LDS in the candidates' order, and
//                 whenever it holds 64 every lane takes one: neighbour k of the query, in that order, is lane k % 64's
//                 (k / 64)-th term, so the arithmetic runs on full waves.  Pass 1 keeps 10 double partials per lane (sum w,
//                 sum w q, sum w q q^T) and the count; pass 2, for order 2 with six neighbours or more, 27 (the upper triangle
//                 of M, and g).  The lanes' partials meet in device_util.hpp's fixed tree.  The 3 x 3 eigen-solve (sym_eig3.hpp)
//                 and the 6 x 6 solve (icp_solve6.hpp) are run by every lane on the same numbers -- wave-uniform -- and lane 0
//                 writes the record under the point's ORIGINAL index
//   k_mls_stats   the five counts and the longest displacement: integer adds and a maximum, so order-free
//   k_mls_apply   a lane per record: (float)((double)p + disp), the colour word and an invalid record as they were
// The summation order is a function of the grid -- which is a function of the cloud and the radius -- and of nothing else: no
// atomic and no launch geometry enters a floating-point sum.  Every loop is counted: cell ranges, spans, a fixed number of
// Jacobi sweeps.  No block reads what another wrote in the same launch.  No size is refused: the sums stream, a ball that
// holds the whole cloud costs n candidates per query and no memory.
#include <cmath>
#include <cstring>

#include "capi_guard.hpp"
#include "drivers.hpp"
#include "device_util.hpp"
#include "icp_solve6.hpp"
#include "radius_grid.hpp"
#include "sym_eig3.hpp"

namespace mm3d {

namespace {

constexpr int kMlsThreads = 256;            // four waves, a query each
constexpr int kMlsWaves = kMlsThreads / kWave;
constexpr int kMlsRing = 2 * kWave;         // a wave's ring of neighbours: fewer than 64 held over, at most 64 more from one step
constexpr int kMlsSweepBlocks = 256;        // k_mls_stats: this many blocks stride over the records
constexpr double kMlsGapTau = 1e-6;         // DEGENERATE: lambda1 - lambda0 <= this * trace
constexpr double kMlsPivotTau = 1e-9;       // order 2 singular: a pivot <= this * trace(M) / 6
constexpr int kMlsPolyMin = 6;              // order 2 needs as many neighbours as it has coefficients

enum { kInvalid = 0, kFew = 1, kDegenerate = 2, kPlane = 3, kPolynomial = 4 };

// lane 0's double in every lane (all 64 lanes enabled: the first active lane is lane 0)
__device__ __forceinline__ double mls_lane0(double v)
{
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)b), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double mls_total(double v) { return mls_lane0(wave_sum(v)); }

struct MlsBox { int x0, x1, y0, y1, z0, z1; };

// f(p, d2) for every neighbour of q among the box's candidates, neighbour k -- in the order of the spans and of the points in
// them -- on lane k % 64.  `ring` is this wave's kMlsRing records of LDS: a step's neighbours are written behind those held
// (x, y, z and d2 in the colour's place), and once 64 are held every lane takes one.  Everything but the two bodies under
// `k < end` and `lane < held` is wave-uniform: the box, the spans, `held` and `head` (popcounts of ballots).
template <class F>
__device__ __forceinline__ void mls_walk(const GridView &g, const MlsBox &b, int lane, const float4 &q, double r2, float4 *ring, F &&f)
{
  int head = 0, held = 0;
  for (int z = b.z0; z <= b.z1; ++z)
    for (int y = b.y0; y <= b.y1; ++y) {
      const int row = (z * g.dy + y) * g.dx;
      const int beg = g.cell_start[row + b.x0], end = g.cell_start[row + b.x1 + 1];   // (a row of cells is one span of points)
      for (int k0 = beg; k0 < end; k0 += kWave) {
        const int k = k0 + lane;
        bool hit = false;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < end) {
          p = g.pts[k];
          p.w = dist2(p.x, p.y, p.z, q.x, q.y, q.z);
          hit = (double)p.w <= r2;
        }
        const unsigned long long hits = ballot(hit);
        if (hit) ring[(head + held + __popcll(hits & ((1ull << lane) - 1ull))) & (kMlsRing - 1)] = p;
        held += __popcll(hits);                           // (below 64 before, so at most 127: the ring holds them)
        if (held >= kWave) {
          wave_lds_fence();
          const float4 e = ring[(head + lane) & (kMlsRing - 1)];
          f(e, e.w);
          wave_lds_fence();                               // (the next step's writes come after these reads)
          head = (head + kWave) & (kMlsRing - 1);
          held -= kWave;
        }
      }
    }
  wave_lds_fence();
  if (lane < held) {
    const float4 e = ring[(head + lane) & (kMlsRing - 1)];
    f(e, e.w);
  }
  wave_lds_fence();                                       // (the second pass writes the ring again)
}

__global__ void __launch_bounds__(kMlsThreads)
k_mls_fit(GridView g, int s /* cells to either side */, double r, int order, int min_neighbours, double *__restrict__ disp /* [n][3] */,
          int *__restrict__ state, int *__restrict__ count)
{
  __shared__ float4 s_ring[kMlsWaves][kMlsRing];         // 8 KiB a block; a wave touches its own row alone, so no block barrier
  const unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const int j = (int)bid * kMlsWaves + wave;
  if (j >= g.n) return;                                   // (the whole wave: every lane below is enabled at every reduction)
  float4 *const ring = s_ring[wave];
  const float4 q = g.pts[j];
  const int i = __float_as_int(q.w);
  const double r2 = r * r;
  MlsBox b;
  {
    const int cx = clampi(cell_floor(q.x, g.minx, g.inv), 0, g.dx - 1);
    const int cy = clampi(cell_floor(q.y, g.miny, g.inv), 0, g.dy - 1);
    const int cz = clampi(cell_floor(q.z, g.minz, g.inv), 0, g.dz - 1);
    b.x0 = max(cx - s, 0); b.x1 = min(cx + s, g.dx - 1);
    b.y0 = max(cy - s, 0); b.y1 = min(cy + s, g.dy - 1);
    b.z0 = max(cz - s, 0); b.z1 = min(cz + s, g.dz - 1);
  }
  const double qx = (double)q.x, qy = (double)q.y, qz = (double)q.z;

  // ---- pass 1: the weighted moments about the query point
  double a[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) a[k] = 0.0;
  int cnt = 0;
  mls_walk(g, b, lane, q, r2, ring, [&](const float4 &p, float d2) {
    const double w = exp(-(double)d2 / r2);
    const double x = (double)p.x - qx, y = (double)p.y - qy, z = (double)p.z - qz;
    const double wx = w * x, wy = w * y, wz = w * z;
    a[0] += w;
    a[1] += wx; a[2] += wy; a[3] += wz;
    a[4] += wx * x; a[5] += wx * y; a[6] += wx * z;
    a[7] += wy * y; a[8] += wy * z; a[9] += wz * z;
    ++cnt;
  });
#pragma unroll
  for (int k = 0; k < 10; ++k) a[k] = mls_total(a[k]);
  cnt = wave_sum(cnt);

  // ---- the plane (wave-uniform from here to the second pass)
  int st = kFew;
  double n[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0}, o[3] = {0.0, 0.0, 0.0};
  if (cnt >= min_neighbours) {
    const double sw = a[0];
    const double mu[3] = {a[1] / sw, a[2] / sw, a[3] / sw};
    double C[3][3], ev[3], V[3][3];
    C[0][0] = a[4] / sw - mu[0] * mu[0];
    C[0][1] = C[1][0] = a[5] / sw - mu[0] * mu[1];
    C[0][2] = C[2][0] = a[6] / sw - mu[0] * mu[2];
    C[1][1] = a[7] / sw - mu[1] * mu[1];
    C[1][2] = C[2][1] = a[8] / sw - mu[1] * mu[2];
    C[2][2] = a[9] / sw - mu[2] * mu[2];
    const double trace = (C[0][0] + C[1][1]) + C[2][2];
    sym_eig3(C, ev, V);
#pragma unroll
    for (int k = 0; k < 3; ++k) { n[k] = V[k][0]; u[k] = V[k][1]; v[k] = V[k][2]; }
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] /= len;
    const double t = (mu[0] * n[0] + mu[1] * n[1]) + mu[2] * n[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = t * n[k];
    const bool finite = isfinite(trace) && isfinite(ev[0]) && isfinite(ev[1]) && isfinite(ev[2]) && isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]);
    st = (finite && trace > 0.0 && ev[1] - ev[0] > kMlsGapTau * trace) ? kPlane : kDegenerate;
  }
  double d[3] = {0.0, 0.0, 0.0};
  if (st == kPlane) { d[0] = o[0]; d[1] = o[1]; d[2] = o[2]; }

  // ---- pass 2: the quadratic over the plane, h = c . (1, a, b, a^2, a b, b^2)
  if (st == kPlane && order == 2 && cnt >= kMlsPolyMin) {
    double m[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) m[k] = 0.0;
    mls_walk(g, b, lane, q, r2, ring, [&](const float4 &p, float d2) {
      const double w = exp(-(double)d2 / r2);
      const double ex = ((double)p.x - qx) - o[0], ey = ((double)p.y - qy) - o[1], ez = ((double)p.z - qz) - o[2];
      const double ca = ((ex * u[0] + ey * u[1]) + ez * u[2]) / r, cb = ((ex * v[0] + ey * v[1]) + ez * v[2]) / r;
      const double h = (ex * n[0] + ey * n[1]) + ez * n[2];
      const double phi[6] = {1.0, ca, cb, ca * ca, ca * cb, cb * cb};
#pragma unroll
      for (int k = 0; k < 21; ++k) m[k] += (w * phi[kUi[k]]) * phi[kUj[k]];
#pragma unroll
      for (int k = 0; k < 6; ++k) m[21 + k] += (w * phi[k]) * h;
    });
#pragma unroll
    for (int k = 0; k < 27; ++k) m[k] = mls_total(m[k]);
    double A[36], g6[6], c6[6];
#pragma unroll
    for (int k = 0; k < 21; ++k) A[kUi[k] * 6 + kUj[k]] = A[kUj[k] * 6 + kUi[k]] = m[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) g6[k] = m[21 + k];
    const double trM = ((((A[0] + A[7]) + A[14]) + A[21]) + A[28]) + A[35];
    if (solve6_ldlt(A, g6, kMlsPivotTau * trM / 6.0, c6)) {
      const double px = o[0] + c6[0] * n[0], py = o[1] + c6[0] * n[1], pz = o[2] + c6[0] * n[2];
      const double len2 = sqrt((px * px + py * py) + pz * pz);
      if (isfinite(len2) && len2 <= r) { d[0] = px; d[1] = py; d[2] = pz; st = kPolynomial; }
    }
  }
  if (lane == 0) {
    disp[(size_t)i * 3 + 0] = d[0];
    disp[(size_t)i * 3 + 1] = d[1];
    disp[(size_t)i * 3 + 2] = d[2];
    state[i] = st;
    count[i] = cnt;
  }
}

// ctl[s] = the records of state s (0 .. 4); ctl[5] = the bits of the longest displacement, a double >= 0, whose bits order as
// the numbers do.  A lane keeps its own counts over its slices, the wave folds them, and a wave issues its atomics once.
__global__ void __launch_bounds__(256)
k_mls_stats(const double *__restrict__ disp, const int *__restrict__ state, int n, unsigned long long *__restrict__ ctl)
{
  int c[5] = {0, 0, 0, 0, 0};
  double longest = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {   // (counted)
    const int s = state[i];
#pragma unroll
    for (int k = 0; k < 5; ++k) c[k] += s == k ? 1 : 0;
    const double x = disp[i * 3 + 0], y = disp[i * 3 + 1], z = disp[i * 3 + 2];
    longest = fmax(longest, sqrt((x * x + y * y) + z * z));
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) c[k] = wave_sum(c[k]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) longest = fmax(longest, __shfl_xor(longest, o, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (c[k]) atomicAdd(&ctl[k], (unsigned long long)c[k]);
    if (longest > 0.0) atomicMax(&ctl[5], (unsigned long long)__double_as_longlong(longest));
  }
}

__global__ void __launch_bounds__(256)
k_mls_apply(const float4 *__restrict__ pts, const double *__restrict__ disp, const int *__restrict__ state, int n, float4 *__restrict__ out)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float4 p = pts[i];
  if (state[i] != kInvalid) {
    p.x = (float)((double)p.x + disp[(size_t)i * 3 + 0]);
    p.y = (float)((double)p.y + disp[(size_t)i * 3 + 1]);
    p.z = (float)((double)p.z + disp[(size_t)i * 3 + 2]);
  }
  out[i] = p;
}

// ---------------------------------------------------------------- host
bool mls_radius_ok(double radius, bool zero_ok) { return std::isfinite(radius) && (radius > 0.0 || (zero_ok && radius == 0.0)); }
bool mls_args_ok(double radius, int order, int min_neighbours) { return mls_radius_ok(radius, false) && (order == 1 || order == 2) && min_neighbours >= 3; }

struct MlsWork {
  DevBuf<double> disp;                    // [n][3], zero where the point stays
  DevBuf<int> state, count;               // [n] each
  DevBuf<unsigned long long> ctl;         // k_mls_stats' six words
};

// The rule for every record, on the device, nothing waited for beyond the cloud's box and its grid.  in->n > 0.
void mls_fit(Context *c, const mm3d_cloud *in_, double radius, int order, int min_neighbours, MlsWork &w)
{
  auto *in = const_cast<mm3d_cloud *>(in_);
  const size_t n = in->n;
  w.disp = DevBuf<double>(c, n * 3);
  w.state = DevBuf<int>(c, n);
  w.count = DevBuf<int>(c, n);
  w.ctl = DevBuf<unsigned long long>(c, 8);
  MM3D_HIP(hipMemsetAsync(w.disp.get(), 0, n * 3 * sizeof(double), c->stream));
  MM3D_HIP(hipMemsetAsync(w.state.get(), 0, n * sizeof(int), c->stream));            // (kInvalid: the grid holds the valid points only)
  MM3D_HIP(hipMemsetAsync(w.count.get(), 0, n * sizeof(int), c->stream));
  MM3D_HIP(hipMemsetAsync(w.ctl.get(), 0, 8 * sizeof(unsigned long long), c->stream));
  cloud_bbox(c, in);
  if (in->n_finite > 0) {
    const Grid &g = cloud_grid(c, in, radius_cell(in, radius));
    const int s = radius_reach(g, radius);
    MM3D_LAUNCH(c, "mls_fit", g.n * (16.0 + 32.0), k_mls_fit, dim3(div_up((size_t)g.n, kMlsWaves)), dim3(kMlsThreads), 0, g.view(), s, radius, order,
                min_neighbours, w.disp.get(), w.state.get(), w.count.get());
  }
  MM3D_LAUNCH(c, "mls_stats", n * 28.0, k_mls_stats, dim3(std::min<unsigned>((unsigned)div_up(n, 256), kMlsSweepBlocks)), dim3(256), 0,
              (const double *)w.disp.get(), (const int *)w.state.get(), (int)n, w.ctl.get());
}

void mls_stats(size_t n, const unsigned long long *h, mm3d_smooth_stats *st)
{
  st->points = (long long)n;
  st->valid = (long long)n - (long long)h[kInvalid];
  st->few = (long long)h[kFew];
  st->degenerate = (long long)h[kDegenerate];
  st->plane = (long long)h[kPlane];
  st->polynomial = (long long)h[kPolynomial];
  std::memcpy(&st->max_displacement, &h[5], sizeof(double));
}

mm3d_cloud *smooth_cloud(Context *c, const mm3d_cloud *in, double radius, int order, int min_neighbours, mm3d_smooth_stats *stats)
{
  MM3D_REQUIRE(mls_args_ok(radius, order, min_neighbours), "smoothing: the radius must be finite and > 0, the order 1 or 2, min_neighbours >= 3");
  MM3D_REQUIRE(in->n < ((size_t)1 << 31), "smoothing: more than 2^31 - 1 points");
  const size_t n = in->n;
  if (n == 0) {
    if (stats) *stats = mm3d_smooth_stats{0, 0, 0, 0, 0, 0, 0.0};
    return cloud_from_device(c, DevBuf<float4>(c, 0), 0);
  }
  MlsWork w;
  mls_fit(c, in, radius, order, min_neighbours, w);
  DevBuf<float4> out(c, n);
  MM3D_LAUNCH(c, "mls_apply", n * 60.0, k_mls_apply, dim3(div_up(n, 256)), dim3(256), 0, in->pts.get(), (const double *)w.disp.get(),
              (const int *)w.state.get(), (int)n, out.get());
  unsigned long long *h = (unsigned long long *)c->pin(64);
  std::memset(h, 0, 64);
  MM3D_HIP(hipMemcpyAsync(h, w.ctl.get(), 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  c->sync();                                            // the one wait: the counts; the work buffers go back to the pool behind it
  if (stats) mls_stats(n, h, stats);
  // (voxel_leaf stays 0: the moved points are no voxel grid's centroids any more, and cloud_grid must not size cells by a leaf)
  return cloud_from_device(c, std::move(out), n);
}

struct SmootherMls final : SmootherBase {
  mm3d_cloud *smooth(Context *c, const mm3d_cloud *in, const mm3d_smooth_options &o, double resolution, mm3d_smooth_stats *stats) const override
  {
    return smooth_cloud(c, in, o.radius > 0.0 ? o.radius : 3.0 * resolution, o.order, o.min_neighbours, stats);
  }
};
const SmootherMls g_mls;

bool options_ok(const mm3d_smooth_options *o)
{
  if (!o || (o->method != MM3D_SMOOTH_OFF && o->method != MM3D_SMOOTH_MLS)) return false;
  if (o->where == 0 || (o->where & ~(MM3D_SMOOTH_MAPS | MM3D_SMOOTH_COMPOSED))) return false;
  return (o->order == 1 || o->order == 2) && o->min_neighbours >= 3 && mls_radius_ok(o->radius, true);
}

}  // namespace

}  // namespace mm3d

using namespace mm3d;

extern "C" {

int mm3d_smooth_displacements(mm3d_ctx *ctx, const mm3d_cloud *points, double radius, int order, int min_neighbours, double *disp, int *state,
                              int *neighbours, size_t capacity, mm3d_smooth_stats *stats)
{
  if (!ctx || !points || !disp || !mls_args_ok(radius, order, min_neighbours) || points->n >= ((size_t)1 << 31)) return MM3D_EINVAL;
  if (capacity < points->n) return MM3D_ECAPACITY;
  if (points->n == 0) {
    if (stats) *stats = mm3d_smooth_stats{0, 0, 0, 0, 0, 0, 0.0};
    return MM3D_OK;
  }
  return guarded(ctx, [&] {
    const size_t n = points->n;
    MlsWork w;
    mls_fit(ctx, points, radius, order, min_neighbours, w);
    unsigned long long *h = (unsigned long long *)ctx->pin(64);
    std::memset(h, 0, 64);
    MM3D_HIP(hipMemcpyAsync(h, w.ctl.get(), 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    MM3D_HIP(hipMemcpyAsync(disp, w.disp.get(), n * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (state) MM3D_HIP(hipMemcpyAsync(state, w.state.get(), n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (neighbours) MM3D_HIP(hipMemcpyAsync(neighbours, w.count.get(), n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    if (stats) mls_stats(n, h, stats);
  });
}

int mm3d_smooth_cloud(mm3d_ctx *ctx, const mm3d_cloud *in, double radius, int order, int min_neighbours, mm3d_cloud **out)
{
  if (!ctx || !in || !out) return MM3D_EINVAL;
  *out = nullptr;
  if (!mls_args_ok(radius, order, min_neighbours) || in->n >= ((size_t)1 << 31)) return MM3D_EINVAL;
  return guarded(ctx, [&] { *out = smooth_cloud(ctx, in, radius, order, min_neighbours, &ctx->last_smooth_stats); });
}

int mm3d_set_smoothing(mm3d_ctx *ctx, const mm3d_smooth_options *options)
{
  if (!ctx || !options_ok(options)) return MM3D_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the stage changes)
  return select_stage(ctx, Stage::Smoothing, [&](StageSelection &s) {
    s.smooth_options = *options;
    s.smoother = stage_active(Stage::Smoothing, s) ? &g_mls : nullptr;
  });
}

int mm3d_get_smoothing(const mm3d_ctx *ctx, mm3d_smooth_options *options)
{
  if (!ctx || !options) return MM3D_EINVAL;
  *options = ctx->sel.smooth_options;
  return MM3D_OK;
}

int mm3d_last_smooth_stats(const mm3d_ctx *ctx, mm3d_smooth_stats *stats)
{
  if (!ctx || !stats) return MM3D_EINVAL;
  *stats = ctx->last_smooth_stats;
  return MM3D_OK;
}

}  // extern "C"

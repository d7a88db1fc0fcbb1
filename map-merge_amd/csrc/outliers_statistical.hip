// outliers_statistical.hip -- statistical outlier removal on gfx950: every point's mean distance to its k nearest neighbours,
// held against the cloud's own mean and standard deviation of that distance (mm3d_knn_mean_distances,
// mm3d_remove_outliers_statistical, mm3d_set_outlier_filter; include/mm3d.h states the rule to the operation).
// Not a reference stage: the reference only has the radius filter.
//
// One pass family per cloud, one host wait (the compaction's):
//   cloud_grid      the library's cell-sorted grid, at a cell sized from the cloud's box and size so that a point's k nearest
//                   usually lie inside its 3 x 3 x 3 cells (sor_cell)
//   k_sor_knn       a lane per cell-sorted query; its k smallest d2 so far live in LDS, [k][threads], kept ascending by
//                   a min / max pass per insertion.  The box of cells grows until the k-th distance fits inside it (sor_fits), to 5^3 cells
//                   at the most: a query that needs more leaves its index on a counted list and is done
//   k_sor_knn_wide  a wave per listed query, sized by nothing the host has to wait for (the count is read on the device): the 64
//                   smallest d2 ascending one per lane, candidates 64 at a time, the box grows by half its width a step up to
//                   the whole grid.  The isolated points this filter is for cost a few waves, not their neighbours' time
//   k_sor_partials  S, Q and the valid count of 4096 points per block in a fixed order, doubles, no atomics
//   k_sor_threshold one lane adds the blocks' partials in block order and leaves mu, sigma, t
//   k_sor_keep      a lane per point: valid and d <= t
//   compact         grid.hip::cloud_of_kept, behind whose wait the statistics come back too
// A query's result is a function of the multiset of its candidates' d2 alone, so nothing depends on which pass served it, on
// the order the list was filled in, or on the launch geometry.
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "capi_guard.hpp"
#include "drivers.hpp"
#include "device_util.hpp"

namespace mm3d {

namespace {

constexpr int kSorMaxK = 64;           // one wave's width (k_sor_knn_wide keeps a query's nearest one per lane)
constexpr int kSorThreads = 128;       // k_sor_knn: 4 k bytes of LDS per lane; 128 lanes at k = 64 are 32 KiB, five blocks per CU
constexpr int kSorRings = 2;           // k_sor_knn looks at the 3^3 and the 5^3 box
constexpr int kSorChunk = 4096;        // points per partial sum: the summation order is a function of the cloud's size alone
constexpr int kSorWideBlocks = 256;    // k_sor_knn_wide: 1024 waves take the listed queries in turn
constexpr double kSorCellFactor = 0.7;      // the cell over the estimated k-nearest radius (sor_cell; DESIGN.md section 7n has the sweep)
// Cells per axis at the most: sor_fits' margin of 1e-3 cells is sized for it.  It holds because sor_cell never returns a cell below
// the longest extent over this, and cloud_grid only ever grows a cell; a cloud_grid hit on a colliding key (lround(cell * 1e4), cells
// below 5e-5 m) can only return a grid this same function's cell built for the same cloud, so the bound holds for it as well.
constexpr float kSorAxisCells = 1000.0f;

// A query in the grid's cell coordinates, formed exactly as k_cell_keys forms the cell of a point (device_util.hpp::cell_floor).
struct SorQuery {
  float x, y, z;          // the point
  float tx, ty, tz;       // (v - min) * inv per axis
  int cx, cy, cz;         // its cell, clamped like the grid's
  int self;               // its cell-sorted index: not its own neighbour
};
__device__ __forceinline__ SorQuery sor_query(const GridView &g, const float4 &q, int self)
{
  SorQuery s;
  s.x = q.x; s.y = q.y; s.z = q.z;
  s.tx = (q.x - g.minx) * g.inv; s.ty = (q.y - g.miny) * g.inv; s.tz = (q.z - g.minz) * g.inv;
  s.cx = clampi(cell_floor(q.x, g.minx, g.inv), 0, g.dx - 1);
  s.cy = clampi(cell_floor(q.y, g.miny, g.inv), 0, g.dy - 1);
  s.cz = clampi(cell_floor(q.z, g.minz, g.inv), 0, g.dz - 1);
  s.self = self;
  return s;
}

// Is the k-th smallest d2 final once the box of cells within s of the query's has been scanned?  A point outside the box has a
// cell index beyond one of the box's faces, so its t lies beyond that integer; the query's t minus that integer, the gap, is
// exact in float.  Both t carry at most 3 * 2^-24 * (cells per axis) <= 1.8e-4 cells of rounding, d2 and its root a few 1e-7
// relative: a k-th distance of at most gap - 1e-3 cells (and 1e-5 relative) leaves every outside point at least as far.  A face on
// the grid's border has nothing behind it.  All faces on the border: the whole grid was scanned.
__device__ __forceinline__ float sor_gap(const GridView &g, const SorQuery &q, int s)
{
  float gap = INFINITY;
  if (q.cx - s > 0) gap = fminf(gap, q.tx - (float)(q.cx - s));
  if (q.cx + s < g.dx - 1) gap = fminf(gap, (float)(q.cx + s + 1) - q.tx);
  if (q.cy - s > 0) gap = fminf(gap, q.ty - (float)(q.cy - s));
  if (q.cy + s < g.dy - 1) gap = fminf(gap, (float)(q.cy + s + 1) - q.ty);
  if (q.cz - s > 0) gap = fminf(gap, q.tz - (float)(q.cz - s));
  if (q.cz + s < g.dz - 1) gap = fminf(gap, (float)(q.cz + s + 1) - q.tz);
  return gap;
}
__device__ __forceinline__ bool sor_fits(const GridView &g, float gap, float kth)
{
  if (gap == INFINITY) return true;
  return kth < INFINITY && sqrtf(kth) * g.inv * 1.00001f + 1e-3f <= gap;
}
__device__ __forceinline__ bool sor_final(const GridView &g, const SorQuery &q, int s, float kth) { return sor_fits(g, sor_gap(g, q, s), kth); }
// No d2 above this can pass sor_fits at this gap (generously: it only spares candidates that cannot decide an insertion).
__device__ __forceinline__ float sor_reach(const GridView &g, float gap)
{
  if (gap == INFINITY) return INFINITY;
  const float r = gap / g.inv;
  return r * r * 1.001f;
}

// The cells of the box of half width s that the box of half width prev (< s; -1: none) did not have, as spans of cell-sorted
// points: item r of 2 * rows is half (r & 1) of row (r >> 1) of the box's (y, z) rows.  A row outside the inner box is one span
// (its half 1 is empty); a row through it is the two spans left and right of it.
struct SorBox { int x0, x1, y0, y1, z0, z1, ny, items; };
__device__ __forceinline__ SorBox sor_box(const GridView &g, const SorQuery &q, int s)
{
  SorBox b;
  b.x0 = max(q.cx - s, 0); b.x1 = min(q.cx + s, g.dx - 1);
  b.y0 = max(q.cy - s, 0); b.y1 = min(q.cy + s, g.dy - 1);
  b.z0 = max(q.cz - s, 0); b.z1 = min(q.cz + s, g.dz - 1);
  b.ny = b.y1 - b.y0 + 1;
  b.items = 2 * b.ny * (b.z1 - b.z0 + 1);
  return b;
}
__device__ __forceinline__ void sor_span(const GridView &g, const SorQuery &q, const SorBox &b, int prev, int r, int &beg, int &end)
{
  const int ri = r >> 1, half = r & 1;
  const int z = b.z0 + ri / b.ny, y = b.y0 + ri % b.ny;
  const bool inner = prev >= 0 && abs(z - q.cz) <= prev && abs(y - q.cy) <= prev;
  int xa, xb;                                   // inclusive; empty when xa > xb
  if (!inner) { xa = half ? 1 : b.x0; xb = half ? 0 : b.x1; }
  else if (!half) { xa = b.x0; xb = q.cx - prev - 1; }
  else { xa = q.cx + prev + 1; xb = b.x1; }
  beg = end = 0;
  if (xa <= xb) {
    const int row = (z * g.dy + y) * g.dx;
    beg = g.cell_start[row + xa];
    end = g.cell_start[row + xb + 1];
  }
}

// One atomic per wave for whichever of its lanes are here: the lane's own number of counter's old value on.
__device__ __forceinline__ int sor_take(int *counter)
{
  const unsigned long long act = ballot(true);
  const int lane = threadIdx.x & (kWave - 1), lead = __ffsll((long long)act) - 1;
  int base = 0;
  if (lane == lead) base = atomicAdd(counter, __popcll(act));
  base = __shfl(base, lead, kWave);
  return base + __popcll(act & ((1ull << lane) - 1ull));
}

// ---------------------------------------------------------------- a lane per query
__global__ void __launch_bounds__(kSorThreads)
k_sor_knn(GridView g, int kk, double *__restrict__ d_out /* by original index */, int *__restrict__ ov_list, int *__restrict__ ctl /* [0] listed, [1] queries that looked past the first box (counted only when `count_past`: mm3d_set_debug) */, int count_past)
{
  extern __shared__ float s_near[];             // [kk][kSorThreads]: lane l's column is s_near[j * kSorThreads + l], one bank whatever j
  const unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
  const int i = bid * kSorThreads + threadIdx.x;
  if (i >= g.n) return;
  const float4 p0 = g.pts[i];
  const SorQuery q = sor_query(g, p0, i);
  float *col = s_near + threadIdx.x;
  for (int j = 0; j < kk; ++j) col[j * kSorThreads] = INFINITY;
  float kth = INFINITY;
  bool done = false;
  // Each box is scanned whole, and only up to the largest d2 that could still be final in it (sor_reach): about half of a 3^3
  // box's points lie beyond, and need no place in the column.  With k of them within reach the k-th is the box's k-th and
  // decides; with fewer, the next box starts over, its reach being another.
  for (int s = 1; s <= kSorRings; ++s) {
    if (s == 2) {
      if (count_past) (void)sor_take(&ctl[1]);
      for (int j = 0; j < kk; ++j) col[j * kSorThreads] = INFINITY;
      kth = INFINITY;
    }
    const float gap = sor_gap(g, q, s), reach = sor_reach(g, gap);
    const SorBox b = sor_box(g, q, s);
    for (int r = 0; r < b.items; r += 2) {         // (whole rows: the odd items are the right halves of a shell's rows)
      int beg, end;
      sor_span(g, q, b, -1, r, beg, end);
      for (int j = beg; j < end; ++j) {
        if (j == i) continue;
        const float4 p = g.pts[j];
        const float d = dist2(q.x, q.y, q.z, p.x, p.y, p.z);
        if (d < kth && d <= reach) {              // (ties with the k-th stay out: they cannot change the sum)
          // one pass down the column, the larger of each pair carried on: no branch of a lane's own, so the lanes of a wave
          // that insert at different places cost what one of them costs
          float carry = d, low = d;
#pragma unroll 4
          for (int at = 0; at < kk; ++at) {
            const float x = col[at * kSorThreads];
            low = fminf(x, carry);
            carry = fmaxf(x, carry);
            col[at * kSorThreads] = low;
          }
          kth = low;
        }
      }
    }
    if (sor_fits(g, gap, kth)) { done = true; break; }
  }
  if (!done) {
    ov_list[sor_take(&ctl[0])] = i;                // (the list's order decides nothing)
    return;
  }
  double sum = 0.0;
  for (int j = 0; j < kk; ++j) sum += sqrt((double)col[j * kSorThreads]);
  d_out[__float_as_int(p0.w)] = sum / (double)kk;
}

// ---------------------------------------------------------------- a wave per listed query
__device__ __forceinline__ float sor_readlane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

__global__ void __launch_bounds__(256)
k_sor_knn_wide(GridView g, int kk, const int *__restrict__ ov_list, const int *__restrict__ ctl, double *__restrict__ d_out)
{
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave), n_waves = gridDim.x * (blockDim.x / kWave);
  const int listed = min(ctl[0], g.n);
  for (int o = wave; o < listed; o += n_waves) {       // (wave-uniform: every loop below is)
    const int i = ov_list[o];
    const float4 p0 = g.pts[i];
    const SorQuery q = sor_query(g, p0, i);
    float a = INFINITY;                                 // the 64 smallest d2 so far, ascending over the lanes
    float kth = INFINITY;                               // lane kk - 1's
    int prev = -1, s = kSorRings + 1;
    for (;;) {
      const SorBox b = sor_box(g, q, s);
      for (int r0 = 0; r0 < b.items; r0 += kWave) {
        int beg = 0, end = 0;
        if (r0 + lane < b.items) sor_span(g, q, b, prev, r0 + lane, beg, end);
        unsigned long long rows = ballot(end > beg);
        while (rows) {
          const int src = __ffsll((long long)rows) - 1;
          rows &= rows - 1ull;
          const int bb = __builtin_amdgcn_readlane(beg, src), ee = __builtin_amdgcn_readlane(end, src);
          for (int j0 = bb; j0 < ee; j0 += kWave) {
            const int j = j0 + lane;
            float d = INFINITY;
            if (j < ee && j != i) {
              const float4 p = g.pts[j];
              d = dist2(q.x, q.y, q.z, p.x, p.y, p.z);
            }
            unsigned long long cand = ballot(d < kth);
            while (cand) {
              const int cl = __ffsll((long long)cand) - 1;
              cand &= cand - 1ull;
              const float v = sor_readlane_f(d, cl);
              if (!(v < kth)) continue;                 // (an earlier candidate of this batch lowered the k-th)
              const float below = __shfl_up(a, 1, kWave);
              a = (a <= v) ? a : ((lane == 0 || below <= v) ? v : below);
              kth = sor_readlane_f(a, kk - 1);
            }
          }
        }
      }
      if (sor_final(g, q, s, kth)) break;               // (at the latest when the box is the whole grid)
      prev = s;
      s += 1 + s / 2;
    }
    const double root = sqrt((double)a);
    double sum = 0.0;
    for (int j = 0; j < kk; ++j) {
      const long long bits = __double_as_longlong(root);
      const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)bits, j), hi = (unsigned)__builtin_amdgcn_readlane((int)(bits >> 32), j);
      sum += __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    }
    if (lane == 0) d_out[__float_as_int(p0.w)] = sum / (double)kk;
  }
}

// ---------------------------------------------------------------- the threshold
// d is NaN exactly at the invalid points (a valid point's is a sum of roots of d2 >= 0 or +inf).  Block b sums points
// [b * kSorChunk, (b + 1) * kSorChunk): lane l its 16 points l, l + 256, ... in that order, the wave by device_util.hpp's fixed
// tree, the four waves in order.
struct SorPartial { double s, q; long long n; long long pad; };
__global__ void __launch_bounds__(256)
k_sor_partials(const double *__restrict__ d, size_t n, SorPartial *__restrict__ part)
{
  const size_t base = (size_t)blockIdx.x * kSorChunk;
  double s = 0.0, q = 0.0;
  int cnt = 0;
  for (int u = 0; u < kSorChunk / 256; ++u) {
    const size_t i = base + (size_t)u * 256 + threadIdx.x;
    const double v = i < n ? d[i] : __longlong_as_double(-1ll);
    if (v == v) { s += v; q += v * v; ++cnt; }
  }
  s = wave_sum(s); q = wave_sum(q); cnt = wave_sum(cnt);
  __shared__ double s_s[4], s_q[4];
  __shared__ int s_n[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_s[wave] = s; s_q[wave] = q; s_n[wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    SorPartial p;
    p.s = ((s_s[0] + s_s[1]) + s_s[2]) + s_s[3];
    p.q = ((s_q[0] + s_q[1]) + s_q[2]) + s_q[3];
    p.n = (long long)s_n[0] + s_n[1] + s_n[2] + s_n[3];
    p.pad = 0;
    part[blockIdx.x] = p;
  }
}

struct SorStats { double mean, stddev, threshold; long long valid; };
__global__ void k_sor_threshold(const SorPartial *__restrict__ part, int blocks, double mult, SorStats *__restrict__ out)
{
  if (blockIdx.x || threadIdx.x) return;
  double S = 0.0, Q = 0.0;
  long long nv = 0;
  for (int b = 0; b < blocks; ++b) { S += part[b].s; Q += part[b].q; nv += part[b].n; }
  SorStats st{0.0, 0.0, 0.0, nv};
  if (nv > 1) {
    st.mean = S / (double)nv;
    const double var = fmax(0.0, (Q - S * S / (double)nv) / (double)(nv - 1));
    st.stddev = sqrt(var);
    st.threshold = st.mean + mult * st.stddev;
  }
  *out = st;
}

__global__ void __launch_bounds__(256)
k_sor_keep(const float4 *__restrict__ pts, const double *__restrict__ d, const SorStats *__restrict__ st, size_t n, int every_valid,
           int *__restrict__ flags)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (every_valid) {                                     // (at most one valid point: it is kept, and has no distance)
    const float4 p = pts[i];
    flags[i] = (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) ? 1 : 0;
    return;
  }
  flags[i] = d[i] <= st->threshold ? 1 : 0;              // (NaN, an invalid point, compares false)
}

// ---------------------------------------------------------------- host
std::atomic<long long> g_sor_search[3];                  // queries, looked past the first box, listed (mm3d_debug_outlier_search)

bool sor_args_ok(int mean_k, double stddev_mult) { return mean_k >= 1 && mean_k <= kSorMaxK && std::isfinite(stddev_mult) && stddev_mult >= 0.0; }

// The grid's cell: kSorCellFactor (0.7; MM3D_SOR_CELL_FACTOR overrides it, an A/B knob) times the radius that holds k + 1 points at the cloud's mean density, taken as the largest of a line's, a
// sheet's and a solid's over the bounding box (a room's walls are between the last two), so that the first box usually decides.
// A wrong guess costs time, never the result.  Bounds: a voxel-filtered cloud's cell need not exceed four times the radius at one
// point per leaf^2; at most kSorAxisCells cells per axis (sor_final) and about eight cells per point (the table's memory).
float sor_cell(const mm3d_cloud *in, int kk)
{
  const double pi = 3.14159265358979323846;
  const double n = (double)in->n_finite, m = kk + 1.0;
  double e[3];
  for (int a = 0; a < 3; ++a) e[a] = std::max(0.0, (double)in->bmax[a] - (double)in->bmin[a]);
  const double emax = std::max(e[0], std::max(e[1], e[2]));
  const double line = m * emax / (2.0 * n);
  const double sheet = std::sqrt(m * (e[0] * e[1] + e[1] * e[2] + e[0] * e[2]) / (pi * n));
  const double solid = std::cbrt(3.0 * m * e[0] * e[1] * e[2] / (4.0 * pi * n));
  static const double factor = [] { const char *e = getenv("MM3D_SOR_CELL_FACTOR"); return e && atof(e) > 0.0 ? atof(e) : kSorCellFactor; }();   // A/B knob
  double cell = factor * std::max(line, std::max(sheet, solid));
  if (in->voxel_leaf > 0.f) cell = std::min(cell, 4.0 * factor * (double)in->voxel_leaf * std::sqrt(m / pi));
  cell = std::max(cell, emax / (double)kSorAxisCells);
  if (!(cell >= 1e-30) || !std::isfinite(cell)) cell = emax > 0.0 && std::isfinite(emax) ? emax : 1.0;   // (every point in one place)
  const double cap = std::max(8.0 * n, 32768.0);
  for (;;) {
    const double cells = (std::floor(e[0] / cell) + 2) * (std::floor(e[1] / cell) + 2) * (std::floor(e[2] / cell) + 2);
    if (!(cells > cap)) break;
    cell *= 1.26;
  }
  return (float)cell;
}

// step 3 of the rule for every point into d (device, n doubles by input index, NaN where the rule has none); returns k'.
// `list` is the kernels' scratch: the caller keeps it until it has waited for the stream.
int sor_mean_distances(Context *c, const mm3d_cloud *in_, int mean_k, double *d, DevBuf<int> &list)
{
  auto *in = const_cast<mm3d_cloud *>(in_);
  const size_t n = in->n;
  MM3D_HIP(hipMemsetAsync(d, 0xFF, n * sizeof(double), c->stream));       // (all ones: a NaN)
  cloud_bbox(c, in);
  if (in->n_finite <= 1) return 0;
  const int kk = (int)std::min<size_t>((size_t)mean_k, in->n_finite - 1);
  const Grid &g = cloud_grid(c, in, sor_cell(in, kk));
  list = DevBuf<int>(c, (size_t)g.n + 16);
  int *const ctl = list.get() + g.n;
  MM3D_HIP(hipMemsetAsync(ctl, 0, 16 * sizeof(int), c->stream));
  MM3D_LAUNCH(c, "sor_knn", g.n * (16.0 + 8.0), k_sor_knn, dim3(div_up((size_t)g.n, kSorThreads)), dim3(kSorThreads),
              (size_t)kk * kSorThreads * sizeof(float), g.view(), kk, d, list.get(), ctl, c->debug ? 1 : 0);
  MM3D_LAUNCH(c, "sor_knn_wide", 0.0, k_sor_knn_wide, dim3(std::min<unsigned>(kSorWideBlocks, div_up((size_t)g.n, 4))), dim3(256), 0, g.view(), kk,
              (const int *)list.get(), (const int *)ctl, d);
  if (c->debug) {                                                          // (mm3d_set_debug: counters that cost a wait)
    int *h = (int *)c->pin(64);
    MM3D_HIP(hipMemcpyAsync(h, ctl, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    c->sync();
    g_sor_search[0] += g.n; g_sor_search[1] += h[1]; g_sor_search[2] += h[0];
  }
  return kk;
}

mm3d_cloud *remove_outliers_statistical(Context *c, const mm3d_cloud *in, int mean_k, double stddev_mult, mm3d_outlier_stats *stats)
{
  MM3D_REQUIRE(sor_args_ok(mean_k, stddev_mult), "statistical outlier removal: mean_k must be 1 .. 64, stddev_mult finite and >= 0");
  MM3D_REQUIRE(in->n < ((size_t)1 << 31), "statistical outlier removal: more than 2^31 - 1 points");
  const size_t n = in->n;
  mm3d_outlier_stats st{(long long)n, 0, 0, 0, 0.0, 0.0, 0.0};
  if (n == 0) {
    if (stats) *stats = st;
    return cloud_from_device(c, DevBuf<float4>(c, 0), 0);
  }
  DevBuf<double> d(c, n);
  DevBuf<int> list;
  const int kk = sor_mean_distances(c, in, mean_k, d.get(), list);
  const int blocks = (int)div_up(n, kSorChunk);
  DevBuf<SorPartial> part(c, (size_t)blocks + 1);       // (+ 1: the SorStats record behind the partials)
  SorStats *const dst = (SorStats *)(part.get() + blocks);
  static_assert(sizeof(SorStats) == sizeof(SorPartial), "one buffer for both");
  DevBuf<int> keep(c, n + 1);
  SorStats *h = (SorStats *)c->pin(64);
  std::memset(h, 0, sizeof(SorStats));
  if (kk > 0) {
    MM3D_LAUNCH(c, "sor_partials", n * 8.0, k_sor_partials, dim3(blocks), dim3(256), 0, (const double *)d.get(), n, part.get());
    MM3D_LAUNCH(c, "sor_threshold", blocks * 32.0, k_sor_threshold, dim3(1), dim3(64), 0, (const SorPartial *)part.get(), blocks, stddev_mult, dst);
    MM3D_HIP(hipMemcpyAsync(h, dst, sizeof(SorStats), hipMemcpyDeviceToHost, c->stream));
  }
  MM3D_LAUNCH(c, "sor_keep", n * 12.0, k_sor_keep, dim3(div_up(n, 256)), dim3(256), 0, in->pts.get(), (const double *)d.get(), (const SorStats *)dst, n,
              kk > 0 ? 0 : 1, keep.get());
  size_t m = 0;
  mm3d_cloud *res = cloud_of_kept(c, in, keep.get(), true, &m);      // the one wait: count, box and the statistics (a subset of a voxel grid's centroids)
  st.valid = kk > 0 ? h->valid : (long long)in->n_finite;
  st.kept = (long long)m;
  st.k = kk;
  st.mean = h->mean; st.stddev = h->stddev; st.threshold = h->threshold;
  if (stats) *stats = st;
  return res;
}

struct OutliersStatistical final : OutlierFilterBase {
  int method() const override { return MM3D_OUTLIERS_STATISTICAL; }
  mm3d_cloud *filter(Context *c, const mm3d_cloud *in, const mm3d_outlier_options &o, mm3d_outlier_stats *stats) const override
  {
    return remove_outliers_statistical(c, in, o.mean_k, o.stddev_mult, stats);
  }
};
const OutliersStatistical g_statistical;

bool options_ok(const mm3d_outlier_options *o)
{
  if (!o || (o->method != MM3D_OUTLIERS_RADIUS && o->method != MM3D_OUTLIERS_STATISTICAL)) return false;
  return sor_args_ok(o->mean_k, o->stddev_mult);
}

}  // namespace

}  // namespace mm3d

using namespace mm3d;

extern "C" {

int mm3d_knn_mean_distances(mm3d_ctx *ctx, const mm3d_cloud *points, int mean_k, double *out, size_t capacity)
{
  if (!ctx || !points || !out || !sor_args_ok(mean_k, 0.0) || points->n >= ((size_t)1 << 31)) return MM3D_EINVAL;
  if (capacity < points->n) return MM3D_ECAPACITY;
  if (points->n == 0) return MM3D_OK;
  return guarded(ctx, [&] {
    DevBuf<double> d(ctx, points->n);
    DevBuf<int> list;
    (void)sor_mean_distances(ctx, points, mean_k, d.get(), list);
    MM3D_HIP(hipMemcpyAsync(out, d.get(), points->n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
  });
}

int mm3d_remove_outliers_statistical(mm3d_ctx *ctx, const mm3d_cloud *in, int mean_k, double stddev_mult, mm3d_cloud **out)
{
  if (!ctx || !in || !out) return MM3D_EINVAL;
  *out = nullptr;
  if (!sor_args_ok(mean_k, stddev_mult) || in->n >= ((size_t)1 << 31)) return MM3D_EINVAL;
  return guarded(ctx, [&] { *out = remove_outliers_statistical(ctx, in, mean_k, stddev_mult, &ctx->last_outlier_stats); });
}

int mm3d_set_outlier_filter(mm3d_ctx *ctx, const mm3d_outlier_options *options)
{
  if (!ctx || !options_ok(options)) return MM3D_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the filter changes)
  return select_stage(ctx, Stage::Outliers, [&](StageSelection &s) {
    s.outlier_options = *options;
    s.outliers = stage_active(Stage::Outliers, s) ? &g_statistical : nullptr;
  });
}

int mm3d_get_outlier_filter(const mm3d_ctx *ctx, mm3d_outlier_options *options)
{
  if (!ctx || !options) return MM3D_EINVAL;
  *options = ctx->sel.outlier_options;
  return MM3D_OK;
}

int mm3d_last_outlier_stats(const mm3d_ctx *ctx, mm3d_outlier_stats *stats)
{
  if (!ctx || !stats) return MM3D_EINVAL;
  *stats = ctx->last_outlier_stats;
  return MM3D_OK;
}

void mm3d_debug_outlier_search(long long out[3], int reset)
{
  for (int i = 0; i < 3; ++i) {
    if (out) out[i] = g_sor_search[i].load();
    if (reset) g_sor_search[i] = 0;
  }
}

}  // extern "C"

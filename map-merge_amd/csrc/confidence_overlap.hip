// confidence_overlap.hip -- the overlap confidence, the opt-in alternative to a pair record's 1 / transformScore
// (mm3d_set_confidence; include/mm3d.h states the rule to the operation).  A two-way voxel agreement of the two maps under the
// pair's transform: every point of one map that falls where the other map has looked asks whether the other map has a point
// within one voxel.  No search: one index computation, one byte load and one word load per point.  Every count is an integer
// sum, so the result depends on neither launch shape, batch nor stream count.  Not a reference stage, no PCL counterpart
// (audit row 16d).
//
// The table of a map (ovl_build_table), no host wait beyond the cloud's cached bounding box:
//   (fill)         occ words and view-cell counts to zero
//   k_ovl_mark     a lane per point: a 64-bit atomicOr of the voxel's bit into its brick's occ word, an integer atomicAdd on
//                  its view cell's count -- integer atomics only, so the table does not depend on the launch
//   k_ovl_dilate   a thread per brick: the brick and its 26 neighbours, dilated by one voxel along i, then j, then k -- shifts
//                  and masks inside the word plus the carries from the neighbours' faces (the edges and corners arrive through
//                  the separable passes); bricks outside the box read as 0
//   k_ovl_view     a thread per view cell: count >= min_points, ORed over the 27 cells around it under view_margin = 1
// The score of a batch (ovl_count): one launch, blockIdx.y = 2 * pair + direction, a lane per point of the cloud's Hilbert
// copy (a wave's lanes land in a few bricks); ballots and popcounts per wave, LDS per block, ONE atomic per block and counter;
// one host wait brings the batch's counts and the host forms the confidence.
#include <cmath>
#include <cstring>

#include "capi_guard.hpp"
#include "drivers.hpp"
#include "lattice.hpp"
#include "map_kept.hpp"

namespace mm3d {

namespace {

// include/mm3d.h: at most 2^24 words per table, and voxel indices below 2^30 in magnitude
constexpr double kOvlMaxWords = 16777216.0;
constexpr float kOvlIndexLimit = 1073741824.0f;
// mm3d_set_confidence with voxel = 0: the voxel side is params.resolution times this
constexpr double kOvlDefaultMultiple = 2.0;

// the two dense boxes of a table: bricks and view cells, minimum and extent per axis
struct OvlBox { int b0[3], nb[3], c0[3], nc[3]; };

// bits of a brick word whose i (j, k) is 0 or 3: what crosses into the neighbouring brick when the word is shifted
constexpr unsigned long long kI0 = 0x1111111111111111ull, kI3 = 0x8888888888888888ull;
constexpr unsigned long long kJ0 = 0x000F000F000F000Full, kJ3 = 0xF000F000F000F000ull;
constexpr unsigned long long kK0 = 0x000000000000FFFFull, kK3 = 0xFFFF000000000000ull;

__global__ void __launch_bounds__(256)
k_ovl_mark(const float4 *__restrict__ pts, int n, float inv, OvlBox box, unsigned long long *__restrict__ occ, int *__restrict__ cnt)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) return;
  const float f[3] = {lattice_index(p.x, inv), lattice_index(p.y, inv), lattice_index(p.z, inv)};
  int v[3], b[3], c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!(fabsf(f[a]) < kOvlIndexLimit)) return;          // (the host refused such a cloud: nothing is read of this table)
    v[a] = (int)f[a];
    b[a] = (v[a] >> 2) - box.b0[a];
    c[a] = (v[a] >> 3) - box.c0[a];
    // every finite point lies inside the boxes made from the cloud's bounding box; a point that does not is not written
    if ((unsigned)b[a] >= (unsigned)box.nb[a] || (unsigned)c[a] >= (unsigned)box.nc[a]) return;
  }
  const size_t word = ((size_t)b[0] * box.nb[1] + b[1]) * box.nb[2] + b[2];
  const int bit = (v[0] & 3) | ((v[1] & 3) << 2) | ((v[2] & 3) << 4);
  atomicOr(&occ[word], 1ull << bit);
  atomicAdd(&cnt[((size_t)c[0] * box.nc[1] + c[1]) * box.nc[2] + c[2]], 1);
}

// brick (i, j, k) of the occ words, counted from the box's minimum; 0 outside the box
__device__ __forceinline__ unsigned long long ovl_brick(const unsigned long long *__restrict__ occ, const OvlBox &box, int i, int j, int k)
{
  if ((unsigned)i >= (unsigned)box.nb[0] || (unsigned)j >= (unsigned)box.nb[1] || (unsigned)k >= (unsigned)box.nb[2]) return 0ull;
  return occ[((size_t)i * box.nb[1] + j) * box.nb[2] + k];
}
// one axis of the dilation: the word's own bits moved one step either way inside the brick, plus the face that the brick
// below (m) and the brick above (p) push across the boundary.  step = 1 / 4 / 16 bit positions for i / j / k.
__device__ __forceinline__ unsigned long long ovl_dilate_axis(unsigned long long m, unsigned long long w, unsigned long long p,
                                                              unsigned long long lo, unsigned long long hi, int step)
{
  return w | ((w & ~hi) << step) | ((w & ~lo) >> step) | ((m & hi) >> (3 * step)) | ((p & lo) << (3 * step));
}

__global__ void __launch_bounds__(256)
k_ovl_dilate(const unsigned long long *__restrict__ occ, OvlBox box, unsigned long long *__restrict__ near)
{
  const size_t words = (size_t)box.nb[0] * box.nb[1] * box.nb[2];
  const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= words) return;
  const int bk = (int)(w % (size_t)box.nb[2]), bj = (int)(w / (size_t)box.nb[2] % (size_t)box.nb[1]),
            bi = (int)(w / ((size_t)box.nb[2] * box.nb[1]));
  unsigned long long y[3];
#pragma unroll
  for (int dk = -1; dk <= 1; ++dk) {
    unsigned long long x[3];
#pragma unroll
    for (int dj = -1; dj <= 1; ++dj)
      x[dj + 1] = ovl_dilate_axis(ovl_brick(occ, box, bi - 1, bj + dj, bk + dk), ovl_brick(occ, box, bi, bj + dj, bk + dk),
                                  ovl_brick(occ, box, bi + 1, bj + dj, bk + dk), kI0, kI3, 1);
    y[dk + 1] = ovl_dilate_axis(x[0], x[1], x[2], kJ0, kJ3, 4);
  }
  near[w] = ovl_dilate_axis(y[0], y[1], y[2], kK0, kK3, 16);
}

__global__ void __launch_bounds__(256)
k_ovl_view(const int *__restrict__ cnt, OvlBox box, int min_points, int margin, unsigned char *__restrict__ view)
{
  const size_t cells = (size_t)box.nc[0] * box.nc[1] * box.nc[2];
  const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= cells) return;
  const int ck = (int)(w % (size_t)box.nc[2]), cj = (int)(w / (size_t)box.nc[2] % (size_t)box.nc[1]),
            ci = (int)(w / ((size_t)box.nc[2] * box.nc[1]));
  bool seen = false;
  for (int di = -margin; di <= margin; ++di)
    for (int dj = -margin; dj <= margin; ++dj)
      for (int dk = -margin; dk <= margin; ++dk) {
        const int i = ci + di, j = cj + dj, k = ck + dk;
        if ((unsigned)i >= (unsigned)box.nc[0] || (unsigned)j >= (unsigned)box.nc[1] || (unsigned)k >= (unsigned)box.nc[2]) continue;
        seen = seen || cnt[((size_t)i * box.nc[1] + j) * box.nc[2] + k] >= min_points;
      }
  view[w] = seen ? 1 : 0;
}

// one direction of one pair: the points of A (Hilbert copy, all finite), the matrix that takes them into B's frame, B's table
struct OvlJob {
  const float4 *pts;
  int n;
  float inv;
  float M[16];
  const unsigned long long *near;
  const unsigned char *view;
  OvlBox box;
  unsigned long long *counts;     // {in, hit}
};

__global__ void __launch_bounds__(256) k_ovl_score(const OvlJob *__restrict__ jobs)
{
  const OvlJob &J = jobs[blockIdx.y];
  const int n = J.n;
  if ((int)(blockIdx.x * 256u) >= n) return;                   // (block-uniform)
  const float inv = J.inv;
  const OvlBox &box = J.box;
  unsigned in_w = 0, hit_w = 0;                                // wave-uniform
  for (int base = blockIdx.x * 256; base < n; base += gridDim.x * 256) {
    const int i = base + (int)threadIdx.x;
    bool in = false, hit = false;
    if (i < n) {
      const float4 p = J.pts[i];
      const float3 s = xform(J.M, p.x, p.y, p.z);
      const float f[3] = {__fmul_rn(s.x, inv), __fmul_rn(s.y, inv), __fmul_rn(s.z, inv)};
      // in float, before any conversion: a NaN, an infinity and an index beyond the limit all fail this
      if (fabsf(f[0]) < kOvlIndexLimit && fabsf(f[1]) < kOvlIndexLimit && fabsf(f[2]) < kOvlIndexLimit) {
        const int v[3] = {(int)floorf(f[0]), (int)floorf(f[1]), (int)floorf(f[2])};
        const int c[3] = {(v[0] >> 3) - box.c0[0], (v[1] >> 3) - box.c0[1], (v[2] >> 3) - box.c0[2]};
        if ((unsigned)c[0] < (unsigned)box.nc[0] && (unsigned)c[1] < (unsigned)box.nc[1] && (unsigned)c[2] < (unsigned)box.nc[2])
          in = J.view[((size_t)c[0] * box.nc[1] + c[1]) * box.nc[2] + c[2]] != 0;
        if (in) {
          const int b[3] = {(v[0] >> 2) - box.b0[0], (v[1] >> 2) - box.b0[1], (v[2] >> 2) - box.b0[2]};
          if ((unsigned)b[0] < (unsigned)box.nb[0] && (unsigned)b[1] < (unsigned)box.nb[1] && (unsigned)b[2] < (unsigned)box.nb[2]) {
            const unsigned long long word = J.near[((size_t)b[0] * box.nb[1] + b[1]) * box.nb[2] + b[2]];
            hit = (word >> ((v[0] & 3) | ((v[1] & 3) << 2) | ((v[2] & 3) << 4))) & 1ull;
          }
        }
      }
    }
    in_w += (unsigned)__popcll(__ballot(in));
    hit_w += (unsigned)__popcll(__ballot(hit));
  }
  __shared__ unsigned s_in[4], s_hit[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_in[wave] = in_w; s_hit[wave] = hit_w; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long a = (unsigned long long)s_in[0] + s_in[1] + s_in[2] + s_in[3];
    const unsigned long long h = (unsigned long long)s_hit[0] + s_hit[1] + s_hit[2] + s_hit[3];
    if (a) atomicAdd(&J.counts[0], a);
    if (h) atomicAdd(&J.counts[1], h);
  }
}

// everything but the voxel's "0 = default", which only mm3d_set_confidence admits
bool ovl_options_ok(const mm3d_confidence_options *o)
{
  if (!o || (o->method != MM3D_CONFIDENCE_REFERENCE && o->method != MM3D_CONFIDENCE_OVERLAP)) return false;
  if (o->min_points < 1) return false;
  if (o->view_margin != 0 && o->view_margin != 1) return false;
  return o->min_overlap >= 0.0 && o->min_overlap <= 1.0;      // (false for NaN)
}

size_t ovl_words(const OvlBox &b) { return (size_t)b.nb[0] * b.nb[1] * b.nb[2]; }
size_t ovl_cells(const OvlBox &b) { return (size_t)b.nc[0] * b.nc[1] * b.nc[2]; }
OvlBox ovl_box(const OverlapTable &t)
{
  OvlBox b;
  for (int a = 0; a < 3; ++a) { b.b0[a] = t.b0[a]; b.nb[a] = t.nb[a]; b.c0[a] = t.c0[a]; b.nc[a] = t.nc[a]; }
  return b;
}

// The table of `cl` at the given options: enqueued on c's stream (the caller waits before anybody else reads it).  The limits
// are decided here, on the host, from the cloud's cached bounding box: floorf(x * inv) is monotone, so the voxels of the box's
// corners bound every point's.
std::unique_ptr<OverlapTable> ovl_build_table(Context *c, const mm3d_cloud *cl, double voxel, int min_points, int view_margin)
{
  MM3D_REQUIRE(lattice_side_ok(voxel), "overlap confidence: the voxel must be positive and finite, as a float and its reciprocal too");
  MM3D_REQUIRE(cl->n < ((size_t)1 << 31), "overlap confidence: more than 2^31 - 1 points");
  std::unique_ptr<OverlapTable> t(new OverlapTable());
  t->voxel = voxel; t->min_points = min_points; t->view_margin = view_margin;
  t->inv = 1.0f / (float)voxel;
  cloud_bbox(c, const_cast<mm3d_cloud *>(cl));
  t->n_finite = cl->n_finite;
  if (cl->n_finite == 0) return t;                       // every lookup reads 0
  double words = 1.0;
  for (int a = 0; a < 3; ++a) {
    const float lo = lattice_index(cl->bmin[a], t->inv), hi = lattice_index(cl->bmax[a], t->inv);
    if (!(std::fabs(lo) < kOvlIndexLimit) || !(std::fabs(hi) < kOvlIndexLimit))
      throw Error(MM3D_EUNSUPPORTED, "overlap confidence: a voxel index of magnitude 2^30 or more at this voxel size");
    const int v_lo = (int)lo, v_hi = (int)hi;
    t->b0[a] = (v_lo - 1) >> 2;
    t->nb[a] = ((v_hi + 1) >> 2) - t->b0[a] + 1;
    const int b1 = t->b0[a] + t->nb[a] - 1;
    t->c0[a] = (t->b0[a] >> 1) - view_margin;
    t->nc[a] = ((b1 >> 1) + view_margin) - t->c0[a] + 1;
    words *= (double)t->nb[a];
  }
  if (!(words <= kOvlMaxWords)) {
    for (int a = 0; a < 3; ++a) t->nb[a] = t->nc[a] = 0;
    throw Error(MM3D_EUNSUPPORTED, "overlap confidence: the brick box of the points needs more than 2^24 words at this voxel size");
  }
  const OvlBox box = ovl_box(*t);
  const size_t nw = ovl_words(box), ncell = ovl_cells(box);
  const int n = (int)cl->n;
  t->near = DevBuf<unsigned long long>(c, nw);
  t->view = DevBuf<unsigned char>(c, ncell);
  DevBuf<unsigned long long> occ(c, nw);
  DevBuf<int> cnt(c, ncell);
  MM3D_HIP(hipMemsetAsync(occ.get(), 0, nw * sizeof(unsigned long long), c->stream));
  MM3D_HIP(hipMemsetAsync(cnt.get(), 0, ncell * sizeof(int), c->stream));
  MM3D_LAUNCH(c, "ovl_mark", n * 28.0, k_ovl_mark, dim3(div_up((size_t)n, 256)), dim3(256), 0, cl->pts.get(), n, t->inv, box, occ.get(), cnt.get());
  MM3D_LAUNCH(c, "ovl_dilate", nw * 16.0, k_ovl_dilate, dim3(div_up(nw, 256)), dim3(256), 0, (const unsigned long long *)occ.get(), box,
              t->near.get());
  MM3D_LAUNCH(c, "ovl_view", ncell * 5.0, k_ovl_view, dim3(div_up(ncell, 256)), dim3(256), 0, (const int *)cnt.get(), box, min_points,
              view_margin, t->view.get());
  c->settle();                                            // (the scratch words and counts go back to the pool)
  return t;
}

// the rigid inverse of the rule: R' = R^T, t' = -R^T t in double from T's float entries, rounded to float once
void ovl_inverse(const float T[16], float out[16])
{
  for (int r = 0; r < 3; ++r) {
    for (int col = 0; col < 3; ++col) out[col * 4 + r] = T[r * 4 + col];
    const double t = -(((double)T[r * 4 + 0] * (double)T[12] + (double)T[r * 4 + 1] * (double)T[13]) + (double)T[r * 4 + 2] * (double)T[14]);
    out[12 + r] = (float)t;
    out[r * 4 + 3] = 0.0f;
  }
  out[15] = 1.0f;
}

// a T with a non-finite entry, or the all-zero matrix, scores nothing
bool ovl_transform_ok(const float T[16])
{
  bool any = false;
  for (int i = 0; i < 16; ++i) {
    if (!std::isfinite(T[i])) return false;
    any = any || T[i] != 0.0f;
  }
  return any;
}

struct OvlSide { const mm3d_cloud *cloud; const OverlapTable *table; };
// The counts of a batch of pairs, both directions each, and their confidences: one launch, one wait.
void ovl_count(Context *c, const OvlSide *src, const OvlSide *tgt, const float *const *T, size_t n, double min_overlap, mm3d_overlap_stats *out)
{
  if (n == 0) return;
  const size_t n_jobs = 2 * n;
  OvlJob *hj = (OvlJob *)c->pin(sizeof(OvlJob) * n_jobs + 64);
  DevBuf<OvlJob> d_jobs(c, n_jobs);
  DevBuf<unsigned long long> d_counts(c, 2 * n_jobs);
  int max_n = 0;
  double bytes = 0.0;
  for (size_t i = 0; i < n; ++i) {
    const bool ok = ovl_transform_ok(T[i]);
    for (int dir = 0; dir < 2; ++dir) {
      const OvlSide &A = dir == 0 ? src[i] : tgt[i], &B = dir == 0 ? tgt[i] : src[i];
      OvlJob J;
      std::memset(&J, 0, sizeof(J));
      if (ok && A.cloud->n && B.table->n_finite) {
        cloud_hilbert(c, A.cloud);                        // (cached on the cloud: the ICP's source order)
        J.pts = A.cloud->hil_pts.get();
        J.n = (int)A.cloud->n_finite;
      }
      J.inv = B.table->inv;
      if (dir == 0) std::memcpy(J.M, T[i], sizeof(J.M));
      else if (ok) ovl_inverse(T[i], J.M);
      J.near = B.table->near.get();
      J.view = B.table->view.get();
      J.box = ovl_box(*B.table);
      J.counts = d_counts.get() + 2 * (2 * i + dir);
      hj[2 * i + dir] = J;
      max_n = std::max(max_n, J.n);
      bytes += J.n * 25.0;
    }
  }
  unsigned long long *hc = (unsigned long long *)c->pin(sizeof(unsigned long long) * 2 * n_jobs + 64);
  std::memset(hc, 0, sizeof(unsigned long long) * 2 * n_jobs);
  if (max_n > 0) {
    MM3D_HIP(hipMemcpyAsync(d_jobs.get(), hj, sizeof(OvlJob) * n_jobs, hipMemcpyHostToDevice, c->stream));
    MM3D_HIP(hipMemsetAsync(d_counts.get(), 0, sizeof(unsigned long long) * 2 * n_jobs, c->stream));
    const unsigned grid_x = std::min<unsigned>(div_up((size_t)max_n, 256), 2048);
    MM3D_LAUNCH(c, "ovl_score", bytes, k_ovl_score, dim3(grid_x, (unsigned)n_jobs), dim3(256), 0, (const OvlJob *)d_jobs.get());
    MM3D_HIP(hipMemcpyAsync(hc, d_counts.get(), sizeof(unsigned long long) * 2 * n_jobs, hipMemcpyDeviceToHost, c->stream));
    c->sync();                                            // the one wait: the batch's counts
  }
  for (size_t i = 0; i < n; ++i) {
    mm3d_overlap_stats s;
    s.points_st = (long long)src[i].table->n_finite; s.in_st = (long long)hc[4 * i + 0]; s.hit_st = (long long)hc[4 * i + 1];
    s.points_ts = (long long)tgt[i].table->n_finite; s.in_ts = (long long)hc[4 * i + 2]; s.hit_ts = (long long)hc[4 * i + 3];
    s.confidence = 0.0;
    if (s.in_st != 0 && s.in_ts != 0 && !((double)s.in_st < min_overlap * (double)s.points_st) &&
        !((double)s.in_ts < min_overlap * (double)s.points_ts))
      s.confidence = std::min((double)s.hit_st / (double)s.in_st, (double)s.hit_ts / (double)s.in_ts);
    out[i] = s;
  }
}

struct ConfidenceOverlap final : ConfidenceMethodBase {
  // the map's table at the context's options (map_kept.hpp)
  const OverlapTable *table(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p) const
  {
    const mm3d_confidence_options &o = ctx->sel.confidence_options;
    const double voxel = o.voxel > 0.0 ? o.voxel : kOvlDefaultMultiple * p->resolution;
    return map_kept(
        ctx, m, &mm3d_map::overlap,
        [&](const OverlapTable &h) { return h.voxel == voxel && h.min_points == o.min_points && h.view_margin == o.view_margin; },
        [&] { return ovl_build_table(ctx, m->points, voxel, o.min_points, o.view_margin); });
  }
  void prepare(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p) const override { (void)table(ctx, m, p); }
  void score(mm3d_ctx *ctx, ConfidencePair *pairs, size_t n, const mm3d_params *p, mm3d_overlap_stats *stats) const override
  {
    std::vector<OvlSide> src(n), tgt(n);
    std::vector<const float *> T(n);
    for (size_t i = 0; i < n; ++i) {
      src[i] = OvlSide{pairs[i].s->points, table(ctx, pairs[i].s, p)};
      tgt[i] = OvlSide{pairs[i].t->points, table(ctx, pairs[i].t, p)};
      T[i] = pairs[i].T;
    }
    std::vector<mm3d_overlap_stats> out(n);
    ovl_count(ctx, src.data(), tgt.data(), T.data(), n, ctx->sel.confidence_options.min_overlap, out.data());
    for (size_t i = 0; i < n; ++i) pairs[i].confidence = out[i].confidence;
    if (stats && n) *stats = out[n - 1];
  }
};
const ConfidenceOverlap g_overlap;

}  // namespace

}  // namespace mm3d

using namespace mm3d;

extern "C" {

int mm3d_set_confidence(mm3d_ctx *ctx, const mm3d_confidence_options *options)
{
  if (!ctx || !ovl_options_ok(options)) return MM3D_EINVAL;
  if (options->voxel != 0.0 && !lattice_side_ok(options->voxel)) return MM3D_EINVAL;     // (also catches NaN)
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the method changes)
  return select_stage(ctx, Stage::Confidence, [&](StageSelection &s) {
    s.confidence_options = *options;
    s.confidence = stage_active(Stage::Confidence, s) ? &g_overlap : nullptr;
  });
}

int mm3d_get_confidence(const mm3d_ctx *ctx, mm3d_confidence_options *options)
{
  if (!ctx || !options) return MM3D_EINVAL;
  *options = ctx->sel.confidence_options;
  return MM3D_OK;
}

int mm3d_last_confidence_stats(const mm3d_ctx *ctx, mm3d_overlap_stats *stats)
{
  if (!ctx || !stats) return MM3D_EINVAL;
  *stats = ctx->last_confidence_stats;
  return MM3D_OK;
}

int mm3d_transform_overlap(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target, const float T[16],
                           const mm3d_confidence_options *options, mm3d_overlap_stats *stats)
{
  if (!ctx || !source || !target || !T || !stats || !ovl_options_ok(options) || !lattice_side_ok(options->voxel)) return MM3D_EINVAL;
  std::memset(stats, 0, sizeof(*stats));
  return guarded(ctx, [&] {
    // (both tables are decided -- and may be refused -- before either is read)
    std::unique_ptr<OverlapTable> ts = ovl_build_table(ctx, source, options->voxel, options->min_points, options->view_margin);
    std::unique_ptr<OverlapTable> tt = ovl_build_table(ctx, target, options->voxel, options->min_points, options->view_margin);
    const OvlSide s{source, ts.get()}, t{target, tt.get()};
    ovl_count(ctx, &s, &t, &T, 1, options->min_overlap, stats);
    ctx->last_confidence_stats = *stats;
    ctx->sync();                                    // (the throw-away tables go back to the pool behind their last reader)
  });
}

int mm3d_debug_overlap_table(mm3d_ctx *ctx, const mm3d_cloud *cloud, const mm3d_confidence_options *options, int box[12],
                             unsigned long long *words, size_t word_cap, unsigned char *view, size_t view_cap)
{
  if (!ctx || !cloud || !box || !ovl_options_ok(options) || !lattice_side_ok(options->voxel)) return MM3D_EINVAL;
  if ((word_cap && !words) || (view_cap && !view)) return MM3D_EINVAL;
  std::memset(box, 0, 12 * sizeof(int));
  return guarded(ctx, [&] {
    std::unique_ptr<OverlapTable> t = ovl_build_table(ctx, cloud, options->voxel, options->min_points, options->view_margin);
    for (int a = 0; a < 3; ++a) { box[a] = t->b0[a]; box[3 + a] = t->nb[a]; box[6 + a] = t->c0[a]; box[9 + a] = t->nc[a]; }
    const size_t nw = t->near.size(), ncell = t->view.size();
    if (nw && word_cap >= nw) MM3D_HIP(hipMemcpyAsync(words, t->near.get(), nw * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    if (ncell && view_cap >= ncell) MM3D_HIP(hipMemcpyAsync(view, t->view.get(), ncell, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
  });
}

}  // extern "C"

// clusters_euclidean.hip -- Euclidean clustering on gfx950: the connected components of the graph that joins the points of a
// cloud lying within a tolerance of each other, and the filter that drops the components too small to be structure
// (mm3d_cluster_labels, mm3d_remove_small_clusters, mm3d_set_cluster_filter; include/mm3d.h states the rule to the operation).
// Not a reference stage.
//
// One pass family per cloud, one host wait (the compaction's):
//   cloud_grid     the library's cell-sorted grid at a cell just above the tolerance (radius_grid.hpp: radius_cell), so that a point's neighbours
//                  lie in its 3 x 3 x 3 cells; where the cell had to grow, in as many cells as cover the tolerance (radius_reach)
//   k_cc_init      parent[i] = i for a valid record, -1 for an invalid one: a forest over the ORIGINAL record indices
//   k_cc_hook      a lane per cell-sorted point i walks the candidates of its box of cells; for an adjacent candidate of larger
//                  index it finds both roots and hangs the larger under the smaller with a compare-and-swap.  A parent is
//                  always below its child, so a tree's root is its smallest member, whoever won which swap
//   k_cc_flatten   every record's label is its root; the roots' sizes by integer adds, one per (wave, root) at the most and far
//                  fewer for the root most records share, whose count a wave carries over its slices of the records
//   k_cc_roots     the number of clusters, of clusters of at least min_size, and the arg-max over (size, smaller label) as an
//                  atomic max on a packed 64-bit key, folded per block first -- all integer, so order-free
//   k_cc_keep      a lane per record: its cluster's size against min_size, or its label against the arg-max's
//   compact        grid.hip::cloud_of_kept, behind whose wait the counts come back too
// No wave waits for another: the walk towards a root only descends, a failed swap means that another lane hooked that root, and
// every other loop is counted.  One launch of k_cc_hook serves any topology -- a chain through hundreds of cells like a blob in
// one -- so there are no rounds for the host to bound.
#include <cmath>
#include <cstring>

#include "capi_guard.hpp"
#include "drivers.hpp"
#include "device_util.hpp"
#include "radius_grid.hpp"

namespace mm3d {

namespace {

constexpr int kCcThreads = 256;
constexpr int kCcSweepBlocks = 512;           // k_cc_flatten, k_cc_roots: this many blocks stride over the records (2048 waves)

// The forest is read and written by lanes of every workgroup at once: relaxed device-scope accesses, which the compiler neither
// caches in a register nor tears.  A stale value is harmless by construction -- every value a word ever held is an ancestor of
// its record, and only the compare-and-swap decides.
__device__ __forceinline__ int cc_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_store(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x's tree, halving the path on the way: a record is pointed at its grandparent, an ancestor like any other.  Only
// records that have a parent are written, and such a record never becomes a root again, so no store here meets the swap of
// cc_unite.  parent[y] < y for every y that is not a root: the walk strictly descends, at most x steps.
__device__ __forceinline__ int cc_find(int *parent, int x)
{
  int p = cc_load(parent + x);
  while (p != x) {
    const int gp = cc_load(parent + p);
    if (gp != p) cc_store(parent + x, gp);
    x = p;
    p = gp;
  }
  return x;
}

// One tree out of a's and b's; returns a record of it that is at most a.  Lock-free: the swap fails only when another lane
// has hooked that root in the meantime, after which the forest has one root fewer.
__device__ __forceinline__ int cc_unite(int *parent, int a, int b)
{
  for (;;) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return a;
    const int lo = min(a, b), hi = max(a, b);
    int seen = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return lo;
    a = lo;
    b = seen;                                         // (where hi points now: below hi)
  }
}

__global__ void __launch_bounds__(kCcThreads)
k_cc_init(const float4 *__restrict__ pts, int n, int *__restrict__ parent)
{
  const int i = blockIdx.x * kCcThreads + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  parent[i] = (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) ? i : -1;
}

// A lane per cell-sorted point.  Each adjacent pair is united once, by the lane of its smaller index.  `root` is a record of the
// lane's own tree, as near the root as the lane has seen: a candidate whose parent it already is needs nothing.
__global__ void __launch_bounds__(kCcThreads)
k_cc_hook(GridView g, int s /* cells to either side */, double tol2, int *__restrict__ parent)
{
  const unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
  const int j = (int)bid * kCcThreads + (int)threadIdx.x;
  if (j >= g.n) return;
  const float4 q = g.pts[j];
  const int i = __float_as_int(q.w);
  const int cx = clampi(cell_floor(q.x, g.minx, g.inv), 0, g.dx - 1);
  const int cy = clampi(cell_floor(q.y, g.miny, g.inv), 0, g.dy - 1);
  const int cz = clampi(cell_floor(q.z, g.minz, g.inv), 0, g.dz - 1);
  const int x0 = max(cx - s, 0), x1 = min(cx + s, g.dx - 1);
  const int y0 = max(cy - s, 0), y1 = min(cy + s, g.dy - 1);
  const int z0 = max(cz - s, 0), z1 = min(cz + s, g.dz - 1);
  int root = i;
  for (int z = z0; z <= z1; ++z)
    for (int y = y0; y <= y1; ++y) {
      const int row = (z * g.dy + y) * g.dx;
      const int beg = g.cell_start[row + x0], end = g.cell_start[row + x1 + 1];   // (a row of cells is one span of points)
      for (int k = beg; k < end; ++k) {
        const float4 p = g.pts[k];
        const int ic = __float_as_int(p.w);
        if (ic <= i) continue;
        const float d2 = dist2(q.x, q.y, q.z, p.x, p.y, p.z);
        if (!((double)d2 <= tol2)) continue;
        if (cc_load(parent + ic) == root) continue;
        root = cc_unite(parent, root, ic);
      }
    }
}

// labels = the forest, flattened in place (a record pointed at its root meanwhile is still pointed at an ancestor).  No hook
// runs beside this kernel, so the roots are final.  The lanes of a wave that share a root add their number to its size once;
// and since one word takes about 90 atomics a microsecond from the whole chip, and most records of a map share ONE root, a
// wave goes over several slices of the records (kCcSweepBlocks blocks stride over them) and carries the count of the root
// its slices begin with in a register: what reaches the large cluster's word is one add per wave and change of root, not one
// per 64 records.  Integer sums: whatever is carried or added when, the sizes are the same.
__global__ void __launch_bounds__(kCcThreads)
k_cc_flatten(int *__restrict__ parent, int n, int *__restrict__ size)
{
  const int lane = threadIdx.x & (kWave - 1);
  int cur = -1, carried = 0;                                       // (wave-uniform)
  for (long long base = (long long)blockIdx.x * kCcThreads; base < n; base += (long long)gridDim.x * kCcThreads) {   // (block-uniform; counted)
    const long long i = base + threadIdx.x;
    int r = -1;
    if (i < n) {
      const int first = cc_load(parent + i);
      if (first >= 0) {
        int x = (int)i, p = first;
        while (p != x) { x = p; p = cc_load(parent + x); }        // (strictly descending)
        r = x;
        if (r != first) cc_store(parent + i, r);
      }
    }
    unsigned long long todo = ballot(r >= 0);
    bool head = true;
    while (todo) {                                                 // (wave-uniform; at most 64 turns)
      const int lead = __ffsll((long long)todo) - 1;
      const int rl = __builtin_amdgcn_readlane(r, lead);
      const unsigned long long same = ballot(r == rl);
      const int c = __popcll(same);
      if (rl == cur) carried += c;
      else if (head) {
        if (carried && lane == 0) atomicAdd(size + cur, carried);
        cur = rl;
        carried = c;
      } else if (lane == lead) atomicAdd(size + rl, c);
      head = false;
      todo &= ~same;
    }
  }
  if (carried && lane == 0) atomicAdd(size + cur, carried);
}

// ctl[0] clusters, ctl[1] clusters of at least min_size, ctl[2] max over the roots of (size << 32 | ~label): the largest
// cluster, the smallest label among equals; 0 = no cluster.  A map of random surface samples has thousands of roots: a lane
// keeps its own counts over its slices, the wave and the block fold them, and a block issues its three atomics once.
__global__ void __launch_bounds__(kCcThreads)
k_cc_roots(const int *__restrict__ labels, const int *__restrict__ size, int n, int min_size, unsigned long long *__restrict__ ctl)
{
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  int roots = 0, big = 0;
  unsigned long long key = 0ull;
  for (long long i = (long long)blockIdx.x * kCcThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kCcThreads) {   // (counted)
    if (labels[i] != (int)i) continue;
    const int sz = size[i];
    const unsigned long long k = ((unsigned long long)(unsigned)sz << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
    ++roots;
    big += sz >= min_size ? 1 : 0;
    key = k > key ? k : key;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    roots += __shfl_xor(roots, o, kWave);
    big += __shfl_xor(big, o, kWave);
    const unsigned long long other = __shfl_xor(key, o, kWave);
    key = other > key ? other : key;
  }
  __shared__ int s_roots[kCcThreads / kWave], s_big[kCcThreads / kWave];
  __shared__ unsigned long long s_key[kCcThreads / kWave];
  if (lane == 0) { s_roots[wave] = roots; s_big[wave] = big; s_key[wave] = key; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kCcThreads / kWave; ++w) {
      roots += s_roots[w];
      big += s_big[w];
      key = s_key[w] > key ? s_key[w] : key;
    }
    if (roots) {
      atomicAdd(&ctl[0], (unsigned long long)roots);
      if (big) atomicAdd(&ctl[1], (unsigned long long)big);
      atomicMax(&ctl[2], key);
    }
  }
}

__global__ void __launch_bounds__(kCcThreads)
k_cc_keep(const int *__restrict__ labels, const int *__restrict__ size, int n, int method, int min_size, const unsigned long long *__restrict__ ctl,
          int *__restrict__ flags)
{
  const int i = blockIdx.x * kCcThreads + threadIdx.x;
  if (i >= n) return;
  const int l = labels[i];
  int keep = 0;
  if (l >= 0) {
    if (method == MM3D_CLUSTERS_MIN_SIZE) keep = size[l] >= min_size ? 1 : 0;
    else keep = (0xFFFFFFFFu - (unsigned)ctl[2]) == (unsigned)l ? 1 : 0;       // (a valid point exists, so ctl[2] != 0)
  }
  flags[i] = keep;
}

// ---------------------------------------------------------------- host
bool cc_tolerance_ok(double tolerance, bool zero_ok) { return std::isfinite(tolerance) && (tolerance > 0.0 || (zero_ok && tolerance == 0.0)); }
bool cc_method_ok(int method, bool off_ok) { return method == MM3D_CLUSTERS_MIN_SIZE || method == MM3D_CLUSTERS_LARGEST || (off_ok && method == MM3D_CLUSTERS_OFF); }

struct CcWork {
  DevBuf<int> labels, size;               // [n] each: the flattened forest; a root's slot holds its cluster's size
  DevBuf<unsigned long long> ctl;         // k_cc_roots' three words
};

// Steps 1 - 3 of the rule on the device, nothing waited for beyond the cloud's box and its grid.  in->n > 0.
void cc_components(Context *c, const mm3d_cloud *in_, double tolerance, int min_size, CcWork &w)
{
  auto *in = const_cast<mm3d_cloud *>(in_);
  const int n = (int)in->n;
  const dim3 blocks(div_up((size_t)n, kCcThreads)), threads(kCcThreads);
  w.labels = DevBuf<int>(c, (size_t)n);
  w.size = DevBuf<int>(c, (size_t)n);
  w.ctl = DevBuf<unsigned long long>(c, 8);
  MM3D_HIP(hipMemsetAsync(w.size.get(), 0, (size_t)n * sizeof(int), c->stream));
  MM3D_HIP(hipMemsetAsync(w.ctl.get(), 0, 8 * sizeof(unsigned long long), c->stream));
  MM3D_LAUNCH(c, "cc_init", n * 20.0, k_cc_init, blocks, threads, 0, in->pts.get(), n, w.labels.get());
  cloud_bbox(c, in);
  if (in->n_finite > 1) {
    const Grid &g = cloud_grid(c, in, radius_cell(in, tolerance));
    const int s = radius_reach(g, tolerance);
    MM3D_LAUNCH(c, "cc_hook", g.n * (16.0 + 8.0), k_cc_hook, dim3(div_up((size_t)g.n, kCcThreads)), threads, 0, g.view(), s, tolerance * tolerance,
                w.labels.get());
  }
  const dim3 sweep(std::min<unsigned>(blocks.x, kCcSweepBlocks));
  MM3D_LAUNCH(c, "cc_flatten", n * 12.0, k_cc_flatten, sweep, threads, 0, w.labels.get(), n, w.size.get());
  MM3D_LAUNCH(c, "cc_roots", n * 8.0, k_cc_roots, sweep, threads, 0, (const int *)w.labels.get(), (const int *)w.size.get(), n, min_size, w.ctl.get());
}

void cc_stats(const mm3d_cloud *in, const unsigned long long *h, int method, long long kept, mm3d_cluster_stats *st)
{
  st->points = (long long)in->n;
  st->valid = (long long)in->n_finite;
  st->kept = kept;
  st->clusters = (long long)h[0];
  st->kept_clusters = method == MM3D_CLUSTERS_OFF ? (long long)h[0] : method == MM3D_CLUSTERS_MIN_SIZE ? (long long)h[1] : (h[2] ? 1 : 0);
  st->largest = (long long)(h[2] >> 32);
}

mm3d_cloud *remove_small_clusters(Context *c, const mm3d_cloud *in, double tolerance, int method, int min_size, mm3d_cluster_stats *stats)
{
  MM3D_REQUIRE(cc_tolerance_ok(tolerance, false) && cc_method_ok(method, false) && min_size >= 1,
               "cluster filter: the tolerance must be finite and > 0, the method MIN_SIZE or LARGEST, min_size >= 1");
  MM3D_REQUIRE(in->n < ((size_t)1 << 31), "cluster filter: more than 2^31 - 1 points");
  const size_t n = in->n;
  if (n == 0) {
    if (stats) *stats = mm3d_cluster_stats{0, 0, 0, 0, 0, 0};
    return cloud_from_device(c, DevBuf<float4>(c, 0), 0);
  }
  CcWork w;
  cc_components(c, in, tolerance, min_size, w);
  DevBuf<int> keep(c, n + 1);
  MM3D_LAUNCH(c, "cc_keep", n * 12.0, k_cc_keep, dim3(div_up(n, kCcThreads)), dim3(kCcThreads), 0, (const int *)w.labels.get(), (const int *)w.size.get(),
              (int)n, method, min_size, (const unsigned long long *)w.ctl.get(), keep.get());
  unsigned long long *h = (unsigned long long *)c->pin(64);
  std::memset(h, 0, 64);
  MM3D_HIP(hipMemcpyAsync(h, w.ctl.get(), 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  size_t m = 0;
  mm3d_cloud *res = cloud_of_kept(c, in, keep.get(), true, &m);      // the one wait: count, box and the counts above (a subset of a voxel grid's centroids)
  if (stats) cc_stats(in, h, method, (long long)m, stats);
  return res;
}

struct ClustersEuclidean final : ClusterFilterBase {
  mm3d_cloud *filter(Context *c, const mm3d_cloud *in, const mm3d_cluster_options &o, double resolution, mm3d_cluster_stats *stats) const override
  {
    return remove_small_clusters(c, in, o.tolerance > 0.0 ? o.tolerance : 2.0 * resolution, o.method, o.min_size, stats);
  }
};
const ClustersEuclidean g_euclidean;

bool options_ok(const mm3d_cluster_options *o) { return o && cc_method_ok(o->method, true) && o->min_size >= 1 && cc_tolerance_ok(o->tolerance, true); }

}  // namespace

}  // namespace mm3d

using namespace mm3d;

extern "C" {

int mm3d_cluster_labels(mm3d_ctx *ctx, const mm3d_cloud *points, double tolerance, int *labels, size_t capacity, mm3d_cluster_stats *stats)
{
  if (!ctx || !points || !labels || !cc_tolerance_ok(tolerance, false) || points->n >= ((size_t)1 << 31) || capacity < points->n) return MM3D_EINVAL;
  if (points->n == 0) {
    if (stats) *stats = mm3d_cluster_stats{0, 0, 0, 0, 0, 0};
    return MM3D_OK;
  }
  return guarded(ctx, [&] {
    CcWork w;
    cc_components(ctx, points, tolerance, 1, w);
    unsigned long long *h = (unsigned long long *)ctx->pin(64);
    std::memset(h, 0, 64);
    MM3D_HIP(hipMemcpyAsync(h, w.ctl.get(), 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    MM3D_HIP(hipMemcpyAsync(labels, w.labels.get(), points->n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    if (stats) cc_stats(points, h, MM3D_CLUSTERS_OFF, (long long)points->n_finite, stats);
  });
}

int mm3d_remove_small_clusters(mm3d_ctx *ctx, const mm3d_cloud *in, double tolerance, int method, int min_size, mm3d_cloud **out)
{
  if (!ctx || !in || !out) return MM3D_EINVAL;
  *out = nullptr;
  if (!cc_tolerance_ok(tolerance, false) || !cc_method_ok(method, false) || min_size < 1 || in->n >= ((size_t)1 << 31)) return MM3D_EINVAL;
  return guarded(ctx, [&] { *out = remove_small_clusters(ctx, in, tolerance, method, min_size, &ctx->last_cluster_stats); });
}

int mm3d_set_cluster_filter(mm3d_ctx *ctx, const mm3d_cluster_options *options)
{
  if (!ctx || !options_ok(options)) return MM3D_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the filter changes)
  return select_stage(ctx, Stage::Clusters, [&](StageSelection &s) {
    s.cluster_options = *options;
    s.clusters = stage_active(Stage::Clusters, s) ? &g_euclidean : nullptr;
  });
}

int mm3d_get_cluster_filter(const mm3d_ctx *ctx, mm3d_cluster_options *options)
{
  if (!ctx || !options) return MM3D_EINVAL;
  *options = ctx->sel.cluster_options;
  return MM3D_OK;
}

int mm3d_last_cluster_stats(const mm3d_ctx *ctx, mm3d_cluster_stats *stats)
{
  if (!ctx || !stats) return MM3D_EINVAL;
  *stats = ctx->last_cluster_stats;
  return MM3D_OK;
}

}  // extern "C"

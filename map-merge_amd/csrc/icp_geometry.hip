// icp_geometry.hip -- what the geometric ICP rejectors read of a map, opt-in (mm3d_set_icp_geometry_rejection): the boundary flags
// of its points (Turk and Levoy 1994; PCL's BoundaryEstimation), the stage call mm3d_boundary_points, and the selection's
// setter and binder.  include/mm3d.h states the rule; step 1b itself, which drops the correspondences, is icp_reject.hip's.
//
// k_boundary: a wave per point of the cloud's cell-sorted grid (the cell just above the radius, so a neighbourhood is 3^3 cells),
// four waves to a block, no atomics, no scratch, nothing shared between waves.
//   collect   the wave's lanes stride over the candidate rows; a lane that holds a neighbour with a direction appends it to
//             the wave's LDS arena at the rank a ballot gives it.  The arena holds `cap` directions (16 B each: x, y in double).
//   decide    a lane per direction a (64 at a time), the inner loop over b as LDS broadcast reads: "does b fill a's wedge".
//             Left as soon as every a of the chunk is filled; a chunk that ends with an unfilled a ends the point: boundary.
//   streamed  a neighbourhood of more than `cap` directions: the a's stay in the arena `cap` at a time (by their rank, which
//             is the same in every pass), and the b's come from the grid once more, 64 at a time through a small LDS tile.
//             Any size is served; the cost is two more walks over the neighbourhood per `cap` directions.
// The decision is an existence test over unordered pairs in exact-by-construction double arithmetic, so neither the path nor
// the order of the candidates shows in a flag.
#include <atomic>
#include <cmath>
#include <cstring>

#include "capi_guard.hpp"
#include "drivers.hpp"
#include "device_util.hpp"
#include "map_kept.hpp"
#include "nn_core.hpp"
#include "radius_grid.hpp"

namespace mm3d {

namespace {

constexpr int kBndCap = 512;          // directions a wave keeps in LDS (8 KiB)
constexpr int kBndWaves = 4;

struct BndArgs {
  int s;                // cells to either side
  int cap;              // <= kBndCap
  int min_neighbours;
  double r2, c, c2;     // r * r, cos(theta), c * c
};

// b fills the wedge of a: counter-clockwise of a by an angle in (0, theta]
__device__ __forceinline__ bool bnd_fills(double ax, double ay, double aa, double bx, double by, double c, double c2)
{
  const double cross = ax * by - ay * bx, dot = ax * bx + ay * by;
  if (!(cross > 0.0 || (cross == 0.0 && dot < 0.0))) return false;
  const double rhs = c2 * (aa * (bx * bx + by * by)), dd = dot * dot;
  return c >= 0.0 ? (dot >= 0.0 && dd >= rhs) : (dot >= 0.0 || dd <= rhs);
}

// the query's frame and box, wave-uniform
struct BndQuery {
  double px, py, pz, ux, uy, uz, vx, vy, vz;
  int x0, x1, y0, y1, z0, z1;
};

// The walk over the query's candidates, 64 at a time: f(has, x, y, rank, mask) is called by the whole wave once per step; `has`
// says whether the lane holds a direction (x, y), rank is its ordinal among all directions of the walk, mask the step's ballot.
// Returns the number of directions.
template <class F>
__device__ __forceinline__ int bnd_walk(const GridView &g, const BndQuery &q, double r2, int lane, F &&f)
{
  int count = 0;
  for (int z = q.z0; z <= q.z1; ++z)
    for (int y = q.y0; y <= q.y1; ++y) {
      const int row = (z * g.dy + y) * g.dx;
      const int beg = g.cell_start[row + q.x0], end = g.cell_start[row + q.x1 + 1];
      for (int base = beg; base < end; base += kWave) {
        const int j = base + lane;
        bool has = false;
        double x = 0.0, y2 = 0.0;
        if (j < end) {
          const float4 p = g.pts[j];
          if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
            const double dx = (double)p.x - q.px, dy = (double)p.y - q.py, dz = (double)p.z - q.pz;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 <= r2 && (dx != 0.0 || dy != 0.0 || dz != 0.0)) {
              x = (q.ux * dx + q.uy * dy) + q.uz * dz;
              y2 = (q.vx * dx + q.vy * dy) + q.vz * dz;
              has = x != 0.0 || y2 != 0.0;
            }
          }
        }
        const unsigned long long mask = ballot(has);
        const int rank = count + __popcll(mask & ((1ull << lane) - 1ull));
        f(has, x, y2, rank, mask);
        count += __popcll(mask);
      }
    }
  return count;
}

__global__ void __launch_bounds__(64 * kBndWaves)
k_boundary(GridView g, const float4 *__restrict__ nrm, BndArgs a, unsigned char *__restrict__ flags)
{
  __shared__ double2 s_dir[kBndWaves][kBndCap];
  __shared__ double2 s_tile[kBndWaves][kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = (int)blockIdx.x * kBndWaves + wave;
  if (j >= g.n) return;                              // (wave-uniform; no block barrier below)
  double2 *dir = s_dir[wave], *tile = s_tile[wave];
  const float4 p = g.pts[j];
  const int i = __float_as_int(p.w);
  const float4 nf = nrm[i];
  const bool ok = isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(nf.x) && isfinite(nf.y) && isfinite(nf.z) &&
                  (nf.x != 0.f || nf.y != 0.f || nf.z != 0.f);
  if (!ok) {
    if (lane == 0) flags[i] = 0;
    return;
  }
  BndQuery q;
  q.px = p.x; q.py = p.y; q.pz = p.z;
  {
    const double nx = nf.x, ny = nf.y, nz = nf.z;
    const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
    const int k = (ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2);
    const double ex = k == 0 ? 1.0 : 0.0, ey = k == 1 ? 1.0 : 0.0, ez = k == 2 ? 1.0 : 0.0;
    q.ux = ey * nz - ez * ny; q.uy = ez * nx - ex * nz; q.uz = ex * ny - ey * nx;
    q.vx = ny * q.uz - nz * q.uy; q.vy = nz * q.ux - nx * q.uz; q.vz = nx * q.uy - ny * q.ux;
  }
  const int cx = clampi(cell_floor(p.x, g.minx, g.inv), 0, g.dx - 1);
  const int cy = clampi(cell_floor(p.y, g.miny, g.inv), 0, g.dy - 1);
  const int cz = clampi(cell_floor(p.z, g.minz, g.inv), 0, g.dz - 1);
  q.x0 = max(cx - a.s, 0); q.x1 = min(cx + a.s, g.dx - 1);
  q.y0 = max(cy - a.s, 0); q.y1 = min(cy + a.s, g.dy - 1);
  q.z0 = max(cz - a.s, 0); q.z1 = min(cz + a.s, g.dz - 1);
  const int cap = a.cap;

  // collect: the first `cap` directions into the arena
  const int m = bnd_walk(g, q, a.r2, lane, [&](bool has, double x, double y, int rank, unsigned long long) {
    if (has && rank < cap) dir[rank] = make_double2(x, y);
  });
  wave_lds_sync();
  bool boundary = false;
  if (m >= a.min_neighbours && m <= cap) {
    // decide, everything in LDS
    for (int a0 = 0; a0 < m && !boundary; a0 += kWave) {
      const bool valid = a0 + lane < m;
      const double2 da = valid ? dir[a0 + lane] : make_double2(1.0, 0.0);
      const double aa = da.x * da.x + da.y * da.y;
      bool filled = !valid;
      for (int b0 = 0; b0 < m; b0 += 8) {
        const int be = min(b0 + 8, m);
        for (int b = b0; b < be; ++b) {
          const double2 db = dir[b];                 // (broadcast)
          filled = filled || bnd_fills(da.x, da.y, aa, db.x, db.y, a.c, a.c2);
        }
        if (ballot(!filled) == 0ull) break;
      }
      boundary = ballot(!filled) != 0ull;
    }
  } else if (m >= a.min_neighbours) {
    // streamed: the a's `cap` at a time by rank, the b's from the grid again
    for (int s0 = 0; s0 < m && !boundary; s0 += cap) {
      const int na = min(cap, m - s0);
      if (s0 > 0) {
        wave_lds_sync();
        bnd_walk(g, q, a.r2, lane, [&](bool has, double x, double y, int rank, unsigned long long) {
          if (has && rank >= s0 && rank < s0 + na) dir[rank - s0] = make_double2(x, y);
        });
        wave_lds_sync();
      }
      unsigned filled = 0u;                          // bit t: direction s0 + t * 64 + lane (cap <= 512: 8 bits)
      bnd_walk(g, q, a.r2, lane, [&](bool has, double x, double y, int rank, unsigned long long mask) {
        const int nb = __popcll(mask);
        if (nb == 0) return;                         // (wave-uniform)
        if (has) tile[__popcll(mask & ((1ull << lane) - 1ull))] = make_double2(x, y);
        wave_lds_sync();
        for (int t = 0; t * kWave < na; ++t) {
          const bool live = t * kWave + lane < na && !((filled >> t) & 1u);
          if (ballot(live) == 0ull) continue;
          const double2 da = live ? dir[t * kWave + lane] : make_double2(1.0, 0.0);
          const double aa = da.x * da.x + da.y * da.y;
          bool f = false;
          for (int b = 0; b < nb; ++b) {
            const double2 db = tile[b];              // (broadcast)
            f = f || bnd_fills(da.x, da.y, aa, db.x, db.y, a.c, a.c2);
          }
          if (live && f) filled |= 1u << t;
        }
        wave_lds_sync();
      });
      for (int t = 0; t * kWave < na; ++t)
        if (ballot(t * kWave + lane < na && !((filled >> t) & 1u)) != 0ull) boundary = true;
    }
  }
  if (lane == 0) flags[i] = boundary ? 1 : 0;
}

// the number of set flags: one integer add per wave that has any
__global__ void __launch_bounds__(256) k_boundary_count(const unsigned char *__restrict__ flags, size_t n, unsigned long long *__restrict__ out)
{
  int mine = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) mine += flags[i] ? 1 : 0;
  const int total = wave_sum(mine);
  if ((threadIdx.x & 63) == 0 && total) atomicAdd(out, (unsigned long long)total);
}

std::atomic<int> g_boundary_cap{kBndCap};      // mm3d_debug_boundary_lds_cap

// cos(theta) as the rule wants it: the host's libm, but exact at the two angles where the exact value is a double
double cos_deg(double deg)
{
  if (deg == 90.0) return 0.0;
  if (deg == 180.0) return -1.0;
  return std::cos(deg * (M_PI / 180.0));
}

}  // namespace

void boundary_flags(Context *c, const mm3d_cloud *points, const float4 *normals_dev, double radius, double angle_deg, int min_neighbours,
                    unsigned char *flags_dev)
{
  if (points->n == 0) return;
  // (a record the grid does not hold -- a non-finite one -- keeps flag 0)
  MM3D_HIP(hipMemsetAsync(flags_dev, 0, points->n, c->stream));
  cloud_bbox(c, const_cast<mm3d_cloud *>(points));
  if (points->n_finite == 0) return;
  const Grid &g = cloud_grid(c, points, radius_cell(points, radius));
  if (g.n == 0) return;
  const double cs = cos_deg(angle_deg);
  const BndArgs a{radius_reach(g, radius), g_boundary_cap.load(), min_neighbours, radius * radius, cs, cs * cs};
  MM3D_LAUNCH(c, "boundary_points", g.n * (16.0 * 27.0 + 17.0), k_boundary, dim3(div_up((size_t)g.n, (size_t)kBndWaves)), dim3(64 * kBndWaves), 0,
              g.view(), normals_dev, a, flags_dev);
}

long long boundary_count(Context *c, const unsigned char *flags_dev, size_t n)
{
  if (n == 0) return 0;
  DevBuf<unsigned long long> d(c, 1);
  unsigned long long *h = (unsigned long long *)c->pin(64);
  MM3D_HIP(hipMemsetAsync(d.get(), 0, sizeof(unsigned long long), c->stream));
  MM3D_LAUNCH(c, "boundary_count", (double)n, k_boundary_count, dim3((unsigned)std::min<size_t>(div_up(n, (size_t)256), 1024)), dim3(256), 0, flags_dev, n,
              d.get());
  MM3D_HIP(hipMemcpyAsync(h, d.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  c->sync();
  return (long long)*h;
}

bool icp_geometry_options_valid(const mm3d_icp_geometry_options *o)
{
  if ((o->boundary != 0 && o->boundary != 1) || (o->normals != 0 && o->normals != 1)) return false;
  if (!(o->boundary_radius >= 0.0) || !std::isfinite(o->boundary_radius)) return false;
  if (!(o->boundary_angle_deg > 0.0 && o->boundary_angle_deg <= 180.0)) return false;
  if (o->boundary_min_neighbours < 3) return false;
  return o->normal_angle_deg > 0.0 && o->normal_angle_deg <= 90.0;
}

namespace {

// a map's flags at the context's options (radius 0: normal_radius), from its normals
const BoundaryFlags *map_boundary(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p)
{
  const mm3d_icp_geometry_options &o = ctx->sel.geometry_options;
  const double radius = o.boundary_radius > 0.0 ? o.boundary_radius : p->normal_radius;
  return map_kept(
      ctx, m, &mm3d_map::boundary,
      [&](const BoundaryFlags &b) {
        return b.radius == radius && b.angle_deg == o.boundary_angle_deg && b.min_neighbours == o.boundary_min_neighbours && b.n == m->points->n;
      },
      [&] {
        const mm3d_normals *nrm = map_normals(ctx, m, p);
        std::unique_ptr<BoundaryFlags> b(new BoundaryFlags());
        b->radius = radius; b->angle_deg = o.boundary_angle_deg; b->min_neighbours = o.boundary_min_neighbours;
        b->n = m->points->n;
        b->flags = DevBuf<unsigned char>(ctx, b->n ? b->n : 1);
        MM3D_REQUIRE(radius > 0.0 && std::isfinite(radius), "boundary rejector: the radius must be positive and finite");
        boundary_flags(ctx, m->points, (const float4 *)nrm->nrm.get(), radius, b->angle_deg, b->min_neighbours, b->flags.get());
        b->n_boundary = boundary_count(ctx, b->flags.get(), b->n);
        return b;
      });
}

struct IcpGeometry final : IcpGeometryBase {
  void prepare(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p) const override
  {
    (void)map_normals(ctx, m, p);
    if (ctx->sel.geometry_options.boundary) (void)map_boundary(ctx, m, p);
  }
  void bind(mm3d_ctx *ctx, const mm3d_map *s, const mm3d_map *t, const mm3d_params *p, IcpScoreJob *job) const override
  {
    const mm3d_icp_geometry_options &o = ctx->sel.geometry_options;
    job->geometry = &o;
    if (o.boundary) {
      const BoundaryFlags *b = map_boundary(ctx, t, p);
      job->tgt_boundary = b->flags.get();
      job->tgt_boundary_points = b->n_boundary;
    }
    if (o.normals) {
      job->src_normals = map_normals(ctx, s, p);
      job->geo_tgt_normals = map_normals(ctx, t, p);
    }
  }
};
const IcpGeometry g_icp_geometry;

}  // namespace
}  // namespace mm3d

using namespace mm3d;

extern "C" {

int mm3d_set_icp_geometry_rejection(mm3d_ctx *ctx, const mm3d_icp_geometry_options *options)
{
  if (!ctx || !options || !icp_geometry_options_valid(options)) return MM3D_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the selection changes)
  return select_stage(ctx, Stage::Geometry, [&](StageSelection &s) {
    s.geometry_options = *options;
    s.geometry = stage_active(Stage::Geometry, s) ? &g_icp_geometry : nullptr;
  });
}

int mm3d_get_icp_geometry_rejection(const mm3d_ctx *ctx, mm3d_icp_geometry_options *options)
{
  if (!ctx || !options) return MM3D_EINVAL;
  *options = ctx->sel.geometry_options;
  return MM3D_OK;
}

int mm3d_last_icp_geometry_stats(const mm3d_ctx *ctx, mm3d_icp_geometry_stats *stats)
{
  if (!ctx || !stats) return MM3D_EINVAL;
  *stats = ctx->last_geometry_stats;
  return MM3D_OK;
}

int mm3d_boundary_points(mm3d_ctx *ctx, const mm3d_cloud *points, const mm3d_normals *normals, double radius, double angle_deg,
                         int min_neighbours, unsigned char *flags, size_t capacity, long long *n_boundary)
{
  if (!ctx || !points || !normals || !flags) return MM3D_EINVAL;
  if (!(radius > 0.0) || !std::isfinite(radius) || !(angle_deg > 0.0 && angle_deg <= 180.0) || min_neighbours < 3) return MM3D_EINVAL;
  if (normals->n != points->n || capacity < points->n) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    long long count = 0;
    if (points->n) {
      DevBuf<unsigned char> d(ctx, points->n);
      boundary_flags(ctx, points, (const float4 *)normals->nrm.get(), radius, angle_deg, min_neighbours, d.get());
      MM3D_HIP(hipMemcpyAsync(flags, d.get(), points->n, hipMemcpyDeviceToHost, ctx->stream));
      count = boundary_count(ctx, d.get(), points->n);      // (ends in the wait)
    }
    if (n_boundary) *n_boundary = count;
  });
}

int mm3d_debug_boundary_lds_cap(int cap)
{
  if (cap == 0) g_boundary_cap.store(kBndCap);
  else if (cap >= 1 && cap <= kBndCap) g_boundary_cap.store(cap);
  return g_boundary_cap.load();
}

}  // extern "C"

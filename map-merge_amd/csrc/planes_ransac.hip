// planes_ransac.hip -- plane segmentation by RANSAC on gfx950: the dominant planes of a cloud, one per round, each the best of
// `samples` three-point hypotheses by its integer inlier count, optionally refitted to its inliers; and the stage that removes
// them from a map or sets them aside while the cluster filter looks at the rest (mm3d_segment_planes, mm3d_remove_planes,
// mm3d_set_planes; include/mm3d.h states the rule to the operation).  Not a reference stage.
//
// Every round is enqueued, nothing comes back to the host before the end: one wait per call, whatever samples and max_planes are.
//   k_pl_init      label NONE for a valid record, INVALID for another; the valid count
// and per round p, each kernel returning at once when an earlier round has raised ctl->stop:
//   compact        scan_fused.hpp: idx[rank] = record for the records still labelled NONE, m = their number
//   k_pl_hyp       a lane per draw: three distinct ranks from the counter-based stream, the hypothesis record (a, nrm, rhs) with
//                  rhs = distance^2 * len2, or -1 for a draw that cannot win; m < 3 raises stop
//   k_pl_count     the hot path, samples x m tests: a block of four waves keeps four points per lane in registers as doubles and
//                  walks a tile of 128 records, staged in LDS where a wave's lanes read one address (a broadcast); the lanes'
//                  votes are folded by ballot and popcount, the four waves' counts in LDS, and one integer atomicAdd per (block,
//                  draw) reaches the global count.  A draw without a count is skipped by a scalar branch; a NaN votes for nothing
//   k_pl_pick      one block: the maximum of (count << 32 | ~h) over the surviving draws -- the highest count, the lower h among
//                  equals -- and the stop threshold T; no survivor or a count below T raises stop
//   k_pl_sums      (refit) N, S, P over the winner's inliers, 4096 ranks a block in a fixed order, doubles, no atomics
//   k_pl_decide    (refit) one wave adds the blocks' partials in block order, a lane per component; lane 0 solves the 3 x 3 and
//                  leaves the candidate plane
//   k_pl_recount   (refit) the candidate's inliers over R_p, an integer
//   k_pl_apply     the adopted plane's inliers get the label p; one lane writes planes[p]
// Launches that depend on m are sized by n, which the host knows, and look m up on the device.
#include <cmath>
#include <cstring>

#include "capi_guard.hpp"
#include "drivers.hpp"
#include "device_util.hpp"
#include "scan_fused.hpp"
#include "sym_eig3.hpp"

namespace mm3d {

namespace {

constexpr int kPlThreads = 256;
constexpr int kPlPerLane = 4;                                  // k_pl_count: points a lane keeps in registers
constexpr int kPlBlockPoints = kPlThreads * kPlPerLane;        // ... and a block covers
constexpr int kPlTile = 128;                                   // hypothesis records a block of k_pl_count stages in LDS and walks (7 KB)
constexpr int kPlChunk = 4096;                                 // ranks per partial sum of the refit: the order is a function of R_p alone
constexpr int kPlMaxPlanes = 8;
constexpr int kPlSweepBlocks = 256;                             // k_pl_init, k_pl_recount: this many blocks stride over the records

struct PlHyp { double a[3], n[3], rhs; };                      // 56 bytes
static_assert(sizeof(PlHyp) == 56, "the LDS tile is read as 7 doubles a record");

struct PlPartial { double s[3], p[6]; long long n; };

// What the rounds leave each other on the device.  Words a kernel writes are read only by later launches.
struct PlCtl {
  int m, stop, planes, rounds, win_h, cand;
  long long n_valid, draws, degenerate, off_axis, on_planes, cnt_h;
  unsigned long long cnt_r;
  double rn[3], rc[3];                                         // the refit candidate: unit normal and a point of the plane
};

struct PlOpts {                                                // the rule's constants, by value to every kernel
  int samples, refit, has_axis;
  unsigned seed;
  double distance, dist2, min_fraction, axis[3], aa, c2;
};

// splitmix64's finaliser on ((seed << 32) | (p << 24) | h) + (j + 1) * golden gamma: word j of draw h of round p (include/mm3d.h)
__device__ __forceinline__ uint64_t pl_word(uint64_t base, int j)
{
  uint64_t z = base + (uint64_t)(j + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ int pl_bounded(uint64_t w, int n) { return (int)(((w >> 32) * (uint64_t)(uint32_t)n) >> 32); }

// (x*x' + y*y') + z*z' in double, every operation rounded once
__device__ __forceinline__ double pl_dot(double x, double y, double z, double a, double b, double c)
{
  return __dadd_rn(__dadd_rn(__dmul_rn(x, a), __dmul_rn(y, b)), __dmul_rn(z, c));
}
__device__ __forceinline__ bool pl_valid(const float4 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// the hypothesis test of step 6: s * s <= rhs with s = nrm . (q - a)
__device__ __forceinline__ bool pl_vote(const PlHyp &H, double qx, double qy, double qz)
{
  const double s = pl_dot(H.n[0], H.n[1], H.n[2], __dsub_rn(qx, H.a[0]), __dsub_rn(qy, H.a[1]), __dsub_rn(qz, H.a[2]));
  return __dmul_rn(s, s) <= H.rhs;
}
// the refit test of step 8: |s'| <= distance with s' = n' . (q - c)
__device__ __forceinline__ bool pl_vote_refit(const PlCtl *ctl, double distance, double qx, double qy, double qz)
{
  const double s = pl_dot(ctl->rn[0], ctl->rn[1], ctl->rn[2], __dsub_rn(qx, ctl->rc[0]), __dsub_rn(qy, ctl->rc[1]), __dsub_rn(qz, ctl->rc[2]));
  return fabs(s) <= distance;
}
// step 9's sign: with an axis n . axis >= 0, without one the first non-zero of (nz, ny, nx) positive
__device__ __forceinline__ void pl_orient(const PlOpts &o, double n[3])
{
  bool flip;
  if (o.has_axis) flip = pl_dot(n[0], n[1], n[2], o.axis[0], o.axis[1], o.axis[2]) < 0.0;
  else flip = n[2] < 0.0 || (n[2] == 0.0 && (n[1] < 0.0 || (n[1] == 0.0 && n[0] < 0.0)));
  if (flip) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
}

// At most kPlSweepBlocks blocks stride over the records and add their valid counts once each: one word takes about 90 atomics
// a microsecond from the whole chip, and a block per 256 records would queue 1 600 of them for a headline map.
__global__ void __launch_bounds__(kPlThreads)
k_pl_init(const float4 *__restrict__ pts, int n, int *__restrict__ labels, PlCtl *__restrict__ ctl)
{
  int mine = 0;
  for (long long i = (long long)blockIdx.x * kPlThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kPlThreads) {   // (counted)
    const bool ok = pl_valid(pts[i]);
    labels[i] = ok ? MM3D_PLANE_NONE : MM3D_PLANE_INVALID;
    mine += ok ? 1 : 0;
  }
  __shared__ int s_n[kPlThreads / kWave];
  const int c = wave_sum(mine);
  if ((threadIdx.x & (kWave - 1)) == 0) s_n[threadIdx.x / kWave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    if (t) atomicAdd((unsigned long long *)&ctl->n_valid, (unsigned long long)t);
  }
}

// R_p: the records still without a plane, in the cloud's order; element n of the scan carries their number
struct PlNoneLoad {
  const int *labels; size_t n;
  __device__ __forceinline__ int operator()(size_t j) const { return j < n ? (labels[j] == MM3D_PLANE_NONE ? 1 : 0) : 0; }
};
struct PlRankStore {
  int *idx; size_t n; PlCtl *ctl;
  __device__ __forceinline__ void operator()(size_t j, int prefix, int v) const
  {
    if (j == n) { ctl->m = prefix; return; }
    if (v) idx[prefix] = (int)j;
  }
  __device__ __forceinline__ void done() const {}
};

__global__ void __launch_bounds__(kPlThreads)
k_pl_hyp(const float4 *__restrict__ pts, const int *__restrict__ idx, PlOpts o, int round, PlCtl *__restrict__ ctl, PlHyp *__restrict__ hyp,
         unsigned *__restrict__ counts)
{
  if (ctl->stop) return;
  const int m = ctl->m;
  const int h = blockIdx.x * kPlThreads + threadIdx.x;
  if (m < 3) {                                                   // step 3: the rule ends (every lane of the launch sees the same m)
    if (h == 0) ctl->stop = 1;
    return;
  }
  const bool live = h < o.samples;
  bool degenerate = false, off_axis = false;
  if (live) {
    const uint64_t base = ((uint64_t)o.seed << 32) | ((uint64_t)round << 24) | (uint64_t)h;
    const int i0 = pl_bounded(pl_word(base, 0), m);
    int i1 = pl_bounded(pl_word(base, 1), m - 1);
    i1 += i1 >= i0 ? 1 : 0;
    int i2 = pl_bounded(pl_word(base, 2), m - 2);
    const int lo = min(i0, i1), hi = max(i0, i1);
    i2 += i2 >= lo ? 1 : 0;
    i2 += i2 >= hi ? 1 : 0;
    const float4 a = pts[idx[i0]], b = pts[idx[i1]], c = pts[idx[i2]];
    PlHyp H;
    H.a[0] = (double)a.x; H.a[1] = (double)a.y; H.a[2] = (double)a.z;
    const double ux = __dsub_rn((double)b.x, H.a[0]), uy = __dsub_rn((double)b.y, H.a[1]), uz = __dsub_rn((double)b.z, H.a[2]);
    const double vx = __dsub_rn((double)c.x, H.a[0]), vy = __dsub_rn((double)c.y, H.a[1]), vz = __dsub_rn((double)c.z, H.a[2]);
    H.n[0] = __dsub_rn(__dmul_rn(uy, vz), __dmul_rn(uz, vy));
    H.n[1] = __dsub_rn(__dmul_rn(uz, vx), __dmul_rn(ux, vz));
    H.n[2] = __dsub_rn(__dmul_rn(ux, vy), __dmul_rn(uy, vx));
    const double len2 = pl_dot(H.n[0], H.n[1], H.n[2], H.n[0], H.n[1], H.n[2]);
    const double uu = pl_dot(ux, uy, uz, ux, uy, uz), vv = pl_dot(vx, vy, vz, vx, vy, vz);
    degenerate = !(len2 > __dmul_rn(1e-12, __dmul_rn(uu, vv)));
    if (!degenerate && o.has_axis) {
      const double dn = pl_dot(H.n[0], H.n[1], H.n[2], o.axis[0], o.axis[1], o.axis[2]);
      off_axis = !(__dmul_rn(dn, dn) >= __dmul_rn(__dmul_rn(o.c2, len2), o.aa));
    }
    H.rhs = (degenerate || off_axis) ? -1.0 : __dmul_rn(o.dist2, len2);
    hyp[h] = H;
    counts[h] = 0u;
  }
  const int nd = __popcll(ballot(degenerate)), na = __popcll(ballot(off_axis));
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (nd) atomicAdd((unsigned long long *)&ctl->degenerate, (unsigned long long)nd);
    if (na) atomicAdd((unsigned long long *)&ctl->off_axis, (unsigned long long)na);
  }
  if (h == 0) {
    ctl->rounds += 1;
    ctl->draws += o.samples;
    ctl->cand = 0;
    ctl->cnt_r = 0ull;
  }
}

// The count of every draw over R_p.  Block (b, t) keeps ranks [b * 1024, (b + 1) * 1024) in registers, lane l of the block the
// ranks b * 1024 + k * 256 + l, and walks tile t of the draws, kPlTile of them, staged in LDS; a rank past m is a NaN, which votes
// for nothing.  (One block per 1 024 ranks walking every tile left a headline map with 398 blocks for 256 compute units, a wave
// per SIMD and nothing to hide a latency behind; the tiles as a second grid dimension give every SIMD several waves, and the
// atomics stay one per (1 024 ranks, draw).)  Lane j % 64 of a wave carries the wave's count of draw j until 64 draws are
// through; the four waves' counts meet in LDS.  Integer sums: no order can move them.
__global__ void __launch_bounds__(kPlThreads)
k_pl_count(const float4 *__restrict__ pts, const int *__restrict__ idx, const PlCtl *__restrict__ ctl, const PlHyp *__restrict__ hyp, int samples,
           unsigned *__restrict__ counts)
{
  if (ctl->stop) return;
  const int m = ctl->m;
  const long long base = (long long)blockIdx.x * kPlBlockPoints;
  if (base >= m) return;                                        // (block-uniform)
  __shared__ double s_h[kPlTile * 7];
  __shared__ int s_c[kPlThreads / kWave][kPlTile];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int t0 = (int)blockIdx.y * kPlTile, nt = min(kPlTile, samples - t0);
  const double *flat = (const double *)hyp;
  for (int i = threadIdx.x; i < nt * 7; i += kPlThreads) s_h[i] = flat[(size_t)t0 * 7 + i];
  double qx[kPlPerLane], qy[kPlPerLane], qz[kPlPerLane];
#pragma unroll
  for (int k = 0; k < kPlPerLane; ++k) {
    const long long r = base + (long long)k * kPlThreads + threadIdx.x;
    qx[k] = qy[k] = qz[k] = __longlong_as_double(0x7ff8000000000000ll);
    if (r < m) {
      const float4 p = pts[idx[r]];
      qx[k] = (double)p.x; qy[k] = (double)p.y; qz[k] = (double)p.z;
    }
  }
  __syncthreads();
  for (int j0 = 0; j0 < nt; j0 += kWave) {                      // (block-uniform; counted)
    const int nj = min(kWave, nt - j0);
    int mine = 0;
    for (int j = 0; j < nj; ++j) {                              // (wave-uniform)
      const double *r = s_h + (size_t)(j0 + j) * 7;             // one address for the wave: an LDS broadcast
      const double ax = r[0], ay = r[1], az = r[2], nx = r[3], ny = r[4], nz = r[5], rhs = r[6];
      int c = 0;
      if (__builtin_amdgcn_readfirstlane(__double2hiint(rhs)) >= 0) {   // (a scalar branch: rhs = -1 marks a draw without a count)
#pragma unroll
        for (int k = 0; k < kPlPerLane; ++k) {
          const double s = pl_dot(nx, ny, nz, __dsub_rn(qx[k], ax), __dsub_rn(qy[k], ay), __dsub_rn(qz[k], az));
          c += __popcll(ballot(__dmul_rn(s, s) <= rhs));
        }
      }
      mine = lane == j ? c : mine;
    }
    if (lane < nj) s_c[wave][j0 + lane] = mine;
  }
  __syncthreads();
  if ((int)threadIdx.x < nt) {
    const int t = (s_c[0][threadIdx.x] + s_c[1][threadIdx.x]) + (s_c[2][threadIdx.x] + s_c[3][threadIdx.x]);
    if (t) atomicAdd(counts + t0 + threadIdx.x, (unsigned)t);
  }
}

// One block.  key = count << 32 | ~h: the highest count, the lower h among equals; 0 = no surviving draw (a survivor counts at
// least its own record a, whose s is 0).
__global__ void __launch_bounds__(kPlThreads)
k_pl_pick(const PlHyp *__restrict__ hyp, const unsigned *__restrict__ counts, PlOpts o, PlCtl *__restrict__ ctl)
{
  if (ctl->stop) return;
  unsigned long long key = 0ull;
  for (int h = threadIdx.x; h < o.samples; h += kPlThreads) {
    if (!(hyp[h].rhs >= 0.0)) continue;
    const unsigned long long k = ((unsigned long long)counts[h] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)h);
    key = k > key ? k : key;
  }
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
    const unsigned long long other = __shfl_xor(key, w, kWave);
    key = other > key ? other : key;
  }
  __shared__ unsigned long long s_key[kPlThreads / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) s_key[threadIdx.x / kWave] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kPlThreads / kWave; ++w) key = s_key[w] > key ? s_key[w] : key;
    const double t = ceil(__dmul_rn(o.min_fraction, (double)ctl->n_valid));
    const long long T = t > 3.0 ? (long long)t : 3ll;
    const long long best = (long long)(key >> 32);
    if (key == 0ull || best < T) ctl->stop = 1;                 // step 7: round p finds no plane, the rule ends
    else { ctl->win_h = (int)(0xFFFFFFFFu - (unsigned)key); ctl->cnt_h = best; }
  }
}

// Block b sums the inliers among ranks [b * 4096, (b + 1) * 4096): lane l its sixteen ranks l, l + 256, ... in that order, the
// wave by device_util.hpp's fixed tree, the four waves in order.  q = record - a.
__global__ void __launch_bounds__(kPlThreads)
k_pl_sums(const float4 *__restrict__ pts, const int *__restrict__ idx, const PlCtl *__restrict__ ctl, const PlHyp *__restrict__ hyp,
          PlPartial *__restrict__ part)
{
  if (ctl->stop) return;
  const int m = ctl->m;
  const long long base = (long long)blockIdx.x * kPlChunk;
  if (base >= m) return;
  const PlHyp H = hyp[ctl->win_h];
  double s[3] = {0.0, 0.0, 0.0}, p[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int cnt = 0;
  for (int u = 0; u < kPlChunk / kPlThreads; ++u) {
    const long long r = base + (long long)u * kPlThreads + threadIdx.x;
    if (r >= m) continue;
    const float4 f = pts[idx[r]];
    if (!pl_vote(H, (double)f.x, (double)f.y, (double)f.z)) continue;
    const double x = (double)f.x - H.a[0], y = (double)f.y - H.a[1], z = (double)f.z - H.a[2];
    s[0] += x; s[1] += y; s[2] += z;
    p[0] += x * x; p[1] += x * y; p[2] += x * z; p[3] += y * y; p[4] += y * z; p[5] += z * z;
    ++cnt;
  }
  __shared__ double s_v[kPlThreads / kWave][9];
  __shared__ int s_n[kPlThreads / kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
  for (int a = 0; a < 3; ++a) s[a] = wave_sum(s[a]);
#pragma unroll
  for (int a = 0; a < 6; ++a) p[a] = wave_sum(p[a]);
  cnt = wave_sum(cnt);
  if (lane == 0) {
    for (int a = 0; a < 3; ++a) s_v[wave][a] = s[a];
    for (int a = 0; a < 6; ++a) s_v[wave][3 + a] = p[a];
    s_n[wave] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    PlPartial P;
    for (int a = 0; a < 3; ++a) P.s[a] = ((s_v[0][a] + s_v[1][a]) + s_v[2][a]) + s_v[3][a];
    for (int a = 0; a < 6; ++a) P.p[a] = ((s_v[0][3 + a] + s_v[1][3 + a]) + s_v[2][3 + a]) + s_v[3][3 + a];
    P.n = (long long)s_n[0] + s_n[1] + s_n[2] + s_n[3];
    part[blockIdx.x] = P;
  }
}

// One wave: lane k < 9 adds component k of the partials in block order, lane 9 the counts; lane 0 then forms the covariance about
// the mean and its smallest eigenvector.  The candidate stands when step 8's tests on the matrix hold (the inlier count is
// k_pl_recount's, the comparison k_pl_apply's).
static_assert(sizeof(PlPartial) == 80, "k_pl_decide reads a partial as ten 8-byte words");
__global__ void __launch_bounds__(kWave)
k_pl_decide(const PlPartial *__restrict__ part, const PlHyp *__restrict__ hyp, PlOpts o, PlCtl *__restrict__ ctl)
{
  if (blockIdx.x || ctl->stop) return;
  const int blocks = (ctl->m + kPlChunk - 1) / kPlChunk;
  const int lane = threadIdx.x;
  // (64 partials at a time come to LDS with every lane loading, so that the additions wait for LDS and not, one after the
  // other, for memory: a lane alone adding straight from memory took 25 us for a headline map's 100 partials)
  const unsigned long long *flat = (const unsigned long long *)part;
  __shared__ unsigned long long s_p[kWave * 10];
  double acc = 0.0;
  long long cnt = 0;
  for (int b0 = 0; b0 < blocks; b0 += kWave) {                  // (wave-uniform; counted)
    const int nb = min(kWave, blocks - b0);
    __syncthreads();
    for (int i = lane; i < nb * 10; i += kWave) s_p[i] = flat[(size_t)b0 * 10 + i];
    __syncthreads();
    if (lane < 9)
      for (int b = 0; b < nb; ++b) acc += __longlong_as_double((long long)s_p[b * 10 + lane]);
    else if (lane == 9)
      for (int b = 0; b < nb; ++b) cnt += (long long)s_p[b * 10 + 9];
  }
  double S[3], P[6];
#pragma unroll
  for (int a = 0; a < 3; ++a) S[a] = __shfl(acc, a, kWave);
#pragma unroll
  for (int a = 0; a < 6; ++a) P[a] = __shfl(acc, 3 + a, kWave);
  const long long N = __shfl(cnt, 9, kWave);
  if (lane) return;
  if (N < 1) return;
  const double inv = (double)N;
  const double mu[3] = {S[0] / inv, S[1] / inv, S[2] / inv};
  double C[3][3], w[3], V[3][3];
  C[0][0] = P[0] / inv - mu[0] * mu[0];
  C[0][1] = C[1][0] = P[1] / inv - mu[0] * mu[1];
  C[0][2] = C[2][0] = P[2] / inv - mu[0] * mu[2];
  C[1][1] = P[3] / inv - mu[1] * mu[1];
  C[1][2] = C[2][1] = P[4] / inv - mu[1] * mu[2];
  C[2][2] = P[5] / inv - mu[2] * mu[2];
  const double trace = (C[0][0] + C[1][1]) + C[2][2];
  sym_eig3(C, w, V);
  double nn[3] = {V[0][0], V[1][0], V[2][0]};
  pl_orient(o, nn);
  const PlHyp H = hyp[ctl->win_h];
  const double c[3] = {H.a[0] + mu[0], H.a[1] + mu[1], H.a[2] + mu[2]};
  bool ok = trace > 0.0 && (w[1] - w[0]) > 1e-6 * trace;
  for (int a = 0; a < 3; ++a) ok = ok && isfinite(nn[a]) && isfinite(c[a]) && isfinite(w[a]);
  if (ok && o.has_axis) {
    const double dn = pl_dot(nn[0], nn[1], nn[2], o.axis[0], o.axis[1], o.axis[2]);
    ok = dn * dn >= o.c2 * o.aa;
  }
  if (!ok) return;
  for (int a = 0; a < 3; ++a) { ctl->rn[a] = nn[a]; ctl->rc[a] = c[a]; }
  ctl->cand = 1;
}

__global__ void __launch_bounds__(kPlThreads)
k_pl_recount(const float4 *__restrict__ pts, const int *__restrict__ idx, double distance, PlCtl *__restrict__ ctl)
{
  if (ctl->stop || !ctl->cand) return;
  const int m = ctl->m;
  int mine = 0;
  for (long long r = (long long)blockIdx.x * kPlThreads + threadIdx.x; r < m; r += (long long)gridDim.x * kPlThreads) {   // (counted)
    const float4 f = pts[idx[r]];
    mine += pl_vote_refit(ctl, distance, (double)f.x, (double)f.y, (double)f.z) ? 1 : 0;
  }
  __shared__ int s_n[kPlThreads / kWave];
  const int c = wave_sum(mine);
  if ((threadIdx.x & (kWave - 1)) == 0) s_n[threadIdx.x / kWave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    if (t) atomicAdd(&ctl->cnt_r, (unsigned long long)t);
  }
}

// The adopted plane's inliers get the label `round`.  The refit is adopted when it is a candidate with at least the hypothesis'
// count (every lane reads the same words).  Lane 0 of the launch writes the plane's record.
__global__ void __launch_bounds__(kPlThreads)
k_pl_apply(const float4 *__restrict__ pts, const int *__restrict__ idx, PlOpts o, int round, PlCtl *__restrict__ ctl, const PlHyp *__restrict__ hyp,
           int *__restrict__ labels, mm3d_plane *__restrict__ planes)
{
  if (ctl->stop) return;
  const int m = ctl->m;
  const bool adopted = ctl->cand && (long long)ctl->cnt_r >= ctl->cnt_h;
  const PlHyp H = hyp[ctl->win_h];
  const long long r = (long long)blockIdx.x * kPlThreads + threadIdx.x;
  if (r < m) {
    const int i = idx[r];
    const float4 f = pts[i];
    const bool in = adopted ? pl_vote_refit(ctl, o.distance, (double)f.x, (double)f.y, (double)f.z) : pl_vote(H, (double)f.x, (double)f.y, (double)f.z);
    if (in) labels[i] = round;
  }
  if (r == 0) {
    mm3d_plane P;
    double nn[3], through[3];
    if (adopted) {
      for (int a = 0; a < 3; ++a) { nn[a] = ctl->rn[a]; through[a] = ctl->rc[a]; }
    } else {
      const double len = sqrt(pl_dot(H.n[0], H.n[1], H.n[2], H.n[0], H.n[1], H.n[2]));
      for (int a = 0; a < 3; ++a) { nn[a] = H.n[a] / len; through[a] = H.a[a]; }
      pl_orient(o, nn);
    }
    for (int a = 0; a < 3; ++a) P.normal[a] = nn[a];
    P.d = -pl_dot(nn[0], nn[1], nn[2], through[0], through[1], through[2]);
    P.inliers = adopted ? (long long)ctl->cnt_r : ctl->cnt_h;
    P.draw = ctl->win_h;
    P.refit = adopted ? 1 : 0;
    planes[round] = P;
  }
}

// Read by the launch after the last k_pl_apply, so that the counters above are final: planes and on_planes from the records
__global__ void k_pl_finish(const mm3d_plane *__restrict__ planes, int max_planes, PlCtl *__restrict__ ctl)
{
  if (blockIdx.x || threadIdx.x) return;
  int np = 0;
  long long on = 0;
  for (int p = 0; p < max_planes; ++p)
    if (planes[p].inliers > 0) { ++np; on += planes[p].inliers; }
  ctl->planes = np;
  ctl->on_planes = on;
}

__global__ void __launch_bounds__(kPlThreads)
k_pl_flags(const int *__restrict__ labels, int n, int *__restrict__ none, int *__restrict__ on_plane)
{
  const int i = blockIdx.x * kPlThreads + threadIdx.x;
  if (i >= n) return;
  const int l = labels[i];
  none[i] = l == MM3D_PLANE_NONE ? 1 : 0;
  if (on_plane) on_plane[i] = l >= 0 ? 1 : 0;
}

// ---------------------------------------------------------------- host
bool pl_options_ok(const mm3d_plane_options *o, bool stage_call)
{
  if (!o) return false;
  if (!stage_call && o->method != MM3D_PLANES_OFF && o->method != MM3D_PLANES_REMOVE && o->method != MM3D_PLANES_SET_ASIDE) return false;
  if (o->max_planes < 1 || o->max_planes > kPlMaxPlanes || o->samples < 1 || o->samples > 65536 || (o->refit != 0 && o->refit != 1)) return false;
  if (!std::isfinite(o->distance) || o->distance < 0.0 || (stage_call && !(o->distance > 0.0))) return false;
  if (!(o->min_fraction >= 0.0 && o->min_fraction <= 1.0)) return false;        // (false for NaN)
  if (!std::isfinite(o->axis[0]) || !std::isfinite(o->axis[1]) || !std::isfinite(o->axis[2])) return false;
  return o->max_angle_deg >= 0.0 && o->max_angle_deg <= 90.0;
}

struct PlWork {
  DevBuf<int> labels;                     // [n]
  DevBuf<PlCtl> ctl;                      // one record
  DevBuf<mm3d_plane> planes;              // [8]
};
struct PlHome { const PlCtl *ctl; const mm3d_plane *planes; };     // pinned, read after the caller's wait

// The whole rule on the device, nothing waited for.  in->n > 0.  The pinned copies of the control record and the planes are
// enqueued behind it; they are home after the caller's next wait on the stream.
PlHome pl_segment(Context *c, const mm3d_cloud *in, const mm3d_plane_options &opt, double distance, PlWork &w)
{
  const int n = (int)in->n;
  PlOpts o;
  o.samples = opt.samples; o.refit = opt.refit; o.seed = opt.seed;
  o.distance = distance; o.dist2 = distance * distance; o.min_fraction = opt.min_fraction;
  for (int a = 0; a < 3; ++a) o.axis[a] = opt.axis[a];
  o.aa = (opt.axis[0] * opt.axis[0] + opt.axis[1] * opt.axis[1]) + opt.axis[2] * opt.axis[2];
  o.has_axis = (opt.axis[0] != 0.0 || opt.axis[1] != 0.0 || opt.axis[2] != 0.0) ? 1 : 0;
  const double cs = std::cos(opt.max_angle_deg * M_PI / 180.0);
  o.c2 = cs * cs;
  w.labels = DevBuf<int>(c, (size_t)n);
  w.ctl = DevBuf<PlCtl>(c, 1);
  w.planes = DevBuf<mm3d_plane>(c, kPlMaxPlanes);
  DevBuf<int> idx(c, (size_t)n);
  DevBuf<PlHyp> hyp(c, (size_t)opt.samples);
  DevBuf<unsigned> counts(c, (size_t)opt.samples);
  const unsigned sum_blocks = (unsigned)div_up((size_t)n, kPlChunk);
  DevBuf<PlPartial> part(c, opt.refit ? sum_blocks : 0);
  MM3D_HIP(hipMemsetAsync(w.ctl.get(), 0, sizeof(PlCtl), c->stream));
  MM3D_HIP(hipMemsetAsync(w.planes.get(), 0, kPlMaxPlanes * sizeof(mm3d_plane), c->stream));
  const dim3 threads(kPlThreads), per_point(div_up((size_t)n, kPlThreads)), per_draw(div_up((size_t)opt.samples, kPlThreads));
  const dim3 sweep(std::min<unsigned>(per_point.x, kPlSweepBlocks));
  const float4 *pts = in->pts.get();
  MM3D_LAUNCH(c, "pl_init", n * 20.0, k_pl_init, sweep, threads, 0, pts, n, w.labels.get(), w.ctl.get());
  for (int p = 0; p < opt.max_planes; ++p) {
    scan_fused(c, "pl_compact", n * 8.0, (size_t)n + 1, PlNoneLoad{w.labels.get(), (size_t)n}, PlRankStore{idx.get(), (size_t)n, w.ctl.get()});
    MM3D_LAUNCH(c, "pl_hyp", opt.samples * 110.0, k_pl_hyp, per_draw, threads, 0, pts, (const int *)idx.get(), o, p, w.ctl.get(), hyp.get(), counts.get());
    MM3D_LAUNCH(c, "pl_count", n * 20.0, k_pl_count, dim3(div_up((size_t)n, kPlBlockPoints), div_up((size_t)opt.samples, kPlTile)), threads, 0, pts, (const int *)idx.get(),
                (const PlCtl *)w.ctl.get(), (const PlHyp *)hyp.get(), opt.samples, counts.get());
    MM3D_LAUNCH(c, "pl_pick", opt.samples * 12.0, k_pl_pick, dim3(1), threads, 0, (const PlHyp *)hyp.get(), (const unsigned *)counts.get(), o, w.ctl.get());
    if (opt.refit) {
      MM3D_LAUNCH(c, "pl_sums", n * 20.0, k_pl_sums, dim3(sum_blocks), threads, 0, pts, (const int *)idx.get(), (const PlCtl *)w.ctl.get(),
                  (const PlHyp *)hyp.get(), part.get());
      MM3D_LAUNCH(c, "pl_decide", sum_blocks * 80.0, k_pl_decide, dim3(1), dim3(kWave), 0, (const PlPartial *)part.get(), (const PlHyp *)hyp.get(), o,
                  w.ctl.get());
      MM3D_LAUNCH(c, "pl_recount", n * 20.0, k_pl_recount, sweep, threads, 0, pts, (const int *)idx.get(), distance, w.ctl.get());
    }
    MM3D_LAUNCH(c, "pl_apply", n * 24.0, k_pl_apply, per_point, threads, 0, pts, (const int *)idx.get(), o, p, w.ctl.get(), (const PlHyp *)hyp.get(),
                w.labels.get(), w.planes.get());
  }
  MM3D_LAUNCH(c, "pl_finish", 512.0, k_pl_finish, dim3(1), dim3(kWave), 0, (const mm3d_plane *)w.planes.get(), opt.max_planes, w.ctl.get());
  static_assert(sizeof(PlCtl) <= 192, "the pinned block below");
  char *h = (char *)c->pin(192 + kPlMaxPlanes * sizeof(mm3d_plane));
  std::memset(h, 0, 192 + kPlMaxPlanes * sizeof(mm3d_plane));
  MM3D_HIP(hipMemcpyAsync(h, w.ctl.get(), sizeof(PlCtl), hipMemcpyDeviceToHost, c->stream));
  MM3D_HIP(hipMemcpyAsync(h + 192, w.planes.get(), kPlMaxPlanes * sizeof(mm3d_plane), hipMemcpyDeviceToHost, c->stream));
  return PlHome{(const PlCtl *)h, (const mm3d_plane *)(h + 192)};
}

void pl_results(size_t n, const PlHome &home, mm3d_plane_stats *stats, mm3d_plane *planes, int *n_planes)
{
  const PlCtl &k = *home.ctl;
  if (stats) {
    stats->points = (long long)n; stats->valid = k.n_valid; stats->on_planes = k.on_planes; stats->kept = k.n_valid - k.on_planes;
    stats->draws = k.draws; stats->degenerate = k.degenerate; stats->off_axis = k.off_axis; stats->planes = k.planes; stats->rounds = k.rounds;
  }
  if (planes) std::memcpy(planes, home.planes, (size_t)k.planes * sizeof(mm3d_plane));
  if (n_planes) *n_planes = k.planes;
}
void pl_nothing(mm3d_plane_stats *stats, int *n_planes)
{
  if (stats) *stats = mm3d_plane_stats{0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (n_planes) *n_planes = 0;
}

// Step 10's second call: the records labelled NONE as a cloud of their own; with on_plane, the plane records as another.
// One wait per cloud, the first of which brings the counts and the planes home.
mm3d_cloud *pl_split(Context *c, const mm3d_cloud *in, const mm3d_plane_options &opt, double distance, mm3d_plane_stats *stats, mm3d_plane *planes,
                     std::unique_ptr<mm3d_cloud> *on_plane)
{
  MM3D_REQUIRE(in->n < ((size_t)1 << 31), "plane stage: more than 2^31 - 1 points");
  const size_t n = in->n;
  if (n == 0) {
    pl_nothing(stats, nullptr);
    if (on_plane) on_plane->reset(cloud_from_device(c, DevBuf<float4>(c, 0), 0));
    return cloud_from_device(c, DevBuf<float4>(c, 0), 0);
  }
  PlWork w;
  const PlHome home = pl_segment(c, in, opt, distance, w);
  DevBuf<int> none(c, n + 1), plane(c, on_plane ? n + 1 : 0);
  MM3D_LAUNCH(c, "pl_flags", n * 12.0, k_pl_flags, dim3(div_up(n, kPlThreads)), dim3(kPlThreads), 0, (const int *)w.labels.get(), (int)n, none.get(),
              on_plane ? plane.get() : (int *)nullptr);
  std::unique_ptr<mm3d_cloud> rest(cloud_of_kept(c, in, none.get(), true));          // the wait
  pl_results(n, home, stats, planes, nullptr);
  if (on_plane) on_plane->reset(cloud_of_kept(c, in, plane.get(), true));
  return rest.release();
}

struct PlanesRansac final : PlaneFilterBase {
  mm3d_cloud *filter(Context *c, mm3d_cloud *in, const mm3d_plane_options &o, double resolution, const ClusterFilterBase *clusters,
                     const mm3d_cluster_options &co, mm3d_plane_stats *stats, mm3d_plane *planes, mm3d_cluster_stats *cluster_stats) const override
  {
    const double distance = o.distance > 0.0 ? o.distance : 0.5 * resolution;
    MM3D_REQUIRE(std::isfinite(distance) && distance > 0.0, "plane stage: the distance must be finite and > 0");
    if (o.method == MM3D_PLANES_REMOVE) {
      std::unique_ptr<mm3d_cloud> rest(pl_split(c, in, o, distance, stats, planes, nullptr));
      if (!clusters) return rest.release();
      return clusters->filter(c, rest.get(), co, resolution, cluster_stats);
    }
    if (!clusters) return in;                                          // SET_ASIDE with nothing to look at the rest: nothing runs
    std::unique_ptr<mm3d_cloud> on_plane;
    std::unique_ptr<mm3d_cloud> rest(pl_split(c, in, o, distance, stats, planes, &on_plane));
    std::unique_ptr<mm3d_cloud> kept(clusters->filter(c, rest.get(), co, resolution, cluster_stats));
    // the set-aside records in the cloud's order, then the cluster filter's result: still one point per voxel of the input's lattice
    const size_t np = on_plane->n, nk = kept->n;
    DevBuf<float4> both(c, np + nk);
    if (np) MM3D_HIP(hipMemcpyAsync(both.get(), on_plane->pts.get(), np * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    if (nk) MM3D_HIP(hipMemcpyAsync(both.get() + np, kept->pts.get(), nk * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    c->settle();                                                       // (the two parts go back to the pool behind the copies)
    mm3d_cloud *res = cloud_from_device(c, std::move(both), np + nk);
    res->voxel_leaf = in->voxel_leaf;
    return res;
  }
};
const PlanesRansac g_ransac;

}  // namespace

}  // namespace mm3d

using namespace mm3d;

extern "C" {

int mm3d_segment_planes(mm3d_ctx *ctx, const mm3d_cloud *points, const mm3d_plane_options *options, int *labels, size_t capacity,
                        mm3d_plane *planes, int *n_planes, mm3d_plane_stats *stats)
{
  if (!ctx || !points || !labels || !planes || !n_planes || !pl_options_ok(options, true)) return MM3D_EINVAL;
  if (points->n >= ((size_t)1 << 31) || capacity < points->n) return MM3D_EINVAL;
  *n_planes = 0;
  if (points->n == 0) {
    pl_nothing(stats, n_planes);
    return MM3D_OK;
  }
  return guarded(ctx, [&] {
    PlWork w;
    const PlHome home = pl_segment(ctx, points, *options, options->distance, w);
    MM3D_HIP(hipMemcpyAsync(labels, w.labels.get(), points->n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();                                                       // the one wait
    pl_results(points->n, home, stats, planes, n_planes);
  });
}

int mm3d_remove_planes(mm3d_ctx *ctx, const mm3d_cloud *in, const mm3d_plane_options *options, mm3d_cloud **out)
{
  if (!ctx || !in || !out) return MM3D_EINVAL;
  *out = nullptr;
  if (!pl_options_ok(options, true) || in->n >= ((size_t)1 << 31)) return MM3D_EINVAL;
  return guarded(ctx, [&] { *out = pl_split(ctx, in, *options, options->distance, &ctx->last_plane_stats, ctx->last_planes, nullptr); });
}

int mm3d_set_planes(mm3d_ctx *ctx, const mm3d_plane_options *options)
{
  if (!ctx || !pl_options_ok(options, false)) return MM3D_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the stage changes)
  return select_stage(ctx, Stage::Planes, [&](StageSelection &s) {
    s.plane_options = *options;
    s.planes = stage_active(Stage::Planes, s) ? &g_ransac : nullptr;
  });
}

int mm3d_get_planes(const mm3d_ctx *ctx, mm3d_plane_options *options)
{
  if (!ctx || !options) return MM3D_EINVAL;
  *options = ctx->sel.plane_options;
  return MM3D_OK;
}

int mm3d_last_plane_stats(const mm3d_ctx *ctx, mm3d_plane_stats *stats)
{
  if (!ctx || !stats) return MM3D_EINVAL;
  *stats = ctx->last_plane_stats;
  return MM3D_OK;
}

int mm3d_last_planes(const mm3d_ctx *ctx, mm3d_plane *planes, int capacity, int *n)
{
  if (!ctx || !planes || !n || capacity < 0) return MM3D_EINVAL;
  *n = ctx->last_plane_stats.planes;
  std::memcpy(planes, ctx->last_planes, (size_t)std::min(*n, capacity) * sizeof(mm3d_plane));
  return MM3D_OK;
}

}  // extern "C"

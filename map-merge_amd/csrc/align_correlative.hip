// align_correlative.hip -- the correlative coarse alignment, the opt-in initial estimate that reads no descriptors
// (mm3d_set_coarse_alignment; include/mm3d.h states the rule to the operation).  The maps come from robots that know gravity,
// so a pair's pose is close to a yaw and a shift in the plane: every yaw and shift is scored on a coarse 2-D occupancy of the
// vertical structure, as the correlative scan matchers of 2-D SLAM front ends do (Olson 2009), the best few are refined on
// the fine grid, and height and tilt are read off the two ground surfaces.  Not a reference stage (DESIGN.md section 7f,
// audit row 16c).  Everything that decides is an integer count: nothing depends on launch geometry or arrival order.
//
// The signature of a map, built once per map and option set (corr_build_signature), one host wait -- the one that sizes it:
//   corr_range      the 2-D cell index range of the counted points (lattice.hpp::k_lattice_range, as every stage of the global lattice)
//   k_corr_keys     a lane per point: ((cell relative to the range's minimum, i most significant) << 1) | class, class 0 =
//                   structure, 1 = ground; points of neither class get the key that sorts last
//   radix sort      (key, input index) pairs, stable: a (cell, class) becomes a run in ascending input index
//   scan_fused x 2  heads of the runs of one class that are at least min_points long (sorted keys: position + min_points - 1
//                   still holds the head's key) -> the start of every structure cell's run, of every ground cell's run, and
//                   their numbers
//   (the wait: range and counts; lists and dense maps are allocated)
//   k_corr_cells    a wave per cell: the run's length, and for a ground cell the mean z in double (lane l takes the run's
//                   positions l, l + 64, ..., the lanes meet in wave_sum's fixed butterfly, as k_ndt_voxels); lane 0 stores the
//                   list entry and the cell's word of the dense occupancy / height map, and flags the coarse cell
//   k_corr_dilate   a lane per dense cell: set when one of the 3 x 3 occupancy words around it is
//   scan_fused      the flagged coarse cells in ascending order; their number stays on the device
// A pair (corr_align), two host waits -- the candidate count, and the statistics:
//   k_corr_vote     blockIdx.y = the coarse yaw index, a lane per source coarse cell, the target's coarse cells through LDS in
//                   tiles of 256: one integer atomic per (source, target) on the accumulator acc[q][u][v]
//   scan_fused      the non-maximum test of every accumulator cell (27 loads) -> the candidates as (0xFFFFFFFF - votes, linear
//                   index) pairs in ascending index, and their number (the wait)
//   radix sort      stable, by the key: votes descending, index ascending
//   k_corr_fine     a block per (candidate, g): lanes over the source's fine structure cells, one rotation per cell, the
//                   (2F + 1)^2 shifts tested against the target's dilated map, wave ballots counted into LDS
//   k_corr_finish   one block: the winner (a 64-bit maximum of score << 32 | ~position), the ground pairs' nine sums in double
//                   in a fixed order, the 3 x 3 solve and the composition on one lane
#include <cmath>
#include <cstring>

#include "capi_guard.hpp"
#include "drivers.hpp"
#include "map_kept.hpp"
#include "icp_solve6.hpp"
#include "lattice.hpp"
#include "scan_fused.hpp"

namespace mm3d {

namespace {

// the dense maps hold one word per cell of the 2-D cell box: at most 2^24 cells; the accumulator at most 2^26 words
// (include/mm3d.h and INTEGRATION.md "Size limits" state both)
constexpr double kCorrMaxCells = 16777216.0;
constexpr double kCorrMaxAcc = 67108864.0;
// mm3d_set_coarse_alignment with cell = 0: the fine cell is params.resolution times this
constexpr double kCorrDefaultMultiple = 5.0;
constexpr int kCorrMaxF = 16;
constexpr int kCorrFitMin = 16;                       // ground pairs a plane fit needs
constexpr double kCorrMaxSlope = 0.36397023426620234;  // tan 20 deg

// the centre of cell i of side c: one add, one multiply
__device__ __forceinline__ float corr_centre(int i, float c) { return __fmul_rn(__fadd_rn((float)i, 0.5f), c); }
__host__ __device__ inline int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// the 2-D cell box of the range words is within the limits: its cells, and minima that the int arithmetic on them can take
// (false for the inf or NaN of an infinite index or an untouched range)
__host__ __device__ inline bool corr_fits(const LatticeFrame<2> &f)
{
  return f.cells <= kCorrMaxCells && fabs(f.mn[0]) < 1e9 && fabs(f.mn[1]) < 1e9;
}

// the counted points: finite, with a finite normal
struct CorrCounted {
  const float4 *nrm;
  __device__ __forceinline__ static bool ok(const float4 &p, const float4 &nr)
  {
    return isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(nr.x) && isfinite(nr.y) && isfinite(nr.z);
  }
  __device__ __forceinline__ bool operator()(int i, const float4 &p) const { return ok(p, nrm[i]); }
};

__global__ void __launch_bounds__(256)
k_corr_keys(const float4 *__restrict__ pts, const float4 *__restrict__ nrm, int n, float inv, float wall_nz, float ground_nz,
            const unsigned *__restrict__ range, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i], nr = nrm[i];
  vals[i] = (uint32_t)i;
  uint32_t key = kLatticeInvalid;
  if (CorrCounted::ok(p, nr)) {
    const float az = fabsf(nr.z);
    const int cls = az <= wall_nz ? 0 : az >= ground_nz ? 1 : -1;
    const LatticeFrame<2> f = lattice_frame<2>(range);
    if (cls >= 0 && corr_fits(f)) {                       // (a box beyond the limit: the host refuses it, the runs are not read)
      const uint32_t ri = (uint32_t)((double)lattice_index(p.x, inv) - f.mn[0]), rj = (uint32_t)((double)lattice_index(p.y, inv) - f.mn[1]);
      key = ((ri * (uint32_t)f.d[1] + rj) << 1) | (uint32_t)cls;      // < 2^25
    }
  }
  keys[i] = key;
}

// a cell of class `cls` starts where the sorted key changes to one of that class, and counts when min_points - 1 places
// further the key is still the same
struct CorrHeadLoad {
  const uint32_t *keys; size_t n; uint32_t cls; int min_points;
  __device__ __forceinline__ int operator()(size_t j) const
  {
    const uint32_t k = keys[j];
    if (k == kLatticeInvalid || (k & 1u) != cls || (j > 0 && keys[j - 1] == k)) return 0;
    const size_t last = j + (size_t)(min_points - 1);
    return last < n && keys[last] == k ? 1 : 0;
  }
};
struct CorrStartStore {
  size_t n; int *starts; unsigned *count;
  __device__ __forceinline__ void operator()(size_t j, int prefix, int v) const
  {
    if (v) starts[prefix] = (int)j;
    if (j == n - 1) *count = (unsigned)(prefix + v);
  }
  __device__ __forceinline__ void done() const {}
};

struct CorrDense { int mn[2], dims[2], cmn[2], cdims[2]; int umn[2]; int udy; int F; };   // umn / udy: the unpadded box the keys count from

__global__ void __launch_bounds__(256)
k_corr_cells(const float4 *__restrict__ pts, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ order, int n,
             const int *__restrict__ starts, int n_cells, int ground, CorrDense D, int4 *__restrict__ cells,
             unsigned char *__restrict__ occ, float *__restrict__ gh, int *__restrict__ cflag)
{
  const int lane = threadIdx.x & 63;
  const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (v >= n_cells) return;                              // (wave-uniform)
  const int b = starts[v];
  const uint32_t key = keys[b];
  int cnt = 0;
  double s = 0.0;
  for (int base = b; base < n; base += kWave) {          // the run ends where the key changes
    const int j = base + lane;
    const bool in = j < n && keys[j] == key;
    if (in) {
      ++cnt;
      if (ground) s += (double)pts[order[j]].z;
    }
    if (ballot(in) != ~0ull) break;
  }
  cnt = wave_sum(cnt);
  s = wave_sum(s);
  if (lane != 0) return;
  const uint32_t cell = key >> 1;
  const int i = D.umn[0] + (int)(cell / (uint32_t)D.udy), j = D.umn[1] + (int)(cell % (uint32_t)D.udy);
  const size_t word = (size_t)(i - D.mn[0]) * D.dims[1] + (j - D.mn[1]);
  if (ground) {
    const float h = (float)(s / (double)cnt);
    cells[v] = make_int4(i, j, cnt, __float_as_int(h));
    gh[word] = h;
  } else {
    cells[v] = make_int4(i, j, cnt, 0);
    occ[word] = 1;
    cflag[(size_t)(floor_div(i, D.F) - D.cmn[0]) * D.cdims[1] + (floor_div(j, D.F) - D.cmn[1])] = 1;   // (every writer stores 1)
  }
}

__global__ void __launch_bounds__(256)
k_corr_dilate(const unsigned char *__restrict__ occ, int d0, int d1, unsigned char *__restrict__ dil)
{
  const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= (size_t)d0 * d1) return;
  const int i = (int)(w / (size_t)d1), j = (int)(w % (size_t)d1);
  unsigned char any = 0;
  for (int a = max(i - 1, 0); a <= min(i + 1, d0 - 1); ++a)
    for (int b = max(j - 1, 0); b <= min(j + 1, d1 - 1); ++b) any |= occ[(size_t)a * d1 + b];
  dil[w] = any;
}

struct CorrFlagLoad {
  const int *flag;
  __device__ __forceinline__ int operator()(size_t j) const { return flag[j]; }
};
struct CorrCoarseStore {
  size_t n; int cmn0, cmn1, cd1; int2 *cells; int *count;
  __device__ __forceinline__ void operator()(size_t j, int prefix, int v) const
  {
    if (v) cells[prefix] = make_int2(cmn0 + (int)(j / (size_t)cd1), cmn1 + (int)(j % (size_t)cd1));
    if (j == n - 1) *count = prefix + v;
  }
  __device__ __forceinline__ void done() const {}
};

// ---------------------------------------------------------------- the pair
struct CorrPair {
  float c, inv, C, invC;
  int F, G, Q, yaw_steps;
  int u0, v0, U, V;                                     // the accumulator's box
  const float2 *yaw;                                    // [yaw_steps] (cs, sn)
};

__global__ void __launch_bounds__(256)
k_corr_vote(CorrPair P, const int2 *__restrict__ src, const int *__restrict__ n_src, const int2 *__restrict__ tgt,
            const int *__restrict__ n_tgt, int *__restrict__ acc)
{
  __shared__ float2 tile[256];
  const int ns = *n_src, nt = *n_tgt;
  if ((int)(blockIdx.x * blockDim.x) >= ns) return;      // (block-uniform: the grid covers the list's capacity)
  const int q = blockIdx.y;
  const float2 y = P.yaw[q * P.G];
  const int si = blockIdx.x * blockDim.x + threadIdx.x;
  float rx = 0.f, ry = 0.f;
  if (si < ns) {
    const int2 sc = src[si];
    const float px = corr_centre(sc.x, P.C), py = corr_centre(sc.y, P.C);
    rx = __fsub_rn(__fmul_rn(y.x, px), __fmul_rn(y.y, py));
    ry = __fadd_rn(__fmul_rn(y.y, px), __fmul_rn(y.x, py));
  }
  int *__restrict__ plane = acc + (size_t)q * P.U * P.V;
  for (int base = 0; base < nt; base += 256) {
    __syncthreads();
    if (base + (int)threadIdx.x < nt) {
      const int2 tc = tgt[base + threadIdx.x];
      tile[threadIdx.x] = make_float2(corr_centre(tc.x, P.C), corr_centre(tc.y, P.C));
    }
    __syncthreads();
    if (si >= ns) continue;
    const int m = min(256, nt - base);
    for (int k = 0; k < m; ++k) {
      const float2 t = tile[k];
      const float uf = floorf(__fadd_rn(__fmul_rn(__fsub_rn(t.x, rx), P.invC), 0.5f));
      const float vf = floorf(__fadd_rn(__fmul_rn(__fsub_rn(t.y, ry), P.invC), 0.5f));
      const float ur = uf - (float)P.u0, vr = vf - (float)P.v0;      // (integer-valued and small: exact)
      if (ur >= 0.0f && ur < (float)P.U && vr >= 0.0f && vr < (float)P.V) atomicAdd(&plane[(int)ur * P.V + (int)vr], 1);
    }
  }
}

// the non-maximum test of accumulator cell `idx`: its votes when it is a candidate, else 0
__device__ __forceinline__ int corr_nms(const int *__restrict__ acc, int Q, int U, int V, size_t idx)
{
  const int votes = acc[idx];
  if (votes < 1) return 0;
  const int v = (int)(idx % (size_t)V), u = (int)(idx / (size_t)V % (size_t)U), q = (int)(idx / ((size_t)V * U));
  for (int dq = -1; dq <= 1; ++dq) {
    const int qq = (q + dq + Q) % Q;
    for (int uu = max(u - 1, 0); uu <= min(u + 1, U - 1); ++uu)
      for (int vv = max(v - 1, 0); vv <= min(v + 1, V - 1); ++vv) {
        const size_t o = ((size_t)qq * U + uu) * V + vv;
        if (o == idx) continue;
        const int ov = acc[o];
        if (ov > votes || (ov == votes && o < idx)) return 0;
      }
  }
  return votes;
}
struct CorrNmsLoad {
  const int *acc; int Q, U, V;
  __device__ __forceinline__ int operator()(size_t j) const { return corr_nms(acc, Q, U, V, j) > 0 ? 1 : 0; }
};
struct CorrNmsStore {
  const int *acc; size_t n; size_t cap; uint32_t *keys, *vals; int *count;
  __device__ __forceinline__ void operator()(size_t j, int prefix, int v) const
  {
    if (v && (size_t)prefix < cap) { keys[prefix] = 0xFFFFFFFFu - (uint32_t)acc[j]; vals[prefix] = (uint32_t)j; }
    if (j == n - 1) *count = prefix + v;
  }
  __device__ __forceinline__ void done() const {}
};

struct CorrDenseView { int mn[2], dims[2]; const unsigned char *dil; const float *gh; };

__global__ void __launch_bounds__(256)
k_corr_fine(CorrPair P, const uint32_t *__restrict__ cand, const int4 *__restrict__ scells, int ns, CorrDenseView T,
            int *__restrict__ scores)
{
  __shared__ int cnt[(2 * kCorrMaxF + 1) * (2 * kCorrMaxF + 1)];
  const int W = 2 * P.F + 1, W2 = W * W;
  for (int k = threadIdx.x; k < W2; k += blockDim.x) cnt[k] = 0;
  __syncthreads();
  const uint32_t idx = cand[blockIdx.x];
  const int v = (int)(idx % (uint32_t)P.V) + P.v0, u = (int)(idx / (uint32_t)P.V % (uint32_t)P.U) + P.u0, q = (int)(idx / ((uint32_t)P.V * P.U));
  const int g = (int)blockIdx.y - P.G;
  const float2 y = P.yaw[((q * P.G + g) % P.yaw_steps + P.yaw_steps) % P.yaw_steps];
  const int lane = threadIdx.x & 63;
  for (int base = 0; base < ns; base += blockDim.x) {    // (whole waves: the ballots below want every lane)
    const int si = base + threadIdx.x;
    float rx = 0.f, ry = 0.f;
    if (si < ns) {
      const int4 sc = scells[si];
      const float px = corr_centre(sc.x, P.c), py = corr_centre(sc.y, P.c);
      rx = __fsub_rn(__fmul_rn(y.x, px), __fmul_rn(y.y, py));
      ry = __fadd_rn(__fmul_rn(y.y, px), __fmul_rn(y.x, py));
    }
    for (int a = -P.F; a <= P.F; ++a) {
      const float ci = lattice_index(__fadd_rn(rx, __fmul_rn((float)(u * P.F + a), P.c)), P.inv) - (float)T.mn[0];
      const bool in_i = si < ns && ci >= 0.0f && ci < (float)T.dims[0];
      for (int b = -P.F; b <= P.F; ++b) {
        const float cj = lattice_index(__fadd_rn(ry, __fmul_rn((float)(v * P.F + b), P.c)), P.inv) - (float)T.mn[1];
        const bool hit = in_i && cj >= 0.0f && cj < (float)T.dims[1] && T.dil[(size_t)(int)ci * T.dims[1] + (int)cj] != 0;
        const int c = __popcll(ballot(hit));
        if (lane == 0 && c) atomicAdd(&cnt[(a + P.F) * W + (b + P.F)], c);
      }
    }
  }
  __syncthreads();
  int *out = scores + ((size_t)blockIdx.x * (2 * P.G + 1) + blockIdx.y) * W2;
  for (int k = threadIdx.x; k < W2; k += blockDim.x) out[k] = cnt[k];
}

struct CorrResult { float T[16]; mm3d_coarse_stats stats; };

// a 3 x 3 symmetric system by the unpivoted LDLt of icp_solve6.hpp, its pivot rule against `floor`
__device__ static bool solve3_ldlt(const double A[9], const double b[3], double floor, double x[3])
{
  double L[9], D[3];
  for (int j = 0; j < 3; ++j) {
    double d = A[j * 3 + j];
    for (int k = 0; k < j; ++k) d -= L[j * 3 + k] * L[j * 3 + k] * D[k];
    if (!(d > floor)) return false;
    D[j] = d;
    for (int i = j + 1; i < 3; ++i) {
      double s = A[i * 3 + j];
      for (int k = 0; k < j; ++k) s -= L[i * 3 + k] * L[j * 3 + k] * D[k];
      L[i * 3 + j] = s / d;
    }
  }
  double y[3];
  for (int i = 0; i < 3; ++i) {
    double s = b[i];
    for (int k = 0; k < i; ++k) s -= L[i * 3 + k] * y[k];
    y[i] = s;
  }
  for (int i = 2; i >= 0; --i) {
    double s = y[i] / D[i];
    for (int k = i + 1; k < 3; ++k) s -= L[k * 3 + i] * x[k];
    x[i] = s;
  }
  return true;
}

__global__ void __launch_bounds__(256)
k_corr_finish(CorrPair P, const uint32_t *__restrict__ cand_keys, const uint32_t *__restrict__ cand, int n_cand,
              const int *__restrict__ scores, const int4 *__restrict__ gcells, int ng, CorrDenseView T, int ns, int nt,
              double accept_fraction, CorrResult *__restrict__ out)
{
  __shared__ unsigned long long s_best[4];
  __shared__ double red[4][9];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int W = 2 * P.F + 1, W2 = W * W, GW = 2 * P.G + 1;
  const size_t total = (size_t)n_cand * GW * W2;          // < 2^32 (1024 x 33 x 1089)
  unsigned long long best = 0ull;
  for (size_t k = threadIdx.x; k < total; k += blockDim.x) {
    const unsigned long long key = ((unsigned long long)(uint32_t)scores[k] << 32) | (uint32_t)~(uint32_t)k;
    best = key > best ? key : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o, kWave);
    best = other > best ? other : best;
  }
  if (lane == 0) s_best[wave] = best;
  __syncthreads();
  best = s_best[0];
  for (int w = 1; w < 4; ++w) best = s_best[w] > best ? s_best[w] : best;
  const int score = (int)(best >> 32);
  const uint32_t pos = ~(uint32_t)(best & 0xFFFFFFFFull);
  const int b = (int)(pos % (uint32_t)W) - P.F, a = (int)(pos / (uint32_t)W % (uint32_t)W) - P.F;
  const int g = (int)(pos / (uint32_t)W2 % (uint32_t)GW) - P.G, rank = (int)(pos / ((uint32_t)W2 * GW));
  const uint32_t idx = cand[rank];
  const int v = (int)(idx % (uint32_t)P.V) + P.v0, u = (int)(idx / (uint32_t)P.V % (uint32_t)P.U) + P.u0, q = (int)(idx / ((uint32_t)P.V * P.U));
  const int kyaw = ((q * P.G + g) % P.yaw_steps + P.yaw_steps) % P.yaw_steps;
  const float2 y = P.yaw[kyaw];
  const float sx = __fmul_rn((float)(u * P.F + a), P.c), sy = __fmul_rn((float)(v * P.F + b), P.c);

  // the ground pairs: n, x, y, xx, xy, yy, d, xd, yd
  double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = threadIdx.x; k < ng; k += blockDim.x) {
    const int4 gc = gcells[k];
    const float px = corr_centre(gc.x, P.c), py = corr_centre(gc.y, P.c);
    const float xf = __fadd_rn(__fsub_rn(__fmul_rn(y.x, px), __fmul_rn(y.y, py)), sx);
    const float yf = __fadd_rn(__fadd_rn(__fmul_rn(y.y, px), __fmul_rn(y.x, py)), sy);
    const float ci = lattice_index(xf, P.inv) - (float)T.mn[0], cj = lattice_index(yf, P.inv) - (float)T.mn[1];
    if (!(ci >= 0.0f && ci < (float)T.dims[0] && cj >= 0.0f && cj < (float)T.dims[1])) continue;
    const float ht = T.gh[(size_t)(int)ci * T.dims[1] + (int)cj];
    if (!(ht == ht)) continue;                            // NaN: no ground cell there
    const double d = (double)ht - (double)__int_as_float(gc.w), xd = (double)xf, yd = (double)yf;
    acc[0] += 1.0; acc[1] += xd; acc[2] += yd; acc[3] += xd * xd; acc[4] += xd * yd; acc[5] += yd * yd;
    acc[6] += d; acc[7] += xd * d; acc[8] += yd * d;
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const double s = wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double S[9];
  for (int k = 0; k < 9; ++k) S[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  const int n = (int)S[0];
  double alpha = 0.0, beta = 0.0, gamma = n > 0 ? S[6] / S[0] : 0.0;
  if (n >= kCorrFitMin) {
    const double A[9] = {S[3], S[4], S[1], S[4], S[5], S[2], S[1], S[2], S[0]}, rhs[3] = {S[7], S[8], S[6]};
    double x[3];
    if (solve3_ldlt(A, rhs, kPlanePivotTau * (S[3] + S[5] + S[0]) / 3.0, x) && isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]) &&
        sqrt(x[0] * x[0] + x[1] * x[1]) <= kCorrMaxSlope) {
      alpha = x[0]; beta = x[1]; gamma = x[2];
    }
  }
  // Trans(0, 0, gamma) Rx(atan beta) Ry(-atan alpha) [Rz | s]
  const double ia = 1.0 / sqrt(1.0 + alpha * alpha), ib = 1.0 / sqrt(1.0 + beta * beta);
  const double cphi = ia, sphi = -alpha * ia, cpsi = ib, spsi = beta * ib;       // Ry's angle phi = -atan alpha, Rx's psi = atan beta
  const double M[9] = {cphi, 0.0, sphi,
                       spsi * sphi, cpsi, -spsi * cphi,
                       -cpsi * sphi, spsi, cpsi * cphi};                          // Rx Ry, row-major
  const double cs = (double)y.x, sn = (double)y.y;
  const double Rz[9] = {cs, -sn, 0.0, sn, cs, 0.0, 0.0, 0.0, 1.0};
  const double sh[3] = {(double)sx, (double)sy, 0.0};
  CorrResult r;
  for (int row = 0; row < 3; ++row) {
    for (int col = 0; col < 3; ++col)
      r.T[col * 4 + row] = (float)((M[row * 3] * Rz[col] + M[row * 3 + 1] * Rz[3 + col]) + M[row * 3 + 2] * Rz[6 + col]);
    r.T[12 + row] = (float)(((M[row * 3] * sh[0] + M[row * 3 + 1] * sh[1]) + M[row * 3 + 2] * sh[2]) + (row == 2 ? gamma : 0.0));
  }
  r.T[3] = r.T[7] = r.T[11] = 0.0f;
  r.T[15] = 1.0f;
  r.stats.source_cells = ns;
  r.stats.target_cells = nt;
  r.stats.coarse_votes = (int)(0xFFFFFFFFu - cand_keys[rank]);
  r.stats.candidates = n_cand;
  r.stats.score = score;
  r.stats.yaw_index = kyaw;
  r.stats.ground_pairs = n;
  r.stats.converged = (double)score >= accept_fraction * (double)ns ? 1 : 0;
  *out = r;
}

// ---------------------------------------------------------------- host
// everything but the cell's "0 = default", which only mm3d_set_coarse_alignment admits
bool corr_options_ok(const mm3d_coarse_options *o)
{
  if (!o || (o->method != MM3D_COARSE_NONE && o->method != MM3D_COARSE_CORRELATIVE)) return false;
  if (o->cell_factor < 1 || o->cell_factor > kCorrMaxF) return false;
  if (o->yaw_steps < 8 || o->yaw_steps > 7200 || o->yaw_factor < 1 || o->yaw_steps % o->yaw_factor != 0) return false;
  if (o->candidates < 1 || o->candidates > 1024 || o->min_points < 1) return false;
  if (!(o->wall_nz >= 0.0 && o->wall_nz <= 1.0) || !(o->ground_nz > o->wall_nz && o->ground_nz <= 1.0)) return false;   // (false for NaN)
  return o->accept_fraction >= 0.0 && o->accept_fraction <= 1.0;
}

bool corr_same_options(const mm3d_coarse_options &a, const mm3d_coarse_options &b)
{
  // what a signature depends on (the search's options are read per pair)
  return a.cell == b.cell && a.cell_factor == b.cell_factor && a.wall_nz == b.wall_nz && a.ground_nz == b.ground_nz && a.min_points == b.min_points;
}

// The signature of `pts` with normals `nrm` (one per point): complete on c's stream on return (the caller waits before anybody
// else reads it).  o.cell > 0.
std::unique_ptr<CoarseSignature> corr_build_signature(Context *c, const mm3d_cloud *pts, const mm3d_normals *nrm, const mm3d_coarse_options &o)
{
  MM3D_REQUIRE(lattice_side_ok(o.cell), "correlative alignment: the cell must be positive and finite, as a float and its reciprocal too");
  MM3D_REQUIRE(nrm->n == pts->n, "correlative alignment: one normal per point");
  MM3D_REQUIRE(pts->n < ((size_t)1 << 31), "correlative alignment: more than 2^31 - 1 points");
  std::unique_ptr<CoarseSignature> sg(new CoarseSignature());
  sg->opt = o;
  sg->c = (float)o.cell;
  sg->inv = 1.0f / sg->c;
  const int n = (int)pts->n;
  if (n == 0) return sg;
  const unsigned blocks = div_up((size_t)n, 256);
  DevBuf<unsigned> range(c, 8);                           // min i j, max i j | structure cells, ground cells
  lattice_range<2>(c, "corr_range", n * 32.0, pts->pts.get(), n, sg->inv, CorrCounted{nrm->nrm.get()}, range.get());
  DevBuf<uint32_t> keys(c, n), vals(c, n), keys2(c, n), vals2(c, n);
  MM3D_LAUNCH(c, "corr_keys", n * 40.0, k_corr_keys, dim3(blocks), dim3(256), 0, pts->pts.get(), nrm->nrm.get(), n, sg->inv, (float)o.wall_nz,
              (float)o.ground_nz, (const unsigned *)range.get(), keys.get(), vals.get());
  sort_pairs_u32(c, keys.get(), keys2.get(), vals.get(), vals2.get(), (size_t)n, 32);
  DevBuf<int> sstarts(c, n), gstarts(c, n);               // (at most one cell per point)
  scan_fused(c, "corr_runs", n * 8.0, (size_t)n, CorrHeadLoad{keys2.get(), (size_t)n, 0u, o.min_points},
             CorrStartStore{(size_t)n, sstarts.get(), range.get() + 4});
  scan_fused(c, "corr_runs", n * 8.0, (size_t)n, CorrHeadLoad{keys2.get(), (size_t)n, 1u, o.min_points},
             CorrStartStore{(size_t)n, gstarts.get(), range.get() + 5});
  unsigned *hr = (unsigned *)c->pin(64);
  MM3D_HIP(hipMemcpyAsync(hr, range.get(), 32, hipMemcpyDeviceToHost, c->stream));
  c->sync();                                              // the one wait: what sizes the signature
  const int ns = (int)hr[4], ng = (int)hr[5];
  if (ns == 0 && ng == 0) return sg;                      // no cell of either class (no counted point among them)
  const LatticeFrame<2> f = lattice_frame<2>(hr);
  if (!corr_fits(f))
    throw Error(MM3D_EUNSUPPORTED, "correlative alignment: the map's 2-D cell box holds more than 2^24 cells at this cell size");
  CorrDense D;
  for (int a = 0; a < 2; ++a) {
    D.umn[a] = (int)f.mn[a];
    D.mn[a] = sg->mn[a] = D.umn[a] - 1;                   // one cell of padding: the dilation, and lookups just outside
    D.dims[a] = sg->dims[a] = (int)f.d[a] + 2;
    D.cmn[a] = sg->cmn[a] = floor_div(D.umn[a], o.cell_factor);
    D.cdims[a] = sg->cdims[a] = floor_div(D.umn[a] + (int)f.d[a] - 1, o.cell_factor) - D.cmn[a] + 1;
  }
  D.udy = (int)f.d[1];
  D.F = o.cell_factor;
  sg->n_struct = ns; sg->n_ground = ng;
  const size_t words = (size_t)D.dims[0] * D.dims[1], cwords = (size_t)D.cdims[0] * D.cdims[1];
  sg->scells = DevBuf<int4>(c, (size_t)ns);
  sg->gcells = DevBuf<int4>(c, (size_t)ng);
  sg->ccells = DevBuf<int2>(c, std::min((size_t)ns, cwords));
  sg->n_coarse = DevBuf<int>(c, 1);
  sg->dil = DevBuf<unsigned char>(c, words);
  sg->gh = DevBuf<float>(c, words);
  DevBuf<unsigned char> occ(c, words);
  DevBuf<int> cflag(c, cwords);
  MM3D_HIP(hipMemsetAsync(occ.get(), 0, words, c->stream));
  MM3D_HIP(hipMemsetAsync(sg->gh.get(), 0xFF, words * sizeof(float), c->stream));    // NaN: no ground cell
  MM3D_HIP(hipMemsetAsync(cflag.get(), 0, cwords * sizeof(int), c->stream));
  MM3D_HIP(hipMemsetAsync(sg->n_coarse.get(), 0, sizeof(int), c->stream));
  if (ns)
    MM3D_LAUNCH(c, "corr_cells", ns * 64.0, k_corr_cells, dim3(div_up((size_t)ns, 4)), dim3(256), 0, pts->pts.get(), (const uint32_t *)keys2.get(),
                (const uint32_t *)vals2.get(), n, (const int *)sstarts.get(), ns, 0, D, sg->scells.get(), occ.get(), sg->gh.get(), cflag.get());
  if (ng)
    MM3D_LAUNCH(c, "corr_cells", ng * 64.0, k_corr_cells, dim3(div_up((size_t)ng, 4)), dim3(256), 0, pts->pts.get(), (const uint32_t *)keys2.get(),
                (const uint32_t *)vals2.get(), n, (const int *)gstarts.get(), ng, 1, D, sg->gcells.get(), occ.get(), sg->gh.get(), cflag.get());
  MM3D_LAUNCH(c, "corr_dilate", words * 10.0, k_corr_dilate, dim3(div_up(words, 256)), dim3(256), 0, (const unsigned char *)occ.get(), D.dims[0],
              D.dims[1], sg->dil.get());
  scan_fused(c, "corr_coarse", cwords * 4.0, cwords, CorrFlagLoad{cflag.get()},
             CorrCoarseStore{cwords, D.cmn[0], D.cmn[1], D.cdims[1], sg->ccells.get(), sg->n_coarse.get()});
  c->settle();                                            // (the sort's buffers go back to the pool)
  return sg;
}

void corr_identity(float T[16])
{
  std::memset(T, 0, sizeof(float) * 16);
  T[0] = T[5] = T[10] = T[15] = 1.0f;
}

// what the debug hook of the search takes home
struct CorrDebug {
  int q = 0; int *frame = nullptr; int *acc = nullptr; size_t acc_cap = 0; int *cands = nullptr; int *scores = nullptr; size_t cand_cap = 0;
  size_t *n_cands = nullptr;
};

// the whole search of a pair; f as estimate_pair_front leaves it
void corr_align(Context *c, const mm3d_coarse_options &o, const CoarseSignature &S, const CoarseSignature &Tg, PairFront &f,
                mm3d_coarse_stats *stats, const CorrDebug *dbg = nullptr)
{
  corr_identity(f.T0);
  f.on_device = false;
  f.sac_h = 0;
  mm3d_coarse_stats st{S.n_struct, Tg.n_struct, 0, 0, 0, -1, 0, 0};
  if (stats) *stats = st;
  if (dbg) { std::memset(dbg->frame, 0, sizeof(int) * 5); *dbg->n_cands = 0; }
  if (S.n_struct == 0 || Tg.n_struct == 0) return;
  const int F = o.cell_factor, G = o.yaw_factor, Q = o.yaw_steps / G;
  CorrPair P;
  P.c = S.c; P.inv = S.inv;
  P.C = P.c * (float)F; P.invC = 1.0f / P.C;
  P.F = F; P.G = G; P.Q = Q; P.yaw_steps = o.yaw_steps;
  // the accumulator's box from the two coarse frames: every rotated source centre lies within the largest corner radius
  // of the source's coarse box, so d = t - r lies in the target's box widened by it (two cells of margin for the rounding)
  const double C = (double)P.C;
  double R = 0.0;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) {
      const double x = ((double)(S.cmn[0] + (a ? S.cdims[0] - 1 : 0)) + 0.5) * C, y = ((double)(S.cmn[1] + (b ? S.cdims[1] - 1 : 0)) + 0.5) * C;
      R = std::max(R, std::sqrt(x * x + y * y));
    }
  const double Rc = R / C;
  double lo[2], hi[2];
  for (int a = 0; a < 2; ++a) {
    lo[a] = std::floor((double)Tg.cmn[a] + 0.5 - Rc) - 2.0;
    hi[a] = std::ceil((double)(Tg.cmn[a] + Tg.cdims[a] - 1) + 0.5 + Rc) + 2.0;
  }
  const double Ud = hi[0] - lo[0] + 1.0, Vd = hi[1] - lo[1] + 1.0;
  if (!((double)Q * Ud * Vd <= kCorrMaxAcc) || !(std::fabs(lo[0]) < 1e8 && std::fabs(lo[1]) < 1e8 && std::fabs(hi[0]) < 1e8 && std::fabs(hi[1]) < 1e8))
    throw Error(MM3D_EUNSUPPORTED, "correlative alignment: the pair's coarse accumulator needs more than 2^26 words");
  P.u0 = (int)lo[0]; P.v0 = (int)lo[1]; P.U = (int)Ud; P.V = (int)Vd;
  // the fine shifts (u F + a) are formed in int
  MM3D_REQUIRE(std::fabs(lo[0]) * F < 1e9 && std::fabs(hi[0]) * F < 1e9 && std::fabs(lo[1]) * F < 1e9 && std::fabs(hi[1]) * F < 1e9,
               "correlative alignment: shifts out of range");
  // a position in the score cubes is a 32-bit word of the winner's key
  if (!((double)o.candidates * (2.0 * G + 1.0) * (2.0 * F + 1.0) * (2.0 * F + 1.0) < 2147483648.0))
    throw Error(MM3D_EUNSUPPORTED, "correlative alignment: candidates x (2G + 1) x (2F + 1)^2 fine scores need more than 2^31 words");
  const size_t words = (size_t)Q * P.U * P.V;

  // the yaw table, in double on the host
  float2 *hy = (float2 *)c->pin(sizeof(float2) * (size_t)o.yaw_steps);
  for (int k = 0; k < o.yaw_steps; ++k) {
    const double th = 2.0 * M_PI * (double)k / (double)o.yaw_steps;
    hy[k] = make_float2((float)std::cos(th), (float)std::sin(th));
  }
  DevBuf<float2> yaw(c, (size_t)o.yaw_steps);
  MM3D_HIP(hipMemcpyAsync(yaw.get(), hy, sizeof(float2) * (size_t)o.yaw_steps, hipMemcpyHostToDevice, c->stream));
  P.yaw = yaw.get();

  DevBuf<int> acc(c, words);
  MM3D_HIP(hipMemsetAsync(acc.get(), 0, words * sizeof(int), c->stream));
  const size_t src_cap = S.ccells.size();
  MM3D_LAUNCH(c, "corr_vote", (double)Q * (double)src_cap * (double)Tg.ccells.size() * 4.0, k_corr_vote, dim3(div_up(src_cap, 256), Q), dim3(256), 0, P,
              (const int2 *)S.ccells.get(), (const int *)S.n_coarse.get(), (const int2 *)Tg.ccells.get(), (const int *)Tg.n_coarse.get(), acc.get());
  // candidates: no two of them are neighbours, so every aligned 2 x 2 x 2 block of the accumulator holds at most one
  const size_t cap = (size_t)((Q + 1) / 2) * (size_t)((P.U + 1) / 2) * (size_t)((P.V + 1) / 2);
  DevBuf<uint32_t> ck(c, cap), cv(c, cap);
  DevBuf<int> n_cand_dev(c, 1);
  scan_fused(c, "corr_nms", words * 112.0, words, CorrNmsLoad{acc.get(), Q, P.U, P.V},
             CorrNmsStore{acc.get(), words, cap, ck.get(), cv.get(), n_cand_dev.get()});
  int *hn = (int *)c->pin(64);
  MM3D_HIP(hipMemcpyAsync(hn, n_cand_dev.get(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
  c->sync();                                              // the first wait: how many candidates
  const int M = hn[0];
  if (M <= 0 || (size_t)M > cap) throw Error(MM3D_EDEVICE, "correlative alignment: the candidate count is out of range");
  DevBuf<uint32_t> ck2(c, (size_t)M), cv2(c, (size_t)M);
  sort_pairs_u32(c, ck.get(), ck2.get(), cv.get(), cv2.get(), (size_t)M, 32);
  const int K = std::min(M, o.candidates);
  const int W = 2 * F + 1, GW = 2 * G + 1;
  DevBuf<int> scores(c, (size_t)K * GW * W * W);
  CorrDenseView TV;
  for (int a = 0; a < 2; ++a) { TV.mn[a] = Tg.mn[a]; TV.dims[a] = Tg.dims[a]; }
  TV.dil = Tg.dil.get(); TV.gh = Tg.gh.get();
  MM3D_LAUNCH(c, "corr_fine", (double)K * GW * (double)S.n_struct * (16.0 + W * W), k_corr_fine, dim3((unsigned)K, (unsigned)GW), dim3(256), 0, P,
              (const uint32_t *)cv2.get(), (const int4 *)S.scells.get(), S.n_struct, TV, scores.get());
  DevBuf<CorrResult> res(c, 1);
  MM3D_LAUNCH(c, "corr_finish", (double)K * GW * W * W * 4.0 + S.n_ground * 20.0, k_corr_finish, dim3(1), dim3(256), 0, P, (const uint32_t *)ck2.get(),
              (const uint32_t *)cv2.get(), K, (const int *)scores.get(), (const int4 *)S.gcells.get(), S.n_ground, TV, S.n_struct, Tg.n_struct,
              o.accept_fraction, res.get());
  CorrResult *hres = (CorrResult *)c->pin(sizeof(CorrResult));
  MM3D_HIP(hipMemcpyAsync(hres, res.get(), sizeof(CorrResult), hipMemcpyDeviceToHost, c->stream));
  f.dT0 = DevBuf<float>(c, 16);
  MM3D_HIP(hipMemcpyAsync(f.dT0.get(), res.get(), sizeof(float) * 16, hipMemcpyDeviceToDevice, c->stream));
  std::vector<uint32_t> hk, hv;
  if (dbg) {
    const int frame[5] = {Q, P.u0, P.v0, P.U, P.V};
    std::memcpy(dbg->frame, frame, sizeof(frame));
    const size_t plane = (size_t)P.U * P.V;
    if (dbg->acc && dbg->acc_cap >= plane && dbg->q >= 0 && dbg->q < Q)
      MM3D_HIP(hipMemcpyAsync(dbg->acc, acc.get() + (size_t)dbg->q * plane, plane * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    const size_t take = std::min((size_t)K, dbg->cand_cap);
    hk.resize(take); hv.resize(take);
    if (take) {
      MM3D_HIP(hipMemcpyAsync(hk.data(), ck2.get(), take * 4, hipMemcpyDeviceToHost, c->stream));
      MM3D_HIP(hipMemcpyAsync(hv.data(), cv2.get(), take * 4, hipMemcpyDeviceToHost, c->stream));
      if (dbg->scores)
        MM3D_HIP(hipMemcpyAsync(dbg->scores, scores.get(), take * GW * W * W * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
  }
  c->sync();                                              // the second wait: the statistics
  f.on_device = true;
  if (stats) *stats = hres->stats;
  if (dbg) {
    *dbg->n_cands = (size_t)K;
    for (size_t r = 0; r < hv.size() && dbg->cands; ++r) {
      const uint32_t idx = hv[r];
      dbg->cands[4 * r] = (int)(idx / ((uint32_t)P.V * P.U));
      dbg->cands[4 * r + 1] = (int)(idx / (uint32_t)P.V % (uint32_t)P.U) + P.u0;
      dbg->cands[4 * r + 2] = (int)(idx % (uint32_t)P.V) + P.v0;
      dbg->cands[4 * r + 3] = (int)(0xFFFFFFFFu - hk[r]);
    }
  }
}

mm3d_coarse_options corr_resolved(const mm3d_coarse_options &o, const mm3d_params *p)
{
  mm3d_coarse_options r = o;
  if (!(r.cell > 0.0)) r.cell = kCorrDefaultMultiple * p->resolution;
  return r;
}

struct CoarseCorrelative final : CoarseMethodBase {
  // the map's signature at the context's options, and the normals it is made from (map_kept.hpp)
  const CoarseSignature *signature(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p) const
  {
    const mm3d_coarse_options o = corr_resolved(ctx->sel.coarse_options, p);
    return map_kept(
        ctx, m, &mm3d_map::coarse, [&](const CoarseSignature &h) { return corr_same_options(h.opt, o); },
        [&] { return corr_build_signature(ctx, m->points, map_normals(ctx, m, p), o); });
  }
  void prepare(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p) const override { (void)signature(ctx, m, p); }
  void front(mm3d_ctx *ctx, const mm3d_map *s, const mm3d_map *t, const mm3d_params *p, PairFront &f, mm3d_coarse_stats *stats) const override
  {
    const CoarseSignature *S = signature(ctx, s, p), *T = signature(ctx, t, p);
    corr_align(ctx, corr_resolved(ctx->sel.coarse_options, p), *S, *T, f, stats);
  }
};
const CoarseCorrelative g_correlative;

// the stand-alone calls' argument check: MM3D_OK, or the status and the context's error text
int corr_call_check(mm3d_ctx *ctx, const mm3d_cloud *s, const mm3d_normals *sn, const mm3d_cloud *t, const mm3d_normals *tn,
                    const mm3d_coarse_options *o)
{
  if (!ctx || !s || !sn || !corr_options_ok(o) || !lattice_side_ok(o->cell)) return MM3D_EINVAL;
  if ((t || tn) && (!t || !tn)) return MM3D_EINVAL;
  if (sn->n != s->n || (t && tn->n != t->n)) {
    ctx->err = "correlative alignment: the normals must be one per point";
    return MM3D_EINVAL;
  }
  return MM3D_OK;
}

}  // namespace

}  // namespace mm3d

using namespace mm3d;

extern "C" {

int mm3d_set_coarse_alignment(mm3d_ctx *ctx, const mm3d_coarse_options *options)
{
  if (!ctx || !corr_options_ok(options)) return MM3D_EINVAL;
  if (options->cell != 0.0 && !lattice_side_ok(options->cell)) return MM3D_EINVAL;     // (also catches NaN)
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the method changes)
  return select_stage(ctx, Stage::Coarse, [&](StageSelection &s) {
    s.coarse_options = *options;
    s.coarse = stage_active(Stage::Coarse, s) ? &g_correlative : nullptr;
  });
}

int mm3d_get_coarse_alignment(const mm3d_ctx *ctx, mm3d_coarse_options *options)
{
  if (!ctx || !options) return MM3D_EINVAL;
  *options = ctx->sel.coarse_options;
  return MM3D_OK;
}

int mm3d_last_coarse_stats(const mm3d_ctx *ctx, mm3d_coarse_stats *stats)
{
  if (!ctx || !stats) return MM3D_EINVAL;
  *stats = ctx->last_coarse_stats;
  return MM3D_OK;
}

int mm3d_estimate_transform_correlative(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_normals *source_normals, const mm3d_cloud *target,
                                        const mm3d_normals *target_normals, const mm3d_coarse_options *options, float T[16],
                                        mm3d_coarse_stats *stats)
{
  if (!target || !target_normals || !T) return MM3D_EINVAL;
  const int st = corr_call_check(ctx, source, source_normals, target, target_normals, options);
  if (st != MM3D_OK) return st;
  return guarded(ctx, [&] {
    std::unique_ptr<CoarseSignature> S = corr_build_signature(ctx, source, source_normals, *options);
    std::unique_ptr<CoarseSignature> Tg = corr_build_signature(ctx, target, target_normals, *options);
    PairFront f;
    corr_align(ctx, *options, *S, *Tg, f, &ctx->last_coarse_stats);
    if (stats) *stats = ctx->last_coarse_stats;
    std::memcpy(T, f.T0, sizeof(f.T0));
    if (f.on_device) {
      float *hT = (float *)ctx->pin(64);
      MM3D_HIP(hipMemcpyAsync(hT, f.dT0.get(), sizeof(float) * 16, hipMemcpyDeviceToHost, ctx->stream));
      ctx->sync();
      std::memcpy(T, hT, sizeof(float) * 16);
    }
  });
}

int mm3d_debug_correlative_signature(mm3d_ctx *ctx, const mm3d_cloud *points, const mm3d_normals *normals, const mm3d_coarse_options *options,
                                     int *structure, int *ground, float *ground_height, int *coarse, size_t cap, size_t n[3])
{
  if (!n || (cap && (!structure || !ground || !ground_height || !coarse))) return MM3D_EINVAL;
  const int st = corr_call_check(ctx, points, normals, nullptr, nullptr, options);
  if (st != MM3D_OK) return st;
  n[0] = n[1] = n[2] = 0;
  return guarded(ctx, [&] {
    std::unique_ptr<CoarseSignature> S = corr_build_signature(ctx, points, normals, *options);
    const size_t ns = (size_t)S->n_struct, ng = (size_t)S->n_ground, ccap = S->ccells.size();
    std::vector<int4> hs(ns), hg(ng);
    std::vector<int2> hc(ccap);
    int nc = 0;
    if (ns) MM3D_HIP(hipMemcpyAsync(hs.data(), S->scells.get(), ns * sizeof(int4), hipMemcpyDeviceToHost, ctx->stream));
    if (ng) MM3D_HIP(hipMemcpyAsync(hg.data(), S->gcells.get(), ng * sizeof(int4), hipMemcpyDeviceToHost, ctx->stream));
    if (ccap) MM3D_HIP(hipMemcpyAsync(hc.data(), S->ccells.get(), ccap * sizeof(int2), hipMemcpyDeviceToHost, ctx->stream));
    if (S->n_coarse.get()) MM3D_HIP(hipMemcpyAsync(&nc, S->n_coarse.get(), sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    n[0] = ns; n[1] = ng; n[2] = (size_t)nc;
    for (size_t k = 0; k < std::min(ns, cap); ++k) { structure[3 * k] = hs[k].x; structure[3 * k + 1] = hs[k].y; structure[3 * k + 2] = hs[k].z; }
    for (size_t k = 0; k < std::min(ng, cap); ++k) {
      ground[3 * k] = hg[k].x; ground[3 * k + 1] = hg[k].y; ground[3 * k + 2] = hg[k].z;
      std::memcpy(&ground_height[k], &hg[k].w, sizeof(float));
    }
    for (size_t k = 0; k < std::min(std::min((size_t)nc, ccap), cap); ++k) { coarse[2 * k] = hc[k].x; coarse[2 * k + 1] = hc[k].y; }
  });
}

int mm3d_debug_correlative_votes(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_normals *source_normals, const mm3d_cloud *target,
                                 const mm3d_normals *target_normals, const mm3d_coarse_options *options, int q, int frame[5], int *acc,
                                 size_t acc_cap, int *cands, int *scores, size_t cand_cap, size_t *n_cands)
{
  if (!target || !target_normals || !frame || !n_cands || (cand_cap && !cands)) return MM3D_EINVAL;
  const int st = corr_call_check(ctx, source, source_normals, target, target_normals, options);
  if (st != MM3D_OK) return st;
  return guarded(ctx, [&] {
    std::unique_ptr<CoarseSignature> S = corr_build_signature(ctx, source, source_normals, *options);
    std::unique_ptr<CoarseSignature> Tg = corr_build_signature(ctx, target, target_normals, *options);
    PairFront f;
    CorrDebug dbg;
    dbg.q = q; dbg.frame = frame; dbg.acc = acc; dbg.acc_cap = acc_cap; dbg.cands = cands; dbg.scores = scores; dbg.cand_cap = cand_cap;
    dbg.n_cands = n_cands;
    corr_align(ctx, *options, *S, *Tg, f, nullptr, &dbg);
  });
}

}  // extern "C"

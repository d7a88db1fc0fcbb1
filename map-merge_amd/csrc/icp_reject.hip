// icp_reject.hip -- correspondence rejection for the pair stage's ICP, opt-in (mm3d_set_icp_rejection): PCL's
// CorrespondenceRejectorOneToOne, CorrespondenceRejectorTrimmed and CorrespondenceRejectorMedianDistance, the three rejectors
// that need nothing but the correspondences.  include/mm3d.h states the rule.
//
// The default ICP fuses the search with its sums (k_nn_wave<0>, k_icp_plane_wave), so an order statistic over one iteration's
// d2 has nowhere to happen.  Here the iteration is a correspondence STAGE of its own between the search and the sums, all of it
// on the device, every launch over the pair batch (blockIdx.y = the pair) and returning at once for a pair that is done:
//   k_rej_begin    one block per pair: the pair's record and its four histograms cleared
//   k_rej_search   nn_search_body.hpp's wave-cooperative search (the same include as k_nn_wave, k_nn_probe and
//                  k_icp_plane_wave); a lane stores {target index, d2 bits} at its point's place in the Hilbert-ordered source
//                  (8 B per source point) and, under one_to_one, takes its target with an integer atomicMin of
//                  d2 bits << 32 | original source index (8 B per target point): no arrival order shows
//   k_rej_hist     pass 0 settles one_to_one in place (a loser keeps its index as -2 - index) and counts the survivors; passes
//                  0 .. 3 are a most-significant-digit-first radix select over the survivors' 32 d2 bits, 8 bits a pass: LDS
//                  histograms, integer atomics into the pair's 256 bins.  d2 >= 0, so the bits order like the values, and the
//                  k-th smallest comes out EXACT.  The digit that holds the wanted rank is found at the head of the NEXT launch,
//                  by every block for itself from the finished histogram (a 256-entry scan): all blocks compute the same
//                  prefix and rank, and block-identical values are what they store.
//   k_rej_reduce   the work item <-> wave <-> lane mapping of the search again: a lane decides "kept" from its 8 bytes and the
//                  threshold, and the kept correspondences' terms (k_nn_wave<0>'s 17, or k_icp_plane_wave's 30 with normals) go
//                  through wave_sum and the block step into the partials, in the default kernels' layout and order.
// k_icp_finalize / k_icp_plane_finalize then run unchanged.  With nothing rejected the partials hold the default kernels' bits.
#include <atomic>
#include <cmath>

#include "capi_guard.hpp"
#include "drivers.hpp"
#include "icp_tail.hpp"
#include "nn_core.hpp"

namespace mm3d {

// What one pair's selection leaves behind, on the device beside the pair's IcpState and back on the host in the copy that brings
// the states: the counts of the last iteration that ran and the state of the radix select (prefix / rank BEFORE pass q of four
// 8-bit passes over the d2 bits).
struct RejRecord {
  unsigned matched, survivors, kept;
  unsigned tau_bits;          // TRIMMED: tau; MEDIAN: m (valid when cut == 0)
  int cut;                    // 0: cut at tau_bits, 1: nothing is cut, 2: everything is cut
  unsigned prefix[4], rank[4];
};
// the search job plus the rejecting stage's working memory; nn.partials: [nblocks][kAcc], or [nblocks][kPlaneAcc] with normals
struct NnRejectJob {
  NnJob nn;
  const float4 *nrm;          // point-to-plane: the target's normals (tgt_ref's order); null: point-to-point
  int2 *corr;                 // [n_src], at the point's place in the Hilbert-ordered source: {target index (-1: none;
                              // -2 - index: lost its target under one_to_one), d2 bits}
  unsigned long long *owner;  // one_to_one: [n_tgt] smallest key d2 bits << 32 | original source index per target point
  unsigned *hist;             // [4][256]
  RejRecord *rec;
  int n_src;                  // finite source points
};

// the options as the kernels take them
struct RejOpts {
  int one_to_one, distance, min_corr;
  double ratio, factor;
};
constexpr int kRejPerBlock = 4096;     // source points per block of a histogram pass

__global__ void __launch_bounds__(256) k_rej_begin(const NnRejectJob *__restrict__ rjobs)
{
  const NnRejectJob &rj = rjobs[blockIdx.x];
  if (rj.nn.st->done) return;
  for (int k = threadIdx.x; k < 4 * 256; k += 256) rj.hist[k] = 0u;
  if (threadIdx.x == 0) {
    RejRecord r;
    r.matched = r.survivors = r.kept = 0u;
    r.tau_bits = 0u;
    r.cut = 1;
    for (int q = 0; q < 4; ++q) { r.prefix[q] = 0u; r.rank[q] = 0u; }
    *rj.rec = r;
  }
}

template <int SPLIT>
__global__ void __launch_bounds__(256) MM3D_NN_ATTR
k_rej_search(const NnRejectJob *__restrict__ rjobs, float max_d2, float rmax)
{
  constexpr int MODE = 0;                                // (nn_search_body.hpp: the keyed search, with the winner's index)
  const NnJob &job = rjobs[blockIdx.y].nn;
  if ((int)blockIdx.x >= job.nblocks) return;            // the grid is as wide as the batch's largest job
  const float4 *__restrict__ src = job.src;
  const int2 *__restrict__ items = job.items;
  const int n_items = job.n_items;
  const GridView g = job.g;
  const IcpState *__restrict__ st = job.st;
  int2 *__restrict__ corr = rjobs[blockIdx.y].corr;
  unsigned long long *__restrict__ owner = rjobs[blockIdx.y].owner;
  RejRecord *__restrict__ rec = rjobs[blockIdx.y].rec;
  const int max_ring = job.max_ring;
  __shared__ float Ts[16];
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
  const bool matched = valid && best <= max_d2;   // false for INFINITY / NaN
  if (valid) {
    const unsigned w = (unsigned)(bkey & 0xffffffffull);
    corr[i] = matched ? make_int2((int)w, __float_as_int(best)) : make_int2(-1, 0x7f800000);
    if (matched && owner)
      atomicMin(&owner[w], ((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)__float_as_uint(src[i].w));
  }
  const int n = __popcll(ballot(matched));
  if (lane == 0 && n) atomicAdd(&rec->matched, (unsigned)n);
}

// ---- step 1b (mm3d_set_icp_geometry_rejection): a launch of its own between the search and the select, so that the kernels
// above and below keep their machine code.  The search of such an iteration gets a job WITHOUT the owner array -- a dropped
// correspondence must not compete for its target -- and the survivors of this step issue the search's atomicMin here.
struct GeoRecord { unsigned on_boundary, mismatch; };
struct NnGeoJob {
  const unsigned char *flags;         // boundary: the target's flags, in its order; null: the bit is off
  const float4 *src_nrm, *tgt_nrm;    // normals: both maps' normals, in their points' order; null: the bit is off
  unsigned long long *owner;          // one_to_one: the pair's owner array
  unsigned char *reason;              // [n_src], at the point's place in the Hilbert-ordered source: 0, 1 boundary, 2 normals
  GeoRecord *rec;
};

__global__ void __launch_bounds__(64) k_geo_begin(const NnRejectJob *__restrict__ rjobs, const NnGeoJob *__restrict__ gjobs)
{
  if (rjobs[blockIdx.x].nn.st->done) return;
  if (threadIdx.x == 0) *gjobs[blockIdx.x].rec = GeoRecord{0u, 0u};
}

__global__ void __launch_bounds__(256) k_rej_geometry(const NnRejectJob *__restrict__ rjobs, const NnGeoJob *__restrict__ gjobs, double c2n)
{
  const NnRejectJob &rj = rjobs[blockIdx.y];
  const NnGeoJob &gj = gjobs[blockIdx.y];
  const IcpState *__restrict__ st = rj.nn.st;
  if (st->done) return;
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if ((int)blockIdx.x * 256 >= rj.n_src) return;
  int reason = 0;
  int2 cr = make_int2(-1, 0x7f800000);
  if (i < rj.n_src) cr = rj.corr[i];
  const bool matched = cr.x >= 0;
  if (matched) {
    if (gj.flags && gj.flags[cr.x]) {
      reason = 1;
    } else if (gj.src_nrm) {
      const float4 s = rj.nn.src[i];
      const float4 ns = gj.src_nrm[__float_as_int(s.w)], nt = gj.tgt_nrm[cr.x];
      const float *T = st->T;
      // m = R n_s by the ICP's float rule
      const float mxf = __fadd_rn(__fadd_rn(__fmul_rn(T[0], ns.x), __fmul_rn(T[4], ns.y)), __fmul_rn(T[8], ns.z));
      const float myf = __fadd_rn(__fadd_rn(__fmul_rn(T[1], ns.x), __fmul_rn(T[5], ns.y)), __fmul_rn(T[9], ns.z));
      const float mzf = __fadd_rn(__fadd_rn(__fmul_rn(T[2], ns.x), __fmul_rn(T[6], ns.y)), __fmul_rn(T[10], ns.z));
      const double mx = mxf, my = myf, mz = mzf, tx = nt.x, ty = nt.y, tz = nt.z;
      const double d = (mx * tx + my * ty) + mz * tz;
      const double mm = (mx * mx + my * my) + mz * mz, tt = (tx * tx + ty * ty) + tz * tz;
      const bool usable = isfinite(ns.x) && isfinite(ns.y) && isfinite(ns.z) && isfinite(nt.x) && isfinite(nt.y) && isfinite(nt.z) &&
                          isfinite(mxf) && isfinite(myf) && isfinite(mzf) && mm > 0.0 && tt > 0.0;
      if (!(usable && d * d >= c2n * (mm * tt))) reason = 2;
    }
    if (reason) rj.corr[i] = make_int2(-2 - cr.x, cr.y);
    else if (gj.owner)
      atomicMin(&gj.owner[cr.x], ((unsigned long long)(unsigned)cr.y << 32) | (unsigned long long)__float_as_uint(rj.nn.src[i].w));
  }
  if (i < rj.n_src) gj.reason[i] = (unsigned char)reason;
  const int nb = __popcll(ballot(reason == 1)), nn = __popcll(ballot(reason == 2));
  if ((threadIdx.x & 63) == 0 && (nb | nn)) {
    if (nb) atomicAdd(&gj.rec->on_boundary, (unsigned)nb);
    if (nn) atomicAdd(&gj.rec->mismatch, (unsigned)nn);
    atomicSub(&rj.rec->matched, (unsigned)(nb + nn));      // (the rejection's `matched` counts what enters step 2)
  }
}

// The select's state before pass q + 1, from pass q's finished histogram and the state before pass q (q == 0: from the number
// of survivors).  Called by all 256 threads of a block; every block of a launch arrives at the same values.
struct RejSel { int cut; unsigned prefix, rank; };
__device__ __forceinline__ RejSel rej_select_step(const NnRejectJob &rj, const RejOpts &o, int q, unsigned *s_scan, unsigned *s_res)
{
  const int t = threadIdx.x;
  const RejRecord *rec = rj.rec;
  int cut = 0;
  unsigned prefix = 0u, rank = 0u;
  if (q == 0) {
    const long long n = (long long)rec->survivors;
    if (o.distance == MM3D_REJECT_TRIMMED) {
      const long long kr = (long long)(o.ratio * (double)n), k = kr > (long long)o.min_corr ? kr : (long long)o.min_corr;
      if (k >= n) cut = 1;
      else if (k == 0) cut = 2;
      else rank = (unsigned)(k - 1);
    } else {
      if (n == 0) cut = 1;
      else rank = (unsigned)(n / 2);
    }
  } else {
    cut = rec->cut;
    prefix = rec->prefix[q];
    rank = rec->rank[q];
  }
  if (cut != 0) return RejSel{cut, 0u, 0u};      // (block-uniform)
  const unsigned h = rj.hist[q * 256 + t];
  s_scan[t] = h;
  if (t < 2) s_res[t] = 0u;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const unsigned v = t >= d ? s_scan[t - d] : 0u;
    __syncthreads();
    s_scan[t] += v;
    __syncthreads();
  }
  const unsigned incl = s_scan[t], excl = incl - h;
  if (rank >= excl && rank < incl) { s_res[0] = (unsigned)t; s_res[1] = rank - excl; }
  __syncthreads();
  const RejSel r{0, (prefix << 8) | s_res[0], s_res[1]};
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(256) k_rej_hist(const NnRejectJob *__restrict__ rjobs, RejOpts o, int pass)
{
  const NnRejectJob &rj = rjobs[blockIdx.y];
  if (rj.nn.st->done) return;
  const int n_src = rj.n_src, base = (int)blockIdx.x * kRejPerBlock;
  if (base >= n_src) return;
  __shared__ unsigned s_h[256], s_scan[256], s_res[2];
  const int t = threadIdx.x;
  unsigned prefix = 0u;
  if (pass > 0) {
    const RejSel sel = rej_select_step(rj, o, pass - 1, s_scan, s_res);
    if (t == 0) {      // (the same values from every block)
      rj.rec->cut = sel.cut;
      rj.rec->prefix[pass] = sel.prefix;
      rj.rec->rank[pass] = sel.rank;
    }
    if (sel.cut != 0) return;
    prefix = sel.prefix;
  }
  s_h[t] = 0u;
  __syncthreads();
  int mine = 0;
  const int shift = 32 - 8 * pass;
  const int end = min(base + kRejPerBlock, n_src);
  for (int i = base + t; i < end; i += 256) {
    const int2 cr = rj.corr[i];
    if (cr.x < 0) continue;                   // no match, or lost its target
    const unsigned bits = (unsigned)cr.y;
    if (pass == 0) {
      if (rj.owner) {
        const unsigned long long key = ((unsigned long long)bits << 32) | (unsigned long long)__float_as_uint(rj.nn.src[i].w);
        if (rj.owner[cr.x] != key) {
          rj.corr[i] = make_int2(-2 - cr.x, cr.y);
          continue;
        }
      }
      ++mine;
      if (o.distance != MM3D_REJECT_NONE) atomicAdd(&s_h[bits >> 24], 1u);
    } else {
      if ((bits >> shift) != prefix) continue;
      atomicAdd(&s_h[(bits >> (shift - 8)) & 255u], 1u);
    }
  }
  __syncthreads();
  if (s_h[t]) atomicAdd(&rj.hist[pass * 256 + t], s_h[t]);
  if (pass == 0) {
    const int total = wave_sum(mine);
    if ((t & 63) == 0 && total) atomicAdd(&rj.rec->survivors, (unsigned)total);
  }
}

// the threshold of the iteration, after the select's last pass: by all 256 threads of a block
struct RejCut { int cut; unsigned tau; };
__device__ __forceinline__ RejCut rej_threshold(const NnRejectJob &rj, const RejOpts &o, unsigned *s_scan, unsigned *s_res)
{
  if (o.distance == MM3D_REJECT_NONE) return RejCut{1, 0u};
  const RejSel sel = rej_select_step(rj, o, 3, s_scan, s_res);
  if (threadIdx.x == 0 && sel.cut == 0) rj.rec->tau_bits = sel.prefix;      // (the same value from every block)
  return RejCut{sel.cut, sel.prefix};
}
__device__ __forceinline__ bool rej_kept(int idx, unsigned bits, const RejCut &c, const RejOpts &o)
{
  if (idx < 0 || c.cut == 2) return false;
  if (c.cut == 1) return true;
  if (o.distance == MM3D_REJECT_TRIMMED) return bits <= c.tau;
  return (double)__uint_as_float(bits) <= (double)__uint_as_float(c.tau) * o.factor;
}

// SPLIT 1: the partials per block of four work items, through k_nn_wave's block step; SPLIT 4: per work item.  Either way a
// block holds four items, one per wave.
template <int SPLIT, bool PLANE>
__global__ void __launch_bounds__(256) k_rej_reduce(const NnRejectJob *__restrict__ rjobs, RejOpts o)
{
  constexpr int NACC = PLANE ? kPlaneAcc : kAcc;
  const NnRejectJob &rj = rjobs[blockIdx.y];
  const NnJob &job = rj.nn;
  const int n_items = job.n_items;
  if ((int)blockIdx.x * 4 >= n_items) return;
  const IcpState *__restrict__ st = job.st;
  if (st->done) return;
  const float4 *__restrict__ src = job.src;
  const float4 *__restrict__ tgt_ref = job.tgt_ref;
  const float4 *__restrict__ nrm = rj.nrm;
  double *__restrict__ partials = job.partials;
  __shared__ float Ts[16];
  __shared__ double red[4][NACC];
  __shared__ unsigned s_scan[256], s_res[2];
  if (threadIdx.x < 16) Ts[threadIdx.x] = st->T[threadIdx.x];
  const RejCut cut = rej_threshold(rj, o, s_scan, s_res);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int item = (int)blockIdx.x * 4 + wave;
  const int2 it = item < n_items ? job.items[item] : make_int2(0, 0);
  const int i = it.x + lane;
  const bool valid = lane < it.y;
  int2 cr = make_int2(-1, 0x7f800000);
  if (valid) cr = rj.corr[i];
  const bool corr = valid && rej_kept(cr.x, (unsigned)cr.y, cut, o);
  const float best = __int_as_float(cr.y);
  float3 p = make_float3(0.f, 0.f, 0.f);
  if (corr) {
    const float4 s = src[i];
    p = xform(Ts, s.x, s.y, s.z);
  }
  const unsigned long long kept_mask = ballot(corr);
  const bool any_corr = kept_mask != 0ull;       // wave-uniform
  if (lane == 0 && any_corr) atomicAdd(&rj.rec->kept, (unsigned)__popcll(kept_mask));
  if (!PLANE) {
    // k_nn_wave<0>'s terms and order
    double acc[kAcc];
#pragma unroll
    for (int k = 0; k < kAcc; ++k) acc[k] = 0.0;
    if (corr) {
      const float4 bq = tgt_ref[cr.x];
      const float bqx = bq.x, bqy = bq.y, bqz = bq.z;
      acc[0] = p.x; acc[1] = p.y; acc[2] = p.z;
      acc[3] = bqx; acc[4] = bqy; acc[5] = bqz;
      acc[6] = (double)bqx * p.x; acc[7] = (double)bqx * p.y; acc[8] = (double)bqx * p.z;
      acc[9] = (double)bqy * p.x; acc[10] = (double)bqy * p.y; acc[11] = (double)bqy * p.z;
      acc[12] = (double)bqz * p.x; acc[13] = (double)bqz * p.y; acc[14] = (double)bqz * p.z;
      acc[15] = best;
      acc[16] = 1.0;
    }
#pragma unroll
    for (int k = 0; k < kAcc; ++k) {
      const double v = any_corr ? wave_sum(acc[k]) : 0.0;
      if (SPLIT == 4) {
        if (lane == 0 && item < n_items) partials[(size_t)item * kAcc + k] = v;
      } else if (lane == 0) {
        red[wave][k] = v;
      }
    }
  } else {
    // point-to-plane's row, terms and order (icp_tail.hpp's, as k_icp_plane_wave)
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double r = 0.0, has_row = 0.0;
    if (corr && icp_plane_row(p, nrm[cr.x], tgt_ref[cr.x], v, r)) has_row = 1.0;
#pragma unroll
    for (int k = 0; k < kPlaneAcc; ++k) {
      const double s = any_corr ? wave_sum(icp_plane_term(k, v, r, corr, best, has_row)) : 0.0;
      if (SPLIT == 4) {
        if (lane == 0 && item < n_items) partials[(size_t)item * kPlaneAcc + k] = s;
      } else if (lane == 0) {
        red[wave][k] = s;
      }
    }
  }
  if (SPLIT == 4) return;
  __syncthreads();
  if (threadIdx.x < NACC) {
    const int k = threadIdx.x;
    partials[(size_t)blockIdx.x * NACC + k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
  }
}

// mm3d_debug_icp_rejection: the reduce kernel's decision per source point, stored at the point's ORIGINAL index
__global__ void __launch_bounds__(256) k_rej_export(const NnRejectJob *__restrict__ rjobs, RejOpts o, int *__restrict__ out_idx,
                                                    float *__restrict__ out_d2, unsigned char *__restrict__ out_kept)
{
  const NnRejectJob &rj = rjobs[0];
  const NnJob &job = rj.nn;
  const int n_items = job.n_items;
  if ((int)blockIdx.x * 4 >= n_items) return;
  __shared__ unsigned s_scan[256], s_res[2];
  const RejCut cut = rej_threshold(rj, o, s_scan, s_res);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int item = (int)blockIdx.x * 4 + wave;
  const int2 it = item < n_items ? job.items[item] : make_int2(0, 0);
  const int i = it.x + lane;
  const bool valid = lane < it.y;
  bool kept = false;
  if (valid) {
    const int2 cr = rj.corr[i];
    kept = rej_kept(cr.x, (unsigned)cr.y, cut, o);
    const int orig = __float_as_int(job.src[i].w);
    out_idx[orig] = cr.x == -1 ? -1 : (cr.x < 0 ? -2 - cr.x : cr.x);
    out_d2[orig] = cr.x == -1 ? INFINITY : __int_as_float(cr.y);
    out_kept[orig] = kept ? 1 : 0;
  }
  const unsigned long long m = ballot(kept);
  if (lane == 0 && m) atomicAdd(&rj.rec->kept, (unsigned)__popcll(m));
}

// mm3d_debug_icp_geometry: the same, with the reason in the kept byte's place: 0 kept, 1 boundary, 2 normals, 3 one-to-one, 4 distance
__global__ void __launch_bounds__(256) k_geo_export(const NnRejectJob *__restrict__ rjobs, const NnGeoJob *__restrict__ gjobs, RejOpts o,
                                                    int *__restrict__ out_idx, float *__restrict__ out_d2, unsigned char *__restrict__ out_reason)
{
  const NnRejectJob &rj = rjobs[0];
  const NnJob &job = rj.nn;
  const int n_items = job.n_items;
  if ((int)blockIdx.x * 4 >= n_items) return;
  __shared__ unsigned s_scan[256], s_res[2];
  const RejCut cut = rej_threshold(rj, o, s_scan, s_res);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int item = (int)blockIdx.x * 4 + wave;
  const int2 it = item < n_items ? job.items[item] : make_int2(0, 0);
  const int i = it.x + lane;
  const bool valid = lane < it.y;
  bool kept = false;
  if (valid) {
    const int2 cr = rj.corr[i];
    kept = rej_kept(cr.x, (unsigned)cr.y, cut, o);
    const int dropped = gjobs[0].reason[i];
    const int orig = __float_as_int(job.src[i].w);
    out_idx[orig] = cr.x == -1 ? -1 : (cr.x < 0 ? -2 - cr.x : cr.x);
    out_d2[orig] = cr.x == -1 ? INFINITY : __int_as_float(cr.y);
    out_reason[orig] = (unsigned char)(kept ? 0 : cr.x == -1 ? 4 : dropped ? dropped : cr.x < 0 ? 3 : 4);
  }
  const unsigned long long m = ballot(kept);
  if (lane == 0 && m) atomicAdd(&rj.rec->kept, (unsigned)__popcll(m));
}

static RejOpts rej_opts(const mm3d_icp_rejection_options &opt)
{
  return RejOpts{opt.one_to_one, opt.distance, opt.min_correspondences, opt.overlap_ratio, opt.median_factor};
}

// begin, search and the select's passes of one iteration.  owner_all / owner_bytes: the batch's owner arrays as one region.
// Step 1b (geo non-null): search_jobs are the jobs without their owner arrays, geo_jobs the step's operands.
struct GeoFront { const NnRejectJob *search_jobs; const NnGeoJob *geo_jobs; double c2n; };
static void reject_front(Context *c, const NnRejectJob *jobs_dev, int count, unsigned grid_x, unsigned max_src, bool split, float max_d2,
                         float rmax, const mm3d_icp_rejection_options &opt, unsigned long long *owner_all, size_t owner_bytes, double bytes,
                         const GeoFront *geo = nullptr)
{
  const RejOpts o = rej_opts(opt);
  MM3D_LAUNCH(c, "icp_reject_begin", count * 4096.0, k_rej_begin, dim3(count), dim3(256), 0, jobs_dev);
  if (opt.one_to_one && owner_bytes) MM3D_HIP(hipMemsetAsync(owner_all, 0xff, owner_bytes, c->stream));
  const NnRejectJob *search_jobs = geo ? geo->search_jobs : jobs_dev;
  if (split)
    MM3D_LAUNCH(c, "icp_reject_search", bytes, k_rej_search<4>, dim3(grid_x, count), dim3(256), 0, search_jobs, max_d2, rmax);
  else
    MM3D_LAUNCH(c, "icp_reject_search", bytes, k_rej_search<1>, dim3(grid_x, count), dim3(256), 0, search_jobs, max_d2, rmax);
  if (geo) {
    MM3D_LAUNCH(c, "icp_geometry_begin", count * 8.0, k_geo_begin, dim3(count), dim3(64), 0, jobs_dev, geo->geo_jobs);
    MM3D_LAUNCH(c, "icp_geometry_drop", (double)max_src * count * 42.0, k_rej_geometry, dim3(div_up(max_src, 256), count), dim3(256), 0, jobs_dev,
                geo->geo_jobs, geo->c2n);
  }
  const int passes = opt.distance != MM3D_REJECT_NONE ? 4 : opt.one_to_one ? 1 : 0;
  for (int pass = 0; pass < passes; ++pass)
    MM3D_LAUNCH(c, "icp_reject_select", (double)max_src * count * 8.0, k_rej_hist, dim3(div_up(max_src, kRejPerBlock), count), dim3(256), 0,
                jobs_dev, o, pass);
}

// a pair's record as the caller sees it (iterations and converged are the state's)
static mm3d_icp_rejection_stats rej_stats(const RejRecord &r, const mm3d_icp_rejection_options &opt, int iterations, int converged)
{
  float tau;
  std::memcpy(&tau, &r.tau_bits, 4);
  return mm3d_icp_rejection_stats{(long long)r.matched, (long long)(opt.one_to_one ? r.survivors : r.matched), (long long)r.kept,
                                  r.cut == 0 ? tau : r.cut == 1 ? INFINITY : -1.0f, iterations, converged};
}
// step 1b's counts beside the rejection's (whose `matched` the step has reduced to what passed)
static mm3d_icp_geometry_stats geo_stats(const RejRecord &r, const GeoRecord &g, long long target_boundary_points)
{
  return mm3d_icp_geometry_stats{(long long)r.matched + g.on_boundary + g.mismatch, (long long)g.on_boundary, (long long)g.mismatch,
                                 (long long)r.matched, target_boundary_points};
}
static double geo_c2n(const mm3d_icp_geometry_options &g)
{
  const double cs = g.normal_angle_deg == 90.0 ? 0.0 : std::cos(g.normal_angle_deg * (M_PI / 180.0));
  return cs * cs;
}
// what step 1b needs of a pair: throws when an operand of a set bit is missing
static void geo_check(const mm3d_icp_geometry_options &g, const IcpScoreJob &J)
{
  if (g.boundary && !J.tgt_boundary) throw Error(MM3D_EINVAL, "boundary rejector: the target has no boundary flags");
  if (g.normals) {
    if (J.icp_src) throw Error(MM3D_EUNSUPPORTED, "normal rejector: a sampled source has no normals");
    if (!J.src_normals || J.src_normals->n != J.src->n) throw Error(MM3D_EINVAL, "normal rejector: the source's normals do not match its points");
    if (!J.geo_tgt_normals || J.geo_tgt_normals->n != J.tgt->n) throw Error(MM3D_EINVAL, "normal rejector: the target's normals do not match its points");
  }
}
static NnGeoJob geo_job(const mm3d_icp_geometry_options &g, const IcpScoreJob &J, unsigned long long *owner, unsigned char *reason, GeoRecord *rec)
{
  return NnGeoJob{g.boundary ? J.tgt_boundary : nullptr, g.normals ? (const float4 *)J.src_normals->nrm.get() : nullptr,
                  g.normals ? (const float4 *)J.geo_tgt_normals->nrm.get() : nullptr, owner, reason, rec};
}
static RejRecord rej_record_init()
{
  RejRecord r;
  std::memset(&r, 0, sizeof(r));
  r.cut = 1;
  return r;
}

static std::atomic<int> g_forced_split{0};      // mm3d_debug_icp_rejection_split: 0 (by size), 1 or 4

namespace {
// One iteration: the correspondence stage and the reduction into the ICP jobs' partials in the default kernels' layout and order,
// then the default finalize kernel -- k_icp_finalize over the batch's NnJobs or, with normals, k_icp_plane_finalize over
// NnPlaneJobs kept here.  The pairs' records ride behind the states.
struct RejectStep final : IcpStep {
  const mm3d_icp_rejection_options opt;
  const bool plane;
  const bool geometric;                   // step 1b runs (mm3d_set_icp_geometry_rejection)
  const mm3d_icp_geometry_options geo;
  StepJobs<NnRejectJob> jobs;
  StepJobs<NnRejectJob> sjobs;            // step 1b: the search's jobs, without the owner arrays
  StepJobs<NnGeoJob> gjobs;
  DevBuf<unsigned char> reason;           // step 1b: the batch's sources, one after the other
  GeoRecord *grec_host = nullptr, *grec_dev = nullptr;
  StepJobs<NnPlaneJob> pjobs;
  DevBuf<int2> corr;                      // the batch's sources, one after the other
  DevBuf<unsigned long long> owner;       // one_to_one: the batch's targets
  DevBuf<unsigned> hist;
  RejRecord *rec_host = nullptr, *rec_dev = nullptr;
  size_t n_src = 0, n_tgt = 0, src_off = 0, tgt_off = 0;
  unsigned max_src = 0;
  RejectStep(const mm3d_icp_rejection_options &o, bool normals, const mm3d_icp_geometry_options *g)
      : opt(o), plane(normals), geometric(g != nullptr), geo(g ? *g : mm3d_icp_geometry_options{0, 0.0, 90.0, 3, 0, 45.0})
  {
    acc = plane ? kPlaneAcc : kAcc;
    forced_split = g_forced_split.load();
  }
  double bytes_per_point(const IcpScoreJob &) const override { return plane ? 28.0 : 12.0; }
  void check(const IcpScoreJob &J) const override
  {
    if (plane) icp_plane_check(J);
    if (geometric) geo_check(geo, J);
  }
  size_t pinned_bytes(int B) const override
  {
    return jobs.bytes(B) + (plane ? pjobs.bytes(B) : 0) + (geometric ? sjobs.bytes(B) + gjobs.bytes(B) : 0);
  }
  size_t record_bytes(int B) const override { return (sizeof(RejRecord) + (geometric ? sizeof(GeoRecord) : 0)) * B; }
  void begin(Context *c, const IcpScoreJob *const *live, int B, char *pinned, void *rh, void *rd) override
  {
    for (int b = 0; b < B; ++b) {
      n_src += live[b]->icp_source()->n_finite;              // (the ICP's source: a sample under mm3d_set_icp_sampling)
      n_tgt += opt.one_to_one ? live[b]->tgt->n : 0;
      max_src = std::max(max_src, (unsigned)live[b]->icp_source()->n_finite);
    }
    pinned = jobs.begin(c, B, pinned);
    if (plane) pinned = pjobs.begin(c, B, pinned);
    if (geometric) {
      pinned = sjobs.begin(c, B, pinned);
      gjobs.begin(c, B, pinned);
      reason = DevBuf<unsigned char>(c, n_src ? n_src : 1);
      grec_host = (GeoRecord *)((RejRecord *)rh + B);
      grec_dev = (GeoRecord *)((RejRecord *)rd + B);
    }
    corr = DevBuf<int2>(c, n_src);
    owner = DevBuf<unsigned long long>(c, n_tgt ? n_tgt : 1);
    hist = DevBuf<unsigned>(c, (size_t)B * 1024);
    rec_host = (RejRecord *)rh;
    rec_dev = (RejRecord *)rd;
  }
  void bind(int b, const NnJob &q, const IcpScoreJob &J) override
  {
    if (plane) pjobs.host[b] = icp_plane_job(q, J);
    jobs.host[b] = NnRejectJob{q, plane ? pjobs.host[b].nrm : nullptr, corr.get() + src_off, opt.one_to_one ? owner.get() + tgt_off : nullptr,
                               hist.get() + (size_t)b * 1024, rec_dev + b, (int)J.icp_source()->n_finite};
    rec_host[b] = rej_record_init();
    if (geometric) {
      sjobs.host[b] = jobs.host[b];
      sjobs.host[b].owner = nullptr;
      gjobs.host[b] = geo_job(geo, J, jobs.host[b].owner, reason.get() + src_off, grec_dev + b);
      grec_host[b] = GeoRecord{0u, 0u};
    }
    src_off += J.icp_source()->n_finite;
    tgt_off += opt.one_to_one ? J.tgt->n : 0;
  }
  void upload(Context *c) override
  {
    jobs.upload(c);
    // (a place of the Hilbert-ordered source that no work item covers holds "no match" for good)
    MM3D_HIP(hipMemsetAsync(corr.get(), 0xff, n_src * sizeof(int2), c->stream));
    if (plane) pjobs.upload(c);
    if (geometric) { sjobs.upload(c); gjobs.upload(c); }
  }
  void iterate(Context *c, const IcpLaunch &L) override
  {
    const NnRejectJob *jobs_dev = jobs.dev.get();
    const GeoFront gf{sjobs.dev.get(), gjobs.dev.get(), geo_c2n(geo)};
    reject_front(c, jobs_dev, L.count, L.grid_x, max_src, L.split, L.max_d2, L.rmax, opt, owner.get(), n_tgt * sizeof(unsigned long long),
                 L.bytes + n_src * 8.0, geometric ? &gf : nullptr);
    const RejOpts o = rej_opts(opt);
    const dim3 grid(L.split ? div_up(L.grid_x, 4) : L.grid_x, L.count);      // four work items per block either way
    const double rbytes = (double)max_src * L.count * 24.0;
    if (L.split && plane) MM3D_LAUNCH(c, "icp_reject_reduce", rbytes, (k_rej_reduce<4, true>), grid, dim3(256), 0, jobs_dev, o);
    else if (L.split) MM3D_LAUNCH(c, "icp_reject_reduce", rbytes, (k_rej_reduce<4, false>), grid, dim3(256), 0, jobs_dev, o);
    else if (plane) MM3D_LAUNCH(c, "icp_reject_reduce", rbytes, (k_rej_reduce<1, true>), grid, dim3(256), 0, jobs_dev, o);
    else MM3D_LAUNCH(c, "icp_reject_reduce", rbytes, (k_rej_reduce<1, false>), grid, dim3(256), 0, jobs_dev, o);
    if (plane) icp_plane_finalize(c, pjobs.dev.get(), L.count, L.finalize_bytes);
    else icp_point_finalize(c, L.jobs_dev, L.count, L.finalize_bytes);
  }
  void close(int b, const IcpState &h, IcpScoreJob &J) override
  {
    J.reject_stats = rej_stats(rec_host[b], opt, h.iters, h.converged);
    if (geometric) J.geometry_stats = geo_stats(rec_host[b], grec_host[b], geo.boundary ? J.tgt_boundary_points : 0);
  }
};
}  // namespace

std::unique_ptr<IcpStep> icp_reject_step(const mm3d_icp_rejection_options &opt, bool normals, const mm3d_icp_geometry_options *geometry)
{
  return std::unique_ptr<IcpStep>(new RejectStep(opt, normals, geometry));
}

static bool icp_rejection_options_valid(const mm3d_icp_rejection_options *o)
{
  if (o->one_to_one != 0 && o->one_to_one != 1) return false;
  if (o->distance != MM3D_REJECT_NONE && o->distance != MM3D_REJECT_TRIMMED && o->distance != MM3D_REJECT_MEDIAN) return false;
  if (!(o->overlap_ratio > 0.0 && o->overlap_ratio <= 1.0)) return false;
  if (o->min_correspondences < 0) return false;
  return o->median_factor > 0.0 && std::isfinite(o->median_factor);
}

// mm3d_debug_icp_rejection: the search set-up as icp_batch derives it, one iteration's begin, search and select passes at T with
// the split forced, and every source point's decision at its original index
// gd (mm3d_debug_icp_geometry): step 1b runs too, and `kept` receives the reason
struct GeoDebug {
  const mm3d_icp_geometry_options *opt;
  const IcpScoreJob *operands;          // tgt_boundary, src_normals, geo_tgt_normals, tgt_boundary_points
  mm3d_icp_geometry_stats *stats;
};
static void debug_icp_rejection(Context *c, const mm3d_cloud *src, const mm3d_cloud *tgt, const float T[16], double max_corr_dist,
                                const mm3d_icp_rejection_options &opt, int split, int *idx, float *d2, unsigned char *kept,
                                mm3d_icp_rejection_stats *stats, const GeoDebug *gd = nullptr)
{
  const NnRange r = nn_range_icp(max_corr_dist);
  mm3d_icp_rejection_stats S{0, 0, 0, INFINITY, 0, 0};
  std::vector<int> h_idx(src->n, -1);
  std::vector<float> h_d2(src->n, INFINITY);
  std::vector<unsigned char> h_kept(src->n, gd ? 4 : 0);
  mm3d_icp_geometry_stats G{0, 0, 0, 0, gd && gd->opt->boundary ? gd->operands->tgt_boundary_points : 0};
  const NnSearch s = nn_search(c, src, tgt, &r);
  if (s.grid) {
    const unsigned nblocks = nn_blocks(s.n_items, split == 4);
    DevBuf<int> d_idx(c, src->n);
    DevBuf<float> d_d2(c, src->n);
    DevBuf<unsigned char> d_kept(c, src->n);
    DevBuf<IcpState> st(c, 2);                       // the state, and the record behind it
    DevBuf<NnRejectJob> d_job(c, 1);
    DevBuf<int2> corr(c, (size_t)s.ns);
    DevBuf<unsigned long long> owner(c, opt.one_to_one ? tgt->n : 1);
    DevBuf<unsigned> hist(c, 1024);
    DevBuf<NnRejectJob> d_sjob(c, 1);
    DevBuf<NnGeoJob> d_gjob(c, 1);
    DevBuf<unsigned char> reason(c, (size_t)s.ns);
    static_assert(sizeof(RejRecord) + sizeof(GeoRecord) <= sizeof(IcpState), "both records ride behind the state");
    char *pinned = (char *)c->pin(2 * sizeof(IcpState) + 2 * sizeof(NnRejectJob) + sizeof(NnGeoJob) + 64);
    IcpState *hs = (IcpState *)pinned;
    RejRecord *hr = (RejRecord *)(hs + 1);
    NnRejectJob *hj = (NnRejectJob *)(pinned + 2 * sizeof(IcpState));
    std::memset(hs, 0, 2 * sizeof(IcpState));
    std::memcpy(hs->T, T, 64);
    *hr = rej_record_init();
    *hj = NnRejectJob{nn_job(s, split == 4, nblocks, st.get(), nullptr, nullptr, nullptr), nullptr, corr.get(),
                      opt.one_to_one ? owner.get() : nullptr, hist.get(), (RejRecord *)(st.get() + 1), s.ns};
    // (non-finite source points are in no work item: they keep -1 / +inf / 0)
    MM3D_HIP(hipMemcpyAsync(d_idx.get(), h_idx.data(), src->n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    MM3D_HIP(hipMemcpyAsync(d_d2.get(), h_d2.data(), src->n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    MM3D_HIP(hipMemsetAsync(d_kept.get(), gd ? 4 : 0, src->n, c->stream));
    MM3D_HIP(hipMemsetAsync(corr.get(), 0xff, (size_t)s.ns * sizeof(int2), c->stream));
    MM3D_HIP(hipMemcpyAsync(st.get(), hs, 2 * sizeof(IcpState), hipMemcpyHostToDevice, c->stream));
    MM3D_HIP(hipMemcpyAsync(d_job.get(), hj, sizeof(NnRejectJob), hipMemcpyHostToDevice, c->stream));
    GeoRecord *hg = (GeoRecord *)(hr + 1);
    GeoFront gf{d_sjob.get(), d_gjob.get(), 0.0};
    if (gd) {
      NnRejectJob *hsj = hj + 1;
      NnGeoJob *hgj = (NnGeoJob *)(hj + 2);
      *hsj = *hj;
      hsj->owner = nullptr;
      *hgj = geo_job(*gd->opt, *gd->operands, hj->owner, reason.get(), (GeoRecord *)((RejRecord *)(st.get() + 1) + 1));
      gf.c2n = geo_c2n(*gd->opt);
      MM3D_HIP(hipMemcpyAsync(d_sjob.get(), hsj, sizeof(NnRejectJob), hipMemcpyHostToDevice, c->stream));
      MM3D_HIP(hipMemcpyAsync(d_gjob.get(), hgj, sizeof(NnGeoJob), hipMemcpyHostToDevice, c->stream));
    }
    reject_front(c, d_job.get(), 1, nblocks, (unsigned)s.ns, split == 4, r.max_d2, r.rmax, opt, owner.get(),
                 opt.one_to_one ? tgt->n * sizeof(unsigned long long) : 0, s.ns * 24.0, gd ? &gf : nullptr);
    if (gd)
      MM3D_LAUNCH(c, "icp_geometry_export", s.ns * 18.0, k_geo_export, dim3(div_up(s.n_items, 4)), dim3(256), 0, (const NnRejectJob *)d_job.get(),
                  (const NnGeoJob *)d_gjob.get(), rej_opts(opt), d_idx.get(), d_d2.get(), d_kept.get());
    else
      MM3D_LAUNCH(c, "icp_reject_export", s.ns * 17.0, k_rej_export, dim3(div_up(s.n_items, 4)), dim3(256), 0, (const NnRejectJob *)d_job.get(),
                  rej_opts(opt), d_idx.get(), d_d2.get(), d_kept.get());
    MM3D_HIP(hipMemcpyAsync(h_idx.data(), d_idx.get(), src->n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MM3D_HIP(hipMemcpyAsync(h_d2.data(), d_d2.get(), src->n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    MM3D_HIP(hipMemcpyAsync(h_kept.data(), d_kept.get(), src->n, hipMemcpyDeviceToHost, c->stream));
    MM3D_HIP(hipMemcpyAsync(hs, st.get(), 2 * sizeof(IcpState), hipMemcpyDeviceToHost, c->stream));
    c->sync();
    S = rej_stats(*hr, opt, 0, 0);
    if (gd) G = geo_stats(*hr, *hg, G.target_boundary_points);
  }
  if (gd && gd->stats) *gd->stats = G;
  if (src->n) {
    std::memcpy(idx, h_idx.data(), src->n * sizeof(int));
    std::memcpy(d2, h_d2.data(), src->n * sizeof(float));
    std::memcpy(kept, h_kept.data(), src->n);
  }
  if (stats) *stats = S;
}

}  // namespace mm3d

using namespace mm3d;

extern "C" {

int mm3d_set_icp_rejection(mm3d_ctx *ctx, const mm3d_icp_rejection_options *options)
{
  if (!ctx || !options || !icp_rejection_options_valid(options)) return MM3D_EINVAL;
  std::lock_guard<std::mutex> lock(ctx->mu);        // (no call is running while the selection changes)
  return select_stage(ctx, Stage::Rejection, [&](StageSelection &s) { s.reject_options = *options; });
}

int mm3d_get_icp_rejection(const mm3d_ctx *ctx, mm3d_icp_rejection_options *options)
{
  if (!ctx || !options) return MM3D_EINVAL;
  *options = ctx->sel.reject_options;
  return MM3D_OK;
}

int mm3d_last_icp_rejection_stats(const mm3d_ctx *ctx, mm3d_icp_rejection_stats *stats)
{
  if (!ctx || !stats) return MM3D_EINVAL;
  *stats = ctx->last_reject_stats;
  return MM3D_OK;
}

int mm3d_estimate_transform_icp_rejecting(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target,
                                          const mm3d_normals *target_normals, const float initial_guess[16], double max_corr_dist,
                                          const mm3d_icp_rejection_options *options, int max_iterations, double eps, float T[16],
                                          mm3d_icp_rejection_stats *stats)
{
  if (!source || !target || !initial_guess || !options || !T || !icp_rejection_options_valid(options)) return MM3D_EINVAL;
  if (target_normals && target_normals->n != target->n) {
    if (ctx) ctx->err = "mm3d_estimate_transform_icp_rejecting: the normals do not match the target's points";
    return MM3D_EINVAL;
  }
  return guarded(ctx, [&] {
    IcpScoreJob J;
    J.src = source; J.tgt = target; J.tgt_normals = target_normals;
    J.reject = options;
    std::memcpy(J.guess_host, initial_guess, sizeof(J.guess_host));
    icp_score_batch(ctx, target_normals ? icp_plane_method() : nullptr, &J, 1, true, max_corr_dist, max_iterations, eps, false, 0.0);
    std::memcpy(T, J.out.T, sizeof(J.out.T));
    ctx->last_reject_stats = J.reject_stats;
    if (stats) *stats = J.reject_stats;
  });
}

int mm3d_debug_icp_rejection_split(int split)
{
  if (split == 0 || split == 1 || split == 4) g_forced_split.store(split);
  return g_forced_split.load();
}

int mm3d_debug_icp_rejection(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_cloud *target, const float T[16],
                             double max_correspondence_distance, const mm3d_icp_rejection_options *options, int split, int *idx, float *d2,
                             unsigned char *kept, mm3d_icp_rejection_stats *stats)
{
  if (!source || !target || !T || !options || !icp_rejection_options_valid(options) || (split != 1 && split != 4)) return MM3D_EINVAL;
  if (!(max_correspondence_distance >= 0.0) || !std::isfinite(max_correspondence_distance)) return MM3D_EINVAL;
  if (source->n && (!idx || !d2 || !kept)) return MM3D_EINVAL;
  return guarded(ctx, [&] { debug_icp_rejection(ctx, source, target, T, max_correspondence_distance, *options, split, idx, d2, kept, stats); });
}

// the argument checks the two stage-level calls of step 1b share
static bool geometry_call_valid(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_normals *source_normals, const mm3d_cloud *target,
                                const mm3d_normals *target_normals, bool needs_target_normals, const mm3d_icp_rejection_options *ro,
                                const mm3d_icp_geometry_options *go)
{
  if (!source || !target || !ro || !go || !icp_rejection_options_valid(ro) || !icp_geometry_options_valid(go)) return false;
  if (go->boundary && !(go->boundary_radius > 0.0)) return false;
  if ((go->normals && !source_normals) || ((go->normals || go->boundary || needs_target_normals) && !target_normals)) return false;
  if ((source_normals && source_normals->n != source->n) || (target_normals && target_normals->n != target->n)) {
    if (ctx) ctx->err = "geometric ICP rejectors: the normals do not match their cloud's points";
    return false;
  }
  return true;
}
// the operands of step 1b for a stage-level call: the target's flags are made here
static void geometry_bind(mm3d_ctx *ctx, IcpScoreJob &J, const mm3d_normals *source_normals, const mm3d_normals *target_normals,
                          const mm3d_icp_geometry_options *go, DevBuf<unsigned char> &flags)
{
  J.geometry = go;
  if (go->boundary) {
    flags = DevBuf<unsigned char>(ctx, J.tgt->n ? J.tgt->n : 1);
    boundary_flags(ctx, J.tgt, (const float4 *)target_normals->nrm.get(), go->boundary_radius, go->boundary_angle_deg, go->boundary_min_neighbours,
                   flags.get());
    J.tgt_boundary = flags.get();
    J.tgt_boundary_points = boundary_count(ctx, flags.get(), J.tgt->n);
  }
  if (go->normals) { J.src_normals = source_normals; J.geo_tgt_normals = target_normals; }
}

int mm3d_estimate_transform_icp_rejecting_geometry(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_normals *source_normals,
                                                   const mm3d_cloud *target, const mm3d_normals *target_normals, int point_to_plane,
                                                   const float initial_guess[16], double max_corr_dist,
                                                   const mm3d_icp_rejection_options *rejection_options,
                                                   const mm3d_icp_geometry_options *geometry_options, int max_iterations, double eps, float T[16],
                                                   mm3d_icp_rejection_stats *rejection_stats, mm3d_icp_geometry_stats *geometry_stats)
{
  if (!initial_guess || !T || (point_to_plane != 0 && point_to_plane != 1)) return MM3D_EINVAL;
  if (!geometry_call_valid(ctx, source, source_normals, target, target_normals, point_to_plane != 0, rejection_options, geometry_options))
    return MM3D_EINVAL;
  return guarded(ctx, [&] {
    IcpScoreJob J;
    J.src = source; J.tgt = target; J.tgt_normals = point_to_plane ? target_normals : nullptr;
    J.reject = rejection_options;
    DevBuf<unsigned char> flags;
    geometry_bind(ctx, J, source_normals, target_normals, geometry_options, flags);
    std::memcpy(J.guess_host, initial_guess, sizeof(J.guess_host));
    icp_score_batch(ctx, point_to_plane ? icp_plane_method() : nullptr, &J, 1, true, max_corr_dist, max_iterations, eps, false, 0.0);
    std::memcpy(T, J.out.T, sizeof(J.out.T));
    ctx->last_reject_stats = J.reject_stats;
    ctx->last_geometry_stats = J.geometry_stats;
    if (rejection_stats) *rejection_stats = J.reject_stats;
    if (geometry_stats) *geometry_stats = J.geometry_stats;
  });
}

int mm3d_debug_icp_geometry(mm3d_ctx *ctx, const mm3d_cloud *source, const mm3d_normals *source_normals, const mm3d_cloud *target,
                            const mm3d_normals *target_normals, const float T[16], double max_correspondence_distance,
                            const mm3d_icp_rejection_options *rejection_options, const mm3d_icp_geometry_options *geometry_options,
                            int split, int *idx, float *d2, unsigned char *reason, mm3d_icp_rejection_stats *rejection_stats,
                            mm3d_icp_geometry_stats *geometry_stats)
{
  if (!T || (split != 1 && split != 4)) return MM3D_EINVAL;
  if (!geometry_call_valid(ctx, source, source_normals, target, target_normals, false, rejection_options, geometry_options)) return MM3D_EINVAL;
  if (!(max_correspondence_distance >= 0.0) || !std::isfinite(max_correspondence_distance)) return MM3D_EINVAL;
  if (source->n && (!idx || !d2 || !reason)) return MM3D_EINVAL;
  return guarded(ctx, [&] {
    IcpScoreJob J;
    J.src = source; J.tgt = target;
    DevBuf<unsigned char> flags;
    geometry_bind(ctx, J, source_normals, target_normals, geometry_options, flags);
    const GeoDebug gd{geometry_options, &J, geometry_stats};
    debug_icp_rejection(ctx, source, target, T, max_correspondence_distance, *rejection_options, split, idx, d2, reason, rejection_stats, &gd);
  });
}

}  // extern "C"

// spfh_replay.hpp -- the float chain "v = 0; repeat hits: v = v + incr" (round to nearest even) in O(binades), as ONE
// host+device source (in the manner of linalg_shared.hpp).
//
// An SPFH bin is that chain with incr = 100 / (|N| - 1) and hits = the bin's votes (fpfh.hip).  While v stays inside one
// binade with ulp U it is a multiple M U, and adding x = q U + rem (0 <= rem < U) rounds on the U grid:
//   rem < U/2: M += q        rem > U/2: M += q + 1        rem == U/2 (a tie): M += q + ((M + q) & 1), to the even neighbour.
// After a tie step M is even, and from an even M every tie step adds the same q + (q & 1).  So inside a binade the step r is
// constant (after at most one step that makes M even) and k steps are M += k r in integers -- as long as the exact sum
// stays below the binade's end 2^24 U, which M + q + 1 <= 2^24 guarantees before every step.  What is left near the end
// of a binade is ONE real addition that crosses into the next.  r == 0: the chain stands still for good.
//
// Inside a binade the float's BIT PATTERN grows with M: bits = ((ev - 1) << 23) + M for v = M 2^(ev - 150), M <= 2^24, ev >= 1
// (denormals: ev = 1).  So the chain is a short list of PIECES (first, c, r): for first <= hits <= the next piece's first,
//   bits(chain(hits)) = c + hits r    (mod 2^32; the sign bit of a negative incr rides in c),
// one or two pieces per binade the chain passes through.  All 33 bins of a point share incr, hence the pieces: fpfh.hip's
// epilogue makes them once per point and takes every bin from them; spfh_replay below does the same for one hit count.
#pragma once

#include <hip/hip_runtime.h>

namespace mm3d {

struct SpfhChain {
  unsigned ex, mx;      // |incr| = mx 2^(ex - 150) (a denormal shares the first binade's ulp: ex = 1)
  unsigned ev, M;       // the chain after h additions: M 2^(ev - 150), M < 2^24
  unsigned h;           // additions made so far = the next piece's first hit count
  unsigned sign;
  float xmag;
  bool done;            // the last piece has no end
};

// incr finite and not zero.  The chain after its first addition: 0 + x = x.
__host__ __device__ inline SpfhChain spfh_chain_begin(float incr)
{
  union { float f; unsigned u; } x;
  x.f = incr;
  SpfhChain c;
  const unsigned xb = x.u & 0x7fffffffu;
  c.sign = x.u & 0x80000000u;
  x.u = xb;
  c.xmag = x.f;
  c.ex = xb >> 23;
  c.mx = xb & 0x7fffffu;
  if (c.ex) c.mx |= 0x800000u; else c.ex = 1u;
  c.ev = c.ex;
  c.M = c.mx;
  c.h = 1u;
  c.done = false;
  return c;
}

// floor(d / r) for d < 2^24, 0 < r <= 2^24.  Below 2^17 -- every quotient a 16-bit hit count can reach -- one reciprocal and a
// correction instead of an integer division: d and r are exact as floats, the product is within 2^-21 of d / r relatively,
// so within 1/16 absolutely, and its integer part is off by at most one either way.
__host__ __device__ inline unsigned spfh_quotient(unsigned d, unsigned r)
{
#if defined(__HIP_DEVICE_COMPILE__)
  const float rr = __builtin_amdgcn_rcpf((float)r);
#else
  const float rr = 1.0f / (float)r;
#endif
  const float qf = (float)d * rr;                       // within 2^-21 of d / r, relatively: below 2^17 the error is under one
  if (!(qf < 131072.0f)) return d / r;                  // (more steps than a 16-bit hit count can ask for: the kernel never gets here)
  unsigned k = (unsigned)qf;
  if (k * r > d) --k;                                   // (k r <= d + r < 2^26)
  else if (d - k * r >= r) ++k;
  return k;
}

// The next piece; the chain moves to the first hit count behind it.
__host__ __device__ inline void spfh_chain_piece(SpfhChain &c, unsigned &first, unsigned &c0, unsigned &r_out)
{
  first = c.h;
  unsigned base = ((c.ev - 1u) << 23) + c.M;
  unsigned r = 0u;
  if (c.ev >= 255u) {                                   // overflowed: inf + x = inf
    base = 0x7f800000u;
    c.done = true;
  } else {
    const unsigned s = c.ev - c.ex;                     // U = 2^s ulps of x
    unsigned q = 0u;
    bool odd_tie = false;
    if (s < 25u) {                                      // (else x < U/2)
      q = c.mx >> s;
      const unsigned rem = c.mx - (q << s), half = s ? (1u << (s - 1u)) : 0u;
      const bool tie = s && rem == half;
      r = q + (rem > half ? 1u : 0u);
      if (tie) {
        r = q + ((c.M + q) & 1u);
        odd_tie = (c.M & 1u) != 0u;                     // this step makes M even; the next piece has the constant step
      }
    }
    if (r == 0u) {
      c.done = true;
    } else {
      const unsigned lim = 0x1000000u - q - 1u;         // a step from M <= lim stays on this binade's grid
      bool fresh = false;                               // M == 2^24: the next binade's first value, exactly
      if (c.M <= lim) {
        const unsigned k = odd_tie ? 1u : spfh_quotient(lim - c.M, r) + 1u;
        c.M += k * r;
        c.h += k;
        if (c.M == 0x1000000u) { c.M = 0x800000u; ++c.ev; fresh = true; }
      }
      if (!fresh && c.M > lim) {                        // one real addition across the binade's end (always right, whatever the step)
        union { float f; unsigned u; } a;
        a.u = ((c.ev - 1u) << 23) + c.M;
        a.f = a.f + c.xmag;
        ++c.h;
        c.ev = a.u >> 23; c.M = a.u & 0x7fffffu;
        if (c.ev) c.M |= 0x800000u; else c.ev = 1u;
      }
    }
  }
  r_out = r;
  c0 = (c.sign | base) - first * r;
}

__host__ __device__ inline float spfh_replay(float incr, unsigned hits)
{
  union { float f; unsigned u; } x;
  if (hits == 0) return 0.0f;
  x.f = incr;
  const unsigned xb = x.u & 0x7fffffffu;
  if (xb == 0u) return 0.0f;                             // 0 + (+-0) = +0, and again
  if (xb == 0x7f800000u) return incr;                    // 0 + inf = inf = inf + inf
  if (xb > 0x7f800000u) {                                // NaN: whatever the additions give
    float v = 0.0f;
    for (unsigned i = 0; i < hits; ++i) v = v + incr;
    return v;
  }
  SpfhChain c = spfh_chain_begin(incr);
  unsigned first, c0, r;
  do spfh_chain_piece(c, first, c0, r); while (!c.done && c.h <= hits);
  x.u = c0 + hits * r;
  return x.f;
}

}  // namespace mm3d

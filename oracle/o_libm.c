/*
 * o_libm.c -- the host libm's expf / atanf / sinf / cosf / atan2f over arrays (TEST INFRASTRUCTURE).
 *
 * The CPU path of the reference (PCL) reaches these functions through libm; the device path uses
 * restatements of them (map-merge_amd/csrc/libm_exact.hpp).  The tests evaluate both on the same
 * arguments and compare bits.  (numpy's float32 ufuncs are its own SIMD code, not libm.)  fn 5 is not libm's:
 * acos(fabs(x)) > acos(fabs(y)) in double, as 1 / 0 -- the expression o_fpfh.c's pair features decide with.
 */
#include "mm3d_oracle.h"

#include <math.h>

void mo_libm_eval(int fn, const float *x, const float *y, int n, float *out)
{
  for (int i = 0; i < n; ++i) {
    switch (fn) {
      case 0: out[i] = expf(x[i]); break;
      case 1: out[i] = atanf(x[i]); break;
      case 2: out[i] = sinf(x[i]); break;
      case 3: out[i] = cosf(x[i]); break;
      case 5: out[i] = mo_acos_abs_greater(x[i], y[i]) ? 1.0f : 0.0f; break;   /* o_fpfh.c: computePairFeatures' switch */
      default: out[i] = atan2f(y[i], x[i]); break;
    }
  }
}

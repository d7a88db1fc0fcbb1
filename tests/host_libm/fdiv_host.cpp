// fdiv_host.cpp -- TEST INFRASTRUCTURE: lm::fdiv_const (csrc/libm_exact.hpp) compiled for the host, over arrays, for
// tests/test_libm_exact.py (built there with g++ into a temporary directory and loaded through ctypes).
//   out[i] = fdiv_const(x[i], y[i], (float)(1.0 / (double)y[i]))  -- the reciprocal as sift.hip prepares SiftScales::rcp
//   or, with rcp != nullptr, with the caller's reciprocal rcp[i]
#include "../../map-merge_amd/csrc/libm_exact.hpp"

extern "C" void fdiv_const_eval(const float *x, const float *y, const float *rcp, long n, float *out)
{
  for (long i = 0; i < n; ++i) out[i] = mm3d::lm::fdiv_const(x[i], y[i], rcp ? rcp[i] : (float)(1.0 / (double)y[i]));
}

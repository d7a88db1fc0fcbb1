// sym_eig3.hpp -- the symmetric 3x3 eigen-solver in double that SHOT's local reference frame (shot.hip) and the MLS smoothing's
// weighted plane (smooth_mls.hip) share: one text, so the two files cannot drift apart.
#pragma once

#include <hip/hip_runtime.h>

namespace mm3d {

// Eigen-decomposition of a symmetric 3x3 in double: cyclic Jacobi, eigenvalues ascending, vectors in
// the columns of V -- the same text as oracle/o_shot.c::sym_eig3 (both stand in for
// Eigen::SelfAdjointEigenSolver<Matrix3d>; the axes' signs are fixed by the disambiguation).
__device__ inline void sym_eig3(double a[3][3], double w[3], double V[3][3])
{
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
    const double dg = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2];
    if (!(off > 4.93e-32 * (dg + 2.0 * off))) break;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        const int r = 3 - p - q;
        const double app = a[p][p], aqq = a[q][q], apr = a[p][r], aqr = a[q][r];
        a[p][p] = app - t * apq;
        a[q][q] = aqq + t * apq;
        a[p][q] = a[q][p] = 0.0;
        a[p][r] = a[r][p] = c * apr - s * aqr;
        a[q][r] = a[r][q] = s * apr + c * aqr;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double vp = V[k][p], vq = V[k][q];
          V[k][p] = c * vp - s * vq;
          V[k][q] = s * vp + c * vq;
        }
      }
  }
  w[0] = a[0][0]; w[1] = a[1][1]; w[2] = a[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2 - i; ++j)
      if (w[j + 1] < w[j]) {
        double t = w[j]; w[j] = w[j + 1]; w[j + 1] = t;
#pragma unroll
        for (int k = 0; k < 3; ++k) { t = V[k][j]; V[k][j] = V[k][j + 1]; V[k][j + 1] = t; }
      }
}

}  // namespace mm3d

// icp_solve6.hpp -- what the two six-parameter estimates of the pair stage share (icp_plane.hip's point-to-plane ICP and
// ndt.hip's NDT): the layout of the 6x6 normal matrix's upper triangle, the degeneracy threshold, and the solve.
#pragma once

namespace mm3d {

// A pivot of the LDLt at or below kPlanePivotTau * trace(AtA) / 6 makes the system degenerate (a single plane leaves three
// directions unconstrained: their pivots are rounding noise, ~1e-16 of the trace).  The loop then stops, not converged, with
// T as it was before the iteration; so it does with fewer than 6 rows.  (PCL would use ATA.inverse() of a singular matrix.)
constexpr double kPlanePivotTau = 1e-12;

// the upper triangle of the 6x6 AtA, row by row: term k = row[kUi[k]] * row[kUj[k]]
__device__ constexpr int kUi[21] = {0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 5};
__device__ constexpr int kUj[21] = {0, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 2, 3, 4, 5, 3, 4, 5, 4, 5, 5};

// AtA x = b by an unpivoted LDLt in double; false when a pivot is at or below `floor` (x is then not written)
__device__ static bool solve6_ldlt(const double A[36], const double b[6], double floor, double x[6])
{
  double L[36], D[6];
  for (int j = 0; j < 6; ++j) {
    double d = A[j * 6 + j];
    for (int k = 0; k < j; ++k) d -= L[j * 6 + k] * L[j * 6 + k] * D[k];
    if (!(d > floor)) return false;                    // (also catches NaN)
    D[j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i * 6 + j];
      for (int k = 0; k < j; ++k) s -= L[i * 6 + k] * L[j * 6 + k] * D[k];
      L[i * 6 + j] = s / d;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double s = b[i];
    for (int k = 0; k < i; ++k) s -= L[i * 6 + k] * y[k];
    y[i] = s;
  }
  for (int i = 5; i >= 0; --i) {
    double s = y[i] / D[i];
    for (int k = i + 1; k < 6; ++k) s -= L[k * 6 + i] * x[k];
    x[i] = s;
  }
  return true;
}

}  // namespace mm3d

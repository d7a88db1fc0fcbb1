// radius_grid.hpp -- the cell-sorted grid of a stage whose neighbours are the points within a fixed distance of each other: the
// cluster filter's tolerance (clusters_euclidean.hip) and the MLS smoothing's radius (smooth_mls.hip).  Host code; one text for
// both, so that the two stages' margins cannot drift apart.
#pragma once

#include <algorithm>
#include <cmath>

#include "types.hpp"

namespace mm3d {

constexpr double kRadiusCellFactor = 1.01;    // the cell over the distance: neighbours in adjacent cells whatever the rounding (radius_reach)
constexpr double kRadiusAxisCells = 1000.0;   // cells per axis at the most, as the statistical filter's grid: the cell grows instead

// The grid's cell: just above the distance, so that the box is 3^3 cells and as few candidates as can be.  Bounds as the
// statistical filter's: at most kRadiusAxisCells cells per axis and about eight cells per point (the table's memory) -- a cloud
// spread over kilometres gets a larger cell and more candidates per point, never another result.  The cloud's box is known.
inline float radius_cell(const mm3d_cloud *in, double distance)
{
  double e[3];
  for (int a = 0; a < 3; ++a) e[a] = std::max(0.0, (double)in->bmax[a] - (double)in->bmin[a]);
  const double emax = std::max(e[0], std::max(e[1], e[2]));
  double cell = std::min(distance * kRadiusCellFactor, 1e30);
  cell = std::max(cell, emax / kRadiusAxisCells);
  if (!(cell >= 1e-30) || !std::isfinite(cell)) cell = 1e-30;
  const double cap = std::max(8.0 * (double)in->n_finite, 32768.0);
  for (;;) {
    const double cells = (std::floor(e[0] / cell) + 2) * (std::floor(e[1] / cell) + 2) * (std::floor(e[2] / cell) + 2);
    if (!(cells > cap)) break;
    cell *= 1.26;
  }
  return (float)cell;
}

// How many cells to either side of a point's own hold everything within the distance of it, for the grid that cloud_grid
// returned (whose cell is the asked one or larger; a grid found under a colliding key may differ in the last digits).  Two
// neighbours are at most distance * (1 + 3e-7) apart -- d2 carries three roundings -- and each point's cell coordinate
// (v - min) * inv carries at most 4e-7 of its value, which is below the cells per axis.  So their coordinates differ by less than
// the integer returned, and their cells by at most that.  Clamping a cell into the grid only brings cells together.
inline int radius_reach(const Grid &g, double distance)
{
  const double axis = (double)std::max(g.dims[0], std::max(g.dims[1], g.dims[2]));
  const double span = distance / (double)g.cell * (1.0 + 1e-6) + 2.0 * 4e-7 * axis + 1e-6;
  return (int)std::min(std::floor(span) + 1.0, axis);
}

}  // namespace mm3d

// map_kept.hpp -- what a map carries for an opt-in stage beyond its bundle (mm3d_map: normals, NDT's voxel table, the correlative
// signature, the overlap table).  Several contexts (streams) may share a map, and a map may arrive without the structure (made
// while the stage was not selected, a cached one of such a call, one from parts) or with one of other options.
#pragma once

#include "types.hpp"

namespace mm3d {

// m's `member` if it is there and is_fresh(*it); otherwise build()'s, complete on the device before anybody else can see it.
// Under the points' lock, which is recursive: a build may ask for another kept structure of the same map.  No wait when
// the structure is there.
template <class T, class Fresh, class Build>
const T *map_kept(mm3d_ctx *ctx, const mm3d_map *m, std::unique_ptr<T> mm3d_map::*member, Fresh &&is_fresh, Build &&build)
{
  std::lock_guard<std::recursive_mutex> lk(m->points->cache_mu);
  if (const T *have = (m->*member).get(); have && is_fresh(*have)) return have;
  std::unique_ptr<T> made = build();
  ctx->sync();
  return (const_cast<mm3d_map *>(m)->*member = std::move(made)).get();
}

// the points' normals (normal_radius): point-to-plane ICP reads them, and the correlative signature is made from them
inline const mm3d_normals *map_normals(mm3d_ctx *ctx, const mm3d_map *m, const mm3d_params *p)
{
  return map_kept(ctx, m, &mm3d_map::normals, [](const mm3d_normals &) { return true; },
                  [&] { return std::unique_ptr<mm3d_normals>(compute_normals(ctx, m->points, p->normal_radius)); });
}

}  // namespace mm3d

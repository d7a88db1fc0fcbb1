// nn_search_body.hpp -- the body of the wave-cooperative exact nearest-neighbour search (nn.hip's header comment), included
// TEXTUALLY inside a kernel's body: by k_nn_wave and k_nn_probe (nn.hip) and k_icp_plane_wave (icp_plane.hip).  A shared
// device function would be the usual way, but it changes how the compiler schedules k_nn_wave; the same tokens in the same
// place compile to the same code, so the recorded counters of k_nn_wave (profiles/) describe all three.  Its wave-wide
// minima, maxima and prefix scans run on the DPP network (device_util.hpp): they sit at the top level of the pass and
// chunk loops, whose bounds are wave-uniform, with all 64 lanes enabled.
//
// Expects in scope: template parameters MODE (0: keyed search, 1: distance only) and SPLIT (1 or 4); `job` (its nblocks),
// src, items, n_items, g, max_ring, Ts (the transform, in LDS, synchronised), max_d2, rmax, and the LDS arrays s_cx, s_cy,
// s_cz, s_cw, s_off, s_beg, s_merge as k_nn_wave declares them.  Defines: bid, lane, wave, it, i, valid, p (the
// transformed query), best (its squared distance, INFINITY for none in range) and, MODE 0, bkey (d2 bits << 32 | index).
  const unsigned bid = xcd_remap(blockIdx.x, (unsigned)job.nblocks);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int item = SPLIT == 4 ? (int)bid : (int)bid * 4 + wave;   // one work item (<= 64 points of one coarse block)
  const int2 it = item < n_items ? items[item] : make_int2(0, 0);
  const int i = it.x + lane;
  const bool valid = lane < it.y;
  float3 p = make_float3(0.f, 0.f, 0.f);
  if (valid) {
    const float4 s = src[i];
    p = xform(Ts, s.x, s.y, s.z);
  }
  const int cx = cell_floor(p.x, g.minx, g.inv), cy = cell_floor(p.y, g.miny, g.inv), cz = cell_floor(p.z, g.minz, g.inv);
  bool active = valid;
  int need = max_ring;          // radius (in cells around the lane's own cell) the lane wants scanned
  float reach_cap = rmax;       // no target point of interest is farther: min(rmax, what the distance transform guarantees)
  if (active) {
    const bool inside = cx >= 0 && cx < g.dx && cy >= 0 && cy < g.dy && cz >= 0 && cz < g.dz;
    if (inside) {
      const int d0 = g.dt[((size_t)cz * g.dy + cy) * g.dx + cx];
      if (d0 > max_ring) active = false;          // nothing within range of this cell
      need = d0 > 1 ? d0 : 1;
      // an occupied cell d0 cells away holds a point within sqrt(3) (d0 + 1) cells of this one (its farthest corner): an upper
      // bound of the nearest-neighbour distance that needs no candidate (used when the corner filter below has dropped them)
      if (MM3D_NN_CORNERS && d0 <= max_ring) reach_cap = fminf(rmax, 1.7321f * (float)(d0 + 1) * g.cell * 1.0001f + 1e-5f);
#if MM3D_NN_LOWER_BOUND
      // The nearest occupied cell is d0 cells away along some axis, so no target point is nearer than (d0 - 1) cells plus the
      // way from this point to the nearest face of its own cell.  Where that already exceeds rmax the lane has no neighbour
      // in range and need not search: with 0.25 m cells and a range of 1 m that is every lane with d0 = 6 and nearly every
      // one with d0 = 5 -- a twelfth of the lanes of a headline ICP launch, and the ones whose boxes (11 and 13 cells wide)
      // were the largest of their waves (round 5; max_ring = ceil(rmax / cell) + 1 admitted them).
      if (active && d0 >= 2) {
        const float fx = p.x - (g.minx + (float)cx * g.cell), fy = p.y - (g.miny + (float)cy * g.cell), fz = p.z - (g.minz + (float)cz * g.cell);
        const float mface = fmaxf(fminf(fminf(fminf(fx, g.cell - fx), fminf(fy, g.cell - fy)), fminf(fz, g.cell - fz)), 0.0f);
        // (the slack scales with the cell and with how far the grid lies from the origin, like the corner filter's `edge`: a
        // point can sit outside its nominal cell faces by the rounding of minx + cx * cell, 3e-5 .. 6e-5 m a kilometre out)
        const float lb_edge = 1e-3f * g.cell + 1e-6f * (fabsf(g.minx) + fabsf(g.miny) + fabsf(g.minz) + (float)(g.dx + g.dy + g.dz) * g.cell);
        if ((float)(d0 - 1) * g.cell + mface * 0.999f - lb_edge >= rmax) active = false;
      }
#endif
    } else {
      // outside the grid: farther than rmax from its box means no neighbour in range
      const float ex = fmaxf(fmaxf(g.minx - p.x, p.x - (g.minx + g.dx * g.cell)), 0.0f);
      const float ey = fmaxf(fmaxf(g.miny - p.y, p.y - (g.miny + g.dy * g.cell)), 0.0f);
      const float ez = fmaxf(fmaxf(g.minz - p.z, p.z - (g.minz + g.dz * g.cell)), 0.0f);
      if (!(fmaxf(ex, fmaxf(ey, ez)) <= rmax)) active = false;
    }
  }
  // (d2 bits, original index) as one 64-bit key: d2 >= 0 so its bits order like the value, and the
  // low word breaks ties towards the lower original index, like the CPU path
  // The key starts at (max_d2, no index): a candidate beyond the correspondence distance is never a correspondence, so it
  // need not be found -- and must not send its group of four through the key-forming path below.  A candidate AT max_d2
  // still wins (any real index is below 0xffffffff), and "nothing in range yet" is the index word 0xffffffff.
  unsigned long long bkey = ((unsigned long long)__float_as_uint(max_d2) << 32) | 0xffffffffull;
  float best = INFINITY, bestd = INFINITY;

#ifdef MM3D_NN_STATS
  long long stat_ticks[3] = {0, 0, 0};
  const long long t_begin = wall_clock64();
  for (int e = 1; e <= 8; ++e) {          // what ring the lanes ask for before the first pass
    const int c_ = __popcll(ballot(active && (e < 8 ? need == e : need >= 8)));
    if (MM3D_NN_STATS == 1 && lane == 0 && c_) atomicAdd(&g_nn_stats[55 + e], (unsigned long long)c_);
  }
#endif
  bool have_old = false;                 // the previous pass's box (wave-uniform; SPLIT 4: the same in the four waves)
  int ox0 = 0, ox1 = -1, oy0 = 0, oy1 = -1, oz0 = 0, oz1 = -1;
  for (int pass = 0; pass < 64; ++pass) {
    if (!ballot(active)) break;
    MM3D_STAT(1, 1);
    MM3D_STAT(4, __popcll(ballot(active)));
    if (pass == 0) MM3D_STAT(0, 1);
    // box = bounding box of the active lanes' OWN boxes (a lane's cell grown by the radius that lane needs).  Until round 5 it
    // was the bounding box of the lanes' cells grown by the LARGEST radius any of them needs; the needs of a patch's lanes
    // differ (the distance transform changes by up to a cell per cell), and a lane with a small need at one end of the patch
    // does not have to be covered as if it had the largest.
    const int E = wave_max_i(active ? need : 0);
    MM3D_TICK(t_pass);
#if MM3D_NN_TIGHT_BOX
    const int bx0 = wave_min_i(active ? cx - need : 0x7fffffff), bx1 = wave_max_i(active ? cx + need : -0x7fffffff);
    const int by0 = wave_min_i(active ? cy - need : 0x7fffffff), by1 = wave_max_i(active ? cy + need : -0x7fffffff);
    const int bz0 = wave_min_i(active ? cz - need : 0x7fffffff), bz1 = wave_max_i(active ? cz + need : -0x7fffffff);
#else
    const int bx0 = wave_min_i(active ? cx : 0x7fffffff) - E, bx1 = wave_max_i(active ? cx : -0x7fffffff) + E;
    const int by0 = wave_min_i(active ? cy : 0x7fffffff) - E, by1 = wave_max_i(active ? cy : -0x7fffffff) + E;
    const int bz0 = wave_min_i(active ? cz : 0x7fffffff) - E, bz1 = wave_max_i(active ? cz : -0x7fffffff) + E;
#endif
    const int x0 = max(bx0, 0), x1 = min(bx1, g.dx - 1);
    const int y0 = max(by0, 0), y1 = min(by1, g.dy - 1);
    const int z0 = max(bz0, 0), z1 = min(bz1, g.dz - 1);
    const int ny = y1 - y0 + 1, nz = z1 - z0 + 1;
    const int nrows = (x0 <= x1 && ny > 0 && nz > 0) ? ny * nz : 0;
    // What this pass's box proves for a lane -- every target point nearer than `guard` has been staged -- is known before the
    // box is read (a face on the grid's own border proves everything beyond it).
    float guard = 0.0f;
    if (active) {
      const float gx0 = (bx0 > 0) ? p.x - (g.minx + (float)bx0 * g.cell) : INFINITY;
      const float gx1 = (bx1 < g.dx - 1) ? (g.minx + (float)(bx1 + 1) * g.cell) - p.x : INFINITY;
      const float gy0 = (by0 > 0) ? p.y - (g.miny + (float)by0 * g.cell) : INFINITY;
      const float gy1 = (by1 < g.dy - 1) ? (g.miny + (float)(by1 + 1) * g.cell) - p.y : INFINITY;
      const float gz0 = (bz0 > 0) ? p.z - (g.minz + (float)bz0 * g.cell) : INFINITY;
      const float gz1 = (bz1 < g.dz - 1) ? (g.minz + (float)(bz1 + 1) * g.cell) - p.z : INFINITY;
      guard = fminf(fminf(fminf(gx0, gx1), fminf(gy0, gy1)), fminf(gz0, gz1)) * 0.9999f - 1e-5f;
    }
#if MM3D_NN_CORNERS
    // Which candidates can matter is known too: none that is farther from a lane than the best that lane has (or, before it
    // has one, than the distance transform's bound).  A candidate farther than the LARGEST such bound of the active lanes from
    // the bounding box of their positions improves nobody's result and is dropped while its tile is staged: the corners of a
    // later pass's box, whose radius is that very bound rounded up to cells.  (The bound must not be what this pass PROVES,
    // `guard`: that drops more, a fifth of a headline ICP launch's candidates, but the next pass skips this pass's box on the
    // ground that its lanes have seen ALL of it -- measured: wrong scores.)
    const float far = active ? fminf(best < INFINITY ? sqrtf(best) : INFINITY, reach_cap) : 0.0f;
    const float keep_r = wave_max_f(far) * 1.0001f + 1e-5f, keep_r2 = keep_r * keep_r;
    const float plx = wave_min_f(active ? p.x : INFINITY), phx = wave_max_f(active ? p.x : -INFINITY);
    const float ply = wave_min_f(active ? p.y : INFINITY), phy = wave_max_f(active ? p.y : -INFINITY);
    const float plz = wave_min_f(active ? p.z : INFINITY), phz = wave_max_f(active ? p.z : -INFINITY);
    const float edge = 1e-3f * g.cell + 1e-6f * (fabsf(g.miny) + fabsf(g.minz) + (float)(g.dy + g.dz) * g.cell);
#endif
    // A later pass only looks at what the earlier ones have not shown its lanes: every lane that is still active scanned ALL
    // the candidates of the previous pass's box (every lane scans every staged candidate), and by induction of every box
    // before it.  So the part of the new box that lies inside the previous one is skipped: a row of the new box whose (y, z)
    // lies in the old box's range contributes the span LEFT of the old box, [x0, ox0 - 1], and -- as one of the `n_inner` extra
    // spans behind the rows -- the span RIGHT of it, [ox1 + 1, x1]; either may be empty.  (Round 5.  The second passes,
    // 0.5 per wave with the tight boxes, staged their first pass's candidates again: a sixth of all staged candidates.)
    const bool skip_old = MM3D_NN_SHELL && have_old && ox0 <= x1 && ox1 >= x0;
    const int iy0 = max(y0, oy0), iy1 = min(y1, oy1), iz0 = max(z0, oz0), iz1 = min(z1, oz1);
    const int iny = iy1 - iy0 + 1, inz = iz1 - iz0 + 1;
    const int n_inner = (skip_old && nrows > 0 && iny > 0 && inz > 0) ? iny * inz : 0;
    const int nspans = nrows + n_inner;
    for (int r0 = 0; r0 < nspans; r0 += kRows) {
      MM3D_TICK(t_hdr);
      // Span headers, FOUR per lane (spans r0 + 4 lane .. + 3): a box of up to 256 rows costs one header round trip and fuller
      // tiles instead of a header, a prefix scan and a ragged last tile per 64 rows (a pass has ~150 - 250 rows, a row ~3 points).
      // Worth 2 % where the searches are short and many (64 maps x 50 k points), nothing on the headline, whose step is bound
      // by instruction issue.  Exclusive scan of the span lengths.
      int hb[kRowsPerLane], hl[kRowsPerLane];
      {
        const int r = r0 + kRowsPerLane * lane;
        // (y, z) of span r: a row of the new box (r < nrows) or an inner row's right-hand span
        bool second = r >= nrows;
        int t = second ? r - nrows : r;
        int wy = second ? iny : ny;                    // rows per z layer of the group
        int zq = t / max(wy, 1), yr = t - zq * wy;
#pragma unroll
        for (int u = 0; u < kRowsPerLane; ++u) {
          hb[u] = 0; hl[u] = 0;
          if (!second && r + u == nrows) { second = true; wy = iny; zq = 0; yr = 0; }   // this lane's spans straddle the two groups
          if (r + u < nspans) {
            const int y = (second ? iy0 : y0) + yr, z = (second ? iz0 : z0) + zq;
            int xa = x0, xb = x1;
            if (second) xa = max(x0, ox1 + 1);
            else if (n_inner && y >= iy0 && y <= iy1 && z >= iz0 && z <= iz1) xb = min(x1, ox0 - 1);
#if MM3D_NN_CORNERS
            {
              // the same bound at cell granularity: of this row only the cells that reach into the ball around the lanes'
              // position box are read at all (`edge`: what the row's points may lie outside their cells' nominal faces)
              const float ylo = g.miny + (float)y * g.cell, zlo = g.minz + (float)z * g.cell;
              const float ey = fmaxf(fmaxf(fmaxf(ylo - phy, ply - (ylo + g.cell)), 0.0f) - edge, 0.0f);
              const float ez = fmaxf(fmaxf(fmaxf(zlo - phz, plz - (zlo + g.cell)), 0.0f) - edge, 0.0f);
              const float rem = keep_r2 - ey * ey - ez * ez;
              if (rem < 0.0f) {
                xb = xa - 1;
              } else {
                const float w = sqrtf(rem) * 1.0001f + edge;
                xa = max(xa, cell_floor(plx - w, g.minx, g.inv));     // (cell_floor is monotone: exact in x)
                xb = min(xb, cell_floor(phx + w, g.minx, g.inv));
              }
            }
#endif
            if (xa <= xb) {
              const int row = (z * g.dy + y) * g.dx;
              hb[u] = g.cell_start[row + xa];
              hl[u] = g.cell_start[row + xb + 1];
            }
          }
          if (++yr == wy) { yr = 0; ++zq; }
        }
      }
      int mine = 0;
#pragma unroll
      for (int u = 0; u < kRowsPerLane; ++u) { hl[u] -= hb[u]; mine += hl[u]; }
      const int incl = wave_scan_incl(mine);
      const int total = __builtin_amdgcn_readlane(incl, kWave - 1);
      MM3D_STAT(2, 1);
      MM3D_STAT(3, total);
      MM3D_STAT(5, min(nspans - r0, kRows));
      wave_lds_sync();                 // previous chunk's readers are done
      {
        int off = incl - mine;
#pragma unroll
        for (int u = 0; u < kRowsPerLane; ++u) {
          s_off[wave][kRowsPerLane * lane + u] = off;
          s_beg[wave][kRowsPerLane * lane + u] = hb[u];
          off += hl[u];
        }
      }
      wave_lds_sync();
      MM3D_TOCK(32, t_hdr);
      // SPLIT 4: this wave's quarter of the chunk's candidates (a multiple of four, so the padding stays at the end)
      const int share = SPLIT == 4 ? ((total + 15) >> 4) << 2 : total;
      const int t_first = SPLIT == 4 ? min(total, wave * share) : 0;
      const int t_last = SPLIT == 4 ? min(total, t_first + share) : total;
      // Tiles of kTile candidates: slot -> (row by binary search over the chunk's offsets) -> sorted target index
      // (all of a lane's gathers are issued before the first LDS store: one memory round trip per tile).
      constexpr int kPer = kTile / kWave;
      float4 stage[kPer];
      auto fetch_tile = [&](int t0, int cnt) {
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
          const int s = lane + u * kWave;
          const int slot = t0 + (s < cnt ? s : 0);
          int lo = 0;
#pragma unroll
          for (int step = kRows / 2; step > 0; step >>= 1)
            if (s_off[wave][lo + step] <= slot) lo += step;   // offsets are non-decreasing; empty rows collapse
          stage[u] = g.pts[s_beg[wave][lo] + (slot - s_off[wave][lo])];
        }
      };
      int t0 = t_first, cnt = min(kTile, t_last - t0);
      if (kPrefetch && cnt > 0) fetch_tile(t0, cnt);
      while (cnt > 0) {
        MM3D_TICK(t_stage);
        if (!kPrefetch) fetch_tile(t0, cnt);
#if MM3D_NN_CORNERS
        {
          int kept = 0;                                  // wave-uniform
#pragma unroll
          for (int u = 0; u < kPer; ++u) {
            const int s = lane + u * kWave;
            const float ex = fmaxf(fmaxf(plx - stage[u].x, stage[u].x - phx), 0.0f), ey = fmaxf(fmaxf(ply - stage[u].y, stage[u].y - phy), 0.0f);
            const float ez = fmaxf(fmaxf(plz - stage[u].z, stage[u].z - phz), 0.0f);
            const bool keep = s < cnt && ex * ex + ey * ey + ez * ez <= keep_r2;
            const unsigned long long m = ballot(keep);
            const int d = kept + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            if (keep) {
              s_cx[wave][d] = stage[u].x; s_cy[wave][d] = stage[u].y; s_cz[wave][d] = stage[u].z;
              s_cw[wave][d] = __float_as_uint(stage[u].w);
            }
            kept += __popcll(m);
          }
          MM3D_STAT(38, cnt - kept);
          cnt = kept;                                    // (the tile's next slot range was fixed above: t0n, cntn)
        }
#else
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
          const int s = lane + u * kWave;
          if (s < cnt) {
            s_cx[wave][s] = stage[u].x; s_cy[wave][s] = stage[u].y; s_cz[wave][s] = stage[u].z;
            s_cw[wave][s] = __float_as_uint(stage[u].w);
          }
        }
#endif
        // pad to a multiple of four with points at infinity (distance +inf never wins)
        if (lane < 4 && cnt + lane < ((cnt + 3) & ~3)) {
          s_cx[wave][cnt + lane] = INFINITY; s_cy[wave][cnt + lane] = INFINITY; s_cz[wave][cnt + lane] = INFINITY;
          s_cw[wave][cnt + lane] = 0x7fffffffu;
        }
        wave_lds_sync();
        const int t0n = t0 + kTile, cntn = min(kTile, t_last - t0n);
        if (kPrefetch && cntn > 0) fetch_tile(t0n, cntn);
        MM3D_TOCK(33, t_stage);
        MM3D_TICK(t_scan);
        if (active) {
          // two candidates per packed instruction; the sums are dist2()'s: ((dx*dx + dy*dy) + dz*dz)
          typedef float f2 __attribute__((ext_vector_type(2)));
          const f2 px2 = {p.x, p.x}, py2 = {p.y, p.y}, pz2 = {p.z, p.z};
          auto d2_pair = [&](float xa, float xb, float ya, float yb, float za, float zb) {
            const f2 dx = px2 - f2{xa, xb}, dy = py2 - f2{ya, yb}, dz = pz2 - f2{za, zb};
            f2 r = dx * dx;
            r += dy * dy;
            r += dz * dz;
            return r;
          };
          // (not unrolled: inside this tile loop the optimizer declines `#pragma unroll 2`, and two groups written out by
          // hand measured the same)
          for (int k = 0; k < cnt; k += 4) {
            const float4 X = *reinterpret_cast<const float4 *>(&s_cx[wave][k]);
            const float4 Y = *reinterpret_cast<const float4 *>(&s_cy[wave][k]);
            const float4 Z = *reinterpret_cast<const float4 *>(&s_cz[wave][k]);
            const f2 da = d2_pair(X.x, X.y, Y.x, Y.y, Z.x, Z.y), db = d2_pair(X.z, X.w, Y.z, Y.w, Z.z, Z.w);
            if (MODE == 1) {
              // transformScore only needs the distance
              bestd = fminf(fminf(bestd, fminf(da.x, da.y)), fminf(db.x, db.y));
            } else {
              // The (distance, index) key is only formed where it can matter: if the nearest of these four candidates is
              // farther than what EVERY active lane already holds, no key of the group can win or tie (d2 >= 0: its bits
              // order like its value; the initial key holds max_d2).  Candidates arrive row by row, so a
              // wave's lanes stop improving together once the rows near their patch are behind them: about half of the
              // groups take this exit, and a group that does costs 3 instead of 22 instructions on top of the distances
              // (round 4: the step is bound by VALU instructions).
              const float m4 = fminf(fminf(da.x, da.y), fminf(db.x, db.y));
              if (ballot(__float_as_uint(m4) <= (unsigned)(bkey >> 32))) {
                const uint4 W = *reinterpret_cast<const uint4 *>(&s_cw[wave][k]);
                const unsigned long long k0 = ((unsigned long long)__float_as_uint(da.x) << 32) | W.x;
                const unsigned long long k1 = ((unsigned long long)__float_as_uint(da.y) << 32) | W.y;
                const unsigned long long k2 = ((unsigned long long)__float_as_uint(db.x) << 32) | W.z;
                const unsigned long long k3 = ((unsigned long long)__float_as_uint(db.y) << 32) | W.w;
                const unsigned long long a = k0 < k1 ? k0 : k1, b2 = k2 < k3 ? k2 : k3;
                const unsigned long long m = a < b2 ? a : b2;
                bkey = m < bkey ? m : bkey;
              }
            }
          }
        }
        wave_lds_sync();                 // the tile's readers are done before the next one is stored
        MM3D_TOCK(34, t_scan);
        t0 = t0n; cnt = cntn;
      }
    }
    if (SPLIT == 4) {      // the four quarters' minima (every wave then goes on with the same state)
      s_merge[wave][lane] = MODE == 1 ? (unsigned long long)__float_as_uint(bestd) : bkey;   // d2 >= 0: bits order like values
      __syncthreads();
      const unsigned long long m0 = s_merge[0][lane], m1 = s_merge[1 % SPLIT][lane], m2 = s_merge[2 % SPLIT][lane],
                               m3 = s_merge[3 % SPLIT][lane];
      const unsigned long long ma = m0 < m1 ? m0 : m1, mb = m2 < m3 ? m2 : m3, m = ma < mb ? ma : mb;
      __syncthreads();
      if (MODE == 1) bestd = __uint_as_float((unsigned)m);
      else bkey = m;
    }
    if (nrows > 0) { have_old = true; ox0 = x0; ox1 = x1; oy0 = y0; oy1 = y1; oz0 = z0; oz1 = z1; }
    // what the scanned box proves: every target point closer than `guard` to this lane has been seen
    best = MODE == 1 ? bestd : (((unsigned)bkey == 0xffffffffu) ? INFINITY : __uint_as_float((unsigned)(bkey >> 32)));
    if (active) {
      if (guard >= rmax || best <= guard * guard) {
        active = false;
      } else {
        const float reach = best < INFINITY ? fminf(sqrtf(best), reach_cap) : reach_cap;
        const int want = (int)ceilf(reach * g.inv * 1.001f + 0.01f);   // guard >= want*cell*0.9999 - 1e-5 >= reach
        // (at least one ring more than this lane had: best > guard^2 and guard >= need cells already make `want` that large;
        // with the common radius of rounds 1 - 4 it was E + 1, the wave's largest plus one)
        need = min(max(want, (MM3D_NN_TIGHT_BOX ? need : E) + 1), max_ring + pass + 1);
      }
    }
#ifdef MM3D_NN_STATS
    if (MM3D_NN_STATS == 1 && lane == 0) {     // per ring size: passes, their ticks, active lanes
      const int e = E < 7 ? E : 7;
      atomicAdd(&g_nn_stats[40 + e], 1ull);
      atomicAdd(&g_nn_stats[48 + e], (unsigned long long)(wall_clock64() - t_pass));
    }
#endif
  }

#ifdef MM3D_NN_STATS
  if (it.y > 0 && lane == 0) {
    const unsigned long long dt = (unsigned long long)(wall_clock64() - t_begin);   // 100 MHz ticks
    atomicMax(&g_nn_stats[6], dt);
    atomicAdd(&g_nn_stats[7], dt);
    for (int k_ = 0; k_ < 3; ++k_) atomicAdd(&g_nn_stats[32 + k_], (unsigned long long)stat_ticks[k_]);
    int b = 0;
    while ((dt >> b) > 1 && b < 30) ++b;
    atomicAdd(&g_nn_stats[8 + b], 1ull);
  }
#endif

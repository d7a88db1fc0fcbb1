"""The Hilbert order and the wave work items of a cloud (csrc/grid.hip: cloud_hilbert) through the test hook
mm3d_debug_hilbert_order, against the numpy restatement tests/nn_cases.py::hilbert_items: the order index for index, the items
pair for pair.  The clouds sit where the kernels take another path: one item and the 64-point split, the fused scan's tile edge
(kScanTile = 4096 elements, the scan running over n + 1), a head at every element, non-finite points, a column past
kHilColumnMax (the radix fallback and the inert first attempt), the box sizes at which the column table's size changes
(4^k columns, k from the box's upper corner), the grown cell, and a box without extent.

An item never straddles the scan's tile edge -- 4096 is a multiple of 64, and every 64th element is a head -- so "begins in the
last 63 elements of tile 0 and ends in tile 1" reads here as: begins there and is ended by tile 1's first head, the one case in
which the next head is looked for behind the tile."""
import numpy as np
import pytest

import nn_cases as nc

pytestmark = pytest.mark.gpu

F = np.float32
TILE = 4096


def restated(src, min_cell=0.25):
    """nn_cases.hilbert_items with the cell rule of cloud_hilbert's min_cell: cell = max(0.25, min_cell, largest side / 1023)."""
    src = np.asarray(src, dtype=F).reshape(-1, 3)
    fin = np.flatnonzero(np.isfinite(src).all(axis=1))
    pts = src[fin]
    if len(pts) == 0:
        return fin, []
    bmin, bmax = pts.min(axis=0), pts.max(axis=0)
    cell = max(max(F(0.25), F(min_cell)), F((bmax - bmin).max()) / F(1023.0))
    inv = F(1.0) / F(cell)
    c = np.clip(np.floor((pts - bmin) * inv), 0, 1023).astype(np.uint64)
    x, y, z = c[:, 0].copy(), c[:, 1].copy(), c[:, 2]
    d = np.zeros(len(pts), dtype=np.uint64)
    s = 512
    while s > 0:
        rx, ry = ((x & s) > 0).astype(np.uint64), ((y & s) > 0).astype(np.uint64)
        d += np.uint64(s * s) * ((np.uint64(3) * rx) ^ ry)
        flip = (ry == 0) & (rx == 1)
        x[flip], y[flip] = 1023 - x[flip], 1023 - y[flip]
        swap = ry == 0
        x[swap], y[swap] = y[swap], x[swap].copy()
        s >>= 1
    key = ((d << np.uint64(10)) | z) & np.uint64(0xFFFFFFFF)
    order = np.argsort(key, kind="stable")
    k = key[order]
    j = np.arange(len(k))
    head = (j & 63) == 0
    head[1:] |= (k[1:] >> np.uint64(16)) != (k[:-1] >> np.uint64(16))
    starts = np.flatnonzero(head)
    counts = np.diff(np.append(starts, len(k)))
    return fin[order], list(zip(starts.tolist(), counts.tolist()))


def max_column(src, min_cell=0.25):
    """the largest column coordinate of the finite points: the column table holds 4^k columns, 2^k above this"""
    src = np.asarray(src, dtype=F).reshape(-1, 3)
    pts = src[np.isfinite(src).all(axis=1)]
    bmin, bmax = pts.min(axis=0), pts.max(axis=0)
    cell = max(max(F(0.25), F(min_cell)), F((bmax - bmin).max()) / F(1023.0))
    c = np.clip(np.floor((pts - bmin) * (F(1.0) / F(cell))), 0, 1023)
    return int(c[:, :2].max())


def in_blocks(rng, blocks):
    """[(bx, by, count)] -> points inside those 2 m x 2 m column blocks (8 x 8 cells of 0.25 m), z within a metre; the first point
    of block (0, 0) is the origin, so the box starts there and the blocks are the order's own."""
    out = []
    for bx, by, m in blocks:
        p = np.empty((m, 3), dtype=F)
        p[:, 0] = 2.0 * bx + rng.uniform(0.01, 1.99, m)
        p[:, 1] = 2.0 * by + rng.uniform(0.01, 1.99, m)
        p[:, 2] = rng.uniform(0.0, 1.0, m)
        if (bx, by) == (0, 0):
            p[0] = 0.0
        out.append(p)
    p = np.concatenate(out)
    return p[rng.permutation(len(p))]


def check(ctx, src, min_cell=0.25):
    """the device's (order, items) equal the restatement's; returns the restatement's"""
    src = np.asarray(src, dtype=F).reshape(-1, 3)
    ref_order, ref_items = restated(src, min_cell)
    if min_cell == 0.25:
        nc_order, nc_items = nc.hilbert_items(src)
        assert np.array_equal(nc_order, ref_order) and nc_items == ref_items, "the restatement here left nn_cases.hilbert_items"
    order, items = ctx.debugHilbertOrder(ctx.cloud(nc.points(src)), min_cell)
    assert len(order) == len(ref_order), (len(order), len(ref_order))
    bad = np.flatnonzero(order != ref_order)
    assert len(bad) == 0, "order differs at %d of %d positions, first %d: device %d, restated %d" % (
        len(bad), len(order), bad[0], order[bad[0]], ref_order[bad[0]])
    got = [tuple(r) for r in items.tolist()]
    assert len(got) == len(ref_items), "%d items, %d restated" % (len(got), len(ref_items))
    wrong = [(a, b) for a, b in zip(got, ref_items) if a != b]
    assert not wrong, "%d of %d items differ, first: device %s, restated %s" % (len(wrong), len(got), wrong[0][0], wrong[0][1])
    return ref_order, ref_items


def test_one_point(ctx):
    _, items = check(ctx, [[3.0, -2.0, 1.0]])
    assert items == [(0, 1)]


@pytest.mark.parametrize("n", [63, 64, 65])
def test_one_column_block(ctx, n):
    """one item of 63, one of 64, and the split at the 64th point"""
    _, items = check(ctx, in_blocks(np.random.default_rng(n), [(0, 0, n)]))
    assert items == ([(0, n)] if n <= 64 else [(0, 64), (64, n - 64)])


@pytest.mark.parametrize("first", [TILE - 30, TILE, TILE + 4])
@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, TILE + 70])
def test_scan_tile_edge(ctx, n, first):
    """Block (0, 0) holds the Hilbert curve's first 64 columns and sorts first, so the block changes at sorted position `first`:
    30 elements before the scan's tile edge (that item runs up to the edge and is ended by tile 1's first head, by the j == n
    element behind the edge at n = 4096, or inside tile 0 by the j == n element at n = 4095), on the edge, or 4 behind it."""
    blocks = [(0, 0, min(first, n))] + ([(1, 0, n - first)] if n > first else [])
    _, items = check(ctx, in_blocks(np.random.default_rng(n * 7 + first), blocks))
    starts = [s for s, _ in items]
    if first < n:
        assert first in starts
    if first == TILE - 30:
        assert (TILE - 64, 34) in items                           # cut short by the block change
        assert (first, min(30, n - first)) in items               # up to the tile edge, or to the last point
    else:
        assert (TILE - 64, min(64, n - (TILE - 64))) in items     # ends exactly on the tile edge, or with the last point
    assert items[-1][0] + items[-1][1] == n                       # the last item's next head is the j == n element


def test_every_element_a_head(ctx):
    """5 000 points, each alone in its column block: a head at every element, across the tile edge"""
    b = np.arange(71 * 71)[:5000]
    p = np.stack([2.0 * (b % 71) + 0.5, 2.0 * (b // 71) + 0.5, np.linspace(0.0, 3.0, len(b))], axis=1).astype(F)
    _, items = check(ctx, p[np.random.default_rng(5).permutation(len(p))])
    assert len(items) == 5000 and all(cnt == 1 for _, cnt in items)


def test_non_finite_points_stay_out(ctx):
    rng = np.random.default_rng(11)
    p = in_blocks(rng, [(0, 0, 300), (1, 1, 150), (3, 0, 250)])
    bad = rng.choice(len(p), 90, replace=False)
    p[bad[:30], 0] = np.nan
    p[bad[30:60], 1] = np.inf
    p[bad[60:], 2] = -np.inf
    order, _ = check(ctx, p)
    assert len(order) == len(p) - 90


@pytest.mark.parametrize("n", [1024, 1100])
def test_long_column(ctx, n):
    """n points in one 0.25 m column: 1 100 is past kHilColumnMax = 1024 -- the counting sort gives up, the first scan is inert,
    the radix sort orders the keys and the second scan makes the items; 1 024 stays with the counting sort.  A second column
    block keeps the items from being one run."""
    rng = np.random.default_rng(n)
    col = np.stack([rng.uniform(0.0, 0.2, n), rng.uniform(0.0, 0.2, n), rng.uniform(0.0, 40.0, n)], axis=1).astype(F)
    col[0] = 0.0
    far = np.stack([rng.uniform(5.0, 9.0, 200), rng.uniform(5.0, 9.0, 200), rng.uniform(0.0, 40.0, 200)], axis=1).astype(F)
    p = np.concatenate([col, far])
    order, items = check(ctx, p[rng.permutation(len(p))])
    assert len(order) == n + 200


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("cells", [63.9, 64.0, 64.1])
def test_column_table_boundary(ctx, cells, swap):
    """the box spans 63.9, 64.0 and 64.1 cells of 0.25 m along one column axis and little along the other: the largest column
    coordinate is 63, 64, 64 -- on either side of the step from 4^6 to 4^7 columns"""
    rng = np.random.default_rng(int(cells * 10) + swap)
    ext = F(cells * 0.25)
    p = np.stack([rng.uniform(0.0, float(ext), 600), rng.uniform(0.0, 1.0, 600), rng.uniform(0.0, 2.0, 600)], axis=1).astype(F)
    p[0] = 0.0
    p[1] = [ext, 1.0, 2.0]
    p[2:40, 0] = ext                                            # a populated last column
    if swap:
        p = p[:, [1, 0, 2]]
    assert max_column(p) == (63 if cells < 64.0 else 64)
    check(ctx, p)


def test_grown_cell(ctx):
    """wider than 1 023 cells of 0.25 m: the cell grows to side / 1023 and the column coordinates use all ten bits"""
    rng = np.random.default_rng(3)
    p = np.stack([rng.uniform(0.0, 300.0, 700), rng.uniform(0.0, 280.0, 700), rng.uniform(0.0, 5.0, 700)], axis=1).astype(F)
    p[0] = 0.0
    p[1] = [300.0, 280.0, 5.0]
    assert max_column(p) >= 1022
    check(ctx, p)


def test_no_extent_in_x_and_y(ctx):
    """every point in one column at the box's corner: a table of one column"""
    rng = np.random.default_rng(4)
    p = np.stack([np.full(200, 7.5), np.full(200, -3.25), rng.uniform(0.0, 30.0, 200)], axis=1).astype(F)
    assert max_column(p) == 0
    _, items = check(ctx, p)
    assert [cnt for _, cnt in items] == [64, 64, 64, 8]


@pytest.mark.parametrize("min_cell", [0.5, 1.0, 2.5])
def test_larger_min_cell(ctx, min_cell):
    """SIFT's later octaves pass a larger cell: the column blocks grow with it"""
    rng = np.random.default_rng(int(min_cell * 10))
    p = np.stack([rng.uniform(-20.0, 25.0, 5000), rng.uniform(0.0, 30.0, 5000), rng.uniform(0.0, 3.0, 5000)], axis=1).astype(F)
    check(ctx, p, min_cell)

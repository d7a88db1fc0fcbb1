"""The correlative coarse alignment (mm3d_set_coarse_alignment, mm3d_estimate_transform_correlative and its two test hooks): a
numpy restatement of the whole rule of include/mm3d.h, and on a planted yard the signature cell by cell, votes / candidates /
fine scores / winner integer by integer, recovery of planted poses, the whole-map call end to end, bit-identical records
across the drivers, and the edge cases."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE, CORRELATIVE = 0, 1
SAC_IA, MATCHING = 1, 0
EINVAL, EUNSUPPORTED = -1, -4
DEFAULT_MULTIPLE = 5.0           # cell = 0 means this times params.resolution (include/mm3d.h)
F32 = np.float32


# ---------------------------------------------------------------- the restatement (also read by test_coarse_cpu.py)
def cells_of(xy, cell):
    """(floorf(x * inv), floorf(y * inv)) with inv = 1.0f / (float)cell, every step one float operation."""
    inv = F32(1.0) / F32(cell)
    return np.floor((np.asarray(xy, dtype=F32) * inv).astype(F32)).astype(np.int64)


def restate_signature(xyz, nrm, cell, F=4, wall_nz=0.5, ground_nz=0.9, min_points=3):
    """A map's signature: structure [n][3] (i, j, count), ground [n][3], ground_height [n] (the double mean rounded once),
    coarse [n][2], each ascending in (i, j)."""
    xyz, nrm = np.asarray(xyz, dtype=F32).reshape(-1, 3), np.asarray(nrm, dtype=F32).reshape(-1, 3)
    ok = np.isfinite(xyz).all(axis=1) & np.isfinite(nrm).all(axis=1)
    xyz, nrm = xyz[ok], nrm[ok]
    with np.errstate(all="ignore"):
        ij = cells_of(xyz[:, :2], cell)
    az = np.abs(nrm[:, 2])
    out = {}
    for name, sel in (("structure", az <= F32(wall_nz)), ("ground", az >= F32(ground_nz))):
        c, z = ij[sel], xyz[sel, 2].astype(np.float64)
        order = np.lexsort((c[:, 1], c[:, 0]))                      # stable: ascending input index inside a cell
        c, z = c[order], z[order]
        heads = np.flatnonzero(np.r_[True, (np.diff(c, axis=0) != 0).any(axis=1)]) if len(c) else np.zeros(0, dtype=np.int64)
        ends = np.r_[heads[1:], len(c)]
        keep = (ends - heads) >= min_points
        out[name] = np.c_[c[heads[keep]], (ends - heads)[keep]].astype(np.int64).reshape(-1, 3)
        if name == "ground":
            out["ground_height"] = np.array([z[a:b].sum() / (b - a) for a, b in zip(heads[keep], ends[keep])]).astype(F32)
    s = out["structure"][:, :2]
    out["coarse"] = np.unique(np.floor_divide(s, F), axis=0).reshape(-1, 2) if len(s) else np.zeros((0, 2), dtype=np.int64)
    return out


def yaw_table(yaw_steps):
    """(float)cos(2 pi k / yaw_steps), (float)sin(...): the angle and the functions in double (libm's, as the host's)."""
    th = [2.0 * math.pi * k / yaw_steps for k in range(yaw_steps)]
    return np.array([math.cos(t) for t in th]).astype(F32), np.array([math.sin(t) for t in th]).astype(F32)


def _centres(ij, side):
    return ((np.asarray(ij)[:, :2].astype(F32) + F32(0.5)) * F32(side)).astype(F32)


def _rotate(cs, sn, p):
    return (cs * p[:, 0]).astype(F32) - (sn * p[:, 1]).astype(F32), (sn * p[:, 0]).astype(F32) + (cs * p[:, 1]).astype(F32)


def restate_votes(src_coarse, tgt_coarse, cell, F, G, yaw_steps):
    """The coarse accumulator on its own tight frame: (acc [Q][U][V], u_min, v_min)."""
    C = F32(cell) * F32(F)
    invC = F32(1.0) / C
    cs, sn = yaw_table(yaw_steps)
    P, T = _centres(src_coarse, C), _centres(tgt_coarse, C)
    Q = yaw_steps // G
    uv = []
    for q in range(Q):
        rx, ry = _rotate(cs[q * G], sn[q * G], P)
        u = np.floor(((T[None, :, 0] - rx[:, None]) * invC).astype(F32) + F32(0.5)).astype(np.int64)
        v = np.floor(((T[None, :, 1] - ry[:, None]) * invC).astype(F32) + F32(0.5)).astype(np.int64)
        uv.append((u.ravel(), v.ravel()))
    u0, v0 = min(u.min() for u, _ in uv), min(v.min() for _, v in uv)
    U, V = max(u.max() for u, _ in uv) - u0 + 1, max(v.max() for _, v in uv) - v0 + 1
    acc = np.zeros((Q, U, V), dtype=np.int64)
    for q, (u, v) in enumerate(uv):
        np.add.at(acc[q], (u - u0, v - v0), 1)
    return acc, int(u0), int(v0)


def restate_candidates(acc, u0, v0, K):
    """[n][4] (q, u, v, votes): cells with >= 1 vote that no other cell of their 3 x 3 x 3 neighbourhood (cyclic in q) beats --
    more votes, or as many and an earlier (q, u, v) -- the K best, votes descending, then (q, u, v) ascending."""
    Q, U, V = acc.shape
    assert Q >= 3
    pad = np.zeros((Q, U + 2, V + 2), dtype=np.int64)
    pad[:, 1:-1, 1:-1] = acc
    lin = np.arange(pad.size).reshape(pad.shape)                       # the order of the linear index, whatever the frame
    own, own_lin = pad[:, 1:-1, 1:-1], lin[:, 1:-1, 1:-1]
    keep = own >= 1
    for dq in (-1, 0, 1):
        rp, rl = np.roll(pad, -dq, axis=0), np.roll(lin, -dq, axis=0)  # rp[q] = pad[(q + dq) mod Q]
        for du in (-1, 0, 1):
            for dv in (-1, 0, 1):
                if (dq, du, dv) == (0, 0, 0):
                    continue
                nv, nl = rp[:, 1 + du:U + 1 + du, 1 + dv:V + 1 + dv], rl[:, 1 + du:U + 1 + du, 1 + dv:V + 1 + dv]
                keep &= ~((nv > own) | ((nv == own) & (nl < own_lin)))
    q, u, v = np.nonzero(keep)
    votes = acc[q, u, v]
    order = np.lexsort((v, u, q, -votes))[:K]
    return np.c_[q[order], u[order] + u0, v[order] + v0, votes[order]].astype(np.int64).reshape(-1, 4)


def _dense(cells, dilate):
    """(boolean or float map, i_min, j_min) over the cells' box padded by two."""
    i0, j0 = cells[:, 0].min() - 2, cells[:, 1].min() - 2
    shape = (cells[:, 0].max() - i0 + 3, cells[:, 1].max() - j0 + 3)
    m = np.zeros(shape, dtype=bool)
    for di in ((-1, 0, 1) if dilate else (0,)):
        for dj in ((-1, 0, 1) if dilate else (0,)):
            m[cells[:, 0] - i0 + di, cells[:, 1] - j0 + dj] = True
    return m, i0, j0


def _lookup(m, i0, j0, ci, cj):
    """m[ci - i0, cj - j0] where inside, False elsewhere (ci, cj broadcast)."""
    a, b = ci - i0, cj - j0
    inside = (a >= 0) & (a < m.shape[0]) & (b >= 0) & (b < m.shape[1])
    return np.where(inside, m[np.clip(a, 0, m.shape[0] - 1), np.clip(b, 0, m.shape[1] - 1)], False)


def restate_fine(src_structure, tgt_structure, cands, cell, F, G, yaw_steps):
    """scores [n][2G+1][2F+1][2F+1] of the candidates."""
    c = F32(cell)
    inv = F32(1.0) / c
    cs, sn = yaw_table(yaw_steps)
    dil, i0, j0 = _dense(tgt_structure, True)
    P = _centres(src_structure, c)
    ab = np.arange(-F, F + 1)
    scores = np.zeros((len(cands), 2 * G + 1, 2 * F + 1, 2 * F + 1), dtype=np.int64)
    for r, (q, u, v, _) in enumerate(cands):
        sx = ((u * F + ab).astype(F32) * c).astype(F32)
        sy = ((v * F + ab).astype(F32) * c).astype(F32)
        for gi, g in enumerate(range(-G, G + 1)):
            k = (q * G + g) % yaw_steps
            rx, ry = _rotate(cs[k], sn[k], P)
            ci = np.floor(((rx[None, :] + sx[:, None]).astype(F32) * inv).astype(F32)).astype(np.int64)     # [a][n]
            cj = np.floor(((ry[None, :] + sy[:, None]).astype(F32) * inv).astype(F32)).astype(np.int64)     # [b][n]
            scores[r, gi] = _lookup(dil, i0, j0, ci[:, None, :], cj[None, :, :]).sum(axis=2)
    return scores


def _ldlt3(A, b, floor):
    L, D = np.zeros((3, 3)), np.zeros(3)
    for j in range(3):
        d = A[j, j] - sum(L[j, k] * L[j, k] * D[k] for k in range(j))
        if not d > floor:
            return None
        D[j] = d
        for i in range(j + 1, 3):
            L[i, j] = (A[i, j] - sum(L[i, k] * L[j, k] * D[k] for k in range(j))) / d
    y = np.zeros(3)
    for i in range(3):
        y[i] = b[i] - sum(L[i, k] * y[k] for k in range(i))
    x = np.zeros(3)
    for i in (2, 1, 0):
        x[i] = y[i] / D[i] - sum(L[k, i] * x[k] for k in range(i + 1, 3))
    return x


def compose(alpha, beta, gamma, cs, sn, sx, sy):
    """Trans(0, 0, gamma) Rx(atan beta) Ry(-atan alpha) [Rz | s] in double, as a float 4 x 4."""
    ia, ib = 1.0 / math.sqrt(1.0 + alpha * alpha), 1.0 / math.sqrt(1.0 + beta * beta)
    cphi, sphi, cpsi, spsi = ia, -alpha * ia, ib, beta * ib
    M = np.array([[cphi, 0.0, sphi], [spsi * sphi, cpsi, -spsi * cphi], [-cpsi * sphi, spsi, cpsi * cphi]])
    Rz = np.array([[cs, -sn, 0.0], [sn, cs, 0.0], [0.0, 0.0, 1.0]], dtype=np.float64)
    T = np.eye(4)
    T[:3, :3] = M @ Rz
    T[:3, 3] = M @ np.array([sx, sy, 0.0], dtype=np.float64) + [0.0, 0.0, gamma]
    return T.astype(F32)


def restate_align(S, T, cell, F=4, G=6, yaw_steps=720, K=32, accept_fraction=0.25):
    """The whole search on two signatures: a dict of T, stats, the plane (alpha, beta, gamma), acc / frame, cands, scores."""
    ns, nt = len(S["structure"]), len(T["structure"])
    stats = dict(source_cells=ns, target_cells=nt, coarse_votes=0, candidates=0, score=0, yaw_index=-1, ground_pairs=0, converged=0)
    if ns == 0 or nt == 0:
        return dict(T=np.eye(4, dtype=F32), stats=stats, plane=(0.0, 0.0, 0.0), cands=np.zeros((0, 4), dtype=np.int64))
    acc, u0, v0 = restate_votes(S["coarse"], T["coarse"], cell, F, G, yaw_steps)
    cands = restate_candidates(acc, u0, v0, K)
    scores = restate_fine(S["structure"], T["structure"], cands, cell, F, G, yaw_steps)
    rank, gi, ai, bi = np.unravel_index(int(np.argmax(scores)), scores.shape)          # the first maximum: lowest (rank, g, a, b)
    q, u, v, votes = (int(x) for x in cands[rank])
    k = (q * G + gi - G) % yaw_steps
    cs, sn = yaw_table(yaw_steps)
    c = F32(cell)
    inv = F32(1.0) / c
    sx, sy = F32(u * F + ai - F) * c, F32(v * F + bi - F) * c
    alpha = beta = gamma = 0.0
    n = 0
    if len(S["ground"]) and len(T["ground"]):
        rx, ry = _rotate(cs[k], sn[k], _centres(S["ground"], c))
        x, y = (rx + sx).astype(F32), (ry + sy).astype(F32)
        ci, cj = np.floor((x * inv).astype(F32)).astype(np.int64), np.floor((y * inv).astype(F32)).astype(np.int64)
        gmap, i0, j0 = _dense(T["ground"], False)
        hmap = np.zeros(gmap.shape)
        hmap[T["ground"][:, 0] - i0, T["ground"][:, 1] - j0] = T["ground_height"].astype(np.float64)
        hit = _lookup(gmap, i0, j0, ci, cj)
        n = int(hit.sum())
        if n:
            x, y = x[hit].astype(np.float64), y[hit].astype(np.float64)
            d = hmap[ci[hit] - i0, cj[hit] - j0] - S["ground_height"][hit].astype(np.float64)
            gamma = d.sum() / n
            if n >= 16:
                A = np.array([[(x * x).sum(), (x * y).sum(), x.sum()], [(x * y).sum(), (y * y).sum(), y.sum()], [x.sum(), y.sum(), float(n)]])
                sol = _ldlt3(A, np.array([(x * d).sum(), (y * d).sum(), d.sum()]), 1e-12 * (A[0, 0] + A[1, 1] + A[2, 2]) / 3.0)
                if sol is not None and np.isfinite(sol).all() and math.hypot(sol[0], sol[1]) <= math.tan(math.radians(20.0)):
                    alpha, beta, gamma = (float(s) for s in sol)
    score = int(scores[rank, gi, ai, bi])
    stats.update(coarse_votes=votes, candidates=len(cands), score=score, yaw_index=int(k), ground_pairs=n,
                 converged=int(float(score) >= accept_fraction * float(ns)))
    return dict(T=compose(alpha, beta, gamma, cs[k], sn[k], sx, sy), stats=stats, plane=(alpha, beta, gamma), acc=acc, frame=(u0, v0),
                cands=cands, scores=scores, shift=(u * F + ai - F, v * F + bi - F))


def plane_of(T, cs, sn):
    """(alpha, beta, gamma) back out of a composed transform whose yaw is (cs, sn): the third row of Rx Ry is
    (alpha, beta sqrt(1 + alpha^2), 1) / (sqrt(1 + alpha^2) sqrt(1 + beta^2))."""
    T = np.asarray(T, dtype=np.float64)
    M = T[:3, :3] @ np.array([[cs, -sn, 0.0], [sn, cs, 0.0], [0.0, 0.0, 1.0]], dtype=np.float64).T      # Rx Ry
    alpha = M[2, 0] / M[2, 2]
    # the translation is M (sx, sy, 0) + (0, 0, gamma): its part along M's third column is gamma's alone
    return alpha, M[2, 1] / M[2, 2] / math.sqrt(1.0 + alpha * alpha), float(M[:, 2] @ T[:3, 3]) / M[2, 2]


# literal vectors (test_coarse_cpu.py reproduces them with the restatement): ten points at cell 0.5, min_points 2, F 2
TEN_POINTS = np.array([[0.10, 0.10, 1.0], [0.20, 0.30, 2.0], [0.49, 0.0, 4.0],      # cell (0, 0): walls, 3 points
                       [-0.10, 0.10, 0.5], [-0.40, 0.20, 0.7],                      # cell (-1, 0): ground, heights 0.5 and 0.7
                       [-0.01, -0.01, 1.0],                                         # cell (-1, -1): one wall point, below min_points
                       [1.60, -0.70, 0.0], [1.90, -0.60, 0.0],                      # cell (3, -2): walls
                       [1.60, -0.70, 0.25], [np.nan, 0.0, 0.0]], dtype=F32)         # (3, -2): one ground point; a NaN point
TEN_NORMALS = np.array([[1, 0, 0], [0, 1, 0.5], [1, 0, 0], [0, 0, 1], [0, 0.3, -0.95], [1, 0, 0], [0, -1, 0], [1, 0, 0.2], [0, 0, 1],
                        [1, 0, 0]], dtype=F32)
TEN_STRUCTURE = [[0, 0, 3], [3, -2, 2]]
TEN_GROUND, TEN_HEIGHT = [[-1, 0, 2]], [0.6]
TEN_COARSE = [[0, 0], [1, -1]]
# a 3 x 3-cell pair at cell 1, F 1, yaw_steps 8, G 2 (Q 4): source coarse cells (0, 0) (1, 0), target (0, 1) (1, 1) (2, 0).
# q = 0 is the identity: (u, v) = t - s; q = 1 a quarter turn: r = (-py, px), so s (0, 0) -> (-0.5, 0.5), s (1, 0) -> (-0.5, 1.5)
PAIR_SRC, PAIR_TGT = [[0, 0], [1, 0]], [[0, 1], [1, 1], [2, 0]]
PAIR_VOTES = {0: {(0, 1): 2, (1, 1): 1, (2, 0): 1, (-1, 1): 1, (1, 0): 1},
              1: {(1, 1): 1, (2, 1): 1, (3, 0): 1, (1, 0): 1, (2, 0): 1, (3, -1): 1}}


# ---------------------------------------------------------------- the planted yard
CELL = 0.5
BOXES = [(-8.0, -7.0, 3.0, 2.0, 2.5), (-2.5, 5.5, 2.0, 4.0, 1.5), (3.0, -3.5, 1.5, 1.5, 3.0), (7.5, 6.0, 4.0, 1.0, 2.0),
         (-6.5, 2.0, 1.0, 3.0, 1.0), (1.5, -9.0, 5.0, 1.5, 1.8)]                 # (x, y of the low corner, size x, size y, height)


def _ground(x, y):
    z = 0.15 * np.sin(x / 4.0) * np.cos(y / 5.0)
    n = np.c_[-0.15 / 4.0 * np.cos(x / 4.0) * np.cos(y / 5.0), 0.15 / 5.0 * np.sin(x / 4.0) * np.sin(y / 5.0), np.ones_like(x)]
    return z, n / np.linalg.norm(n, axis=1, keepdims=True)


def yard(seed=5, n_ground=36000, wall_density=40.0):
    """(xyz, normals) of the whole yard in the world frame, double: rolling ground of 24 m x 24 m and six boxes."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(-12.0, 12.0, size=(n_ground, 2))
    for bx, by, sx, sy, _ in BOXES:
        g = g[~((g[:, 0] > bx) & (g[:, 0] < bx + sx) & (g[:, 1] > by) & (g[:, 1] < by + sy))]
    z, n = _ground(g[:, 0], g[:, 1])
    pts, nrm = [np.c_[g, z]], [n]
    for bx, by, sx, sy, h in BOXES:
        for axis, at, sign in ((0, bx, -1.0), (0, bx + sx, 1.0), (1, by, -1.0), (1, by + sy, 1.0)):
            length = sy if axis == 0 else sx
            m = int(wall_density * length * h)
            along, up = rng.uniform(0.0, length, m), rng.uniform(0.2, h, m)
            p = np.c_[np.full(m, at), by + along, up] if axis == 0 else np.c_[bx + along, np.full(m, at), up]
            pts.append(p)
            nrm.append(np.tile([sign, 0.0, 0.0] if axis == 0 else [0.0, sign, 0.0], (m, 1)))
        m = int(60.0 * sx * sy)
        pts.append(np.c_[rng.uniform(bx, bx + sx, m), rng.uniform(by, by + sy, m), np.full(m, h)])
        nrm.append(np.tile([0.0, 0.0, 1.0], (m, 1)))
    return np.concatenate(pts), np.concatenate(nrm)


def pose(yaw_deg=0.0, shift=(0.0, 0.0), tilt_x_deg=0.0, tilt_y_deg=0.0, height=0.0):
    """Trans(0, 0, height) Rx Ry [Rz | shift] in double: the transform source -> target of a planted pair."""
    a, b, t = math.radians(tilt_x_deg), math.radians(tilt_y_deg), math.radians(yaw_deg)
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rz = np.array([[math.cos(t), -math.sin(t), 0], [math.sin(t), math.cos(t), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rx @ Ry @ Rz
    T[:3, 3] = Rx @ Ry @ np.array([shift[0], shift[1], 0.0]) + [0.0, 0.0, height]
    return T


def carried(xyz, nrm, T_to_world):
    """The window's points and normals in a map frame whose transform to the world frame is T_to_world."""
    Ti = np.linalg.inv(T_to_world)
    return (xyz @ Ti[:3, :3].T + Ti[:3, 3]).astype(F32), (nrm @ Ti[:3, :3].T).astype(F32)


WINDOWS = [(-12.0, 6.0, -12.0, 12.0), (-6.0, 12.0, -12.0, 12.0), (-12.0, 12.0, -6.0, 12.0)]      # x0 x1 y0 y1: >= 60 % shared
POSES = [pose(), pose(35.0, (3.0, -2.0)), pose(-110.0, (-1.5, 4.0))]           # map frame -> world: 5 deg steps, whole cells


@pytest.fixture(scope="module")
def scene():
    """Three maps of the yard, each a window carried by its pose: [(xyz, normals)], and the world sample."""
    xyz, nrm = yard()
    maps = []
    for (x0, x1, y0, y1), P in zip(WINDOWS, POSES):
        sel = (xyz[:, 0] >= x0) & (xyz[:, 0] <= x1) & (xyz[:, 1] >= y0) & (xyz[:, 1] <= y1)
        maps.append(carried(xyz[sel], nrm[sel], P))
    return maps


def truth(s, t):
    return np.linalg.inv(POSES[t]) @ POSES[s]


def records(xyz):
    out = np.zeros(len(xyz), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")])
    out["x"], out["y"], out["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out["rgba"] = 0xff808080
    return out


def normal_records(nrm):
    out = np.zeros(len(nrm), dtype=[("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("curvature", "<f4")])
    out["nx"], out["ny"], out["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    return out


def _upload(c, m):
    return c.cloud(records(m[0])), c.normals(normal_records(m[1]))


SMALL = dict(cell=CELL, cell_factor=2, yaw_steps=72, yaw_factor=2, candidates=8)
# The recovery tests' options.  A wall is one cell thick and the target's map is dilated by one cell, so a yaw error moves a
# cell out of it only once it displaces the cell by 0.5 .. 1 m: at the yard's 12 m that is 2.5 .. 5 deg.  Finer yaw steps than
# that tie over several steps, and the rule sends ties to the lowest g; 5 deg steps are what +- 1 step can be asked of here.
RECOVER = dict(cell=CELL, cell_factor=4, yaw_steps=72, yaw_factor=2, candidates=32)


# ---------------------------------------------------------------- 1. signature
def test_signature_cell_by_cell(mm, scene):
    c = mm.Context(0)
    for m in scene[:2]:
        assert 25000 <= len(m[0]) <= 40000
        ref = restate_signature(m[0], m[1], CELL, 2)
        got = c.correlativeSignature(*_upload(c, m), method=CORRELATIVE, **SMALL)
        assert len(ref["structure"]) > 50 and len(ref["ground"]) > 1000
        for k in ("structure", "ground", "coarse"):
            assert np.array_equal(got[k], ref[k]), k
        # both sides take a double mean and round once; only the double summation order differs
        ulp = np.spacing(np.abs(ref["ground_height"]))
        assert (np.abs(got["ground_height"].astype(np.float64) - ref["ground_height"].astype(np.float64)) <= ulp).all()
    c.close()


def test_signature_when_blocks_of_the_range_launch_count_nothing(mm):
    """4 100 rows make the cell-range launch three blocks.  Every row below 4 096 is not counted -- the point is not a number
    in the even rows, the normal in the odd ones -- so the four counted rows fall to one block and the other two count nothing;
    then no row is counted, no block counts anything, the range words keep their initial values and the signature has no cell."""
    rng = np.random.default_rng(9)
    xyz = rng.uniform(-40, 40, (4100, 3)).astype(F32)
    nrm = np.tile(np.array([[1, 0, 0], [0, 0, 1]], dtype=F32), (2050, 1))
    xyz[np.arange(0, 4096, 2), np.arange(2048) % 3] = np.nan
    nrm[np.arange(1, 4096, 2), np.arange(2048) % 3] = np.array([np.nan, np.inf] * 1024, dtype=F32)
    xyz[4096:] = [[1.6, -0.7, 0.0], [1.1, -0.8, 0.25], [1.9, -0.6, 1.0], [1.2, -0.9, 0.75]]      # walls in cell (3, -2), ground in (2, -2)
    c = mm.Context(0)
    opt = dict(method=CORRELATIVE, cell=0.5, cell_factor=2, min_points=2)
    ref = restate_signature(xyz, nrm, 0.5, 2, min_points=2)
    got = c.correlativeSignature(c.cloud(records(xyz)), c.normals(normal_records(nrm)), **opt)
    assert ref["structure"].tolist() == [[3, -2, 2]] and ref["ground"].tolist() == [[2, -2, 2]] and ref["coarse"].tolist() == [[1, -1]]
    for k in ("structure", "ground", "coarse"):
        assert np.array_equal(got[k], ref[k]), k
    assert got["ground_height"].tolist() == ref["ground_height"].tolist() == [0.5]
    nrm[4096:, 2] = np.nan
    got = c.correlativeSignature(c.cloud(records(xyz)), c.normals(normal_records(nrm)), **opt)
    assert all(len(v) == 0 for v in got.values())
    c.close()


def test_literal_signature_and_votes(mm):
    c = mm.Context(0)
    got = c.correlativeSignature(c.cloud(records(TEN_POINTS)), c.normals(normal_records(TEN_NORMALS)), method=CORRELATIVE, cell=0.5,
                                 cell_factor=2, min_points=2)
    assert got["structure"].tolist() == TEN_STRUCTURE and got["ground"].tolist() == TEN_GROUND and got["coarse"].tolist() == TEN_COARSE
    assert got["ground_height"].tolist() == [float(F32(0.5 * (float(F32(0.5)) + float(F32(0.7)))))]
    c.close()


# ---------------------------------------------------------------- 2. votes, candidates, fine scores, winner
def test_search_integer_by_integer(mm, scene):
    c = mm.Context(0)
    (s, t) = scene[1], scene[0]
    S, T = restate_signature(*s, CELL, 2), restate_signature(*t, CELL, 2)
    ref = restate_align(S, T, CELL, 2, 2, 72, 8)
    su, tu = _upload(c, s), _upload(c, t)
    u0, v0 = ref["frame"]
    for q in range(36):
        got = c.correlativeVotes(*su, *tu, q, method=CORRELATIVE, **SMALL)
        Q, gu0, gv0, U, V = got["frame"]
        assert Q == 36
        full = np.zeros((U, V), dtype=np.int64)
        a = ref["acc"][q]
        full[u0 - gu0:u0 - gu0 + a.shape[0], v0 - gv0:v0 - gv0 + a.shape[1]] = a          # (the device's box holds the tight one)
        assert np.array_equal(got["acc"], full), q
    assert np.array_equal(got["cands"], ref["cands"])
    assert np.array_equal(got["scores"], ref["scores"])
    Tg, st = c.estimateTransformCorrelative(*su, *tu, method=CORRELATIVE, **SMALL)
    assert st == ref["stats"]
    assert np.allclose(Tg, ref["T"], rtol=0, atol=1e-5)            # (the plane's double sums may differ in order)
    assert np.array_equal(Tg[:2, :2], ref["T"][:2, :2]) or ref["plane"][:2] != (0.0, 0.0)
    c.close()


# ---------------------------------------------------------------- 3. recovery
def _planted_pair(T_true, window=(-9.0, 9.0, -12.0, 12.0)):
    """Target: the yard in the world frame; source: a window of it carried so that source -> target is T_true."""
    xyz, nrm = yard()
    x0, x1, y0, y1 = window
    sel = (xyz[:, 0] >= x0) & (xyz[:, 0] <= x1) & (xyz[:, 1] >= y0) & (xyz[:, 1] <= y1)
    return carried(xyz[sel], nrm[sel], T_true), (xyz.astype(F32), nrm.astype(F32))


def _check_lattice(stats_yaw, T, yaw_deg, shift, yaw_steps):
    step = 360.0 / yaw_steps
    k_true = round(yaw_deg / step) % yaw_steps
    assert min((stats_yaw - k_true) % yaw_steps, (k_true - stats_yaw) % yaw_steps) <= 1, (stats_yaw, k_true)
    assert abs(T[0, 3] - shift[0]) <= CELL + 1e-6 and abs(T[1, 3] - shift[1]) <= CELL + 1e-6, (T[:2, 3], shift)


# The plane's tolerance.  The restatement's own error on the tilted scene (its fitted alpha, beta, gamma against the planted
# tan(tilt) and height) is measured once on the CPU by test_coarse_cpu.py, which asserts it stays below PLANE_ERROR; the
# device is allowed twice that.  The error is not rounding: a 0.5 m cell's mean height is taken at the cell's centre although
# its points lie anywhere in it, a yaw one step off shears the pairing, and box edges mix top and ground.
# Measured there: |alpha - planted| 4.05e-5, |beta - planted| 3.81e-4, |gamma - planted| 5.13e-3 (1754 ground pairs).
PLANE_ERROR = (4.1e-5, 3.9e-4, 5.2e-3)
TILTED = dict(yaw_deg=40.0, shift=(2.0, -3.0), tilt_x_deg=3.0 * math.sin(math.radians(30.0)), tilt_y_deg=-3.0 * math.cos(math.radians(30.0)),
              height=0.4)                   # a 3 deg tilt about an axis 30 deg off x, to first order


def planted_plane(tilt_x_deg=0.0, tilt_y_deg=0.0, height=0.0, **_):
    """pose() has the form of the estimate's composition with Rx's angle atan beta and Ry's -atan alpha: what the fit should find."""
    return -math.tan(math.radians(tilt_y_deg)), math.tan(math.radians(tilt_x_deg)), height


@pytest.mark.parametrize("yaw_deg,shift", [(35.0, (3.0, -2.0)), (-110.0, (-1.5, 4.0)), (180.0, (0.5, 0.5))])
def test_recovers_a_lattice_pose(mm, yaw_deg, shift):
    src, tgt = _planted_pair(pose(yaw_deg, shift))
    c = mm.Context(0)
    T, st = c.estimateTransformCorrelative(*_upload(c, src), *_upload(c, tgt), method=CORRELATIVE, **RECOVER)
    print(st, T[:3, 3])
    assert st["converged"] == 1
    _check_lattice(st["yaw_index"], T, yaw_deg, shift, 72)
    assert abs(T[2, 3]) < 0.02 and abs(T[2, 0]) < 2e-3 and abs(T[2, 1]) < 2e-3       # no tilt, no height planted
    c.close()


def test_recovers_tilt_and_height(mm):
    T_true = pose(**TILTED)
    src, tgt = _planted_pair(T_true)
    c = mm.Context(0)
    T, st = c.estimateTransformCorrelative(*_upload(c, src), *_upload(c, tgt), method=CORRELATIVE, **RECOVER)
    cs, sn = yaw_table(72)
    got, want = plane_of(T, cs[st["yaw_index"]], sn[st["yaw_index"]]), planted_plane(**TILTED)
    print(st, got, want)
    assert st["converged"] == 1 and st["ground_pairs"] >= 1000
    _check_lattice(st["yaw_index"], T, TILTED["yaw_deg"], TILTED["shift"], 72)
    for g, w, e in zip(got, want, PLANE_ERROR):
        assert abs(g - w) <= 2.0 * e, (got, want)
    c.close()


# ---------------------------------------------------------------- 4. end to end
def _params(mm, method=SAC_IA, **kw):
    return mm.MapMergingParams(descriptor_type=2, estimation_method=method, **kw)


def _ctx(mm, streams=1, cache=0, method_first=True, coarse=CORRELATIVE, **kw):
    c = mm.Context(0)
    c.setKeypoints(source=1)                              # uniform keypoints: grey maps are live
    if method_first:
        c.setCoarseAlignment(method=coarse, **kw)
    c.setStreams(streams)
    if not method_first:
        c.setCoarseAlignment(method=coarse, **kw)
    if cache:
        c.setMapCache(cache)
    return c


def _run(c, clouds, p, seed=1):
    c.srand(seed)
    T, pairs = c.estimateMapsTransforms(clouds, p, return_pairs=True)
    return np.stack(T), pairs


def _same(a, b):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1].view(np.uint8), b[1].view(np.uint8))


@pytest.fixture(scope="module")
def clouds(scene):
    return [records(m[0]) for m in scene]


@pytest.fixture(scope="module")
def baseline(mm, clouds):
    c = _ctx(mm, 1)
    out = _run(c, clouds, _params(mm))
    return out, c.lastCoarseStats()


def test_end_to_end_three_maps(mm, clouds, baseline):
    (_, pairs), stats = baseline
    assert len(pairs) == 3
    for r in pairs:
        s, t = int(r["source_idx"]), int(r["target_idx"])
        err = np.linalg.norm(r["transform"].reshape(4, 4).T.astype(np.float64) - truth(s, t))
        print(s, t, "Frobenius", err, "iterations", int(r["icp_iterations"]), "confidence", float(r["confidence"]))
        assert err <= 1.0, (s, t, err)
        assert int(r["n_correspondences"]) == 0 and int(r["n_inliers"]) == 0
    assert stats["converged"] == 1 and stats["score"] > 0


# ---------------------------------------------------------------- 5. invariance
def test_drivers_cache_and_stage_agree_bit_for_bit(mm, clouds, scene, baseline):
    one = baseline[0]
    p = _params(mm)
    _same(one, _run(_ctx(mm, 8), clouds, p))
    _same(one, _run(_ctx(mm, 8, method_first=False), clouds, p))      # set after mm3d_set_streams: the helpers follow
    _same(one, _run(_ctx(mm, 1, cell=DEFAULT_MULTIPLE * p.resolution), clouds, p))
    _same(one, _run(_ctx(mm, 1), clouds, _params(mm, MATCHING)))      # whatever estimation_method says
    cached = _ctx(mm, 8, cache=16)
    _same(one, _run(cached, clouds, p))
    _same(one, _run(cached, clouds, p))                               # served from the cache
    assert cached.mapCacheStats(reset=True)["pairs_reused"] == 3
    # mm3d_pair_estimate against the whole call, the generator untouched, and the stage call against the pair's front
    c = _ctx(mm, 1)
    c.srand(7)
    maps = [c.mapFeatures(c.cloud(x), p) for x in clouds]
    fronts = _run(_ctx(mm, 1), clouds, _params(mm, refine_transform=0))[1]
    c.srand(7)
    for r, f in zip(one[1], fronts):
        s, t = int(r["source_idx"]), int(r["target_idx"])
        assert c.pairEstimate(maps[s], maps[t], p, execute=False)["confidence"] == 0.0
        got = c.pairEstimate(maps[s], maps[t], p)
        assert np.array_equal(got["transform"].view(np.uint32), r["transform"].view(np.uint32)) and got["confidence"] == r["confidence"]
        nrm_s, nrm_t = (c.computeSurfaceNormals(maps[k].points, p.normal_radius) for k in (s, t))
        T, _ = c.estimateTransformCorrelative(maps[s].points, nrm_s, maps[t].points, nrm_t, method=CORRELATIVE,
                                              cell=DEFAULT_MULTIPLE * p.resolution)
        assert np.array_equal(T.T.reshape(16).view(np.uint32), f["transform"].view(np.uint32))
    # the context's generator stands where it stood: a SAC-IA call with the option off equals a fresh context's, seeded alike
    c.setCoarseAlignment(method=NONE)
    fresh = mm.Context(0)
    fresh.setKeypoints(source=1)
    fresh.srand(7)
    a = fresh.estimateMapsTransforms(clouds[:2], p, return_pairs=True)
    b = c.estimateMapsTransforms(clouds[:2], p, return_pairs=True)
    _same((np.stack(a[0]), a[1]), (np.stack(b[0]), b[1]))


# ---------------------------------------------------------------- 6. edges
def test_flat_ground_gives_the_identity(mm):
    rng = np.random.default_rng(3)
    xy = rng.uniform(-6.0, 6.0, size=(20000, 2))
    flat = np.c_[xy, np.zeros(len(xy))].astype(F32)
    up = np.tile(np.array([0.0, 0.0, 1.0], dtype=F32), (len(flat), 1))
    c = mm.Context(0)
    T, st = c.estimateTransformCorrelative(c.cloud(records(flat)), c.normals(normal_records(up)), c.cloud(records(flat)),
                                           c.normals(normal_records(up)), method=CORRELATIVE, cell=CELL)
    assert np.array_equal(T, np.eye(4, dtype=F32))
    assert st == dict(source_cells=0, target_cells=0, coarse_votes=0, candidates=0, score=0, yaw_index=-1, ground_pairs=0, converged=0)
    c.close()
    # behind the whole-map call the record is still produced
    c = _ctx(mm, 1)
    shifted = flat + np.array([0.3, 0.0, 0.0], dtype=F32)
    _, pairs = _run(c, [records(flat), records(shifted)], _params(mm))
    assert len(pairs) == 1 and np.isfinite(pairs[0]["transform"]).all() and c.lastCoarseStats()["converged"] == 0


def test_empty_nan_and_mismatched_inputs(mm, scene):
    c = mm.Context(0)
    xyz, nrm = scene[0]
    ref = c.correlativeSignature(*_upload(c, (xyz, nrm)), method=CORRELATIVE, **SMALL)
    # NaN points and non-finite normals appended: ignored
    bad_xyz = np.r_[xyz, np.full((3, 3), np.nan, dtype=F32), xyz[:2]]
    bad_nrm = np.r_[nrm, nrm[:3], np.array([[np.inf, 0, 0], [0, 0, np.nan]], dtype=F32)]
    got = c.correlativeSignature(*_upload(c, (bad_xyz, bad_nrm)), method=CORRELATIVE, **SMALL)
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k
    empty = (np.zeros((0, 3), dtype=F32), np.zeros((0, 3), dtype=F32))
    got = c.correlativeSignature(*_upload(c, empty), method=CORRELATIVE, **SMALL)
    assert all(len(v) == 0 for v in got.values())
    T, st = c.estimateTransformCorrelative(*_upload(c, empty), *_upload(c, (xyz, nrm)), method=CORRELATIVE, **SMALL)
    assert np.array_equal(T, np.eye(4, dtype=F32)) and st["converged"] == 0 and st["yaw_index"] == -1
    with pytest.raises(mm.Mm3dError) as e:
        c.estimateTransformCorrelative(c.cloud(records(xyz)), c.normals(normal_records(nrm[:-1])), *_upload(c, (xyz, nrm)),
                                       method=CORRELATIVE, **SMALL)
    assert e.value.status == EINVAL
    c.close()


def test_options_that_change_remake_a_cached_signature(mm, clouds, baseline):
    p = _params(mm)
    c = _ctx(mm, 1, cache=16)
    _same(baseline[0], _run(c, clouds, p))
    wide_ref = _run(_ctx(mm, 1, cell=1.0), clouds, p)
    c.setCoarseAlignment(method=CORRELATIVE, cell=1.0)
    c.mapCacheStats(reset=True)
    _same(wide_ref, _run(c, clouds, p))
    st = c.mapCacheStats(reset=True)
    assert st["map_hits"] == 3 and st["pairs_reused"] == 0
    c.setCoarseAlignment(method=CORRELATIVE)
    _same(baseline[0], _run(c, clouds, p))
    assert c.mapCacheStats(reset=True)["pairs_reused"] == 3


def test_device_lists_and_shards_are_unsupported(mm, clouds):
    d = mm.Context(devices=[0])
    with pytest.raises(mm.Mm3dError) as e:
        d.setCoarseAlignment(method=CORRELATIVE)
    assert e.value.status == EUNSUPPORTED
    d.setCoarseAlignment(method=NONE)
    d.close()
    c = mm.Context(0)
    c.setCoarseAlignment(method=CORRELATIVE)
    with pytest.raises(mm.Mm3dError) as e:
        c.shardBegin(clouds[:2], _params(mm), 0, 1)
    assert e.value.status == EUNSUPPORTED
    c.close()

"""The scene and the numpy restatement of the consistency-graph estimator (mm3d_set_estimator; include/mm3d.h states the rule).
Shared by test_consistency_cpu.py, which runs it alone, and test_gpu_consistency.py, which holds the device to it."""
import numpy as np

DEFAULTS = (0, 0.0, 64, 20)          # mm3d_estimator_options_default: RANSAC, tolerance, seeds, consensus
THRESHOLD = 0.5                      # the inlier threshold of every scene here


def scene(seed, C, frac, noise=0.02, room=(20, 15, 3)):
    r = np.random.default_rng(seed)
    p = (r.uniform(0, 1, (C, 3)) * room).astype(np.float32)
    a, b = np.deg2rad(40), np.deg2rad(3)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    R, t = Rz @ Rx, np.array([3., -2., 0.5])
    q = p.astype(np.float64) @ R.T + t + r.normal(0, noise, (C, 3))
    nin = int(round(frac * C)); inl = np.zeros(C, bool); inl[r.permutation(C)[:nin]] = True
    qo = (r.uniform(0, 1, (C, 3)) * room) @ R.T + t
    q[~inl] = qo[~inl]
    return p, q.astype(np.float32), inl, R, t      # correspondence i is (i, i)


def identity_corr(n, dtype):
    corr = np.zeros(n, dtype=dtype)
    corr["index_query"] = corr["index_match"] = np.arange(n)
    return corr


def points(xyz, dtype):
    """N x 3 floats as POINT records."""
    out = np.zeros(len(xyz), dtype=dtype)
    out["x"], out["y"], out["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return out


# ---------------------------------------------------------------- the rule, step by step
def compatibility(src, tgt, s_idx, t_idx, tau, chunk=256):
    """Step 1: A as a C x C bool matrix.  src / tgt: the keypoints' float coordinates; every operation is one float64 operation
    in the written order (numpy fuses nothing)."""
    s_idx, t_idx = np.asarray(s_idx), np.asarray(t_idx)
    P, Q = np.asarray(src, np.float32)[s_idx].astype(np.float64), np.asarray(tgt, np.float32)[t_idx].astype(np.float64)
    C = len(P)
    t2 = np.float64(tau) * np.float64(tau)
    A = np.zeros((C, C), bool)

    def len2(X, r0, r1):
        d = X[r0:r1, None, :] - X[None, :, :]
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]

    with np.errstate(invalid="ignore", over="ignore"):
        for r0 in range(0, C, chunk):
            r1 = min(C, r0 + chunk)
            da, db = len2(P, r0, r1), len2(Q, r0, r1)
            e = (da + db) - t2
            A[r0:r1] = ((s_idx[r0:r1, None] != s_idx[None, :]) & (t_idx[r0:r1, None] != t_idx[None, :]) & (da > t2) & (db > t2) &
                        (e * e <= 4.0 * (da * db)))
    return A


def bit_rows(A):
    """A as the rule's bit rows: [C][ceil(C / 64)] uint64, bit j of row i in word j / 64, bit j % 64."""
    C = len(A)
    W = (C + 63) // 64
    b = np.zeros((C, W * 8), np.uint8)
    if C:
        packed = np.packbits(A, axis=1, bitorder="little")
        b[:, :packed.shape[1]] = packed
    return b.view("<u8").reshape(C, W)


def seed_list(deg, seeds):
    """Step 3: the correspondences with deg >= 2 by (deg descending, i ascending), the first `seeds`."""
    i = np.flatnonzero(deg >= 2)
    return i[np.lexsort((i, -deg[i]))][:seeds]


def second_order(A, seeds):
    """Step 4's S for every seed at once: row r is S_sj of seed r.  (Counts of at most C <= 32 768 are exact in float32.)"""
    Af = A.astype(np.float32)
    return np.where(A[seeds], np.rint(Af[seeds] @ Af).astype(np.int64), 0)


def consensus_set(A, s, consensus, S=None):
    """Step 4: K_s ascending."""
    if S is None:
        S = np.where(A[s], (A & A[s][None, :]).sum(axis=1), 0)
    j = np.flatnonzero(S >= 1)
    j = j[np.lexsort((j, -S[j]))][:consensus - 1]
    return np.sort(np.append(j, s))


def kabsch(P, Q):
    """The rigid fit of Q ~ R P + t in float64, a 4 x 4."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    pm, qm = P.mean(axis=0), Q.mean(axis=0)
    U, _, Vt = np.linalg.svd((Q - qm).T @ (P - pm))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    T = np.eye(4)
    T[:3, :3] = U @ D @ Vt
    T[:3, 3] = qm - T[:3, :3] @ pm
    return T


def d2_float(T, P, Q):
    """Step 6's squared distances as RANSAC's count forms them: the float transform, every operation in float."""
    T, P, Q = np.asarray(T, np.float32), np.asarray(P, np.float32), np.asarray(Q, np.float32)
    x = [((T[r, 0] * P[:, 0] + T[r, 1] * P[:, 1]) + T[r, 2] * P[:, 2]) + T[r, 3] for r in range(3)]
    d = [x[r] - Q[:, r] for r in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def restate(src, tgt, corr, inlier_threshold, tolerance=0.0, seeds=64, consensus=20):
    """The whole rule.  A dict of A, rows, deg, seeds, consensus (a list of ascending arrays), hypotheses (float32 4 x 4, None
    without one), counts (-1 without a hypothesis), winner (rank, -1: none), inliers (indices into corr) and T (float64 Kabsch
    over the inliers; zeros when the estimate fails)."""
    src, tgt = np.asarray(src, np.float32), np.asarray(tgt, np.float32)
    s_idx, t_idx = np.asarray(corr["index_query"]), np.asarray(corr["index_match"])
    C = len(s_idx)
    out = dict(A=np.zeros((C, C), bool), deg=np.zeros(C, np.int64), seeds=np.zeros(0, np.int64), consensus=[], hypotheses=[], counts=[],
               winner=-1, inliers=np.zeros(0, np.int64), T=np.zeros((4, 4)))
    out["rows"] = bit_rows(out["A"])
    if C < 3:
        return out
    tau = tolerance if tolerance > 0 else inlier_threshold
    A = compatibility(src, tgt, s_idx, t_idx, tau)
    deg = A.sum(axis=1)
    out.update(A=A, rows=bit_rows(A), deg=deg, seeds=seed_list(deg, seeds))
    P, Q = src[s_idx], tgt[t_idx]
    thr2 = np.float64(inlier_threshold) * np.float64(inlier_threshold)
    with np.errstate(invalid="ignore", over="ignore"):
        Sm = second_order(A, out["seeds"])
        for r, s in enumerate(out["seeds"]):
            K = consensus_set(A, s, consensus, Sm[r])
            out["consensus"].append(K)
            if len(K) < 3:
                out["hypotheses"].append(None)
                out["counts"].append(-1)
                continue
            T = kabsch(P[K], Q[K]).astype(np.float32)
            out["hypotheses"].append(T)
            out["counts"].append(int((d2_float(T, P, Q).astype(np.float64) < thr2).sum()))
        counts = np.array(out["counts"], dtype=np.int64)
        if len(counts) == 0 or counts.max() < 0:
            return out
        out["winner"] = int(np.argmax(counts))           # the first maximum
        inl = np.flatnonzero(d2_float(out["hypotheses"][out["winner"]], P, Q).astype(np.float64) < thr2)
    if len(inl) >= 3:
        out["inliers"] = inl
        out["T"] = kabsch(P[inl], Q[inl])
    return out


def meets_the_conditions(found, truth):
    """The issue's two conditions on an inlier set: it holds at least 90 % of the true inliers, and at most 10 % of it is not
    true inliers.  Returns (held, others)."""
    found = np.asarray(found, dtype=np.int64)
    held = int(truth[found].sum())
    others = len(found) - held
    assert held >= 0.9 * truth.sum(), (held, int(truth.sum()))
    assert others <= 0.1 * len(found), (others, len(found))
    return held, others

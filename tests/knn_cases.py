"""Inputs for the descriptor k-NN (csrc/desc_knn.hip) on which its rounding-error certificate is the only thing between the
matrix-core |a|^2 + |b|^2 - 2ab expansion and a wrong row: a non-candidate within rounding error of the k-th distance.  A plain
module: tests/test_knn_cases_cpu.py shows on the CPU that every case holds the ties / near-ties it claims and that the expansion,
emulated in float32, does misrank them; tests/test_gpu_desc_knn_certificates.py runs them on the device, route by route.

Every builder is seeded and returns (A, B, k, adversarial_rows, note): float32 queries and targets, k, the rows of A built to sit
on a tie, and a line for the log.  Row norms are about 10 at every width (components ~ 10 / sqrt(dim)), so squared distances
between unrelated rows are about 200.

T  tie_block       integer rows.  Per adversarial query q: k_in < k targets at q +- e_i (d2 = 1), m targets at q +- e_i +- e_j
                   (d2 = 2, all distinct), background far away, everything shuffled: the k-th neighbour lies in a block of m targets
                   at bit-equal distance, the index decides, and m exceeds the candidates a query can have, so a certified row
                   would be a false certificate.  Width 2: (+-1, 0), (0, +-1) stored m / 4 times each, k_in points at (+-1/2, 0).
S  near_tie_shell  k targets at radius r around q, m decoys at r sqrt(1 + g) in random directions, g = 2^-20 or 2^-14: the gap is
                   below the expansion's error, the exact float32 chain still separates most of them.
M  magnitude       S (g = 2^-20) times 2^s: indices unchanged, distances times 2^(2s) exactly (nothing underflows for s >= -32; at s = +50
                   real squared distances exceed 1e30, the finite distance padding targets once had: they then filled the lists of
                   the last tile's wave, were dropped as no rows, and left lists that hid real targets looking empty).
O  common_offset   S (g = 2^-14) plus 4096 in every column (rounded to float32: what the oracle sees is what the device sees).
E  edge            benign rows at the dispatch's size edges, 20 duplicated targets, 10 zero-distance queries.

`python tests/knn_cases.py --run wide_f32|no_filter` runs T and S on the device in this process, for the two selectors that are
read from the environment once per process, and prints one JSON line (mismatching rows, fallbacks, route mask)."""
import math

import numpy as np

F = np.float32
NA = 80                                       # queries per routed case: 3 tiles of 32, the last one partial
N_ADV = 5
K_DEFAULT = 10
GAPS = (2.0 ** -20, 2.0 ** -14)
SCALES = (-32, 0, 32, 50)                     # -50 is left out: squared differences would go subnormal
OFFSET = 4096.0

# one bit per route, as include/mm3d.h names them (MM3D_KNN_PATH_*)
PATH_SMALL, PATH_LIST, PATH_FILTER, PATH_LIST_WIDE, PATH_WIDE_BF16, PATH_WIDE_F32, PATH_ANY = 1, 2, 4, 8, 16, 32, 64

# route -> (row width, targets, tied targets or decoys per adversarial query, expected route bit).  nb = 1000: 32 target tiles, the
# last one with 24 padding rows, at most two parts (128 candidates per query) on every list path; nb = 4001 >= 2017: the filter,
# whose candidate buffer holds kFilterCap = 512.
ROUTES = {
    "list33": (33, 1000, 140, PATH_LIST),
    "filter33": (33, 4001, 600, PATH_FILTER),
    "list2": (2, 1000, 140, PATH_LIST),
    "filter2": (2, 4001, 600, PATH_FILTER),
    "list125": (125, 1000, 140, PATH_LIST_WIDE),
    "bf250": (250, 1000, 140, PATH_WIDE_BF16),
    "bf352": (352, 1000, 140, PATH_WIDE_BF16),
    "bf1344": (1344, 1000, 140, PATH_WIDE_BF16),
    "bf1980": (1980, 1000, 140, PATH_WIDE_BF16),
}
# descriptor type (mm3d Descriptor) of the widths that have one: those also go through ctx.descriptors + findFeatureCorrespondences
DESCRIPTOR_OF = {125: 0, 250: 1, 33: 2, 2: 3, 1344: 4, 1980: 5}

# (dim, na, nb, k, expected route bit): na * nb on either side of 65 536, two and three target tiles, 63 / 64 target tiles
EDGES = (
    (33, 1, 70000, 10, PATH_FILTER),
    (33, 1024, 64, 1, PATH_LIST),
    (33, 1009, 65, 16, PATH_LIST),
    (33, 255, 257, 5, PATH_SMALL),
    (33, 256, 256, 5, PATH_LIST),
    (33, 31, 2200, 10, PATH_FILTER),
    (33, 33, 2016, 10, PATH_LIST),
    (33, 33, 2017, 10, PATH_FILTER),
    (2, 700, 6000, 10, PATH_FILTER),
    (125, 32, 2048, 16, PATH_LIST_WIDE),
    (250, 64, 1100, 5, PATH_WIDE_BF16),
    (352, 64, 1100, 5, PATH_WIDE_BF16),
    (1344, 64, 1100, 5, PATH_WIDE_BF16),
    (1980, 64, 1100, 5, PATH_WIDE_BF16),
    (33, 7, 3, 5, PATH_SMALL),                # fewer targets than k: -1 / +inf tails
    (1344, 7, 3, 5, PATH_SMALL),
)

# shell radius: 1, where the gap g r^2 stays below the expansion's error (which grows with the chain: 2-wide rows have 4 terms);
# at g = 2^-14 the short rows need a smaller shell for that
SHELL_RADIUS = {(GAPS[1], 33): 0.5, (GAPS[1], 2): 0.125}
SHELL_RADIUS_DEFAULT = 1.0


def _sigma(dim):
    return 10.0 / math.sqrt(dim)


def _adv_positions(na, n_adv, rng):
    """Rows of A that hold the adversarial queries: the first and last row and both sides of a tile edge among them."""
    fixed = [p for p in (0, 31, 32, na - 1) if 0 <= p < na]
    rest = [p for p in rng.permutation(na) if p not in fixed]
    return np.array(sorted(set((fixed + rest)[:n_adv])))


def _place(rng, benign_a, adv_q, targets_adv, background):
    """A with the adversarial queries at their rows; B = adversarial targets and background, shuffled."""
    na = len(benign_a) + len(adv_q)
    pos = _adv_positions(na, len(adv_q), rng)
    A = np.empty((na, benign_a.shape[1]))
    mask = np.zeros(na, bool)
    mask[pos] = True
    A[mask], A[~mask] = adv_q, benign_a
    B = np.concatenate([targets_adv, background])
    B = B[rng.permutation(len(B))]
    return np.ascontiguousarray(A, F), np.ascontiguousarray(B, F), pos


def tie_block(dim, k, nb, m, na=NA, n_adv=N_ADV, seed=1):
    rng = np.random.default_rng([seed, dim, k, nb, m])
    k_in = min(2, k - 1) if dim == 2 else k // 2
    n_bg = nb - n_adv * (k_in + m)
    assert n_bg > 0
    if dim == 2:
        assert m % 4 == 0
        q = np.stack([40.0 * np.arange(n_adv) - 20.0 * (n_adv - 1), np.rint(rng.normal(0, 20, n_adv))], axis=1)
        unit = np.array([[1, 0], [-1, 0], [0, 1], [0, -1]], float)
        half = np.array([[0.5, 0], [-0.5, 0]])
        tg = np.concatenate([np.concatenate([qi + half[:k_in], np.repeat(qi + unit, m // 4, axis=0)]) for qi in q])
        pool = np.rint(rng.uniform(-120, 120, (8 * (n_bg + na), 2)))
        pool = pool[(np.abs(pool[:, None, :] - q[None]).max(axis=2) >= 4).all(axis=1)]     # nothing else near a block
        bg, benign = pool[:n_bg], pool[n_bg:n_bg + na - n_adv]
    else:
        assert m <= 4 * math.comb(dim, 2) and k_in <= 2 * dim
        q = np.rint(rng.normal(0, _sigma(dim), (n_adv, dim)))
        blocks = []
        for qi in q:
            ones = rng.choice(2 * dim, k_in, replace=False)                 # (axis, sign)
            rows = np.repeat(qi[None], k_in + m, axis=0)
            rows[np.arange(k_in), ones // 2] += 1.0 - 2.0 * (ones % 2)
            pairs = rng.choice(4 * math.comb(dim, 2), m, replace=False)     # (i < j, two signs)
            iu, ju = np.triu_indices(dim, 1)
            r = k_in + np.arange(m)
            rows[r, iu[pairs // 4]] += 1.0 - 2.0 * (pairs % 2)
            rows[r, ju[pairs // 4]] += 1.0 - 2.0 * (pairs // 2 % 2)
            blocks.append(rows)
        tg = np.concatenate(blocks)
        bg = np.rint(rng.normal(0, _sigma(dim), (n_bg, dim)))
        benign = np.rint(rng.normal(0, _sigma(dim), (na - n_adv, dim)))
    A, B, pos = _place(rng, benign, q, tg, bg)
    return A, B, k, pos, f"T dim={dim} k={k} nb={nb} m={m} k_in={k_in}"


def near_tie_shell(dim, nb, m, g, k=K_DEFAULT, na=NA, n_adv=N_ADV, seed=2):
    rng = np.random.default_rng([seed, dim, k, nb, m, int(round(-math.log2(g)))])
    r = SHELL_RADIUS.get((g, dim), SHELL_RADIUS_DEFAULT)
    n_bg = nb - n_adv * (k + m)
    assert n_bg > 0
    q = rng.normal(0, _sigma(dim), (n_adv, dim))
    if dim == 2:                                           # a plane of radius 10 is crowded: keep the queries apart
        q = 10.0 * np.stack([np.cos(2 * np.pi * np.arange(n_adv) / n_adv), np.sin(2 * np.pi * np.arange(n_adv) / n_adv)], axis=1)

    def directions(n):
        u = rng.normal(0, 1, (n, dim))
        return u / np.linalg.norm(u, axis=1, keepdims=True)

    tg = np.concatenate([np.concatenate([qi + r * directions(k), qi + r * math.sqrt(1.0 + g) * directions(m)]) for qi in q])
    pool = rng.normal(0, _sigma(dim), (4 * (n_bg + na), dim))
    pool = pool[(np.linalg.norm(pool[:, None, :] - q[None], axis=2) >= 4 * r).all(axis=1)]     # (only ever bites at width 2)
    bg = pool[:n_bg]
    benign = pool[n_bg:n_bg + na - n_adv] + rng.normal(0, 0.03 * _sigma(dim), (na - n_adv, dim))
    A, B, pos = _place(rng, benign, q, tg, bg)
    return A, B, k, pos, f"S dim={dim} k={k} nb={nb} m={m} g=2^{int(round(math.log2(g)))} r={r}"


def magnitude(dim, nb, m, s, g=GAPS[0], **kw):           # (radius 1 at every width: squared distances of 2^(2s))
    A, B, k, pos, note = near_tie_shell(dim, nb, m, g, **kw)
    return A * F(2.0 ** s), B * F(2.0 ** s), k, pos, f"M s={s:+d} of {note}"


def common_offset(dim, nb, m, g=GAPS[1], **kw):
    A, B, k, pos, note = near_tie_shell(dim, nb, m, g, **kw)
    return (A + F(OFFSET)).astype(F), (B + F(OFFSET)).astype(F), k, pos, f"O +{OFFSET:g} of {note}"


def edge(dim, na, nb, k, seed=3):
    rng = np.random.default_rng([seed, dim, na, nb, k])
    protos = np.abs(rng.normal(0, _sigma(dim), (64, dim)))
    A = (protos[rng.integers(0, 64, na)] + rng.normal(0, 0.03 * _sigma(dim), (na, dim))).astype(F)
    B = (protos[rng.integers(0, 64, nb)] + rng.normal(0, 0.03 * _sigma(dim), (nb, dim))).astype(F)
    n_dup, n_zero = min(20, nb // 3), min(10, na // 2)
    B[nb - 2 * n_dup:nb - n_dup] = B[:n_dup]                     # duplicated targets: ties go to the lower index
    A[:n_zero] = B[rng.integers(0, nb, n_zero)]                  # zero distances
    return A, B, k, np.arange(n_zero), f"E dim={dim} {na} x {nb} k={k}"


def family_cases(family, route):
    """The cases of one family on one route, as (name, builder thunk) pairs."""
    dim, nb, m, _ = ROUTES[route]
    if family == "T":
        return [(f"T-{route}-k{k}", lambda k=k: tie_block(dim, k, nb, m)) for k in (1, 10, 16)]
    if family == "S":
        return [(f"S-{route}-g{i}", lambda g=g: near_tie_shell(dim, nb, m, g)) for i, g in enumerate(GAPS)]
    if family == "M":
        return [(f"M-{route}-s{s:+d}", lambda s=s: magnitude(dim, nb, m, s)) for s in SCALES]
    if family == "O":
        return [(f"O-{route}", lambda: common_offset(dim, nb, m))]
    raise KeyError(family)


# ---------------------------------------------------------------- the expansion, emulated (CPU)
def emulated_topk(A_rows, B, k):
    """Top-k of the centred |a - mu|^2 + |b - mu|^2 - 2 (a - mu).(b - mu) expansion evaluated as one float32 FMA chain in column
    order (each step: exact product, one rounding of the sum), ties to the lower index: what a selector WITHOUT a certificate
    and without the exact re-rank would answer."""
    A_rows, B = np.asarray(A_rows, F), np.asarray(B, F)
    mu = (B.astype(np.float64).sum(axis=0) / len(B)).astype(F)
    ac, bc = A_rows - mu, B - mu                                      # float32 roundings, as on the device

    def norm2(x):
        acc = np.zeros(len(x), F)
        for d in range(x.shape[1]):
            acc = (acc.astype(np.float64) + x[:, d].astype(np.float64) * x[:, d].astype(np.float64)).astype(F)
        return acc

    na2, nb2 = norm2(ac), norm2(bc)
    m2b = F(-2.0) * bc
    acc = np.zeros((len(ac), len(bc)), F)
    for d in range(ac.shape[1]):
        acc = (acc.astype(np.float64) + ac[:, d, None].astype(np.float64) * m2b[None, :, d].astype(np.float64)).astype(F)
    acc = (acc.astype(np.float64) + na2[:, None].astype(np.float64)).astype(F)
    acc = (acc.astype(np.float64) + nb2[None, :].astype(np.float64)).astype(F)
    order = np.lexsort((np.broadcast_to(np.arange(len(B)), acc.shape), acc), axis=1)
    return order[:, :k]


# ---------------------------------------------------------------- the device side
def bind_debug(L):
    import ctypes as C
    L.mm3d_debug_knn_fallback_rows.restype = L.mm3d_debug_knn_rows.restype = C.c_longlong
    L.mm3d_debug_knn_paths.restype = C.c_uint


def gpu_desc_knn(ctx, L, A, B, k):
    """mm3d_debug_desc_knn with the debug counters on: (idx, d2, fallback rows, route mask)."""
    import ctypes as C
    bind_debug(L)
    idx = np.empty((len(A), k), np.int32)
    d2 = np.empty((len(A), k), F)
    L.mm3d_set_debug(ctx._h, 1)
    try:
        ctx._ck(L.mm3d_debug_desc_knn(ctx._h, A.ctypes.data_as(C.c_void_p), C.c_size_t(len(A)), B.ctypes.data_as(C.c_void_p),
                                      C.c_size_t(len(B)), A.shape[1], k, idx.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p)))
        fb, paths = int(L.mm3d_debug_knn_fallback_rows(ctx._h)), int(L.mm3d_debug_knn_paths(ctx._h))
    finally:
        L.mm3d_set_debug(ctx._h, 0)
    return idx, d2, fb, paths


def mismatching_rows(idx, d2, ref_idx, ref_d2):
    """Rows whose indices or distance WORDS differ from the oracle's (no tolerance)."""
    return np.flatnonzero((idx != ref_idx).any(axis=1) | (d2.view(np.uint32) != ref_d2.view(np.uint32)).any(axis=1))


CHILD_RUNS = {
    # selector switch -> (environment, routes whose shapes it runs, route bit the parent expects)
    "wide_f32": ({"MM3D_KNN_WIDE_BF16": "0"}, ("bf250", "bf1344"), PATH_WIDE_F32),
    "no_filter": ({"MM3D_KNN_NO_FILTER": "1"}, ("filter33", "filter2"), PATH_LIST),
}


def _run_child(which):
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as ge
    env, routes, _ = CHILD_RUNS[which]
    for name, value in env.items():
        assert os.environ.get(name) == value, f"{name}={value} has to be in this process's environment"
    mm, po = ge.load(), ge.load_oracle()
    ctx = mm.Context(0)
    out = {"run": which, "paths": 0, "cases": []}
    for route in routes:
        for family in ("T", "S"):
            for name, make in family_cases(family, route):
                A, B, k, adv, _ = make()
                idx, d2, fb, paths = gpu_desc_knn(ctx, mm.lib(), A, B, k)
                bad = mismatching_rows(idx, d2, *po.desc_knn(A, B, k))
                out["paths"] |= paths
                out["cases"].append({"name": name, "rows": len(A), "adversarial": len(adv), "mismatches": len(bad), "fallbacks": fb})
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", choices=sorted(CHILD_RUNS), required=True)
    _run_child(ap.parse_args().run)

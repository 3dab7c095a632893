"""Doublet detection restated in fp64 NumPy (the spec of include/harmony_mi355x_doublets.h; not a test module).

A synthetic doublet s with parents (a, b), rows of the CSR count matrix of project_ref:
    T_s  = T_a + T_b                      the library sizes over ALL G_all columns (or the caller's totals),
    x_sj = x_aj + x_bj                    for every reference slot j either parent stores -- the counts are added BEFORE the log,
    y    = log1p(x_sj scale / T_s),  w = min(y, mean_j + clip sd_j) / sd_j          (T_s = 0: y = 0),
    P[s,:] = b + sum_j w U[j,:]           b = project_ref.offset: the centring of the genes the query has.
`simulate` evaluates the DENSE form of the definition ((y - mean) / sd on every gene present, zeros included, then the clip, then S @ U), so it
does not rest on the identity the kernel uses; `simulate_sparse` is that identity and `simulate_fp32` its sequential float32 evaluation in
ASCENDING slot order with an fp32 sum x_a + x_b: what honest fp32 gives for the kernel's form.

Error bar (u = 2^-24, n_s the distinct slots either parent stores), derived from the kernel as written, not tuned:
    |P_gpu - P|_sj <= (n_s + 18) u sum_g |w_sg| |U_gj| + 2 u |b_j|
n_s u from the fma chain; 18 = project_ref's 16 (the roundings of x scale / T, log1pf, 1 / sd, the cap, the fp32 U and the final add) plus two
rounding events this kernel adds in front of the log: the second parent's value read as fp32 and the fp32 sum x_a + x_b.  Each is a relative
error of at most u in x, and d log1p(z) / log1p(z) <= dz / z for z >= 0, so each costs at most u in y and in w.

The scores (harmony_amd.doublets) are closed forms of integer neighbour counts; `neighbor_counts` is the brute-force fp64 search of
metrics_ref followed by the count.  `planted` draws the counts of three cell types with 5 % heterotypic doublets and `spec_scores` runs the
whole pipeline on the spec alone: the quality constants of tests/test_gpu_doublets.py are measured from it (tests/test_doublets_cpu.py).
"""
import numpy as np

import metrics_ref as mr
import project_ref as pr

U24 = 2.0 ** -24
BAR_C = 18.0
# AUROC of the spec's doublet score for the planted heterotypic doublets (`planted`: N = 1500, G_all = 600, G = 300, d = 10, r = 2), seeds 0..4,
# as tests/test_doublets_cpu.py::test_quality_constants_from_the_spec_alone measures and pins them
SPEC_AUROC = (0.99818, 0.99849, 0.99821, 0.99855, 0.99979)      # mean 0.99864, min 0.99818, spread 0.00161
SPEC_AUROC_MIN, SPEC_AUROC_SPREAD = min(SPEC_AUROC), max(SPEC_AUROC) - min(SPEC_AUROC)


def _merged(data, indices, indptr, slot, pairs, totals):
    """per synthetic cell: (T_s, sorted slots j, x_sj) in fp64"""
    data = np.asarray(data, dtype=np.float64)
    slot = np.asarray(slot)
    T = pr.row_totals(data, indptr) if totals is None else np.asarray(totals, dtype=np.float64)
    out = []
    for a, b in np.asarray(pairs, dtype=np.int64).reshape(-1, 2):
        acc = {}
        for r in (a, b):
            for e in range(indptr[r], indptr[r + 1]):
                j = int(slot[indices[e]])
                if j >= 0:
                    acc[j] = acc.get(j, 0.0) + data[e]
        js = np.array(sorted(acc), dtype=np.int64)
        out.append((T[a] + T[b], js, np.array([acc[j] for j in js], dtype=np.float64)))
    return out


def simulate(data, indices, indptr, G_all, slot, U, mean, sd, pairs, scale=1e4, clip=None, totals=None):
    """the dense form -> P (n_sim x d) in fp64"""
    X = pr.dense(data, indices, indptr, G_all)
    T = pr.row_totals(data, indptr) if totals is None else np.asarray(totals, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    Xs = X[pairs[:, 0]] + X[pairs[:, 1]]
    Ts = T[pairs[:, 0]] + T[pairs[:, 1]]
    U, mean, sd, slot = np.asarray(U, np.float64), np.asarray(mean, np.float64), np.asarray(sd, np.float64), np.asarray(slot)
    Y = np.zeros_like(Xs)
    pos = Ts > 0
    Y[pos] = np.log1p(Xs[pos] * scale / Ts[pos, None])
    S = np.zeros((Xs.shape[0], U.shape[0]))
    g = np.nonzero(slot >= 0)[0]
    j = slot[g]
    S[:, j] = (Y[:, g] - mean[j]) / sd[j]
    if clip is not None:
        S[:, j] = np.minimum(S[:, j], clip)
    return S @ U


def _weights(T, x, js, mean, sd, scale, clip):
    y = np.log1p(x * scale / T) if T > 0 else np.zeros_like(x)
    cap = mean[js] + clip * sd[js] if clip is not None else np.full(js.shape, np.inf)
    return np.minimum(y, cap) / sd[js]


def simulate_sparse(data, indices, indptr, G_all, slot, U, mean, sd, pairs, scale=1e4, clip=None, totals=None):
    """the sparse identity in fp64"""
    U, mean, sd = np.asarray(U, np.float64), np.asarray(mean, np.float64), np.asarray(sd, np.float64)
    b = pr.offset(slot, U, mean, sd)
    rows = _merged(data, indices, indptr, slot, pairs, totals)
    P = np.tile(b, (len(rows), 1))
    for s, (T, js, x) in enumerate(rows):
        P[s] += _weights(T, x, js, mean, sd, scale, clip) @ U[js]
    return P


def bars(data, indices, indptr, G_all, slot, U, mean, sd, pairs, scale=1e4, clip=None, totals=None):
    """delta (n_sim x d): the error bound of the docstring"""
    U, mean, sd = np.asarray(U, np.float64), np.asarray(mean, np.float64), np.asarray(sd, np.float64)
    b = np.abs(pr.offset(slot, U, mean, sd))
    rows = _merged(data, indices, indptr, slot, pairs, totals)
    out = np.empty((len(rows), U.shape[1]))
    for s, (T, js, x) in enumerate(rows):
        A = np.abs(_weights(T, x, js, mean, sd, scale, clip)) @ np.abs(U[js])
        out[s] = (js.size + BAR_C) * U24 * A + 2.0 * U24 * b
    return out


def simulate_fp32(data, indices, indptr, G_all, slot, U, mean, sd, pairs, scale=1e4, clip=None, totals=None):
    """a sequential float32 NumPy evaluation of the kernel's form (totals and b in fp64): x_a + x_b in fp32, slots ascending"""
    f = np.float32
    data64 = np.asarray(data, dtype=np.float64)
    T = pr.row_totals(data64, indptr) if totals is None else np.asarray(totals, dtype=np.float64)
    U32 = np.asarray(U, np.float64).astype(f)
    mean, sd = np.asarray(mean, np.float64), np.asarray(sd, np.float64)
    inv_sd = (1.0 / sd).astype(f)
    cap = (mean + clip * sd).astype(f) if clip is not None else np.full(sd.shape, np.inf, dtype=f)
    b = pr.offset(slot, U, mean, sd)
    slot = np.asarray(slot)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    P = np.empty((pairs.shape[0], U32.shape[1]), dtype=f)
    for s, (pa, pb) in enumerate(pairs):
        Ts = T[pa] + T[pb]
        r = f(min(scale / Ts, 3.0e38)) if Ts > 0 else f(0)
        tab = {}
        for row in (pa, pb):
            for e in range(indptr[row], indptr[row + 1]):
                j = int(slot[indices[e]])
                if j >= 0:
                    tab[j] = f(tab.get(j, f(0)) + f(data64[e]))
        acc = np.zeros(U32.shape[1], dtype=f)
        for j in sorted(tab):
            if tab[j] > 0:
                y = np.log1p(tab[j] * r, dtype=f)
                w = f(min(y, cap[j]) * inv_sd[j])
                acc = (w * U32[j] + acc).astype(f)
        P[s] = (acc.astype(np.float64) + b).astype(f)
    return P


# ---- the cases of tests/test_gpu_doublets.py, built here so that tests/test_doublets_cpu.py holds honest fp32 to the bar on the same shapes ----
SHAPES = [(1, 1, 1, 1, 1), (17, 70, 40, 3, 5), (300, 900, 300, 50, 601), (120, 500, 500, 128, 64), (90, 400, 257, 68, 7)]      # (N, G_all, G, d, n_sim)
# one G at and one just above each boundary of the plan's tiers (4 | 2 | 1 waves per workgroup), and the largest tables with a partial last sweep
TIER_SHAPES = [(40, G + 300, G, 4, 9) for G in (3840, 3841, 7936, 7937, 16100)]
ROWS = (0, 1, 63, 64, 65, 200)
UNKNOWN_ROW, ZERO_ROW, SAME_A, SAME_B, APART_A, APART_B = 6, 7, 8, 9, 10, 11
# parents of the first synthetic cells wherever the matrix has the rows: every forced row length with its neighbour and with itself, a == b,
# an empty parent, a parent of unknown genes only, stored zeros, parents sharing all of their genes and none
FORCED = [(0, 0), (0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 5), (5, 0), (UNKNOWN_ROW, UNKNOWN_ROW), (UNKNOWN_ROW, 3), (ZERO_ROW, ZERO_ROW),
          (ZERO_ROW, 4), (SAME_A, SAME_B), (APART_A, APART_B), (APART_B, APART_A), (1, 1), (2, 2), (3, 3), (4, 4)]


def case(shape, integer=True, density=None):
    """-> (c: project_ref.random_case's dict with the forced rows, pairs n_sim x 2 int64); read-only arrays"""
    N, G_all, G, d, n_sim = shape
    if density is None:
        density = 0.3 if G > 1000 else 0.1
    seed = sum(shape)
    probe = pr.random_case(N, G_all, G, d, seed=seed, density=density)
    unknown = np.nonzero(probe["slot"] < 0)[0]
    rng = np.random.default_rng(seed + 1)
    if N > APART_B:
        same, apart = min(120, G_all), min(100, G_all // 2)
        lens = ROWS + (min(64, unknown.size), 5, same, same, apart, apart)
    else:
        lens = (1,)
    c = pr.random_case(N, G_all, G, d, seed=seed, row_lengths=lens, integer=integer, density=density)
    assert np.array_equal(c["slot"], probe["slot"])
    pairs = rng.integers(0, N, (n_sim, 2)).astype(np.int64)
    if N > APART_B:
        ip, idx = c["indptr"], c["indices"]
        assert unknown.size > 0 and (c["slot"] >= 0).sum() < G      # genes the reference lacks, reference genes the query lacks
        idx[ip[UNKNOWN_ROW]:ip[UNKNOWN_ROW + 1]] = unknown[:ip[UNKNOWN_ROW + 1] - ip[UNKNOWN_ROW]]
        c["data"][ip[ZERO_ROW]:ip[ZERO_ROW + 1]] = 0.0
        idx[ip[SAME_A]:ip[SAME_A + 1]] = rng.permutation(idx[ip[SAME_B]:ip[SAME_B + 1]])      # the same genes in another order
        two = rng.permutation(G_all)[:2 * apart].astype(np.int32)
        idx[ip[APART_A]:ip[APART_A + 1]], idx[ip[APART_B]:ip[APART_B + 1]] = two[:apart], two[apart:]
        forced = np.array(FORCED[:n_sim], dtype=np.int64)
        pairs[:forced.shape[0]] = forced
    for a in list(c.values()) + [pairs]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c, pairs


def neighbor_counts(X, n_obs, k_adj):
    """every row's synthetic neighbours among its k_adj nearest other rows (rows read as fp32, distances in fp64): (counts int64, idx)"""
    idx, _ = mr.knn(X, k_adj)
    return (idx >= n_obs).sum(axis=1), idx


def auroc(score, positive):
    """the probability that a positive outranks a negative (ties count half)"""
    score, positive = np.asarray(score, dtype=np.float64), np.asarray(positive, dtype=bool)
    order = np.argsort(score, kind="stable")
    ranks = np.empty(score.size)
    s = score[order]
    i = 0
    while i < s.size:                                        # mid-ranks
        j = i
        while j + 1 < s.size and s[j + 1] == s[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    n1, n0 = int(positive.sum()), int((~positive).sum())
    return float((ranks[positive].sum() - n1 * (n1 + 1) / 2.0) / (n1 * n0))


def planted(seed, N=1500, G_all=600, n_types=3, doublet_rate=0.05):
    """Counts of `n_types` cell types with a share `doublet_rate` of heterotypic doublets (the sum of the counts of two cells of different
    types) -> dict(X dense N x G_all float64, is_doublet, types)"""
    rng = np.random.default_rng(1000 + seed)
    base = rng.gamma(0.6, 1.0, G_all) + 0.02
    prof = np.tile(base, (n_types, 1))
    marker = rng.permutation(G_all)[:40 * n_types]
    for t in range(n_types):
        prof[t, marker[40 * t:40 * (t + 1)]] *= 6.0
    prof /= prof.sum(axis=1, keepdims=True)
    types = rng.integers(0, n_types, N)
    X = rng.poisson(prof[types] * rng.uniform(600, 1500, N)[:, None]).astype(np.float64)
    n_dbl = int(round(doublet_rate * N))
    is_doublet = np.zeros(N, dtype=bool)
    cells = rng.permutation(N)[:n_dbl]
    for i in cells:
        other = (types[i] + 1 + rng.integers(0, n_types - 1)) % n_types
        X[i] += rng.poisson(prof[other] * rng.uniform(600, 1500))
        is_doublet[i] = True
    return dict(X=X, is_doublet=is_doublet, types=types)


def fit_tables(X, G, d):
    """the observed cells' own reference tables in fp64 NumPy: the G most variable genes of log1p(CP10k), their mean and sd, the top d
    right singular vectors of the standardised matrix -> (var genes, U G x d, mean, sd)"""
    Y = np.log1p(X * 1e4 / X.sum(axis=1, keepdims=True))
    var = np.sort(np.argsort(-Y.var(axis=0), kind="stable")[:G])
    mean, sd = Y[:, var].mean(axis=0), Y[:, var].std(axis=0, ddof=1)
    S = (Y[:, var] - mean) / sd
    U = np.linalg.svd(S, full_matrices=False)[2][:d].T
    return var, U, mean, sd


def csr_of(X):
    nz = X != 0
    indptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int64)
    return X[nz].astype(np.float64), np.nonzero(nz)[1].astype(np.int32), indptr


def default_k_adj(N, ratio):
    n_neighbors = int(round(0.5 * np.sqrt(N)))
    return int(round(n_neighbors * (1.0 + ratio)))


def spec_scores(p, G=300, d=10, ratio=2.0, seed=0, score_fn=None):
    """the whole pipeline on the spec: tables from the observed cells, fp64 projection of observed and synthetic cells, brute-force kNN,
    `score_fn(counts, k_adj, n_obs, n_sim)` (harmony_amd.doublets.doublet_scores_from_counts) -> (score_obs, score_sim)"""
    X = p["X"]
    N, G_all = X.shape
    var, U, mean, sd = fit_tables(X, G, d)
    slot = np.full(G_all, -1, dtype=np.int32)
    slot[var] = np.arange(G, dtype=np.int32)
    data, indices, indptr = csr_of(X)
    n_sim = int(round(ratio * N))
    pairs = np.random.default_rng(seed).integers(0, N, (n_sim, 2))
    obs = pr.project(data, indices, indptr, G_all, slot, U, mean, sd)
    sim = simulate(data, indices, indptr, G_all, slot, U, mean, sd, pairs)
    k_adj = default_k_adj(N, n_sim / float(N))
    counts, _ = neighbor_counts(np.vstack([obs, sim]), N, k_adj)
    score, _ = score_fn(counts, k_adj, N, n_sim)
    return score[:N], score[N:]

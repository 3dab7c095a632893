"""The reference's PCA from raw counts restated in fp64 NumPy (the spec of include/harmony_mi355x_pca.h and harmony_amd/pca.py; not a test module).

The count matrix, the gene map `slot`, mean, sd, scale, clip and totals are project_ref's (tests/project_ref.py): S is the N x G matrix
    s_ij = min((y_ig - mean_j) / sd_j, clip) for the gene g with slot[g] = j, zeros of the count matrix included; a column no gene maps to is 0,
`dense_S` forms it.  `gene_stats` are the per-gene sums of y and y^2 over all cells.  The operator a fit applies is V -> (P, W), P = S V,
W = S^T P: `apply` on the dense S, `apply_sparse` as the identities the kernels use,
    P[i,:] = b + sum over the stored entries of cell i of w V[j,:],       W[j,:] = sum over the stored entries of gene j of w P[i,:] - (mean_j / sd_j) colsum(P),
and `apply_fp32` their evaluation in float32 in the kernels' documented order (what honest fp32 gives).  `fit` is the subspace iteration of
fit_loadings over any such operator, `exact` the eigen-decomposition of the dense C = S^T S / (N - 1).

Error bars (u = 2^-24; derived, not tuned; DESIGN "Fitting the loadings"):
  P      project_ref.bars with U = V:  (n_i + 16) u sum_j |w_ij| |V_jc| + 2 u |b_c|.
  W      against the spec applied to the SAME fp32 P:  (r_j + 10) u sum_i |w_ij| |P_ic| + (mean_j / sd_j) (N + 2) 2^-53 sum_i |P_ic|.
         r_j = min(n_j, 256): a gene's list is added in fp32 in runs of 256 entries (one rounding per fmaf), the runs in fp64.  10: the weight itself --
         scale / T, x as fp32, x r (3 u in the argument of log1p, whose condition is <= 1), log1pf (2 ulp = 4 u), 1 / sd, the product (or the cap: fewer) --
         is 9 u, one more for the fp64 additions of the runs.  The centring term: N fp64 additions of the column sum, its product and the subtraction.
  s1, s2 u sum_i c_i y_i + n step1, 2 u sum_i c_i y_i^2 + n step2 with c_i = 3 kappa_i + 4: the 3 u in the argument a of log1p reach y through its condition
         kappa = a / ((1 + a) log1p(a)) <= 1 (0.2 - 0.4 at the arguments counts give: with the constant 7 the bar was more than ten times what honest fp32
         does), log1pf's 4 u do not; twice that for the square (formed exactly in fp64); and at most one step per stored entry from the fixed-point
         rounding (half a step in fact).  var: (bar_s2 + 2 |s1| bar_s1 / N) / (N - 1).
  operator  |W_dev - S^T S V| <= bars_W + |S|^T bars_P; eta = its Frobenius norm / (N - 1) at the spec's U.
  fit    sin theta_max(U, E_d) <= bar_sin = sin theta_max(U_spec, E_d) + 2 eta / gap (gap = lambda_d - lambda_(d + 1); the sin 2 theta theorem),
         |explained_variance - lambda| / lambda_1 <= bar_sin^2 + eta / lambda_1.
"""
import numpy as np

import project_ref as pr

U24 = 2.0 ** -24
RUN = 256             # entries of a gene's list added in fp32 before the sums go to fp64
COLSUM_ROWS = 1024    # rows of P added per column before the ranges are added
C_ARG, C_LOG = 3.0, 4.0      # roundings in the argument of log1p (scale / T, x as fp32, their product); log1pf itself, 2 ulp
C_W = C_ARG + C_LOG + 3.0   # ... and 1 / sd, the product with it, the fp64 additions of the runs


def log_normalised(data, indices, indptr, G_all, scale=1e4, totals=None):
    X = pr.dense(data, indices, indptr, G_all)
    T = pr.row_totals(data, indptr) if totals is None else np.asarray(totals, dtype=np.float64)
    Y = np.zeros_like(X)
    pos = T > 0
    Y[pos] = np.log1p(X[pos] * scale / T[pos, None])
    return Y, X


def stat_steps(N, scale, totals_given):
    """the fixed-point steps of hmx_gene_stats (harmony_mi355x_pca.h)"""
    ymax = float(np.float32(89.0 if totals_given else 1.001 * np.log1p(scale)))
    F1 = min(40, int(np.floor(62.0 - np.log2(N * ymax))))
    F2 = min(40, int(np.floor(62.0 - np.log2(N * ymax * ymax))))
    return 2.0 ** -F1, 2.0 ** -F2


def gene_stats(data, indices, indptr, G_all, scale=1e4, totals=None):
    """-> dict(n_cells, s1, s2, mean, var) in fp64 from the dense matrix"""
    Y, X = log_normalised(data, indices, indptr, G_all, scale, totals)
    N = Y.shape[0]
    s1, s2 = Y.sum(axis=0), (Y * Y).sum(axis=0)
    return dict(n_cells=(X > 0).sum(axis=0).astype(np.int64), s1=s1, s2=s2, mean=s1 / N, var=(s2 - s1 * s1 / N) / (N - 1))


def gene_stats_bars(data, indices, indptr, G_all, scale=1e4, totals=None):
    """-> dict(s1, s2, var): the bounds of the docstring around the spec's statistics"""
    data = np.asarray(data, dtype=np.float64)
    N = len(indptr) - 1
    T = pr.row_totals(data, indptr) if totals is None else np.asarray(totals, dtype=np.float64)
    q1, q2 = stat_steps(N, scale, totals is not None)
    rows = np.repeat(np.arange(N), np.diff(indptr))
    a = np.where(T[rows] > 0, data * scale / np.where(T[rows] > 0, T[rows], 1.0), 0.0)
    y = np.log1p(a)
    kappa = np.where(a > 0, a / ((1.0 + a) * np.where(a > 0, y, 1.0)), 0.0)      # the condition of log1p at a: <= 1
    c = (C_ARG * kappa + C_LOG) * U24
    cols = np.asarray(indices, dtype=np.int64)
    b1, b2, s1 = np.zeros(G_all), np.zeros(G_all), np.zeros(G_all)
    np.add.at(b1, cols, c * y)
    np.add.at(b2, cols, 2.0 * c * y * y)
    np.add.at(s1, cols, y)
    n = np.bincount(cols[data > 0], minlength=G_all).astype(np.float64)
    b1, b2 = b1 + n * q1, b2 + n * q2
    return dict(s1=b1, s2=b2, var=(b2 + 2.0 * s1 * b1 / N) / (N - 1))


def gene_stats_fp32(data, indices, indptr, G_all, scale=1e4, totals=None):
    """y in float32 as the kernels form it, y and y^2 rounded to the steps and added exactly: what honest fp32 gives"""
    f = np.float32
    data64 = np.asarray(data, dtype=np.float64)
    N = len(indptr) - 1
    T = pr.row_totals(data64, indptr) if totals is None else np.asarray(totals, dtype=np.float64)
    q1, q2 = stat_steps(N, scale, totals is not None)
    rows = np.repeat(np.arange(N), np.diff(indptr))
    r = np.where(T > 0, scale / np.where(T > 0, T, 1.0), 0.0).astype(f)[rows]
    y = np.log1p(data64.astype(f) * r, dtype=f).astype(np.float64)
    k1, k2 = np.rint(y / q1), np.rint(y * y / q2)
    pos = data64 > 0
    cols = np.asarray(indices, dtype=np.int64)
    s1, s2 = np.zeros(G_all), np.zeros(G_all)
    np.add.at(s1, cols[pos], k1[pos])          # (integers below 2^53: exact)
    np.add.at(s2, cols[pos], k2[pos])
    s1, s2 = s1 * q1, s2 * q2
    return dict(n_cells=np.bincount(cols[pos], minlength=G_all).astype(np.int64), s1=s1, s2=s2, mean=s1 / N, var=(s2 - s1 * s1 / N) / (N - 1))


def dense_S(data, indices, indptr, G_all, slot, mean, sd, scale=1e4, clip=None, totals=None):
    """the definition -> S (N x G) in fp64"""
    Y, _ = log_normalised(data, indices, indptr, G_all, scale, totals)
    mean, sd, slot = np.asarray(mean, np.float64), np.asarray(sd, np.float64), np.asarray(slot)
    S = np.zeros((Y.shape[0], mean.size))
    g = np.nonzero(slot >= 0)[0]
    j = slot[g]
    S[:, j] = (Y[:, g] - mean[j]) / sd[j]
    if clip is not None:
        S[:, j] = np.minimum(S[:, j], clip)
    return S


def apply(S, V, P=None):
    """the dense form: (P = S V, W = S^T P); with P given, W of that P"""
    if P is None:
        P = S @ np.asarray(V, np.float64)
    return P, S.T @ np.asarray(P, np.float64)


def ratios(slot, mean, sd):
    """mean / sd of the columns a gene maps to, 0 elsewhere"""
    slot = np.asarray(slot)
    r = np.zeros(len(mean))
    j = slot[slot >= 0]
    r[j] = np.asarray(mean, np.float64)[j] / np.asarray(sd, np.float64)[j]
    return r


def apply_sparse(data, indices, indptr, G_all, slot, V, mean, sd, scale=1e4, clip=None, totals=None, P=None):
    """the sparse identities in fp64"""
    if P is None:
        P = pr.project_sparse(data, indices, indptr, G_all, slot, V, mean, sd, scale, clip, totals)
    P = np.asarray(P, np.float64)
    rows, j, w, _, _ = pr._weights(data, indices, indptr, slot, mean, sd, scale, clip, totals)
    keep = j >= 0
    W = np.zeros((len(mean), P.shape[1]))
    np.add.at(W, j[keep], w[keep, None] * P[rows[keep]])
    return P, W - ratios(slot, mean, sd)[:, None] * P.sum(axis=0)[None, :]


def colsum_fixed(P):
    """the column sums of P in the library's order: ranges of 1024 rows one after the other, then the ranges one after the other (fp64)"""
    P = np.asarray(P, np.float64)
    total = np.zeros(P.shape[1])
    for r0 in range(0, P.shape[0], COLSUM_ROWS):
        s = np.zeros(P.shape[1])
        for i in range(r0, min(r0 + COLSUM_ROWS, P.shape[0])):
            s = s + P[i]
        total = total + s
    return total


def bars_W(data, indices, indptr, G_all, slot, mean, sd, P, scale=1e4, clip=None, totals=None):
    """(G x k): the bound on W for the given P"""
    Pa = np.abs(np.asarray(P, np.float64))
    rows, j, w, _, _ = pr._weights(data, indices, indptr, slot, mean, sd, scale, clip, totals)
    keep = j >= 0
    G, N = len(mean), Pa.shape[0]
    n = np.bincount(j[keep], minlength=G).astype(np.float64)
    A = np.zeros((G, Pa.shape[1]))
    np.add.at(A, j[keep], np.abs(w[keep, None]) * Pa[rows[keep]])
    return (np.minimum(n, RUN)[:, None] + C_W) * U24 * A + ratios(slot, mean, sd)[:, None] * (N + 2.0) * 2.0 ** -53 * Pa.sum(axis=0)[None, :]


def bars_operator(data, indices, indptr, G_all, slot, V, mean, sd, scale=1e4, clip=None, totals=None):
    """(G x k): |W_device - S^T S V| <= bars_W at the exact P plus the bound on P carried through |S|^T"""
    S = dense_S(data, indices, indptr, G_all, slot, mean, sd, scale, clip, totals)
    bP = pr.bars(data, indices, indptr, G_all, slot, V, mean, sd, scale, clip, totals)
    return bars_W(data, indices, indptr, G_all, slot, mean, sd, S @ np.asarray(V, np.float64), scale, clip, totals) + np.abs(S).T @ bP


def _chains_fp32(group, w, row, table, ngroups, run=None):
    """per group, over its items in the order given: acc = fl32(w table[row] + acc) (one rounding: fmaf), every `run` items (None: never) and at
    the end the float32 sums are added into fp64.  All groups advance together, one item each per step."""
    f = np.float32
    n = np.bincount(group, minlength=ngroups)
    pos = np.arange(group.size) - np.concatenate([[0], np.cumsum(n)])[group]        # (items arrive sorted by group)
    by_pos = np.argsort(pos, kind="stable")
    cut = np.searchsorted(pos[by_pos], np.arange(int(n.max()) + 2 if group.size else 1))
    total, acc = np.zeros((ngroups, table.shape[1])), np.zeros((ngroups, table.shape[1]), dtype=f)
    for t in range(len(cut) - 1):
        e = by_pos[cut[t]:cut[t + 1]]
        g = group[e]
        acc[g] = (w[e, None].astype(np.float64) * table[row[e]].astype(np.float64) + acc[g].astype(np.float64)).astype(f)
        if run is not None and (t + 1) % run == 0:
            total += acc
            acc[:] = 0
    return total + acc


def apply_fp32(data, indices, indptr, G_all, slot, V, mean, sd, scale=1e4, clip=None, totals=None):
    """both products in float32 in the documented order -> (P float32, W float64).  P: per cell over its contributing entries in CSR order, one
    chain, b added in fp64 (project_ref.project_fp32's order with a fused multiply-add); W: per gene over its entries in ascending cell order,
    runs of 256 in float32, the runs and the centring in fp64."""
    f = np.float32
    data64 = np.asarray(data, dtype=np.float64)
    N, G = len(indptr) - 1, len(mean)
    T = pr.row_totals(data64, indptr) if totals is None else np.asarray(totals, dtype=np.float64)
    mean, sd, slot = np.asarray(mean, np.float64), np.asarray(sd, np.float64), np.asarray(slot)
    inv_sd = (1.0 / sd).astype(f)
    cap = (mean + clip * sd).astype(f) if clip is not None else np.full(G, np.inf, dtype=f)
    rows = np.repeat(np.arange(N), np.diff(indptr))
    j = slot[np.asarray(indices, dtype=np.int64)]
    r = np.where(T > 0, scale / np.where(T > 0, T, 1.0), 0.0).astype(f)[rows]
    y = np.log1p(data64.astype(f) * r, dtype=f)
    jj = np.maximum(j, 0)
    w = (np.minimum(y, cap[jj]) * inv_sd[jj]).astype(f)
    keep = np.nonzero(j >= 0)[0]
    V32 = np.asarray(V, np.float64).astype(f)
    P = (_chains_fp32(rows[keep], w[keep], j[keep], V32, N) + pr.offset(slot, V, mean, sd)[None, :]).astype(f)
    by_gene = keep[np.argsort(j[keep], kind="stable")]          # entries by gene, cells ascending within a gene
    W = _chains_fp32(j[by_gene], w[by_gene], rows[by_gene], P, G, run=RUN)
    return P, W - ratios(slot, mean, sd)[:, None] * colsum_fixed(P)[None, :]


def fit(op, G, N, d, oversample=10, n_iter=7, seed=0):
    """fit_loadings' loop over an operator op(V) -> W = S^T S V (fp64 algebra) -> (U G x d, explained variance)"""
    k = min(d + oversample, G)
    V = np.linalg.qr(np.random.default_rng(seed).standard_normal((G, k)))[0]
    for _ in range(n_iter):
        V = np.linalg.qr(op(V))[0]
    T = V.T @ op(V)
    lam, Q = np.linalg.eigh((T + T.T) / 2.0 / (N - 1))
    U = V @ Q[:, np.argsort(-lam)[:d]]
    U = U * np.sign(U[np.abs(U).argmax(axis=0), np.arange(d)])
    return U, np.einsum("ij,ij->j", U, op(U)) / (N - 1)


def exact(S, d):
    """eigh of the dense C -> (E_d: G x d leading eigenvectors, all eigenvalues descending)"""
    lam, E = np.linalg.eigh(S.T @ S / (S.shape[0] - 1))
    o = np.argsort(-lam)
    return E[:, o[:d]], lam[o]


def sin_theta_max(A, B):
    """the sine of the largest principal angle between the column spaces of A and B (same dimension)"""
    Qa, Qb = np.linalg.qr(A)[0], np.linalg.qr(B)[0]
    return float(np.linalg.norm(Qa - Qb @ (Qb.T @ Qa), 2))


def fit_bars(data, indices, indptr, G_all, slot, mean, sd, d, scale=1e4, clip=None, totals=None, oversample=10, n_iter=7, seed=0):
    """-> dict(bar_sin, eta, gap, lam, E, U_spec, ev_spec, sin_spec): the end-to-end bar from spec quantities only"""
    S = dense_S(data, indices, indptr, G_all, slot, mean, sd, scale, clip, totals)
    N, G = S.shape
    E, lam = exact(S, d)
    U, ev = fit(lambda V: S.T @ (S @ V), G, N, d, oversample, n_iter, seed)
    eta = float(np.linalg.norm(bars_operator(data, indices, indptr, G_all, slot, U, mean, sd, scale, clip, totals))) / (N - 1)
    gap = float(lam[d - 1] - lam[d])
    s = sin_theta_max(U, E)
    return dict(bar_sin=s + 2.0 * eta / gap, eta=eta, gap=gap, lam=lam, E=E, U_spec=U, ev_spec=ev, sin_spec=s)


def planted_counts(groups, seed=11, N=1000, G_all=400, Nq=0):
    """tests/test_gpu_project.py's planted construction with `groups` groups: marker genes raised six-fold per group -> (X N x G_all counts, labels);
    with Nq > 0 also a query of Nq cells from the same profiles under a per-gene batch shift: (X, labels, Xq, query labels)"""
    rng = np.random.default_rng(seed)
    base = rng.gamma(0.6, 1.0, G_all) + 0.02
    prof = np.stack([base.copy() for _ in range(groups)])
    marker = rng.permutation(G_all)[:40 * groups]
    for g in range(groups):
        prof[g, marker[40 * g:40 * (g + 1)]] *= 6.0
    prof /= prof.sum(axis=1, keepdims=True)
    lab = rng.integers(0, groups, N)
    X = rng.poisson(prof[lab] * rng.uniform(600, 1500, N)[:, None]).astype(np.float64)
    if not Nq:
        return X, lab
    labq = rng.integers(0, groups, Nq)
    shift = np.exp(rng.normal(0.0, 0.35, G_all))
    Xq = rng.poisson(prof[labq] * shift * rng.uniform(300, 900, Nq)[:, None]).astype(np.float64)
    return X, lab, Xq, labq


def top_variance(var, n_cells, n_top):
    """the n_top genes of largest variance among those at least two cells express, ties by gene order"""
    ok = np.nonzero((np.asarray(n_cells) >= 2) & (np.asarray(var) > 0))[0]
    return ok[np.argsort(-np.asarray(var)[ok], kind="stable")][:n_top]


# ---- the cases of the shape sweep (tests/test_pca_cpu.py holds the bars to honest fp32 on them, tests/test_gpu_pca.py the device) -----------
SHAPES = [(2, 3, 2, 1), (17, 70, 40, 3), (255, 70, 40, 3), (256, 70, 40, 3), (257, 900, 300, 68), (1000, 3000, 2000, 60), (333, 500, 500, 128)]      # (N, G_all, G, k)
ROWS = (0, 1, 63, 64, 65, 200)            # forced stored-entry counts of the first rows
UNKNOWN_ROW, ZERO_ROW, FIRST_FREE = 6, 7, 8
COLUMN_COUNTS = (1, 63, 64, 65, 257)      # chosen genes stored by exactly so many cells, where N allows


def sweep_case(shape, integer=True):
    """A count matrix of the shape with project_ref.random_case's tables and: rows of 0, 1, 63, 64, 65 and 200 entries (capped by the genes there
    are), a row of genes outside the chosen set only, a row of stored zeros, unsorted rows; one chosen gene no cell stores, one that every cell
    with a chosen entry stores (all but the empty row and the row of unchosen genes), chosen genes stored by exactly 1, 63, 64, 65, 257 cells
    where the rows behind the forced ones suffice.  N = 2 carries none of these: two rows, one of them one entry long.
    -> (case dict as random_case's with V for U, special: name -> gene)"""
    N, G_all, G, k = shape
    rng = np.random.default_rng(1000 + sum(shape))
    c = pr.random_case(N, G_all, G, k, seed=sum(shape))
    slot = c["slot"]
    if N <= FIRST_FREE:
        rows = [rng.permutation(G_all)[:n] for n in ([G_all, 1] + [2] * N)[:N]]
        special = {}
    else:
        known, unknown = np.nonzero(slot >= 0)[0], np.nonzero(slot < 0)[0]
        assert unknown.size > 0
        counts = [n for n in COLUMN_COUNTS if n <= N - FIRST_FREE]
        pick = rng.permutation(known)[:2 + len(counts)]
        special = {"none": int(pick[0]), "all": int(pick[1])}
        special.update({n: int(g) for n, g in zip(counts, pick[2:])})
        pool = np.setdiff1d(np.arange(G_all), pick)
        lens = [min(n, pool.size) for n in ROWS] + [min(64, unknown.size), 5]
        lens += [int(min(pool.size, max(1, rng.binomial(G_all, 0.1)))) for _ in range(N - len(lens))]
        rows = [rng.permutation(pool)[:n] for n in lens]
        rows[UNKNOWN_ROW] = rng.permutation(unknown)[:lens[UNKNOWN_ROW]]
        for i in range(N):
            if i in (0, UNKNOWN_ROW):
                continue
            if i < FIRST_FREE:
                rows[i][rng.integers(rows[i].size)] = special["all"]          # (the forced lengths stay)
            else:
                rows[i] = np.insert(rows[i], rng.integers(rows[i].size + 1), special["all"])
        for n in counts:
            for i in FIRST_FREE + rng.permutation(N - FIRST_FREE)[:n]:
                rows[i] = np.insert(rows[i], rng.integers(rows[i].size + 1), special[n])
    indptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    vals = rng.geometric(0.4, size=indices.size).astype(np.float64)
    if not integer:
        vals = vals * rng.uniform(0.25, 1.75, size=vals.size)
    if N > FIRST_FREE:
        vals[indptr[ZERO_ROW]:indptr[ZERO_ROW + 1]] = 0.0
    out = dict(data=vals, indices=indices, indptr=indptr, G_all=G_all, slot=slot, U=c["U"], mean=c["mean"], sd=c["sd"])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out, special

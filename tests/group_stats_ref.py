"""Gene statistics per group restated in fp64 NumPy (the spec of include/harmony_mi355x_groups.h and harmony_amd/group_stats.py; not a test module).

Builds on tests/pca_ref.py: y = log1p(x scale / T) is `log_normalised`'s, the fixed-point steps are `stat_steps`' for the WHOLE N.  `codes` holds
every cell's group in [0, B) or -1 (in no group).  `group_stats` are the dense per-group sums; `group_stats_fp32` their evaluation in the
kernel's arithmetic (y in float32, y and y^2 rounded to the steps, added exactly): what honest fp32 gives.

Error bars (u = 2^-24; derived, not tuned; DESIGN "Gene statistics per group"): pca_ref's with the sums restricted to the group,
  s1   u sum_(i in b) c_i y_i + n_bg step1,      s2   2 u sum_(i in b) c_i y_i^2 + n_bg step2,      c_i = 3 kappa_i + 4,
  var  (bar_s2 + 2 |s1| bar_s1 / n_obs) / (n_obs - 1)   (NaN where the group has fewer than two cells, like var itself).
The selection rules (`select`) and the marker formulas (`markers`) are written directly from their definitions on the dense Y.
"""
import numpy as np

import pca_ref as pc
import project_ref as pr

U24 = pc.U24


def _var(n_obs, s1, s2):
    n = np.asarray(n_obs, dtype=np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n >= 1, s1 / n, np.nan), np.where(n >= 2, (s2 - s1 * s1 / n) / (n - 1), np.nan)


def group_stats(data, indices, indptr, G_all, codes, B, scale=1e4, totals=None):
    """-> dict(n_obs, n_cells, s1, s2, mean, var) in fp64 from the dense matrix"""
    Y, X = pc.log_normalised(data, indices, indptr, G_all, scale, totals)
    codes = np.asarray(codes)
    n_obs = np.array([(codes == b).sum() for b in range(B)], dtype=np.int64)
    s1 = np.stack([Y[codes == b].sum(axis=0) for b in range(B)])
    s2 = np.stack([(Y[codes == b] ** 2).sum(axis=0) for b in range(B)])
    n = np.stack([(X[codes == b] > 0).sum(axis=0) for b in range(B)]).astype(np.int64)
    mean, var = _var(n_obs, s1, s2)
    return dict(n_obs=n_obs, n_cells=n, s1=s1, s2=s2, mean=mean, var=var)


def _entries(data, indptr, scale, totals):
    """per stored entry: its row, the argument a of log1p and y = log1p(a), in fp64"""
    data = np.asarray(data, dtype=np.float64)
    N = len(indptr) - 1
    T = pr.row_totals(data, indptr) if totals is None else np.asarray(totals, dtype=np.float64)
    rows = np.repeat(np.arange(N), np.diff(indptr))
    a = np.where(T[rows] > 0, data * scale / np.where(T[rows] > 0, T[rows], 1.0), 0.0)
    return data, T, rows, a, np.log1p(a)


def group_bars(data, indices, indptr, G_all, codes, B, scale=1e4, totals=None):
    """-> dict(s1, s2, var) [B, G_all]: the bounds of the docstring around the spec's statistics"""
    data, T, rows, a, y = _entries(data, indptr, scale, totals)
    N = len(indptr) - 1
    codes = np.asarray(codes)
    q1, q2 = pc.stat_steps(N, scale, totals is not None)
    kappa = np.where(a > 0, a / ((1.0 + a) * np.where(a > 0, y, 1.0)), 0.0)
    c = (pc.C_ARG * kappa + pc.C_LOG) * U24
    cols, grp = np.asarray(indices, dtype=np.int64), codes[rows]
    keep = grp >= 0
    at = (grp[keep], cols[keep])
    b1, b2, s1, n = (np.zeros((B, G_all)) for _ in range(4))
    np.add.at(b1, at, (c * y)[keep])
    np.add.at(b2, at, (2.0 * c * y * y)[keep])
    np.add.at(s1, at, y[keep])
    np.add.at(n, (grp[keep & (data > 0)], cols[keep & (data > 0)]), 1.0)
    b1, b2 = b1 + n * q1, b2 + n * q2
    n_obs = np.array([(codes == b).sum() for b in range(B)], dtype=np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        var = np.where(n_obs >= 2, (b2 + 2.0 * s1 * b1 / n_obs) / (n_obs - 1), np.nan)
    return dict(s1=b1, s2=b2, var=var)


def group_stats_fp32(data, indices, indptr, G_all, codes, B, scale=1e4, totals=None):
    """y in float32 as the kernel forms it, y and y^2 rounded to the steps of the whole N and added exactly, per group"""
    f = np.float32
    data64 = np.asarray(data, dtype=np.float64)
    N = len(indptr) - 1
    codes = np.asarray(codes)
    T = pr.row_totals(data64, indptr) if totals is None else np.asarray(totals, dtype=np.float64)
    q1, q2 = pc.stat_steps(N, scale, totals is not None)
    ymax = f(89.0 if totals is not None else 1.001 * np.log1p(scale))
    rows = np.repeat(np.arange(N), np.diff(indptr))
    r = np.where(T > 0, scale / np.where(T > 0, T, 1.0), 0.0).astype(f)[rows]
    y = np.minimum(np.log1p(data64.astype(f) * r, dtype=f), ymax).astype(np.float64)
    k1, k2 = np.rint(y / q1), np.rint(y * y / q2)
    cols, grp = np.asarray(indices, dtype=np.int64), codes[rows]
    pos = (data64 > 0) & (grp >= 0)
    at = (grp[pos], cols[pos])
    s1, s2, n = (np.zeros((B, G_all)) for _ in range(3))
    np.add.at(s1, at, k1[pos])          # (integers below 2^53: exact)
    np.add.at(s2, at, k2[pos])
    np.add.at(n, at, 1.0)
    s1, s2 = s1 * q1, s2 * q2
    n_obs = np.array([(codes == b).sum() for b in range(B)], dtype=np.int64)
    mean, var = _var(n_obs, s1, s2)
    return dict(n_obs=n_obs, n_cells=n.astype(np.int64), s1=s1, s2=s2, mean=mean, var=var)


def select(var, n_cells, n_obs, n_top, flavor, min_cells=2):
    """the two selection rules, gene by gene.  Within a group of >= 2 cells a gene qualifies with n_cells >= min_cells and var > 0; its rank is the
    number of qualifying genes that come before it (larger variance, or equal variance and smaller index)."""
    var, n_cells = np.asarray(var, dtype=np.float64), np.asarray(n_cells)
    B, G = var.shape
    rank = [[None] * G for _ in range(B)]
    for b in range(B):
        if n_obs[b] < 2:
            continue
        q = [g for g in range(G) if n_cells[b, g] >= min_cells and var[b, g] > 0]
        for g in q:
            rank[b][g] = sum(1 for h in q if var[b, h] > var[b, g] or (var[b, h] == var[b, g] and h < g))
    hits = [sum(1 for b in range(B) if rank[b][g] is not None and rank[b][g] < n_top) for g in range(G)]
    if flavor == "union":
        return np.array([g for g in range(G) if hits[g] > 0], dtype=np.int64)
    cand = [g for g in range(G) if any(rank[b][g] is not None for b in range(B))]
    med = {g: float(np.median([rank[b][g] for b in range(B) if rank[b][g] is not None])) for g in cand}
    return np.array(sorted(cand, key=lambda g: (-hits[g], med[g], g))[:n_top], dtype=np.int64)


def markers(Y, X, codes, B, reference="rest"):
    """Welch's t-test per (group, gene) from the dense log-normalised Y and counts X; reference: "rest" (the other cells with a code >= 0) or a
    group index.  -> dict(mean_in, mean_out, pct_in, pct_out, logfoldchange, score, df, order)"""
    codes = np.asarray(codes)
    G = Y.shape[1]
    out = {k: np.full((B, G), np.nan) for k in ("mean_in", "mean_out", "pct_in", "pct_out", "logfoldchange", "score", "df")}
    for b in range(B):
        inn = codes == b
        oth = ((codes >= 0) & ~inn) if reference == "rest" else (codes == reference)
        n1, n2 = int(inn.sum()), int(oth.sum())
        for g in range(G):
            y1, y2 = Y[inn, g], Y[oth, g]
            m1 = y1.sum() / n1 if n1 else np.nan
            m2 = y2.sum() / n2 if n2 else np.nan
            out["mean_in"][b, g], out["mean_out"][b, g] = m1, m2
            out["pct_in"][b, g] = (X[inn, g] > 0).sum() / n1 if n1 else np.nan
            out["pct_out"][b, g] = (X[oth, g] > 0).sum() / n2 if n2 else np.nan
            if n1 and n2:
                out["logfoldchange"][b, g] = np.log2((np.expm1(m1) + 1e-9) / (np.expm1(m2) + 1e-9))
            if n1 < 2 or n2 < 2:
                continue
            v1, v2 = ((y1 - m1) ** 2).sum() / (n1 - 1), ((y2 - m2) ** 2).sum() / (n2 - 1)
            e1, e2 = v1 / n1, v2 / n2
            if e1 + e2 > 0:
                out["score"][b, g] = (m1 - m2) / np.sqrt(e1 + e2)
                out["df"][b, g] = (e1 + e2) ** 2 / (e1 * e1 / (n1 - 1) + e2 * e2 / (n2 - 1))
            else:
                out["score"][b, g] = 0.0 if m1 == m2 else np.sign(m1 - m2) * np.inf
    out["order"] = np.argsort(-out["score"], axis=1, kind="stable")
    return out


# ---- the cases of the shape sweep (tests/test_group_stats_cpu.py holds the bars to honest fp32 on them, tests/test_gpu_group_stats.py the device) ----
CHUNK = 256           # GROUP_CHUNK of hmx_internal.h: cells of one group per chunk of the work list
STAT_GENES = 7680     # PCA_STAT_GENES: genes per LDS table, one gene range of grid.y
EDGE_GENES = (STAT_GENES - 1, STAT_GENES, 7699)
CASES = ("one_each", "empty_level", "mod5", "chunk-1", "chunk", "chunk+1", "16_17", "two_ranges")


def _with_entries(c, rows, genes, seed):
    """the case with an entry at every gene of `genes` in every row of `rows` (appended where the row does not store the gene)"""
    rng = np.random.default_rng(seed)
    ip, new_rows, new_vals = c["indptr"], [], []
    for i in range(len(ip) - 1):
        idx, val = c["indices"][ip[i]:ip[i + 1]], c["data"][ip[i]:ip[i + 1]]
        if i in rows:
            add = np.array([g for g in genes if g not in set(idx.tolist())], dtype=np.int32)
            idx, val = np.concatenate([idx, add]), np.concatenate([val, rng.geometric(0.4, size=add.size).astype(np.float64)])
        new_rows.append(idx)
        new_vals.append(val)
    out = dict(c)
    out["indptr"] = np.concatenate([[0], np.cumsum([r.size for r in new_rows])]).astype(np.int64)
    out["indices"], out["data"] = np.concatenate(new_rows).astype(np.int32), np.concatenate(new_vals)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def group_case(name, integer=True):
    """-> (case dict of pca_ref.sweep_case with its forced rows, codes [N], B): the smallest shapes that reach each path of the grouped kernel.
    one_each (2, 3, 2): one cell per group.  empty_level (17, 70, 3): no cell carries level 1.  mod5 (257, 900, 5): labels i mod 5.
    chunk-1 / chunk / chunk+1: one group of CHUNK - 1, CHUNK, CHUNK + 1 cells and a second group of one cell.  16_17: groups of exactly 16 and 17
    cells (one and two cells per wave).  two_ranges (40, 7700, 3): entries at genes 7679, 7680 and 7699, on both sides of the LDS tables' range."""
    if name == "one_each":
        shape, codes, B = (2, 3, 2, 1), np.array([0, 1]), 2
    elif name == "empty_level":
        shape, codes, B = (17, 70, 40, 3), 2 * (np.arange(17) % 2), 3
    elif name == "mod5":
        shape, codes, B = (257, 900, 300, 68), np.arange(257) % 5, 5
    elif name in ("chunk-1", "chunk", "chunk+1"):
        n = CHUNK + {"chunk-1": -1, "chunk": 0, "chunk+1": 1}[name]
        shape, codes, B = (n + 1, 900, 300, 68), np.zeros(n + 1, dtype=np.int64), 2
        codes[10] = 1
    elif name == "16_17":
        shape, B = (33, 70, 40, 3), 2
        codes = np.random.default_rng(3).permutation(np.repeat([0, 1], [16, 17]))
    elif name == "two_ranges":
        shape, codes, B = (40, 7700, 40, 3), np.arange(40) % 3, 3
    else:
        raise KeyError(name)
    c = pc.sweep_case(shape, integer)[0]
    if name == "two_ranges":
        c = _with_entries(c, (8, 9, 10, 11), EDGE_GENES, seed=7)
    return c, codes.astype(np.int32), B


# ---- the planted cases of the end-to-end tests ------------------------------------------------------------------------------------------------------
def csr_of(X):
    """dense counts -> (data, indices, indptr, G_all)"""
    nz = X != 0
    indptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int64)
    return X[nz], np.nonzero(nz)[1].astype(np.int32), indptr, X.shape[1]


def shifted_batches(seed=11, n_shift=40, keep=0.08):
    """pca_ref.planted_counts (four cell types, N = 1000, G_all = 400) in two batches: in batch 1 the counts of the n_shift most abundant genes
    that mark no cell type are thinned to `keep` of what they were (a per-gene batch shift).  Pooled, those genes vary most -- between the
    batches; within a batch they vary like any other gene.  -> (X, batch, the shifted genes)"""
    X, lab = pc.planted_counts(4, seed=seed)
    rng = np.random.default_rng(seed + 1)
    batch = rng.integers(0, 2, X.shape[0])
    st = X.mean(axis=0)
    by_type = np.stack([X[lab == t].mean(axis=0) for t in range(4)])
    flat = np.nonzero(by_type.max(axis=0) < 2.0 * by_type.min(axis=0) + 1e-9)[0]      # (a marker is raised six-fold in one type)
    shifted = np.sort(flat[np.argsort(-st[flat], kind="stable")][:n_shift])
    X = X.copy()
    rows = np.nonzero(batch == 1)[0]
    X[np.ix_(rows, shifted)] = rng.binomial(X[np.ix_(rows, shifted)].astype(np.int64), keep)
    return X, batch.astype(np.int32), shifted


def rank_gaps(var, bar, n_cells, n_obs, min_cells=2):
    """per group of >= 2 cells, over its qualifying genes in rank order: the smallest of (gap between neighbours in variance) / (sum of their two
    bars) -- above 1 everywhere (and so above twice the bar at the cut, whatever n_top_genes), the ranks are the same for any variances within the bars"""
    worst = []
    for b in range(var.shape[0]):
        if n_obs[b] < 2:
            continue
        ok = np.nonzero((n_cells[b] >= min_cells) & (var[b] > 0))[0]
        o = ok[np.argsort(-var[b, ok], kind="stable")]
        worst.append(float(((var[b, o[:-1]] - var[b, o[1:]]) / (bar[b, o[:-1]] + bar[b, o[1:]])).min()))
    return worst


def private_genes(seed=11):
    """pca_ref.planted_counts with four groups and one private gene each: only the group's cells store it -> (X, labels, the four genes)"""
    X, lab = pc.planted_counts(4, seed=seed)
    rng = np.random.default_rng(seed + 2)
    genes = np.sort(rng.permutation(X.shape[1])[:4])
    X = X.copy()
    for b, g in enumerate(genes):
        X[:, g] = np.where(lab == b, rng.poisson(30.0, X.shape[0]) + 1, 0)
    return X, lab.astype(np.int32), genes

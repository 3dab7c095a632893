"""gene_stats_by_group(), variable_genes() and rank_genes_groups(): the gene statistics of a count matrix per group of cells.

`gene_stats` treats a reference as one pool of cells.  On several batches the pooled variance is led by the genes that differ between the
batches, so Symphony's buildReference ranks the genes within each batch and takes the union (vargenes_groups), and scanpy's
highly_variable_genes(batch_key=...) ranks them by the number of batches they are variable in: `variable_genes` gives either choice as indices
for fit_loadings(genes_use=genes[idx]).  After knn_predict or a clustering the same sums per label answer which genes mark a label:
`rank_genes_groups` is Welch's t-test on the log-normalised expression, scanpy's default.  Both rest on one primitive, per (group, gene) the
number of expressing cells and the sums of y and y^2, y = log1p(x scale / T): hmx_gene_stats_grouped (include/harmony_mi355x_groups.h), whose
fixed-point sums partition hmx_gene_stats' exactly.  Everything after the sums is fp64 NumPy here: `select_variable_genes` and
`markers_from_sums` are pure functions of the sums.  The Wilcoxon rank-sum test needs ranks, not sums: rank_genes_groups(method="wilcoxon") takes
them from rank_sums.py (hmx_rank_sums).  Seurat's vst, scanpy's binned dispersion and p-values are not implemented (the caller has `score` and `df`).
"""
import ctypes as C

import numpy as np

from .pca import _matrix, _with_handle, choose_genes, gene_stats

MAX_GROUPS = 4096
MAX_CELLS = 1 << 25      # groups x genes
_dp = C.POINTER(C.c_double)
_lp = C.POINTER(C.c_int64)


def _codes(groups, levels, what):
    """-> (int32 code of every cell: the position of its label in `levels`, -1 where it is not among them; the levels)"""
    groups = np.asarray(groups)
    if groups.ndim != 1:
        raise ValueError("%s: groups must be a 1-D array of labels, one per cell" % what)
    if levels is None:
        levels = np.unique(groups)
    else:
        levels = np.asarray(levels).reshape(-1)
        if groups.dtype.kind in "OUS" or levels.dtype.kind in "OUS":
            groups, levels = groups.astype(str), levels.astype(str)
        if len(set(levels.tolist())) != levels.size:
            raise ValueError("%s: levels must be distinct" % what)
    if levels.size < 1:
        raise ValueError("%s: no levels" % what)
    if levels.size > MAX_GROUPS:
        raise ValueError("%s: at most %d groups are supported" % (what, MAX_GROUPS))
    by = np.argsort(levels, kind="stable")
    pos = np.minimum(np.searchsorted(levels[by], groups), levels.size - 1)
    codes = np.where(levels[by][pos] == groups, by[pos], -1)
    return np.ascontiguousarray(codes, dtype=np.int32), levels


def gene_stats_by_group(counts, genes, groups, levels=None, scale=1e4, totals=None, device=None, _handle=None):
    """gene_stats within every group of cells.  counts, genes, scale, totals: as for gene_stats; groups: one label per cell; levels: the labels
    that form the B groups, in the order of the rows returned (default: np.unique(groups)); a cell whose label is not among them is left out.
    -> dict(levels, n_obs [B], n_cells [B, G], s1, s2, mean, var [B, G], step): n_obs the cells of a group, n_cells those that store a positive
    count of the gene, s1 = sum y, s2 = sum y^2 over the group as the library returns them (fixed-point sums of the steps `step`, the same bits
    for any residence, slab size and order of the cells; summed over the groups of a partition they are gene_stats' s1, s2 bit for bit while
    s / step stays below 2^53), mean = s1 / n_obs, var = (s2 - s1^2 / n_obs) / (n_obs - 1); NaN where a group has no (mean) or one cell."""
    what = "gene_stats_by_group"
    genes = np.asarray(genes).astype(str).reshape(-1)
    G_all = int(genes.size)
    if G_all < 1:
        raise ValueError("%s: no genes" % what)
    if not (scale > 0) or not np.isfinite(scale):
        raise ValueError("%s: scale must be positive" % what)
    codes, levels = _codes(groups, levels, what)
    B = int(levels.size)
    ptrs, f32, loc, N, totals, keep = _matrix(counts, G_all, totals, what)
    if codes.size != N:
        raise ValueError("%s: groups must hold one label per cell (%d), got %d" % (what, N, codes.size))
    if B * G_all > MAX_CELLS:
        raise ValueError("%s: groups x genes must not exceed 2^25 (%d x %d)" % (what, B, G_all))
    n_obs = np.zeros(B, dtype=np.int64)
    n = np.zeros((B, G_all), dtype=np.int64)
    s1, s2, step = np.zeros((B, G_all)), np.zeros((B, G_all)), np.zeros(2)

    def run(h):
        st = h.lib.hmx_gene_stats_grouped(h.h, N, G_all, ptrs[0], ptrs[1], ptrs[2], f32, loc, float(scale),
                                          None if totals is None else totals.ctypes.data_as(_dp), codes.ctypes.data_as(C.POINTER(C.c_int32)), B,
                                          n_obs.ctypes.data_as(_lp), n.ctypes.data_as(_lp), s1.ctypes.data_as(_dp), s2.ctypes.data_as(_dp),
                                          step.ctypes.data_as(_dp))
        h.check(st, what)

    _with_handle(run, device, _handle)
    del keep
    mean, var = _moments(n_obs, s1, s2)
    return dict(levels=levels, n_obs=n_obs, n_cells=n, s1=s1, s2=s2, mean=mean, var=var, step=step)


def _moments(n_obs, s1, s2):
    """mean and variance (n - 1 in the denominator) from the sums of n_obs values; NaN where there are none / fewer than two"""
    n = np.asarray(n_obs, dtype=np.float64).reshape(-1, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(n >= 1, s1 / n, np.nan)
        var = np.where(n >= 2, (s2 - s1 * s1 / n) / (n - 1), np.nan)
    return mean, var


def select_variable_genes(var, n_cells, n_obs, n_top_genes=2000, flavor="union", min_cells=2):
    """The choice of variable_genes from per-group statistics ([B, G], [B, G], [B]) -> indices of genes.  Within every group of at least two
    cells the genes that at least min_cells of its cells express and whose variance is positive are ranked by descending variance, ties by
    gene order.  "union": the genes among the first n_top_genes of any group, in gene order.  "rank": at most n_top_genes genes, by the number
    of groups in whose first n_top_genes they fall (descending), then by the median of their ranks over the groups in which they qualify
    (ascending), then by gene order."""
    if flavor not in ("union", "rank"):
        raise ValueError("variable_genes: flavor must be 'union' or 'rank'")
    var, n_cells, n_obs = np.atleast_2d(np.asarray(var, dtype=np.float64)), np.atleast_2d(np.asarray(n_cells)), np.asarray(n_obs).reshape(-1)
    n_top, G = int(n_top_genes), var.shape[1]
    hits, ranks = np.zeros(G, dtype=np.int64), np.full(var.shape, np.nan)
    for b in range(var.shape[0]):
        if n_obs[b] < 2:
            continue
        ok = np.nonzero((n_cells[b] >= min_cells) & (var[b] > 0))[0]
        order = ok[np.argsort(-var[b, ok], kind="stable")]
        ranks[b, order] = np.arange(order.size)
        hits[order[:n_top]] += 1
    if flavor == "union":
        return np.nonzero(hits > 0)[0]
    some = np.nonzero(~np.all(np.isnan(ranks), axis=0))[0]
    median = np.nanmedian(ranks[:, some], axis=0) if some.size else np.zeros(0)
    return some[np.lexsort((some, median, -hits[some]))][:n_top]


def variable_genes(counts, genes, groups=None, n_top_genes=2000, flavor="union", min_cells=2, scale=1e4, totals=None, device=None, _handle=None):
    """The variable genes of a reference of several batches, as indices into `genes` for fit_loadings(genes_use=genes[idx]).  groups: the batch of
    every cell; the genes are ranked by the variance of the log-normalised expression WITHIN each batch (select_variable_genes): flavor "union"
    is Symphony's vargenes_groups (the union of every batch's n_top_genes, in gene order), "rank" scanpy's batch_key rule (exactly n_top_genes,
    or as many as qualify).  groups=None: the pooled choice of fit_loadings (choose_genes on gene_stats, in descending variance)."""
    if flavor not in ("union", "rank"):
        raise ValueError("variable_genes: flavor must be 'union' or 'rank'")
    if int(n_top_genes) < 1:
        raise ValueError("variable_genes: n_top_genes must be positive")
    if groups is None:
        gs = gene_stats(counts, genes, scale=scale, totals=totals, device=device, _handle=_handle)
        return choose_genes(gs["var"], gs["n_cells"], n_top_genes)
    gs = gene_stats_by_group(counts, genes, groups, scale=scale, totals=totals, device=device, _handle=_handle)
    return select_variable_genes(gs["var"], gs["n_cells"], gs["n_obs"], n_top_genes, flavor, min_cells)


def _others(x, reference, step=None):
    """per group the sum over "the rest" (all groups - the group) or the reference group's row.  With `step` the subtraction is checked to be
    exact: x / step are integers, exact in fp64 while the total stays below 2^53; above it the integers themselves are subtracted (int64)."""
    if reference != "rest":
        return np.broadcast_to(x[int(reference)], x.shape).copy()
    if step is not None and x.dtype.kind == "f":
        k = x / step
        if k.size and k.sum(axis=0).max() >= 2.0 ** 53:
            k = k.astype(np.int64)      # (the library's sums are multiples of the step below 2^62: the conversion is exact)
            return (k.sum(axis=0, keepdims=True) - k).astype(np.float64) * step
    return x.sum(axis=0, keepdims=True) - x


def markers_from_sums(n_obs, n_cells, s1, s2, reference="rest", step=None):
    """Welch's t-test of every group against "rest" (all other cells of the groups given) or against the group in row `reference` (an index),
    from the per-group sums of gene_stats_by_group: n_obs [B], n_cells, s1, s2 [B, G]; step: gene_stats_by_group's, which lets the rest sums be
    formed exactly.  -> dict of [B, G] arrays: mean_in, mean_out; pct_in, pct_out (the share of cells that store a positive count);
    logfoldchange = log2((expm1(mean_in) + 1e-9) / (expm1(mean_out) + 1e-9)); score = (m1 - m2) / sqrt(v1 / n1 + v2 / n2); df
    (Welch-Satterthwaite); order: the genes by descending score, ties by gene order (NaN last).  A zero denominator gives score 0 where the
    means are equal and +-inf otherwise (df is then NaN); a side of fewer than two cells gives NaN score and df."""
    n_obs = np.asarray(n_obs, dtype=np.int64).reshape(-1)
    n_cells, s1, s2 = np.atleast_2d(np.asarray(n_cells, dtype=np.int64)), np.atleast_2d(np.asarray(s1, np.float64)), np.atleast_2d(np.asarray(s2, np.float64))
    B = n_obs.size
    if not (n_cells.shape == s1.shape == s2.shape) or s1.shape[0] != B:
        raise ValueError("markers_from_sums: n_obs [B] and n_cells, s1, s2 [B, G] do not agree")
    if not (isinstance(reference, str) and reference == "rest"):
        if isinstance(reference, (str, bytes)) or int(reference) != reference or not 0 <= int(reference) < B:
            raise ValueError("markers_from_sums: reference must be 'rest' or the row of a group")
    st = (None, None) if step is None else (float(step[0]), float(step[1]))
    n1 = n_obs.astype(np.float64).reshape(-1, 1)
    n2 = _others(n_obs.reshape(-1, 1), reference).astype(np.float64)
    c2, a2, b2 = _others(n_cells, reference), _others(s1, reference, st[0]), _others(s2, reference, st[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        m1, m2 = np.where(n1 >= 1, s1 / n1, np.nan), np.where(n2 >= 1, a2 / n2, np.nan)
        v1 = np.maximum((s2 - s1 * s1 / n1) / (n1 - 1), 0.0)
        v2 = np.maximum((b2 - a2 * a2 / n2) / (n2 - 1), 0.0)
        e1, e2 = v1 / n1, v2 / n2
        den = np.sqrt(e1 + e2)
        score = np.where(den > 0, (m1 - m2) / den, np.where(m1 == m2, 0.0, np.sign(m1 - m2) * np.inf))
        df = (e1 + e2) ** 2 / (e1 * e1 / (n1 - 1) + e2 * e2 / (n2 - 1))
        few = (n1 < 2) | (n2 < 2)
        score, df = np.where(few, np.nan, score), np.where(few | ~(den > 0), np.nan, df)
        lfc = np.log2((np.expm1(m1) + 1e-9) / (np.expm1(m2) + 1e-9))
        pct_in, pct_out = np.where(n1 >= 1, n_cells / n1, np.nan), np.where(n2 >= 1, c2 / n2, np.nan)
    order = np.argsort(-score, axis=1, kind="stable")
    return dict(mean_in=m1, mean_out=m2, pct_in=pct_in, pct_out=pct_out, logfoldchange=lfc, score=score, df=df, order=order)


def rank_genes_groups(counts, genes, groups, levels=None, reference="rest", scale=1e4, totals=None, device=None, _handle=None, method="t-test"):
    """The genes that mark each group: Welch's t-test on the log-normalised expression (scanpy's default rank_genes_groups) of every level
    against all other cells of the levels (reference="rest") or against one level.  groups, levels: as for gene_stats_by_group (cells of no level
    are left out of "rest" too).  -> markers_from_sums' dict with `levels` and `n_obs`: order[b, 0] is the gene that marks level b most.
    method="wilcoxon": the Wilcoxon rank-sum test instead (Seurat's and presto's default): `score`, `order` and the new `auc`, `u` come from the
    exact rank sums (rank_sums.wilcoxon_from_rank_sums; the integers `n_pos`, `rank2`, `tie3` are returned with them, `df` is not), while mean_*,
    pct_* and logfoldchange still come from gene_stats_by_group on the same handle.  Cost: one count sweep and one sweep per gene block on top of
    the t-test's single sweep; with reference=<level> the two groups' cells alone are ranked, ONE library call per other level (B - 1 calls,
    each of them sweeping the whole matrix), so prefer "rest" for many levels."""
    what = "rank_genes_groups"
    if method not in ("t-test", "wilcoxon"):
        raise ValueError("%s: method must be 't-test' or 'wilcoxon'" % what)
    codes, lv = _codes(groups, levels, what)
    ref = "rest"
    if not (isinstance(reference, str) and reference == "rest"):
        at = np.nonzero(lv == (str(reference) if lv.dtype.kind in "US" else reference))[0]
        if at.size != 1:
            raise ValueError("%s: reference must be 'rest' or one of the levels, got %r" % (what, reference))
        ref = int(at[0])
    if method == "wilcoxon":
        from .rank_sums import one_handle, wilcoxon_markers
        _handle, owner = one_handle(device, _handle)
    try:
        gs = gene_stats_by_group(counts, genes, groups, levels=levels, scale=scale, totals=totals, device=device, _handle=_handle)
        out = markers_from_sums(gs["n_obs"], gs["n_cells"], gs["s1"], gs["s2"], reference=ref, step=gs["step"])
        out["levels"], out["n_obs"] = gs["levels"], gs["n_obs"]
        if method == "wilcoxon":
            del out["df"]
            out.update(wilcoxon_markers(counts, genes, groups, levels, ref, scale, totals, device, _handle))
    finally:
        if method == "wilcoxon" and owner is not None:
            owner.__exit__()
    return out

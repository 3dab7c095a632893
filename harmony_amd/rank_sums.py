"""rank_sums_by_group() and wilcoxon_from_rank_sums(): the Wilcoxon rank-sum (Mann-Whitney) marker test per group of cells.

Seurat's FindMarkers and presto default to this test and scanpy recommends it.  Sums per (group, gene) cannot give ranks: the library sorts every
gene's positive entries across the kept cells (hmx_rank_sums, include/harmony_mi355x_ranksum.h) and returns integers -- per (group, gene) the
doubled midrank sum and the number of positive entries, per gene the sum of t^3 over the tie blocks -- which are exact: the same bits for any
residence of the matrix, slab size, gene-block budget and order of the cells.  What is ranked is the argument of the log-normalised expression,
key = fl32(fl32(x) fl32(scale / T)); log1p is monotone, so the ranks are those of log1p(key) wherever two keys differ.  Everything after the
integers is fp64 NumPy here: `wilcoxon_from_rank_sums` is a pure function of them (U, AUC and the normal-approximation score with presto's and
Seurat's tie correction; no continuity correction; p-values are the caller's: 2 * norm.sf(|score|)).  `group_stats.rank_genes_groups(method=
"wilcoxon")` puts the two together.  PRECONDITION: a row of the count matrix stores a gene at most once.
"""
import ctypes as C

import numpy as np

from ._call import _Handle
from .group_stats import MAX_CELLS, _codes
from .pca import _matrix, _with_handle

MAX_KEPT = 1 << 30
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)
_up = C.POINTER(C.c_uint64)


def _gene_slot(genes, genes_use, what):
    """-> (int32 output row of every gene or -1, or None for all genes; the names of the output rows)"""
    if genes_use is None:
        return None, genes
    use = np.asarray(genes_use).astype(str).reshape(-1)
    if use.size < 1:
        raise ValueError("%s: genes_use selects no gene" % what)
    if len(set(use.tolist())) != use.size:
        raise ValueError("%s: genes_use must be distinct" % what)
    by = np.argsort(genes, kind="stable")
    pos = np.minimum(np.searchsorted(genes[by], use), genes.size - 1)
    if np.any(genes[by][pos] != use):
        raise ValueError("%s: genes_use names a gene that is not among genes: %r" % (what, use[genes[by][pos] != use][0]))
    if len(set(by[pos].tolist())) != use.size:
        raise ValueError("%s: genes holds a selected name twice" % what)
    slot = np.full(genes.size, -1, dtype=np.int32)
    slot[by[pos]] = np.arange(use.size, dtype=np.int32)
    return slot, use


def _rank_sums_codes(h, ptrs, f32, loc, N, G_all, scale, totals, codes, B, slot, G, what):
    """one library call: labels as codes in [-1, B) -> (n_obs [B], n_pos [B, G], rank2 [B, G] int64, tie3 [G] Python integers)"""
    n_obs = np.zeros(B, dtype=np.int64)
    n_pos, rank2 = np.zeros((B, G), dtype=np.int64), np.zeros((B, G), dtype=np.int64)
    tie = np.zeros((G, 2), dtype=np.uint64)
    st = h.lib.hmx_rank_sums(h.h, N, G_all, ptrs[0], ptrs[1], ptrs[2], f32, loc, float(scale),
                             None if totals is None else totals.ctypes.data_as(_dp), codes.ctypes.data_as(_ip), B,
                             None if slot is None else slot.ctypes.data_as(_ip), G,
                             n_obs.ctypes.data_as(_lp), n_pos.ctypes.data_as(_lp), rank2.ctypes.data_as(_lp), tie.ctypes.data_as(_up))
    h.check(st, what)
    tie3 = np.empty(G, dtype=object)
    for g in range(G):
        tie3[g] = int(tie[g, 0]) + (int(tie[g, 1]) << 64)
    return n_obs, n_pos, rank2, tie3


def _prepare(counts, genes, groups, levels, genes_use, scale, totals, what):
    genes = np.asarray(genes).astype(str).reshape(-1)
    G_all = int(genes.size)
    if G_all < 1:
        raise ValueError("%s: no genes" % what)
    if not (scale > 0) or not np.isfinite(scale):
        raise ValueError("%s: scale must be positive" % what)
    codes, levels = _codes(groups, levels, what)
    slot, names = _gene_slot(genes, genes_use, what)
    ptrs, f32, loc, N, totals, keep = _matrix(counts, G_all, totals, what)
    if codes.size != N:
        raise ValueError("%s: groups must hold one label per cell (%d), got %d" % (what, N, codes.size))
    if int(levels.size) * int(names.size) > MAX_CELLS:
        raise ValueError("%s: groups x selected genes must not exceed 2^25 (%d x %d)" % (what, levels.size, names.size))
    if int((codes >= 0).sum()) > MAX_KEPT:
        raise ValueError("%s: at most 2^30 cells may carry a level" % what)
    return (ptrs, f32, loc, N, G_all, float(scale), totals), codes, levels, slot, names, keep


def rank_sums_by_group(counts, genes, groups, levels=None, genes_use=None, scale=1e4, totals=None, device=None, _handle=None):
    """The exact rank sums of every group.  counts, genes, scale, totals: as for gene_stats; groups, levels: as for gene_stats_by_group (a cell
    whose label is not among the levels is left out of the ranking); genes_use: the names of the genes to rank, in the order of the columns
    returned (default: all).  -> dict(levels, genes, n_obs [B], n_pos [B, G], rank2 [B, G] int64, tie3 [G] Python integers in an object
    array): n_pos the group's cells with a positive key, rank2 the DOUBLED sum of the group's midranks among all kept cells (zeros included),
    tie3 the sum of t^3 over the tie blocks of the positive keys.  rank2.sum(0) = N_k (N_k + 1).  The same bits for any residence, slab size,
    gene-block budget and order of the cells.  A host-resident matrix is uploaded once and once more per gene block."""
    what = "rank_sums_by_group"
    m, codes, levels, slot, names, keep = _prepare(counts, genes, groups, levels, genes_use, scale, totals, what)
    B, G = int(levels.size), int(names.size)
    out = _with_handle(lambda h: _rank_sums_codes(h, *m, codes, B, slot, G, what), device, _handle)
    del keep
    return dict(levels=levels, genes=names, n_obs=out[0], n_pos=out[1], rank2=out[2], tie3=out[3])


def wilcoxon_from_rank_sums(n_obs, n_pos, rank2, tie3, tie_correct=True):
    """The rank-sum test of every group against all other kept cells, from rank_sums_by_group's integers: n_obs [B], n_pos, rank2 [B, G],
    tie3 [G].  With n1 = n_obs[b], n2 = N_k - n1, R = rank2 / 2:  u = R - n1 (n1 + 1) / 2,  auc = u / (n1 n2),
    score = (u - n1 n2 / 2) / sqrt(n1 n2 / 12 ((N_k + 1) - tie / (N_k (N_k - 1)))),  tie = sum over ALL tie blocks of t^3 - t (the zeros form one
    block: (tie3 - P) + (z^3 - z), exact in Python integers); tie_correct=False drops the tie term (scanpy's default).  No continuity
    correction.  score = 0 where the variance is 0; score and auc NaN where n1 = 0 or n2 = 0.  -> dict(u, auc, score [B, G] fp64, order: the
    genes by descending score, ties by gene order, NaN last)."""
    n_obs = np.asarray(n_obs, dtype=np.int64).reshape(-1)
    n_pos, rank2 = np.atleast_2d(np.asarray(n_pos, dtype=np.int64)), np.atleast_2d(np.asarray(rank2, dtype=np.int64))
    B = n_obs.size
    if n_pos.shape != rank2.shape or n_pos.shape[0] != B:
        raise ValueError("wilcoxon_from_rank_sums: n_obs [B] and n_pos, rank2 [B, G] do not agree")
    G = n_pos.shape[1]
    tie3 = np.asarray(tie3, dtype=object).reshape(-1)
    if tie3.size != G:
        raise ValueError("wilcoxon_from_rank_sums: tie3 must hold one integer per gene")
    Nk = int(n_obs.sum())
    tie = np.zeros(G)
    for g in range(G):
        P = int(n_pos[:, g].sum())
        z = Nk - P
        tie[g] = float((int(tie3[g]) - P) + (z ** 3 - z))
    n1i = n_obs.reshape(-1, 1)
    n1, n2 = n1i.astype(np.float64), (Nk - n1i).astype(np.float64)
    u = (rank2 - n1i * (n1i + 1)).astype(np.float64) / 2.0      # (the subtraction in int64: exact)
    with np.errstate(divide="ignore", invalid="ignore"):
        auc = u / (n1 * n2)
        spread = (Nk + 1.0) - (tie / (float(Nk) * (Nk - 1.0)) if tie_correct and Nk > 1 else 0.0)
        var = n1 * n2 / 12.0 * spread * np.ones((1, G))
        score = np.where(var > 0, (u - n1 * n2 / 2.0) / np.sqrt(np.where(var > 0, var, 1.0)), 0.0)
    none = (n1 == 0) | (n2 == 0)
    score, auc = np.where(none, np.nan, score), np.where(none, np.nan, auc)
    order = np.argsort(-score, axis=1, kind="stable")
    return dict(u=u, auc=auc, score=score, order=order)


def wilcoxon_markers(counts, genes, groups, levels, ref, scale, totals, device, _handle, tie_correct=True):
    """rank_genes_groups(method="wilcoxon") behind its argument checks: ref is "rest" or the row of the reference level.  -> dict(score, auc, u,
    order, n_pos, rank2, tie3); with a reference level row b holds level b ranked against the reference's cells alone (tie3 then is [B, G]), and
    the reference's own row is the test of a group against itself: score 0, auc 0.5."""
    what = "rank_genes_groups"
    m, codes, levels, slot, names, keep = _prepare(counts, genes, groups, levels, None, scale, totals, what)
    B, G = int(levels.size), int(names.size)

    def run(h):
        if ref == "rest":
            n_obs, n_pos, rank2, tie3 = _rank_sums_codes(h, *m, codes, B, None, G, what)
            out = wilcoxon_from_rank_sums(n_obs, n_pos, rank2, tie3, tie_correct)
            out.update(n_pos=n_pos, rank2=rank2, tie3=tie3)
            return out
        # one level against the reference level: the two groups' cells only, one library call per other level
        u, auc, score = np.zeros((B, G)), np.full((B, G), 0.5), np.zeros((B, G))
        n_pos, rank2 = np.zeros((B, G), dtype=np.int64), np.zeros((B, G), dtype=np.int64)
        tie3 = np.empty((B, G), dtype=object)
        tie3[:] = 0
        n_ref = int((codes == ref).sum())
        u[ref] = n_ref * n_ref / 2.0
        for b in range(B):
            if b == ref:
                continue
            pair = np.where(codes == b, 0, np.where(codes == ref, 1, -1)).astype(np.int32)
            o = _rank_sums_codes(h, *m, pair, 2, None, G, what)
            w = wilcoxon_from_rank_sums(*o, tie_correct)
            u[b], auc[b], score[b], n_pos[b], rank2[b], tie3[b] = w["u"][0], w["auc"][0], w["score"][0], o[1][0], o[2][0], o[3]
        return dict(u=u, auc=auc, score=score, order=np.argsort(-score, axis=1, kind="stable"), n_pos=n_pos, rank2=rank2, tie3=tie3)

    out = _with_handle(run, device, _handle)
    del keep
    return out


def one_handle(device, _handle):
    """the caller's handle, or a fresh one to close: -> (handle, owner or None)"""
    if _handle is not None:
        return _handle, None
    h = _Handle(device)
    return h, h

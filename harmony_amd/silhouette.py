"""Silhouette widths on the GPU: per cell, per label, optionally within groups.

The silhouette width of a cell is (b - a) / max(a, b): a the mean distance to the other cells of its label, b the smallest mean distance to
the cells of another label (``sklearn.metrics.silhouette_samples``, Euclidean).  Integration benchmarks report two averages of it (scib):
the ASW over the cell type -- are the types still apart? -- and the ASW over the batch *within each cell type* -- are the batches mixed?
Every pair of cells enters (an N x N distance pass, nothing is sampled); it is computed in libharmony_mi355x.so
(include/harmony_mi355x_silhouette.h); arguments are checked here, before the library is loaded.
"""
import ctypes as C

import numpy as np

from ._call import _factor, _factor_column, _Handle, _rows


def _call(lib, handle, check, X, xdt, N, d, codes, n_levels, gcodes, n_groups, return_ab):
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    s = np.empty(N, dtype=np.float64)
    a, b = (np.empty(N, dtype=np.float64), np.empty(N, dtype=np.float64)) if return_ab else (None, None)
    check(lib.hmx_silhouette(handle, None if X is None else C.c_void_p(X.ctypes.data), xdt, 0, N, d, codes.ctypes.data_as(ip), n_levels,
                             None if gcodes is None else gcodes.ctypes.data_as(ip), n_groups, s.ctypes.data_as(dp),
                             None if a is None else a.ctypes.data_as(dp), None if b is None else b.ctypes.data_as(dp)), "silhouette")
    return (s, a, b) if return_ab else s


def _labels_and_groups(labels, groups, N):
    codes, levels = _factor(labels, N, "labels")
    if groups is None:
        if len(levels) < 2:
            raise ValueError("silhouette widths need at least two labels, got %d" % len(levels))
        return codes, len(levels), None, 1
    gcodes, glevels = _factor(groups, N, "groups")
    return codes, len(levels), gcodes, len(glevels)


def silhouette_samples(X, labels, groups=None, device=None, return_ab=False):
    """The silhouette width of every row of X (cells x PCs, float64 or float32) under `labels` (one per cell), Euclidean, as
    sklearn.metrics.silhouette_samples defines it.  With `groups` (one per cell) only cells of one group see each other: a is the mean
    distance to the other cells of the group with the cell's label, b the smallest mean distance to another label's cells of the group.
    The only cell of its label in its group gets 0; the cells of a group with fewer than two labels get NaN.  Returns s, or (s, a, b) with
    return_ab=True, float64 in the order the cells were given in; two calls give identical results."""
    X, xdt = _rows(X, "X")
    N, d = X.shape
    codes, n_levels, gcodes, n_groups = _labels_and_groups(labels, groups, N)
    with _Handle(device) as h:
        return _call(h.lib, h.h, h.check, X, xdt, N, d, codes, n_levels, gcodes, n_groups, return_ab)


def silhouette_label(X, meta_data, label_col, rescale=True, device=None):
    """scib's label ASW: the mean silhouette width over the column `label_col` of meta_data, as (mean + 1) / 2 in [0, 1] when rescaled
    (1: the labels are apart)."""
    X, xdt = _rows(X, "X")
    N, d = X.shape
    codes, levels = _factor_column(meta_data, label_col, N)
    if len(levels) < 2:
        raise ValueError("silhouette widths need at least two labels, got %d" % len(levels))
    with _Handle(device) as h:
        s = _call(h.lib, h.h, h.check, X, xdt, N, d, codes, len(levels), None, 1, False)
    m = float(np.mean(s))
    return (m + 1.0) / 2.0 if rescale else m


def batch_asw(s, batch_codes, group_codes, group_levels, rescale=True):
    """scib's aggregation of batch silhouette widths computed within the groups of `label_col`: groups with one batch, or with as many
    batches as cells, are skipped; per cell 1 - |s| (rescaled) or |s|, then the mean per group, then the mean of the group means.
    Returns (score, {group level: mean}); the score is NaN when every group is skipped."""
    per = {}
    for g, level in enumerate(group_levels):
        sel = group_codes == g
        n = int(np.count_nonzero(sel))
        nb = len(np.unique(batch_codes[sel]))
        if n == 0 or nb == 1 or nb == n:
            continue
        v = np.abs(s[sel])
        per[level.item() if hasattr(level, "item") else level] = float(np.mean(1.0 - v if rescale else v))
    return (float(np.mean(list(per.values()))) if per else float("nan")), per


def silhouette_batch(X, meta_data, batch_col, label_col, rescale=True, device=None):
    """scib's batch ASW: silhouette widths over `batch_col` within each level of `label_col` (both columns of meta_data), aggregated by
    batch_asw: (score, {level of label_col: mean}); with rescale=True, 1 means the batches are mixed within every label."""
    X, xdt = _rows(X, "X")
    N, d = X.shape
    bcodes, blevels = _factor_column(meta_data, batch_col, N)
    gcodes, glevels = _factor_column(meta_data, label_col, N)
    with _Handle(device) as h:
        s = _call(h.lib, h.h, h.check, X, xdt, N, d, bcodes, len(blevels), gcodes, len(glevels), False)
    return batch_asw(s, bcodes, gcodes, glevels, rescale)


def harmony_silhouette(obj, meta_data, label_col, group_col=None, return_ab=False):
    """Harmony.silhouette: silhouette widths of the handle's current Z_corr (a fitted handle or a mapped query), read where it lives in HBM"""
    N = int(obj._scalar("N_local"))
    codes, levels = _factor_column(meta_data, label_col, N)
    gcodes, n_groups = None, 1
    if group_col is None:
        if len(levels) < 2:
            raise ValueError("silhouette widths need at least two labels, got %d" % len(levels))
    else:
        gcodes, glevels = _factor_column(meta_data, group_col, N)
        n_groups = len(glevels)
    return _call(obj._lib, obj._h, obj._check, None, 0, N, 0, codes, len(levels), gcodes, n_groups, return_ab)

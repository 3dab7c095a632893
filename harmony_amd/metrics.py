"""Scoring an integration on the GPU: exact k nearest neighbours, LISI and kNN label transfer.

LISI, the local inverse Simpson's index, is the metric of the Harmony paper (immunogenomics/LISI, ``compute_lisi``): per cell, the effective
number of labels among its neighbours, weighted by a Gaussian kernel whose width is searched for a fixed perplexity.  iLISI is taken over the
batch variable (higher = better mixed), cLISI over the cell type (1 = types kept apart).  ``knn_predict`` transfers labels from reference
cells to mapped query cells by majority vote, as Symphony's ``knnPredict`` does.  Neighbours and LISI are computed in libharmony_mi355x.so
(include/harmony_mi355x_metrics.h); arguments are checked here, before the library is loaded.
"""
import ctypes as C

import numpy as np

from ._call import MAX_D, _column, _factor, _Handle, _rows

MAX_K = 128


def _label_codes(label_codes, n_levels, N):
    codes = np.asarray(label_codes)
    if codes.ndim == 1:
        codes = codes[None, :]
    if codes.ndim != 2 or codes.shape[1] != N:
        raise ValueError("label codes must be n_columns x %d (one code per labelled cell)" % N)
    if not np.issubdtype(codes.dtype, np.integer):
        if not np.all(np.isfinite(codes)) or np.any(codes != np.floor(codes)):
            raise ValueError("label codes must be integers (NaN labels are not accepted)")
    n_levels = np.atleast_1d(np.asarray(n_levels)).astype(np.int64)
    if n_levels.size != codes.shape[0] or np.any(n_levels < 1):
        raise ValueError("n_levels: one positive level count per label column")
    if np.any(codes < 0) or np.any(codes >= n_levels[:, None]):
        raise ValueError("label code outside [0, n_levels)")
    return np.ascontiguousarray(codes, dtype=np.int32), np.ascontiguousarray(n_levels, dtype=np.int32)


def _factor_columns(meta_data, label_colnames, N):
    """the label columns of meta_data through ui.as_factor: (codes n_cols x N, n_levels, [levels])"""
    if isinstance(label_colnames, str):
        label_colnames = [label_colnames]
    names = list(label_colnames) or [None]              # (no name at all: refused as a name that is no column)
    values = [_column(meta_data, c, missing="label_colnames must name columns of meta_data") for c in names]
    codes, n_levels, levels = [], [], []
    for c, v in zip(names, values):
        cd, lv = _factor(v, N, "column %r" % c, wrong_shape="%(what)s has %(shape)s labels for %(N)d cells")
        codes.append(cd)
        n_levels.append(len(lv))
        levels.append(lv)
    return np.ascontiguousarray(np.stack(codes), dtype=np.int32), np.asarray(n_levels, dtype=np.int32), levels


def lisi_neighbours(perplexity, N):
    """m = 3 perplexity - 1 neighbours with self excluded (nn2(k = 3 perplexity) with the self column dropped, as compute_lisi does)"""
    if not (np.isfinite(perplexity) and perplexity > 0):
        raise ValueError("perplexity must be positive")
    m = int(np.floor(3 * perplexity)) - 1
    if m < 1:
        raise ValueError("perplexity %g leaves no neighbours (3 perplexity - 1 < 1)" % perplexity)
    if m > MAX_K:
        raise ValueError("perplexity %g needs %d neighbours: at most %d are supported" % (perplexity, m, MAX_K))
    if m > N - 1:
        raise ValueError("perplexity %g needs %d neighbours, the data has %d other cells" % (perplexity, m, N - 1))
    return m


def knn(data, k, query=None, device=None):
    """Exact k nearest neighbours (Euclidean) of every row of `query` among the rows of `data`, both cells x PCs (float64 or float32).
    query=None: the rows of `data` themselves with self excluded.  Returns (idx, dist): Nq x k int32 indices into `data` and float32
    distances, sorted ascending by (distance, index); ties go to the smaller index, two calls give identical results."""
    X, xdt = _rows(data, "data")
    N, d = X.shape
    if query is None:
        Q, qdt, Nq = None, 0, N
    else:
        Q, qdt = _rows(query, "query")
        Nq = Q.shape[0]
        if Q.shape[1] != d:
            raise ValueError("query has %d PCs, data %d" % (Q.shape[1], d))
    k = int(k)
    if k < 1 or k > MAX_K:
        raise ValueError("k must be in 1 .. %d" % MAX_K)
    if k > N - (1 if query is None else 0):
        raise ValueError("k = %d exceeds the %d candidate cells" % (k, N - (1 if query is None else 0)))
    idx = np.empty((Nq, k), dtype=np.int32)
    dist = np.empty((Nq, k), dtype=np.float32)
    with _Handle(device) as h:
        h.check(h.lib.hmx_knn(h.h, C.c_void_p(X.ctypes.data), xdt, 0, N, None if Q is None else C.c_void_p(Q.ctypes.data), qdt, 0, Nq,
                              d, k, C.c_void_p(idx.ctypes.data), C.c_void_p(dist.ctypes.data), 0), "knn")
    return idx, dist


def lisi_from_knn(idx, dist, label_codes, n_levels, perplexity, device=None):
    """The second stage alone: LISI of Nq cells from their neighbour lists.  idx, dist: Nq x m (indices into the N labelled cells, Euclidean
    distances); label_codes: n_columns x N (or N,) 0-based codes; n_levels: levels per column.  Returns Nq x n_columns float64; -1 where every
    kernel weight underflows, as the LISI package returns."""
    idx = np.asarray(idx)
    dist = np.asarray(dist)
    if idx.ndim != 2 or idx.shape != dist.shape or idx.shape[0] < 1 or idx.shape[1] < 1:
        raise ValueError("idx and dist must be Nq x m matrices of one shape")
    if idx.shape[1] > MAX_K:
        raise ValueError("at most %d neighbours per cell" % MAX_K)
    if not (np.isfinite(perplexity) and perplexity > 0):
        raise ValueError("perplexity must be positive")
    codes = np.asarray(label_codes)
    N = codes.shape[-1] if codes.ndim else 0
    codes, n_levels = _label_codes(codes, n_levels, N)
    if not np.issubdtype(idx.dtype, np.integer) or np.any(idx < 0) or np.any(idx >= N):
        raise ValueError("neighbour indices must be integers in [0, %d)" % N)
    if np.any(np.isnan(dist)):
        raise ValueError("NaN distances")
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    out = np.empty((idx.shape[0], codes.shape[0]), dtype=np.float64)
    ip, fp, dp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)
    with _Handle(device) as h:
        h.check(h.lib.hmx_lisi(h.h, idx.ctypes.data_as(ip), dist.ctypes.data_as(fp), idx.shape[0], idx.shape[1], codes.ctypes.data_as(ip), N,
                               codes.shape[0], n_levels.ctypes.data_as(ip), float(perplexity), out.ctypes.data_as(dp)), "lisi")
    return out


def _compute_lisi(lib, handle, check, X, xdt, N, d, codes, n_levels, perplexity):
    out = np.empty((N, codes.shape[0]), dtype=np.float64)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    check(lib.hmx_compute_lisi(handle, None if X is None else C.c_void_p(X.ctypes.data), xdt, 0, N, d, codes.ctypes.data_as(ip), codes.shape[0],
                               n_levels.ctypes.data_as(ip), float(perplexity), out.ctypes.data_as(dp)), "compute_lisi")
    return out


def compute_lisi(X, meta_data, label_colnames, perplexity=30, device=None):
    """compute_lisi of immunogenomics/LISI: X cells x PCs, meta_data a data.frame-like object (or a mapping of columns), label_colnames the
    columns to score.  Returns N x len(label_colnames) float64.  Every column uses the same m = 3 perplexity - 1 nearest neighbours (self
    excluded); neighbours and scores are computed in one call, the neighbour lists never leave the device."""
    X, xdt = _rows(X, "X")
    N, d = X.shape
    lisi_neighbours(perplexity, N)
    codes, n_levels, _ = _factor_columns(meta_data, label_colnames, N)
    with _Handle(device) as h:
        return _compute_lisi(h.lib, h.h, h.check, X, xdt, N, d, codes, n_levels, perplexity)


def harmony_lisi(obj, meta_data, label_colnames, perplexity=30):
    """Harmony.lisi: LISI of the handle's current Z_corr (a fitted handle or a mapped query), read where it lives in HBM"""
    N = int(obj._scalar("N_local"))
    lisi_neighbours(perplexity, N)
    codes, n_levels, _ = _factor_columns(meta_data, label_colnames, N)
    return _compute_lisi(obj._lib, obj._h, obj._check, None, 0, N, 0, codes, n_levels, perplexity)


def knn_predict(query, reference, reference_labels, k=5, device=None):
    """Symphony's knnPredict: the label of every query cell by majority vote over its k nearest reference cells (both cells x PCs, in the
    reference's corrected space: Z_corr of the fit and of map_query).  Ties go to the smallest level in sorted order.  Returns (labels,
    share): the winning label and the fraction of the k votes it got."""
    R = np.asarray(reference)
    codes, levels = _factor(reference_labels, R.shape[0] if R.ndim == 2 else -1, "reference_labels",
                            wrong_shape="reference_labels must hold one label per reference cell")
    idx, _ = knn(reference, k, query=query, device=device)
    votes = np.zeros((idx.shape[0], len(levels)), dtype=np.int64)
    np.add.at(votes, (np.arange(idx.shape[0])[:, None], codes[idx]), 1)
    win = votes.argmax(axis=1)                          # (first maximum: the smallest sorted level)
    return levels[win], votes[np.arange(len(win)), win] / float(idx.shape[1])

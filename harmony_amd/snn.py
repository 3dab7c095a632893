"""Seurat's shared-nearest-neighbour graph of an embedding on the GPU: what ``FindNeighbors`` builds and ``FindClusters`` reads.

``snn`` is ``FindNeighbors(k.param = k, prune.SNN = prune)`` on exact neighbours: ``nn``, the 0/1 matrix of every cell's k nearest cells (the
cell itself is one of them), and ``snn``, the Jaccard overlap s / (2k - s) of those sets (s = the cells two sets share) with the entries
below ``prune`` dropped; both as ``scipy.sparse.csr_matrix``.  ``snn_from_knn`` runs the SNN stage alone on neighbour lists.  Lists and graph
are computed in libharmony_mi355x.so (include/harmony_mi355x_snn.h); arguments are checked here, before the library is loaded.
"""
import ctypes as C

import numpy as np

from ._call import _Handle, _rows
from .graph import _check_lists, _csr, _fp, _ip, _lp, _neighbor_count

HMX_ERR_LIMIT = 7


def _prune(prune):
    p = float(prune)
    if not 0.0 <= p <= 1.0:                                # (NaN fails both comparisons)
        raise ValueError("prune must lie in [0, 1]")
    return p


def _snn_call(lib, handle, check, run, N, m):
    """run(indptr, indices, weights, capacity) -> status.  One call with min(N * N, 6 N k) entries; when the graph holds more, the library
    says how many (indptr[N]) and one more call with exactly that many follows."""
    indptr = np.empty(N + 1, dtype=np.int64)
    cap = int(min(N * N, 6 * N * (m + 1)))
    indices, weights = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.float32)
    status = run(indptr, indices, weights, cap)
    if status == HMX_ERR_LIMIT and b"entries (indptr is written)" in lib.hmx_last_error(handle):
        cap = int(indptr[N])
        indices, weights = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.float32)
        status = run(indptr, indices, weights, cap)
    check(status, "snn")
    nnz = int(indptr[N])
    if nnz < cap:
        indices, weights = indices[:nnz].copy(), weights[:nnz].copy()
    return _csr(indptr, indices, weights, N)


def _nn_matrix(idx, N, m):
    """A: the cell itself and its valid neighbours, float32 ones, rows ascending"""
    full = np.concatenate([np.arange(N, dtype=np.int32)[:, None], idx], axis=1)
    full = np.sort(np.where(full >= 0, full, np.iinfo(np.int32).max), axis=1)
    filled = full != np.iinfo(np.int32).max
    lens = filled.sum(axis=1)
    indices = full[filled].astype(np.int32)
    return _csr(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), indices, np.ones(indices.size, dtype=np.float32), N)


def _snn_graph(lib, handle, check, X, xdt, N, d, m, prune):
    idx, dist = np.empty((N, m), dtype=np.int32), np.empty((N, m), dtype=np.float32)

    def run(indptr, indices, weights, cap):
        return lib.hmx_snn_graph(handle, None if X is None else C.c_void_p(X.ctypes.data), xdt, 0, N, d, m + 1, prune,
                                 idx.ctypes.data_as(_ip), dist.ctypes.data_as(_fp), indptr.ctypes.data_as(_lp), indices.ctypes.data_as(_ip),
                                 weights.ctypes.data_as(_fp), cap)
    graph = _snn_call(lib, handle, check, run, N, m)
    return _nn_matrix(idx, N, m), graph


def snn(X, k=20, prune=1.0 / 15.0, device=None):
    """Seurat's FindNeighbors on the rows of X (cells x PCs, float64 or float32) with exact neighbours: (nn, snn), scipy.sparse.csr_matrix
    N x N.  Row i of `nn` holds a 1 for cell i and for each of its k - 1 nearest neighbours (k.param counts the cell itself).  `snn` holds
    s / (2k - s) for every pair of cells whose neighbour sets share s cells, without the entries below `prune` (prune.SNN; 0 keeps every
    pair that shares a cell); the diagonal is kept as Seurat keeps it; symmetric, rows ascending, float32.  Two calls give identical
    results."""
    X, xdt = _rows(X, "X")
    N, d = X.shape
    m = _neighbor_count(k, N, "k")
    prune = _prune(prune)
    with _Handle(device) as h:
        return _snn_graph(h.lib, h.h, h.check, X, xdt, N, d, m, prune)


def harmony_snn(obj, k=20, prune=1.0 / 15.0):
    """Harmony.snn: (nn, snn) of the handle's current Z_corr (a fitted handle or a mapped query), read where it lives in HBM"""
    N = int(obj._scalar("N_local"))
    m = _neighbor_count(k, N, "k")
    return _snn_graph(obj._lib, obj._h, obj._check, None, 0, N, 0, m, _prune(prune))


def snn_from_knn(idx, prune=1.0 / 15.0, device=None):
    """The SNN stage alone: the graph of the neighbour lists idx (N x m, self excluded, as knn(X, m) returns them; idx -1 marks an unfilled
    slot; k = m + 1)."""
    idx = _check_lists(idx, no_duplicates=True)[0]
    N, m = idx.shape
    prune = _prune(prune)
    with _Handle(device) as h:
        def run(indptr, indices, weights, cap):
            return h.lib.hmx_snn_from_knn(h.h, idx.ctypes.data_as(_ip), N, m, prune, indptr.ctypes.data_as(_lp), indices.ctypes.data_as(_ip),
                                          weights.ctypes.data_as(_fp), cap)
        return _snn_call(h.lib, h.h, h.check, run, N, m)

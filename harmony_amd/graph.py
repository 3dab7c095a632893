"""The neighbour graph of an embedding on the GPU, in the form scanpy stores it, and what this library does with a graph itself.

``neighbors`` is ``scanpy.pp.neighbors(use_rep=...)``: the exact k nearest neighbours (``distances``) and UMAP's fuzzy simplicial set over them
(``connectivities``: local_connectivity = 1, set_op_mix_ratio = 1, scanpy's values), both as ``scipy.sparse.csr_matrix`` -- what Leiden / Louvain,
UMAP and scib's graph metrics start from.  ``connected_components`` labels every cell with the smallest index of its component, optionally
counting only edges within a label; ``graph_connectivity`` is scib's score over them.  Lists, graph and components are computed in
libharmony_mi355x.so (include/harmony_mi355x_graph.h); arguments are checked here, before the library is loaded.
"""
import ctypes as C

import numpy as np

from ._call import _factor, _factor_column, _Handle, _rows
from .metrics import MAX_K

_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)


def _neighbor_count(value, N, name):
    """scanpy's n_neighbors and Seurat's k.param (`name` says which) count the cell itself: m = value - 1 neighbours with self excluded"""
    n = int(value) if np.isfinite(value) else 0
    if n != value or n < 2 or n > MAX_K + 1:
        raise ValueError("%s must be an integer in 2 .. %d (it counts the cell itself)" % (name, MAX_K + 1))
    if n > N:
        raise ValueError("%s = %d exceeds the %d cells" % (name, n, N))
    return n - 1


def _csr(indptr, indices, data, N):
    import scipy.sparse as sp
    return sp.csr_matrix((data, indices, indptr), shape=(N, N))


def _graph_call(run, N, m, want_lists):
    """one library call: run(idx, dist, indptr, indices, weights, capacity, rho, sigma) -> the trimmed outputs"""
    cap = int(min(2 * N * m, N * (N - 1)))
    indptr = np.empty(N + 1, dtype=np.int64)
    indices, weights = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.float32)
    rho, sigma = np.empty(N, dtype=np.float64), np.empty(N, dtype=np.float64)
    idx = np.empty((N, m), dtype=np.int32) if want_lists else None
    dist = np.empty((N, m), dtype=np.float32) if want_lists else None
    run(idx, dist, indptr, indices, weights, cap, rho, sigma)
    nnz = int(indptr[N])
    return idx, dist, indptr, indices[:nnz].copy(), weights[:nnz].copy(), rho, sigma


def _neighbor_graph(lib, handle, check, X, xdt, N, d, m):
    def run(idx, dist, indptr, indices, weights, cap, rho, sigma):
        check(lib.hmx_neighbor_graph(handle, None if X is None else C.c_void_p(X.ctypes.data), xdt, 0, N, d, m + 1,
                                     idx.ctypes.data_as(_ip), dist.ctypes.data_as(_fp), indptr.ctypes.data_as(_lp), indices.ctypes.data_as(_ip),
                                     weights.ctypes.data_as(_fp), cap, rho.ctypes.data_as(_dp), sigma.ctypes.data_as(_dp)), "neighbors")
    return _graph_call(run, N, m, True)


def _scanpy_pair(out, N, m, prune_zeros):
    idx, dist, indptr, indices, weights = out[:5]
    filled = idx.ravel() >= 0
    lens = (idx >= 0).sum(axis=1)
    distances = _csr(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), idx.ravel()[filled], dist.ravel()[filled], N)
    conn = _csr(indptr, indices, weights, N)
    if prune_zeros:
        conn.eliminate_zeros()
    return distances, conn


def neighbors(X, n_neighbors=15, device=None, prune_zeros=True):
    """scanpy.pp.neighbors on the rows of X (cells x PCs, float64 or float32): (distances, connectivities), scipy.sparse.csr_matrix N x N.
    Row i of `distances` holds the n_neighbors - 1 exact nearest neighbours of cell i in the order the search returns them (ascending by
    (distance, index), self excluded; float32).  `connectivities` is UMAP's fuzzy simplicial set over them: symmetric, rows ascending, float32.
    prune_zeros=True drops the weights that underflowed to 0, as scanpy does; False keeps the library's pattern, which depends on the
    neighbour lists alone.  Two calls give identical results."""
    X, xdt = _rows(X, "X")
    N, d = X.shape
    m = _neighbor_count(n_neighbors, N, "n_neighbors")
    with _Handle(device) as h:
        out = _neighbor_graph(h.lib, h.h, h.check, X, xdt, N, d, m)
    return _scanpy_pair(out, N, m, prune_zeros)


def harmony_neighbors(obj, n_neighbors=15, prune_zeros=True):
    """Harmony.neighbors: the graph of the handle's current Z_corr (a fitted handle or a mapped query), read where it lives in HBM"""
    N = int(obj._scalar("N_local"))
    m = _neighbor_count(n_neighbors, N, "n_neighbors")
    return _scanpy_pair(_neighbor_graph(obj._lib, obj._h, obj._check, None, 0, N, 0, m), N, m, prune_zeros)


def _check_lists(idx, dist=None, no_duplicates=False):
    """neighbour lists idx (N x m, self excluded, -1: an unfilled slot), with their distances or without -> (int32 idx, float32 dist or None)"""
    idx, dist = np.asarray(idx), None if dist is None else np.asarray(dist)
    if idx.ndim != 2 or idx.shape[0] < 1 or idx.shape[1] < 1 or (dist is not None and dist.shape != idx.shape):
        raise ValueError("idx must be an N x m matrix" if dist is None else "idx and dist must be N x m matrices of one shape")
    N, m = idx.shape
    if m > MAX_K:
        raise ValueError("at most %d neighbours per cell" % MAX_K)
    if not np.issubdtype(idx.dtype, np.integer) or np.any(idx < -1) or np.any(idx >= N):
        raise ValueError("neighbour indices must be integers in [-1, %d) (-1: an unfilled slot)" % N)
    if np.any(idx == np.arange(N)[:, None]):
        raise ValueError("a row lists its own cell: the neighbour lists exclude self")
    if dist is not None and np.any(np.isnan(dist) & (idx >= 0)):
        raise ValueError("NaN distances")
    if no_duplicates:
        srt = np.sort(idx, axis=1)
        if np.any((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)):
            raise ValueError("a row lists a cell twice")
    return np.ascontiguousarray(idx, dtype=np.int32), None if dist is None else np.ascontiguousarray(dist, dtype=np.float32)


def graph_from_knn(idx, dist, device=None, prune_zeros=True, return_scales=False):
    """The graph stage alone: `connectivities` of the neighbour lists idx, dist (N x m, self excluded, as knn(X, m) returns them; idx -1 marks
    an unfilled slot).  return_scales=True: (connectivities, rho, sigma), the smooth-kNN distances of every cell (float64)."""
    idx, dist = _check_lists(idx, dist)
    N, m = idx.shape

    with _Handle(device) as h:
        def run(_i, _d, indptr, indices, weights, cap, rho, sigma):
            h.check(h.lib.hmx_graph_from_knn(h.h, idx.ctypes.data_as(_ip), dist.ctypes.data_as(_fp), N, m, indptr.ctypes.data_as(_lp),
                                             indices.ctypes.data_as(_ip), weights.ctypes.data_as(_fp), cap, rho.ctypes.data_as(_dp),
                                             sigma.ctypes.data_as(_dp)), "graph_from_knn")
        _, _, indptr, indices, weights, rho, sigma = _graph_call(run, N, m, False)
    conn = _csr(indptr, indices, weights, N)
    if prune_zeros:
        conn.eliminate_zeros()
    return (conn, rho, sigma) if return_scales else conn


def _pattern(graph):
    """a square scipy.sparse matrix or an (indptr, indices) pair -> (int64 indptr, int32 indices with ascending rows, N)"""
    if hasattr(graph, "tocsr"):
        g = graph.tocsr()
        if g.shape[0] != g.shape[1]:
            raise ValueError("the graph must be square")
        if not g.has_sorted_indices:
            g = g.sorted_indices()
        indptr, indices = g.indptr, g.indices
    else:
        try:
            indptr, indices = graph
        except (TypeError, ValueError):
            raise ValueError("graph must be a scipy.sparse matrix or an (indptr, indices) pair")
    indptr = np.ascontiguousarray(indptr, dtype=np.int64).reshape(-1)
    indices = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
    N = indptr.size - 1
    if N < 1 or indptr[0] != 0 or np.any(np.diff(indptr) < 0) or indptr[N] != indices.size:
        raise ValueError("indptr must ascend from 0 to the number of stored indices")
    return indptr, indices, N


def _components(indptr, indices, N, codes, device):
    comp = np.empty(N, dtype=np.int32)
    n = C.c_int64(0)
    with _Handle(device) as h:
        h.check(h.lib.hmx_graph_components(h.h, N, indptr.ctypes.data_as(_lp), indices.ctypes.data_as(_ip),
                                           None if codes is None else codes.ctypes.data_as(_ip), comp.ctypes.data_as(_ip), C.byref(n)),
                "connected_components")
    return int(n.value), comp


def connected_components(graph, labels=None, device=None):
    """The connected components of a symmetric graph (a scipy.sparse matrix, stored zeros included, or an (indptr, indices) pair):
    (n_components, comp), comp[i] int32 the smallest cell index of i's component.  With `labels` (one per cell) only edges whose two ends carry
    the same label count."""
    indptr, indices, N = _pattern(graph)
    codes = None if labels is None else _factor(labels, N, "labels")[0]
    return _components(indptr, indices, N, codes, device)


def connectivity_from_components(comp, codes, n_levels):
    """scib's score from the components of the same-label edges: the mean over the levels with cells of (largest component) / (cells)"""
    shares = []
    for lev in range(int(n_levels)):
        cells = np.nonzero(codes == lev)[0]
        if cells.size:
            shares.append(np.bincount(comp[cells]).max() / cells.size)
    if not shares:
        raise ValueError("graph_connectivity: no cell carries a label")
    return float(np.mean(shares))


def graph_connectivity(graph_or_X, meta_data, label_col, n_neighbors=15, device=None):
    """scib's graph connectivity of the column `label_col` of meta_data: per label the share of its cells in the largest connected component
    of the graph restricted to that label, averaged over the labels; 1 means no label is torn apart.  graph_or_X: a graph (scipy.sparse, as
    `neighbors` returns its connectivities) or an embedding (cells x PCs), whose graph is built first with `n_neighbors`."""
    if hasattr(graph_or_X, "tocsr"):
        graph = graph_or_X
    else:
        graph = neighbors(graph_or_X, n_neighbors=n_neighbors, device=device)[1]
    indptr, indices, N = _pattern(graph)
    codes, levels = _factor_column(meta_data, label_col, N)
    _, comp = _components(indptr, indices, N, codes, device)
    return connectivity_from_components(comp, codes, len(levels))

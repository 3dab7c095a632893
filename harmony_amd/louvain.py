"""Louvain clustering of a neighbour graph on the GPU: Seurat's ``FindClusters`` step on the graph ``snn`` builds (or scanpy's on the
connectivities of ``neighbors``), as a deterministic algorithm: the result is a pure function of the graph, two calls give identical labels.

``louvain`` maximises the modularity sum_c (in_c / M - resolution (tot_c / M)^2) by local moves in hashed sub-rounds and aggregation, level
by level, and returns the first level of the largest modularity (include/harmony_mi355x_louvain.h has the definition; the order in which
Seurat visits the cells is random, so only the objective is shared with it).  Labels are numbered by decreasing cluster size, ties by the
smallest member cell, as Seurat numbers its clusters.  The work is done in libharmony_mi355x.so; arguments are checked here, before the
library is loaded.
"""
import collections
import ctypes as C

import numpy as np

from ._call import _Handle
from .graph import _dp, _fp, _ip, _lp

MAX_LEVELS, MAX_SWEEPS, MAX_RESOLUTION = 64, 4096, 100.0

Louvain = collections.namedtuple("Louvain", "labels n_clusters modularity levels")


def _count(value, name, top):
    n = int(value) if np.isfinite(value) else 0
    if n != value or n < 1 or n > top:
        raise ValueError("%s must be an integer in 1 .. %d" % (name, top))
    return n


def _resolution(resolution):
    r = float(resolution)
    if not 0.0 < r <= MAX_RESOLUTION:                      # (NaN fails both comparisons)
        raise ValueError("resolution must lie in (0, %g]" % MAX_RESOLUTION)
    return r


def _weighted_graph(graph):
    """a square scipy.sparse matrix or an (indptr, indices, weights) triple -> (int64 indptr, int32 indices ascending per row, float32
    weights, N), symmetric bit for bit with weights in [0, 1]"""
    import scipy.sparse as sp
    if hasattr(graph, "tocsr"):
        g = graph.tocsr()
    else:
        try:
            indptr, indices, weights = graph
            g = sp.csr_matrix((np.asarray(weights), np.asarray(indices), np.asarray(indptr)), shape=(len(indptr) - 1,) * 2)
        except (TypeError, ValueError):
            raise ValueError("graph must be a square scipy.sparse matrix or an (indptr, indices, weights) triple")
    if g.shape[0] != g.shape[1] or g.shape[0] < 1:
        raise ValueError("the graph must be square")
    N = g.shape[0]
    if g.nnz >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 stored entries")
    if g.nnz and (g.indices.min() < 0 or g.indices.max() >= N):
        raise ValueError("an index of the graph is outside [0, %d)" % N)
    if not g.has_sorted_indices:
        g = g.sorted_indices()
    indptr = np.ascontiguousarray(g.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(g.indices, dtype=np.int32)
    weights = np.ascontiguousarray(g.data, dtype=np.float32)
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(indptr))
    if np.any((indices[1:] <= indices[:-1]) & (rows[1:] == rows[:-1])):
        raise ValueError("a row of the graph stores an index twice")
    if not np.all((weights >= 0.0) & (weights <= 1.0)):    # (NaN fails both comparisons)
        raise ValueError("the weights must be finite and lie in [0, 1]: divide by the largest weight first")
    key = rows * N + indices
    mirror = np.argsort(indices.astype(np.int64) * N + rows, kind="stable")      # the entries in the transposed matrix's order
    if not np.array_equal(key, (indices.astype(np.int64) * N + rows)[mirror]):
        raise ValueError("the graph is not symmetric: an edge has no mirror")
    if not np.array_equal(weights.view(np.uint32), weights[mirror].view(np.uint32)):
        raise ValueError("the graph is not symmetric: an edge and its mirror carry different weights")
    return indptr, indices, weights, N


def seurat_order(labels):
    """clusters renumbered by decreasing size, ties by the smallest member cell"""
    ids, first, counts = np.unique(labels, return_index=True, return_counts=True)
    rank = np.empty(ids.size, dtype=np.int32)
    rank[np.lexsort((first, -counts))] = np.arange(ids.size, dtype=np.int32)
    return rank[np.searchsorted(ids, labels)]


def _louvain_call(lib, handle, check, indptr, indices, weights, N, resolution, max_levels, max_sweeps):
    labels = np.empty(N, dtype=np.int32)
    n, q = C.c_int32(0), C.c_double(0.0)
    lc, ls, lq = np.zeros(max_levels, dtype=np.int32), np.zeros(max_levels, dtype=np.int32), np.zeros(max_levels, dtype=np.float64)
    check(lib.hmx_louvain(handle, indptr.ctypes.data_as(_lp), indices.ctypes.data_as(_ip), weights.ctypes.data_as(_fp), N, resolution,
                          max_levels, max_sweeps, labels.ctypes.data_as(_ip), C.byref(n), C.byref(q), lc.ctypes.data_as(_ip),
                          ls.ctypes.data_as(_ip), lq.ctypes.data_as(_dp)), "louvain")
    out = (C.c_double * 1)()
    lib.hmx_get(handle, b"louvain:levels", out, 1)
    levels = [(int(lc[i]), int(ls[i]), float(lq[i])) for i in range(int(out[0]))]
    return Louvain(seurat_order(labels), int(n.value), float(q.value), levels)


def louvain(graph, resolution=1.0, max_levels=10, max_sweeps=32, device=None):
    """Louvain clusters of a symmetric weighted graph (a scipy.sparse matrix as `snn` and `neighbors` return it, or an (indptr, indices,
    weights) triple) with weights in [0, 1] (divide any other graph by its largest weight; the diagonal is ignored): a namedtuple
    (labels, n_clusters, modularity, levels).  labels: int32, one per cell, 0 the largest cluster; modularity: that of the labels at
    `resolution`; levels: (clusters, sweeps, modularity) of every level the call went through, of which the first with the largest modularity
    is returned.  Each level makes at most `max_sweeps` sweeps of local moves; at most `max_levels` levels.  Two calls give identical
    results."""
    indptr, indices, weights, N = _weighted_graph(graph)
    resolution = _resolution(resolution)
    max_levels, max_sweeps = _count(max_levels, "max_levels", MAX_LEVELS), _count(max_sweeps, "max_sweeps", MAX_SWEEPS)
    with _Handle(device) as h:
        return _louvain_call(h.lib, h.h, h.check, indptr, indices, weights, N, resolution, max_levels, max_sweeps)


def harmony_clusters(obj, k=20, prune=1.0 / 15.0, resolution=0.8):
    """Harmony.clusters: Seurat's FindNeighbors and FindClusters on the handle's current Z_corr"""
    resolution = _resolution(resolution)
    graph = obj.snn(k=k, prune=prune)[1]
    indptr, indices, weights, N = _weighted_graph(graph)
    return _louvain_call(obj._lib, obj._h, obj._check, indptr, indices, weights, N, resolution, 10, 32)

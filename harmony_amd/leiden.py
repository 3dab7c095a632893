"""Leiden clustering of a neighbour graph on the GPU: scanpy's default clustering (``sc.tl.leiden`` on the connectivities of ``neighbors``) and
Seurat's ``FindClusters(algorithm = 4)``, as a deterministic algorithm: the result is a pure function of the graph, two calls give identical
labels, and every cluster of a converged result is connected in the graph, which Louvain does not promise.

``leiden`` alternates Louvain's local moves in hashed sub-rounds with a refinement inside the communities and aggregates by the refined
partition, level by level, until every node is a community of its own (include/harmony_mi355x_leiden.h has the definition; Leiden's random
choice among the candidates is replaced by the largest score, so only the objective and the guarantee are shared with leidenalg).  Labels are
numbered by decreasing cluster size, ties by the smallest member cell.  The work is done in libharmony_mi355x.so; arguments are checked here,
before the library is loaded.
"""
import collections
import ctypes as C

import numpy as np

from ._call import _Handle
from .graph import _dp, _fp, _ip, _lp
from .louvain import MAX_LEVELS, MAX_SWEEPS, _count, _resolution, _weighted_graph, seurat_order

Leiden = collections.namedtuple("Leiden", "labels n_clusters modularity levels converged")


def _leiden_call(lib, handle, check, indptr, indices, weights, N, resolution, max_levels, max_sweeps):
    labels = np.empty(N, dtype=np.int32)
    n, q, conv = C.c_int32(0), C.c_double(0.0), C.c_int32(0)
    lc, ln, ls, lr = (np.zeros(max_levels, dtype=np.int32) for _ in range(4))
    lq = np.zeros(max_levels, dtype=np.float64)
    check(lib.hmx_leiden(handle, indptr.ctypes.data_as(_lp), indices.ctypes.data_as(_ip), weights.ctypes.data_as(_fp), N, resolution,
                         max_levels, max_sweeps, labels.ctypes.data_as(_ip), C.byref(n), C.byref(q), C.byref(conv), lc.ctypes.data_as(_ip),
                         ln.ctypes.data_as(_ip), ls.ctypes.data_as(_ip), lr.ctypes.data_as(_ip), lq.ctypes.data_as(_dp)), "leiden")
    out = (C.c_double * 1)()
    lib.hmx_get(handle, b"leiden:levels", out, 1)
    levels = [(int(lc[i]), int(ln[i]), int(ls[i]), int(lr[i]), float(lq[i])) for i in range(int(out[0]))]
    return Leiden(seurat_order(labels), int(n.value), float(q.value), levels, bool(conv.value))


def leiden(graph, resolution=1.0, max_levels=20, max_sweeps=32, device=None):
    """Leiden clusters of a symmetric weighted graph (a scipy.sparse matrix as `neighbors` and `snn` return it, or an (indptr, indices,
    weights) triple) with weights in [0, 1] (divide any other graph by its largest weight; the diagonal and stored zeros are no edges): a
    namedtuple (labels, n_clusters, modularity, levels, converged).  labels: int32, one per cell, 0 the largest cluster, the partition of the
    last level; modularity: that of the labels at `resolution`; levels: (clusters, nodes, sweeps, refine_sweeps, modularity) of every level
    the call went through; converged: the last level made every node a community of its own, and then every cluster is connected.  Each
    phase of a level makes at most `max_sweeps` sweeps; at most `max_levels` levels.  Two calls give identical results."""
    indptr, indices, weights, N = _weighted_graph(graph)
    resolution = _resolution(resolution)
    max_levels, max_sweeps = _count(max_levels, "max_levels", MAX_LEVELS), _count(max_sweeps, "max_sweeps", MAX_SWEEPS)
    with _Handle(device) as h:
        return _leiden_call(h.lib, h.h, h.check, indptr, indices, weights, N, resolution, max_levels, max_sweeps)


def _on_handle(obj, graph, resolution):
    indptr, indices, weights, N = _weighted_graph(graph)
    return _leiden_call(obj._lib, obj._h, obj._check, indptr, indices, weights, N, resolution, 20, 32)


def harmony_leiden(obj, n_neighbors=15, resolution=1.0):
    """Harmony.leiden: scanpy's neighbors and leiden on the handle's current Z_corr"""
    resolution = _resolution(resolution)
    return _on_handle(obj, obj.neighbors(n_neighbors=n_neighbors)[1], resolution)


def harmony_clusters_leiden(obj, k=20, prune=1.0 / 15.0, resolution=0.8):
    """Harmony.clusters(algorithm="leiden"): Seurat's FindNeighbors and FindClusters(algorithm = 4) on the handle's current Z_corr"""
    resolution = _resolution(resolution)
    return _on_handle(obj, obj.snn(k=k, prune=prune)[1], resolution)

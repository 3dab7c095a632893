"""Query cells put into a fitted UMAP layout on the GPU: the last step of reference mapping, the query in the reference's picture.  What
umap-learn's ``transform``, Symphony's ``mapQuery(do_umap=TRUE)`` and Seurat's ``MapQuery(reduction.model="umap")`` do: the reference's
positions stay where they are, a query cell starts at the weighted mean of its nearest reference cells and is then attracted by them and
repelled by hashed samples of the reference.  Every query cell is independent of every other one and the result is a pure function of the
arguments: two calls give identical coordinates.

``umap_query_weights`` turns the lists ``knn(reference, k, query=Q)`` returns into umap-learn's membership weights, ``umap_transform_from_knn``
runs the epochs (include/harmony_mi355x_umap_transform.h has the definition), ``umap_transform`` is the search and the two stages.  The work is
done in libharmony_mi355x.so; arguments are checked here, before the library is loaded.
"""
import ctypes as C

import numpy as np

from ._call import _Handle, _rows
from .graph import _fp, _ip
from .umap import _Params

MAX_K = 128
_dp = C.POINTER(C.c_double)


def _lists(idx, other, n_reference, what):
    """idx and its companion (distances or weights) as [Nq, k] int32 / float32 arrays of one shape with indices in [0, n_reference)"""
    idx, other = np.asarray(idx), np.asarray(other)
    if idx.ndim != 2 or idx.shape != other.shape or idx.shape[0] < 1 or idx.shape[1] < 1:
        raise ValueError("idx and %s must be Nq x k matrices of one shape" % what)
    if idx.shape[1] > MAX_K:
        raise ValueError("at most %d neighbours per cell" % MAX_K)
    Nr = int(n_reference)
    if Nr != n_reference or Nr < 1:
        raise ValueError("n_reference must be a positive integer")
    if idx.shape[1] > Nr:
        raise ValueError("k = %d exceeds the %d reference cells" % (idx.shape[1], Nr))
    if idx.shape[0] * idx.shape[1] >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 list entries")
    if not np.issubdtype(idx.dtype, np.integer) or np.any(idx < 0) or np.any(idx >= Nr):
        raise ValueError("neighbour indices must be integers in [0, %d)" % Nr)
    return np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(other, dtype=np.float32), Nr


def _distances(idx, dist, n_reference):
    idx, dist, Nr = _lists(idx, dist, n_reference, "dist")
    if not np.all(np.isfinite(dist)) or np.any(dist < 0.0):
        raise ValueError("distances must be finite and non-negative")
    return idx, dist, Nr


def _layout(reference_layout):
    Yref = np.ascontiguousarray(reference_layout, dtype=np.float32)
    if Yref.ndim != 2 or Yref.shape[0] < 1 or Yref.shape[1] not in (2, 3):
        raise ValueError("reference_layout must be an [Nr, 2 or 3] array, got shape %s" % (Yref.shape,))
    if not np.all(np.isfinite(Yref)):
        raise ValueError("reference_layout holds values that are not finite")
    return Yref


def _params(Nq, dim, n_epochs, min_dist, spread, a, b, gamma, learning_rate, negative_sample_rate, seed, epochs):
    """umap._Params with transform's defaults: 100 epochs up to 10 000 query cells, else 30"""
    if n_epochs is None:
        n_epochs = 100 if Nq <= 10000 else 30
    return _Params(Nq, dim, n_epochs, min_dist, spread, a, b, gamma, learning_rate, negative_sample_rate, seed, epochs)


def _start(init, Nq, dim):
    if init is None:
        return None
    Y0 = np.ascontiguousarray(init, dtype=np.float32)
    if Y0.shape != (Nq, dim):
        raise ValueError("init must be an [Nq, n_components] = [%d, %d] array, got shape %s" % (Nq, dim, Y0.shape))
    if not np.all(np.isfinite(Y0)):
        raise ValueError("init holds values that are not finite")
    return Y0


def _weights_call(lib, handle, check, idx, dist, Nr, return_scales):
    w = np.empty(idx.shape, dtype=np.float32)
    sigma = np.empty(idx.shape[0], dtype=np.float64) if return_scales else None
    check(lib.hmx_umap_query_weights(handle, idx.ctypes.data_as(_ip), dist.ctypes.data_as(_fp), idx.shape[0], idx.shape[1], Nr,
                                     w.ctypes.data_as(_fp), None if sigma is None else sigma.ctypes.data_as(_dp)), "umap_query_weights")
    return (w, sigma) if return_scales else w


def _transform_call(lib, handle, check, idx, w, Yref, Y0, p, return_init):
    Nq, dim = idx.shape[0], Yref.shape[1]
    Y = np.empty((Nq, dim), dtype=np.float32)
    Yinit = np.empty((Nq, dim), dtype=np.float32) if return_init else None
    check(lib.hmx_umap_transform(handle, idx.ctypes.data_as(_ip), w.ctypes.data_as(_fp), Nq, idx.shape[1], Yref.ctypes.data_as(_fp), Yref.shape[0],
                                 dim, None if Y0 is None else Y0.ctypes.data_as(_fp), p.n_epochs, p.begin, p.end, p.a, p.b, p.gamma,
                                 p.learning_rate / 4.0, p.negative, p.seed, None if Yinit is None else Yinit.ctypes.data_as(_fp),
                                 Y.ctypes.data_as(_fp)), "umap_transform")
    return (Y, Yinit) if return_init else Y


def umap_query_weights(idx, dist, n_reference, return_scales=False, device=None):
    """umap-learn's membership weights of query cells in their nearest reference cells.  idx, dist: Nq x k, what ``knn(reference, k,
    query=Q)`` returns (k = n_neighbors reference cells per query cell, ascending by distance, no self column).  rho is 0, sigma is searched
    over the entries behind the first -- as umap-learn's smooth_knn_dist does -- and w = exp(-d / sigma) for all k entries.  Returns float32
    weights Nq x k, or (weights, sigma) with return_scales."""
    idx, dist, Nr = _distances(idx, dist, n_reference)
    with _Handle(device) as h:
        return _weights_call(h.lib, h.h, h.check, idx, dist, Nr, return_scales)


def umap_transform_from_knn(idx, weights, reference_layout, init=None, n_epochs=None, min_dist=0.5, spread=1.0, a=None, b=None, gamma=1.0,
                            learning_rate=1.0, negative_sample_rate=5, seed=0, epochs=None, return_init=False, device=None):
    """The positions of Nq query cells in a fitted layout from their lists of reference cells (idx, Nq x k) and the lists' weights in [0, 1]
    (``umap_query_weights``).  reference_layout: [Nr, 2 or 3], left as it is.  init=None: the weighted mean of the listed positions, else an
    [Nq, n_components] array.  n_epochs=None: 100 up to 10 000 query cells, else 30; epochs=(begin, end) runs that part of the schedule, so
    that (0, k) then (k, n) from its result equals (0, n).  learning_rate is passed on as alpha0 = learning_rate / 4, as umap-learn's
    transform does.  a, b: fitted from min_dist and spread when not given -- pass the reference layout's.  Returns float32 [Nq, n_components],
    or (positions, start) with return_init.  Two calls give identical coordinates."""
    Yref = _layout(reference_layout)
    idx, w, Nr = _lists(idx, weights, Yref.shape[0], "weights")
    if not np.all(np.isfinite(w)) or np.any(w < 0.0) or np.any(w > 1.0):
        raise ValueError("weights must be finite and lie in [0, 1]")
    Y0 = _start(init, idx.shape[0], Yref.shape[1])
    p = _params(idx.shape[0], Yref.shape[1], n_epochs, min_dist, spread, a, b, gamma, learning_rate, negative_sample_rate, seed, epochs)
    with _Handle(device) as h:
        return _transform_call(h.lib, h.h, h.check, idx, w, Yref, Y0, p, return_init)


def umap_transform(query, reference, reference_layout, n_neighbors=15, init=None, n_epochs=None, min_dist=0.5, spread=1.0, a=None, b=None,
                   gamma=1.0, learning_rate=1.0, negative_sample_rate=5, seed=0, return_init=False, device=None):
    """umap-learn's transform: `query` and `reference` are cells x PCs in one space (Z_corr of map_query and of the fit), reference_layout the
    reference's fitted positions [Nr, 2 or 3].  ``knn(reference, n_neighbors, query=query)``, ``umap_query_weights``, then
    ``umap_transform_from_knn``."""
    from .metrics import knn
    Q, R = _rows(query, "query")[0], _rows(reference, "reference")[0]
    Yref = _layout(reference_layout)
    if Yref.shape[0] != R.shape[0]:
        raise ValueError("reference_layout has %d rows, reference %d cells" % (Yref.shape[0], R.shape[0]))
    Y0 = _start(init, Q.shape[0], Yref.shape[1])
    p = _params(Q.shape[0], Yref.shape[1], n_epochs, min_dist, spread, a, b, gamma, learning_rate, negative_sample_rate, seed, None)
    k = int(n_neighbors)
    if k != n_neighbors or k < 1 or k > MAX_K or k > R.shape[0]:
        raise ValueError("n_neighbors must be an integer in 1 .. %d" % min(MAX_K, R.shape[0]))
    idx, dist = knn(R, k, query=Q, device=device)
    with _Handle(device) as h:
        w = _weights_call(h.lib, h.h, h.check, idx, dist, R.shape[0], False)
        return _transform_call(h.lib, h.h, h.check, idx, w, Yref, Y0, p, return_init)


def harmony_umap_transform(obj, reference, reference_layout, **kwargs):
    """Harmony.umap_transform: the handle's current Z_corr (a fitted handle, or the object map_query(return_object=True) returns) put into
    the reference's layout"""
    return umap_transform(np.ascontiguousarray(np.asarray(obj.getZcorr()).T), reference, reference_layout, **kwargs)

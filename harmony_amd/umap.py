"""The UMAP layout of a neighbour graph on the GPU: the plot a Harmony run is judged by, as a deterministic algorithm: the result is a pure
function of the graph, the starting positions and the seed, two calls give identical coordinates.

``umap_layout`` runs umap-learn's stochastic gradient descent over the fuzzy simplicial set (the `connectivities` of ``neighbors``) in
synchronous epochs: an epoch reads the positions the one before left, an entry fires in the epochs umap-learn's ``epochs_per_sample`` gives
it, negative samples are hashed from the entry, the epoch and the seed (include/harmony_mi355x_umap.h has the definition; umap-learn applies
one edge at a time to positions other threads are changing, so only the objective and the schedule are shared with it).  ``umap`` is
``neighbors`` then ``umap_layout``.  The work is done in libharmony_mi355x.so; arguments are checked here, before the library is loaded.
"""
import ctypes as C

import numpy as np

from ._call import _Handle, _rows
from .graph import _fp, _ip, _lp
from .louvain import _weighted_graph

MAX_EPOCHS, MAX_NEGATIVE = 1 << 20, 31
_M32 = 0xFFFFFFFF


def find_ab_params(spread=1.0, min_dist=0.5):
    """umap-learn's fit of 1 / (1 + a x^(2b)) to the membership curve that is 1 up to min_dist and decays as exp(-(x - min_dist) / spread)
    beyond it: (a, b)"""
    from scipy.optimize import curve_fit
    spread, min_dist = float(spread), float(min_dist)
    if not (spread > 0.0 and np.isfinite(spread)) or not (0.0 <= min_dist < 3.0 * spread):
        raise ValueError("spread must be positive and min_dist lie in [0, 3 spread)")
    xv = np.linspace(0.0, spread * 3.0, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    params, _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2.0 * b)), xv, yv)
    return float(params[0]), float(params[1])


def _fmix32(x):
    x = np.asarray(x, dtype=np.uint64) & _M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & _M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & _M32
    x ^= x >> 16
    return x


def random_init(N, n_components, seed):
    """20 (fmix32(i dim + c ^ fmix32(seed + 0x51ed)) + 0.5) / 2^32 - 10 per coordinate: inside [-10, 10], float32"""
    key = int(_fmix32((int(seed) + 0x51ED) & _M32))
    h = _fmix32(np.arange(N * n_components, dtype=np.uint64) ^ np.uint64(key)).astype(np.float64)
    return (20.0 * (h + 0.5) / 2.0 ** 32 - 10.0).astype(np.float32).reshape(N, n_components)


def pca_init(X, n_components):
    """the top n_components principal axes of X from the d x d covariance (NumPy fp64), each signed so that its largest-magnitude loading is
    positive, scaled to a largest |coordinate| of 10, float32"""
    X = np.asarray(X, dtype=np.float64)
    if X.shape[1] < n_components:
        raise ValueError("init='pca' needs at least n_components = %d columns" % n_components)
    Xc = X - X.mean(axis=0)
    vals, vecs = np.linalg.eigh(Xc.T @ Xc / max(X.shape[0] - 1, 1))
    axes = vecs[:, np.argsort(-vals, kind="stable")[:n_components]]
    axes = axes * np.where(axes[np.abs(axes).argmax(axis=0), np.arange(n_components)] < 0.0, -1.0, 1.0)
    P = Xc @ axes
    top = np.abs(P).max()
    return (P * (10.0 / top if top > 0.0 else 1.0)).astype(np.float32)


def _integer(value, name, low, top):
    n = int(value) if np.isfinite(value) else low - 1
    if n != value or n < low or n > top:
        raise ValueError("%s must be an integer in %d .. %d" % (name, low, top))
    return n


def _positive(value, name, zero_ok=False):
    v = float(value)
    if not np.isfinite(v) or v < 0.0 or (v == 0.0 and not zero_ok):
        raise ValueError("%s must be %s and finite" % (name, "non-negative" if zero_ok else "positive"))
    return v


class _Params(object):
    """the checked scalar arguments of a layout of N cells"""

    def __init__(self, N, n_components, n_epochs, min_dist, spread, a, b, gamma, learning_rate, negative_sample_rate, seed, epochs):
        self.dim = _integer(n_components, "n_components", 2, 3)
        self.n_epochs = (500 if N <= 10000 else 200) if n_epochs is None else _integer(n_epochs, "n_epochs", 1, MAX_EPOCHS)
        if epochs is None:
            self.begin, self.end = 0, self.n_epochs
        else:
            try:
                begin, end = epochs
            except (TypeError, ValueError):
                raise ValueError("epochs must be a pair (begin, end)")
            self.begin, self.end = _integer(begin, "epochs[0]", 0, self.n_epochs), _integer(end, "epochs[1]", 0, self.n_epochs)
            if self.end < self.begin:
                raise ValueError("epochs must be a pair (begin, end) with begin <= end <= n_epochs")
        self.gamma = _positive(gamma, "gamma", zero_ok=True)
        self.learning_rate = _positive(learning_rate, "learning_rate")
        self.negative = _integer(negative_sample_rate, "negative_sample_rate", 0, MAX_NEGATIVE)
        self.seed = _integer(seed, "seed", 0, _M32)
        if a is None or b is None:
            if a is not None or b is not None:
                raise ValueError("give both a and b, or neither (they are then fitted from min_dist and spread)")
            a, b = find_ab_params(spread, min_dist)
        self.a, self.b = _positive(a, "a"), _positive(b, "b")


def _start(init, N, p, X=None):
    if isinstance(init, str):
        if init == "random":
            return random_init(N, p.dim, p.seed)
        if init == "pca" and X is not None:
            return pca_init(X, p.dim)
        raise ValueError("init must be an [N, n_components] array or 'random'" + (" or 'pca'" if X is not None else ""))
    Y0 = np.ascontiguousarray(init, dtype=np.float32)
    if Y0.shape != (N, p.dim):
        raise ValueError("init must be an [N, n_components] = [%d, %d] array, got shape %s" % (N, p.dim, Y0.shape))
    if not np.all(np.isfinite(Y0)):
        raise ValueError("init holds values that are not finite")
    return Y0


def _layout_call(lib, handle, check, indptr, indices, weights, N, Y0, p):
    Y = np.empty((N, p.dim), dtype=np.float32)
    check(lib.hmx_umap_layout(handle, indptr.ctypes.data_as(_lp), indices.ctypes.data_as(_ip), weights.ctypes.data_as(_fp), N, p.dim,
                              Y0.ctypes.data_as(_fp), p.n_epochs, p.begin, p.end, p.a, p.b, p.gamma, p.learning_rate, p.negative, p.seed,
                              Y.ctypes.data_as(_fp)), "umap_layout")
    return Y


def umap_layout(graph, init, n_components=2, n_epochs=None, min_dist=0.5, spread=1.0, a=None, b=None, gamma=1.0, learning_rate=1.0,
                negative_sample_rate=5, seed=0, epochs=None, device=None):
    """The layout of a symmetric weighted graph (a scipy.sparse matrix as `neighbors` returns its connectivities, or an (indptr, indices,
    weights) triple) with weights in [0, 1]: float32 positions [N, n_components], n_components 2 or 3.  init: the starting positions, an
    [N, n_components] array, or "random" (hashed from `seed`, inside [-10, 10]).  n_epochs=None: 500 up to 10 000 cells, else 200;
    epochs=(begin, end) runs that part of the schedule, so that (0, k) then (k, n) from its result equals (0, n).  a, b: the curve's
    parameters, fitted from min_dist and spread when not given (find_ab_params).  Two calls give identical coordinates."""
    indptr, indices, weights, N = _weighted_graph(graph)
    p = _Params(N, n_components, n_epochs, min_dist, spread, a, b, gamma, learning_rate, negative_sample_rate, seed, epochs)
    Y0 = _start(init, N, p)
    with _Handle(device) as h:
        return _layout_call(h.lib, h.h, h.check, indptr, indices, weights, N, Y0, p)


def umap(X, n_neighbors=15, init="pca", n_components=2, n_epochs=None, min_dist=0.5, spread=1.0, a=None, b=None, gamma=1.0,
         learning_rate=1.0, negative_sample_rate=5, seed=0, device=None):
    """UMAP of the rows of X (cells x PCs): `neighbors(X, n_neighbors)`, then `umap_layout` on its connectivities.  init: "pca" (the top
    principal axes of X, scaled to [-10, 10]), "random" or an array."""
    from .graph import neighbors
    X = _rows(X, "X")[0]
    p = _Params(X.shape[0], n_components, n_epochs, min_dist, spread, a, b, gamma, learning_rate, negative_sample_rate, seed, None)
    Y0 = _start(init, X.shape[0], p, X)
    indptr, indices, weights, N = _weighted_graph(neighbors(X, n_neighbors=n_neighbors, device=device)[1])
    with _Handle(device) as h:
        return _layout_call(h.lib, h.h, h.check, indptr, indices, weights, N, Y0, p)


def harmony_umap(obj, n_neighbors=15, min_dist=0.5, init="pca", n_components=2, n_epochs=None, spread=1.0, a=None, b=None, gamma=1.0,
                 learning_rate=1.0, negative_sample_rate=5, seed=0):
    """Harmony.umap: the layout of the handle's current Z_corr"""
    X = np.ascontiguousarray(np.asarray(obj.getZcorr()).T)
    p = _Params(X.shape[0], n_components, n_epochs, min_dist, spread, a, b, gamma, learning_rate, negative_sample_rate, seed, None)
    Y0 = _start(init, X.shape[0], p, X)
    indptr, indices, weights, N = _weighted_graph(obj.neighbors(n_neighbors=n_neighbors)[1])
    return _layout_call(obj._lib, obj._h, obj._check, indptr, indices, weights, N, Y0, p)

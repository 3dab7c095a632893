"""The spec of the UMAP layout (include/harmony_mi355x_umap.h) in NumPy fp64: a synchronous, hashed UMAP epoch.

Input: a symmetric CSR (indptr int64, indices int32 ascending within a row, weights float32 in [0, 1], w_ij == w_ji), positions Y [N][dim].
The diagonal is ignored.  wmax = the largest off-diagonal weight; entry e (its position in the CSR, a uint32) has r_e = dbl(w_e) / dbl(wmax)
and fires in epoch n iff floor(dbl(n + 1) r_e) > floor(dbl(n) r_e).  Epoch n reads a snapshot: for cell i, over the fired entries (i, j) of
its row, the sum of
    2 clip(c_a (y_i - y_j)),            c_a = -2ab d2^(b-1) / (a d2^b + 1)                  (d2 > 0, else 0), and for s < negative_sample_rate
    clip(c_r (y_i - y_k)),              c_r = 2 gamma b / ((0.001 + d2) (a d2^b + 1))       (d2 > 0 and k != i, else 0),
    k = (fmix32(e ^ key(n, s)) N) >> 32,  key(n, s) = fmix32(fmix32(seed) + 32 n + s + 1)   (uint32 arithmetic),
clip to [-4, 4] per coordinate; y_i_new = y_i + alpha sum, alpha = float32(learning_rate (1 - n / n_epochs)).

Beside Y the epoch returns the bound B on what a device that evaluates the terms in fp32 may differ by (`bound_constants` has the count of
its rounded operations).  `sequential` is umap-learn's one-thread loop with its own schedule and generator: what the synchronous form is
measured against, not part of the spec.  `trustworthiness` and `knn_purity` are plain NumPy over a dense distance matrix.
"""
import collections
import math

import numpy as np

from louvain_ref import fmix32, fmix32_array

U = 2.0 ** -24                                             # the unit roundoff of fp32
Epoch = collections.namedtuple("Epoch", "Y B fired")

# ---- the bound: the device's expression, operation by operation (relative errors in units of U; 1 ulp = 2 U) -------------------------------
#   d_c = y_i,c - y_o,c                                    1
#   d2 = sum of d_c d_c (dim products, dim - 1 additions of positive numbers)        2 + 1 + (dim - 1) <= 5
#   L = log2f(d2)  (1 ulp)                                 2 |L| absolute, and 5 / ln 2 absolute from d2
#   t = float(b) L                                         1 (b) + 1 (product): 4 |b L| absolute with L's, and 5 b / ln 2
#   pw = exp2f(t)  (1 ulp)                                 2 + ln 2 (4 b |L| + 5 b / ln 2) = 2 + 5 b + 4 ln 2 b |L|
#   den = float(a) pw + 1                                  1 (a) + 1 (product) + 1 (sum), pw's at a factor a pw / (a pw + 1) <= 1
#   attraction c = (float(-2ab) pw) / (d2 den)             1 + 1 | 5 + 3 + 1 | 2 (the quotient, 1 ulp);  pw's error enters once: pw / (a pw + 1)
#   repulsion  c = float(2 gamma b) / ((0.001f + d2) den)  1 | 5 + 1 | 3 + 1 | 2
#   term_c = clip(c d_c) (x 2: exact)                      1 (product) + 1 (d_c); the clip is 1-Lipschitz and |clipped| E bounds both sides of it
#   y_new = y + alpha sum                                  1 (product) on alpha sum, and U |y_new| <= U (|y| + alpha sum |term|)
# which is K0 = 13 + 2 (pw) + 2 (term) + 2 (the update) = 19 for either term, K1 = 5 per unit of b, K2 = 4 ln 2 per unit of b |log2 d2|; every
# addition a term passes through on its way into the sum costs U sum |term|: DEPTH(len) = ceil(len / 64) (1 + negative_sample_rate) lane
# additions, 6 butterfly steps and 2 for the workgroup's tree.
K0, K1, K2 = 19.0, 5.0, 4.0 * math.log(2.0)


def bound_constants():
    return K0, K1, K2


def depth(lengths, negative_sample_rate):
    return np.ceil(np.asarray(lengths, dtype=np.float64) / 64.0) * (1 + negative_sample_rate) + 8.0


def key(n, s, seed):
    return fmix32(fmix32(seed) + 32 * n + s + 1)


def negative_sample(e, n, s, N, seed):
    """the cell that entry e samples in epoch n, draw s"""
    return (fmix32(e ^ key(n, s, seed)) * N) >> 32


def edges(indptr, indices, weights):
    """-> (src, dst, r, offdiag, wmax): one element per stored entry, in CSR order"""
    indptr, dst = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    N = indptr.size - 1
    src = np.repeat(np.arange(N, dtype=np.int64), np.diff(indptr))
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)
    off = src != dst
    wmax = float(w[off].max()) if off.any() else 0.0
    r = w / np.float64(wmax) if wmax > 0.0 else np.zeros_like(w)
    return src, dst, r, off, wmax


def fires(r, n):
    n = np.float64(n)
    return np.floor((n + 1.0) * r) > np.floor(n * r)


def firings(r, n_epochs):
    """how often an entry fires over the whole schedule"""
    return sum(fires(r, n).astype(np.int64) for n in range(n_epochs))


def alpha_of(n, n_epochs, learning_rate):
    return float(np.float32(learning_rate * (1.0 - n / n_epochs)))


def _terms(Y, i, o, a, b, coef_of, live):
    """clip(c (y_i - y_o)) per coordinate, |log2 d2| (0 where the term is 0)"""
    diff = Y[i] - Y[o]
    d2 = (diff * diff).sum(axis=1)
    ok = (d2 > 0.0) & live
    d2s = np.where(ok, d2, 1.0)
    pw = d2s ** b
    c = np.where(ok, coef_of(d2s, pw), 0.0)
    return np.clip(c[:, None] * diff, -4.0, 4.0), np.where(ok, np.abs(np.log2(d2s)), 0.0)


def epoch(graph, Y, n, n_epochs, a, b, gamma=1.0, learning_rate=1.0, negative_sample_rate=5, seed=0, _edges=None):
    """one epoch from the snapshot Y (any float dtype; computed in fp64) -> Epoch(Y_new, B, fired entries)"""
    indptr = np.asarray(graph[0], dtype=np.int64)
    Y = np.asarray(Y, dtype=np.float64)
    N, dim = Y.shape
    src, dst, r, off, wmax = _edges if _edges is not None else edges(*graph)
    if wmax == 0.0:
        return Epoch(Y.copy(), 2.0 * U * np.abs(Y), 0)
    alpha = alpha_of(n, n_epochs, learning_rate)
    f = np.nonzero(fires(r, n) & off)[0]
    i, j = src[f], dst[f]
    total, weight = np.zeros((N, dim)), np.zeros((N, dim))   # the sum, and the sum of |term| (K0 + K1 b + K2 b |log2 d2|)

    def add(t, l2):
        np.add.at(total, i, t)
        np.add.at(weight, i, np.abs(t) * (K0 + K1 * b + K2 * b * l2)[:, None])

    t, l2 = _terms(Y, i, j, a, b, lambda d2, pw: -2.0 * a * b * (pw / d2) / (a * pw + 1.0), np.ones(f.size, dtype=bool))
    add(2.0 * t, l2)
    abs_sum = np.zeros((N, dim))
    np.add.at(abs_sum, i, np.abs(2.0 * t))
    for s in range(negative_sample_rate):
        k = ((fmix32_array(f.astype(np.uint64) ^ np.uint64(key(n, s, seed))) * np.uint64(N)) >> np.uint64(32)).astype(np.int64)
        t, l2 = _terms(Y, i, k, a, b, lambda d2, pw: 2.0 * gamma * b / ((0.001 + d2) * (a * pw + 1.0)), k != i)
        add(t, l2)
        np.add.at(abs_sum, i, np.abs(t))
    B = alpha * U * (weight + depth(np.diff(indptr), negative_sample_rate)[:, None] * abs_sum) + 2.0 * U * np.abs(Y)
    return Epoch(Y + alpha * total, B, int(f.size))


def layout(graph, Y0, n_epochs, a, b, gamma=1.0, learning_rate=1.0, negative_sample_rate=5, seed=0, epochs=None, snapshots=()):
    """epochs [begin, end) of the schedule from Y0, positions kept in fp64 -> (Y, directed firings, {n: the positions epoch n starts from})"""
    begin, end = (0, n_epochs) if epochs is None else epochs
    Y = np.asarray(Y0, dtype=np.float64).copy()
    E = edges(*graph)
    fired, snap = 0, {}
    for n in range(begin, end):
        if n in snapshots:
            snap[n] = Y.copy()
        step = epoch(graph, Y, n, n_epochs, a, b, gamma, learning_rate, negative_sample_rate, seed, _edges=E)
        Y, fired = step.Y, fired + step.fired
    return Y, fired, snap


# ---- umap-learn's loop on one thread: the quality bar's other side ---------------------------------------------------------------------------
def sequential(graph, Y0, n_epochs, a, b, gamma=1.0, learning_rate=1.0, negative_sample_rate=5, seed=0):
    """optimize_layout_euclidean as umap-learn runs it without numba's threads: every stored entry in order, applied at once to the positions
    the entries before it left (move_other: both ends move), epochs_per_sample = wmax / w, negative samples from a generator"""
    src, dst, r, off, wmax = edges(*graph)
    Y = [list(map(float, row)) for row in np.asarray(Y0, dtype=np.float64)]
    N, dim = len(Y), len(Y[0])
    keep = np.nonzero(off & (r >= 1.0 / n_epochs))[0]
    head, tail = src[keep].tolist(), dst[keep].tolist()
    eps = (1.0 / r[keep]).tolist()
    eps_neg = [x / negative_sample_rate if negative_sample_rate else float("inf") for x in eps]
    nxt, nxt_neg = list(eps), list(eps_neg)
    rng = np.random.RandomState(seed)

    def clip(v):
        return 4.0 if v > 4.0 else -4.0 if v < -4.0 else v

    for n in range(n_epochs):
        alpha = learning_rate * (1.0 - n / n_epochs)
        draws = rng.randint(0, N, size=(len(head), negative_sample_rate + 1)).tolist() if negative_sample_rate else None
        for e in range(len(head)):
            if nxt[e] > n + 1:                               # (umap-learn counts epochs from 1)
                continue
            cur, oth = Y[head[e]], Y[tail[e]]
            d2 = sum((cur[c] - oth[c]) ** 2 for c in range(dim))
            if d2 > 0.0:
                coef = -2.0 * a * b * d2 ** (b - 1.0) / (a * d2 ** b + 1.0)
                for c in range(dim):
                    g = clip(coef * (cur[c] - oth[c]))
                    cur[c] += g * alpha
                    oth[c] -= g * alpha
            nxt[e] += eps[e]
            if negative_sample_rate:
                n_neg = min(int((n + 1 - nxt_neg[e]) / eps_neg[e]), negative_sample_rate)
                for p in range(max(n_neg, 0)):
                    k = draws[e][p]
                    if k == head[e]:
                        continue
                    oth = Y[k]
                    d2 = sum((cur[c] - oth[c]) ** 2 for c in range(dim))
                    if d2 > 0.0:
                        coef = 2.0 * gamma * b / ((0.001 + d2) * (a * d2 ** b + 1.0))
                        for c in range(dim):
                            cur[c] += clip(coef * (cur[c] - oth[c])) * alpha
                nxt_neg[e] += max(n_neg, 0) * eps_neg[e]
    return np.array(Y)


# ---- quality in plain NumPy -------------------------------------------------------------------------------------------------------------------
def _sqdist(X):
    X = np.asarray(X, dtype=np.float64)
    n = (X * X).sum(axis=1)
    D = n[:, None] + n[None, :] - 2.0 * (X @ X.T)
    np.fill_diagonal(D, -1.0)                                # the cell itself ranks first
    return D


def trustworthiness(X, Y, k=15):
    """Venna and Kaski's trustworthiness of the embedding Y of X: 1 - 2 / (N k (2N - 3k - 1)) sum_i sum_{j in the k nearest of i in Y, not in
    X} (rank of j from i in X - k); ranks from dense distance matrices, ties by index"""
    N = len(X)
    order = np.argsort(_sqdist(X), axis=1, kind="stable")   # column 0: the cell itself
    rank = np.empty((N, N), dtype=np.int64)
    rank[np.arange(N)[:, None], order] = np.arange(N)[None, :]
    near = np.argsort(_sqdist(Y), axis=1, kind="stable")[:, 1:k + 1]
    excess = rank[np.arange(N)[:, None], near] - k
    return 1.0 - 2.0 / (N * k * (2.0 * N - 3.0 * k - 1.0)) * float(excess[excess > 0].sum())


def knn_purity(Y, labels, k=15):
    """the share of a cell's k nearest neighbours in Y that carry its label, averaged over the cells"""
    labels = np.asarray(labels)
    near = np.argsort(_sqdist(Y), axis=1, kind="stable")[:, 1:k + 1]
    return float((labels[near] == labels[:, None]).mean())


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
def find_ab(min_dist):
    """the two curve fits the tests use (harmony_amd.umap.find_ab_params reproduces them to 1e-3)"""
    return {0.5: (0.583, 1.334), 0.1: (1.577, 0.895)}[min_dist]


def pca_init(X, dim):
    """the top `dim` principal axes of X from the d x d covariance, each signed so that its largest loading is positive, scaled to a largest
    |coordinate| of 10, as float32"""
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(axis=0)
    vals, vecs = np.linalg.eigh(Xc.T @ Xc / max(len(X) - 1, 1))
    axes = vecs[:, np.argsort(-vals, kind="stable")[:dim]]
    axes = axes * np.where(axes[np.abs(axes).argmax(axis=0), np.arange(axes.shape[1])] < 0.0, -1.0, 1.0)
    P = Xc @ axes
    top = np.abs(P).max()
    return (P * (10.0 / top if top > 0.0 else 1.0)).astype(np.float32)


def random_init(N, dim, seed):
    i = np.arange(N * dim, dtype=np.uint64)
    h = fmix32_array(i ^ np.uint64(fmix32(seed + 0x51ED))).astype(np.float64)
    return (20.0 * (h + 0.5) / 2.0 ** 32 - 10.0).astype(np.float32).reshape(N, dim)


def groups(N, G, d=10, seed=0):
    """planted Gaussian groups: (X float32, labels)"""
    rng = np.random.default_rng(seed)
    lab = np.arange(N) % G
    centres = rng.normal(size=(G, d)) * 6.0
    return (centres[lab] + rng.normal(size=(N, d))).astype(np.float32), lab


def swiss_roll(N, seed=0):
    rng = np.random.default_rng(seed)
    t = 1.5 * np.pi * (1.0 + 2.0 * rng.random(N))
    return np.stack([t * np.cos(t), 21.0 * rng.random(N), t * np.sin(t)], axis=1).astype(np.float32)


def noise(N, d=10, seed=0):
    return np.random.default_rng(seed).normal(size=(N, d)).astype(np.float32)

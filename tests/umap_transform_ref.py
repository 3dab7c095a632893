"""The spec of the projection of query cells into a fitted UMAP layout (include/harmony_mi355x_umap_transform.h) in NumPy fp64.

Input: lists idx [Nq][k] of reference cells ascending by distance with their distances (no self column), the reference's positions Yref.
    weights   rho = 0; sigma by the neighbour graph's bisection over psum = sum_{j >= 1} (d_j > 0 ? exp(-d_j / mid) : 1) -- the list's first
              entry is left out, as umap-learn's smooth_knn_dist leaves out column 0 --, target log2 k, sigma = max(mid, 1e-3 mean of all d);
              w_j = (d_j <= 0 or sigma == 0) ? 1 : exp(-d_j / sigma) for all k entries, rounded to float32 once.
    start     y_i = sum_j w_ij yref_j / sum_j w_ij in the list's order; the plain mean of the listed positions where every weight is 0.
    firing    entry e = i k + j has r_e = dbl(w_e) / dbl(wmax), wmax the largest weight of the call, and fires in epoch n iff
              floor(dbl(n + 1) r_e) > floor(dbl(n) r_e)                                         (umap_ref.fires).
    epoch n   of cell i from y_i as the epoch found it: over the fired entries the sum of
                  clip(c_a (y_i - yref_j)),     c_a = -2ab d2^(b-1) / (a d2^b + 1)              (d2 > 0, else 0), and for s < negative_sample_rate
                  clip(c_r (y_i - yref_m)),     c_r = 2 gamma b / ((0.001 + d2) (a d2^b + 1))   (d2 > 0, else 0),
                  m = (fmix32(e ^ key(n, s)) Nr) >> 32                                          (umap_ref.key),
              clip to [-4, 4] per coordinate; y_i += alpha sum, alpha = float32(alpha0 (1 - n / n_epochs)) (umap_ref.alpha_of).  No factor 2 on
              the attraction and no "m != i" rule: a query cell moves alone and is not in the reference.

Beside Y the epoch returns the bound B on what a device that evaluates the terms in fp32 may differ by: the layout's constants K0, K1, K2
(umap_ref: the expressions are the same ones) and DEPTH = ceil(k / G) (1 + negative_sample_rate) + log2 G additions a term passes through on its
way into the sum, counted from the kernel as written: a lane adds its ceil(k / G) entries' terms one after the other, then log2 G butterfly
steps, with G = 16 lanes per cell for k <= 16 and 64 above.  `sequential` is umap-learn's optimize_layout_euclidean(move_other=False) on one
thread with its own schedule and a NumPy generator: what the synchronous form is measured against, not part of the spec.
"""
import math

import numpy as np

from louvain_ref import fmix32_array
from umap_ref import K0, K1, K2, U, Epoch, alpha_of, fires, key

MAX_STEPS = 64


def group_lanes(k):
    return 16 if k <= 16 else 64


def depth(k, negative_sample_rate):
    G = group_lanes(k)
    return math.ceil(k / G) * (1 + negative_sample_rate) + math.log2(G)


# ---- the weights ------------------------------------------------------------------------------------------------------------------------------
def search(dist):
    """-> (mid [Nq], the steps every row took, the rows that did not stop within MAX_STEPS)"""
    d = np.asarray(dist, dtype=np.float32).astype(np.float64)
    Nq, k = d.shape
    target = np.log2(np.float64(k))
    lo, hi, mid = np.zeros(Nq), np.full(Nq, np.inf), np.ones(Nq)
    done, steps = np.zeros(Nq, dtype=bool), np.zeros(Nq, dtype=np.int64)
    rest = d[:, 1:]
    for _ in range(MAX_STEPS):
        with np.errstate(over="ignore", divide="ignore"):
            psum = np.where(rest > 0.0, np.exp(-rest / mid[:, None]), 1.0).sum(axis=1)
        done |= np.abs(psum - target) < 1e-5
        if done.all():
            break
        go = ~done
        steps[go] += 1
        up = go & (psum > target)
        down = go & ~(psum > target)
        hi[up] = mid[up]
        mid[up] = (lo[up] + hi[up]) / 2.0
        lo[down] = mid[down]
        mid[down] = np.where(np.isinf(hi[down]), mid[down] * 2.0, (lo[down] + hi[down]) / 2.0)
    return mid, steps, ~done


def query_weights(idx, dist):
    """-> (weights float32 [Nq][k], sigma float64 [Nq])"""
    d = np.asarray(dist, dtype=np.float32).astype(np.float64)
    mid = search(dist)[0]
    sigma = np.maximum(mid, 1e-3 * (d.sum() / d.size))
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where((d <= 0.0) | (sigma[:, None] == 0.0), 1.0, np.exp(-d / sigma[:, None]))
    return w.astype(np.float32), sigma


# ---- the start --------------------------------------------------------------------------------------------------------------------------------
def init(idx, weights, Yref):
    """the weighted mean of the listed positions, entry by entry in fp64; the plain mean where every weight of the row is 0"""
    idx = np.asarray(idx, dtype=np.int64)
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)
    Yref = np.asarray(Yref, dtype=np.float64)
    Nq, k = idx.shape
    sw, sy, sm = np.zeros(Nq), np.zeros((Nq, Yref.shape[1])), np.zeros((Nq, Yref.shape[1]))
    for t in range(k):
        sw += w[:, t]
        sy += w[:, t, None] * Yref[idx[:, t]]
        sm += Yref[idx[:, t]]
    none = ~(sw > 0.0)
    return np.where(none[:, None], sm / k, sy / np.where(none, 1.0, sw)[:, None])


# ---- one epoch --------------------------------------------------------------------------------------------------------------------------------
def rates(weights, wmax=None):
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)
    wmax = float(w.max()) if wmax is None else float(wmax)
    return (w / np.float64(wmax) if wmax > 0.0 else np.zeros_like(w)), wmax


def _terms(diff, b, coef_of):
    d2 = (diff * diff).sum(axis=1)
    ok = d2 > 0.0
    d2s = np.where(ok, d2, 1.0)
    pw = d2s ** b
    c = np.where(ok, coef_of(d2s, pw), 0.0)
    return np.clip(c[:, None] * diff, -4.0, 4.0), np.where(ok, np.abs(np.log2(d2s)), 0.0)


def epoch(idx, weights, Yref, Y, n, n_epochs, a, b, gamma=1.0, alpha0=0.25, negative_sample_rate=5, seed=0, wmax=None):
    """one epoch from the positions Y (any float dtype; computed in fp64) -> Epoch(Y_new, B, fired entries)"""
    idx = np.asarray(idx, dtype=np.int64)
    Yref, Y = np.asarray(Yref, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    Nq, k = idx.shape
    Nr, dim = Yref.shape
    r, wmax = rates(weights, wmax)
    if wmax == 0.0:
        return Epoch(Y.copy(), 2.0 * U * np.abs(Y), 0)
    alpha = alpha_of(n, n_epochs, alpha0)
    i, j = np.nonzero(fires(r, n))
    e = (i * k + j).astype(np.uint64)
    total, weight, abs_sum = np.zeros((Nq, dim)), np.zeros((Nq, dim)), np.zeros((Nq, dim))

    def add(t, l2):
        np.add.at(total, i, t)
        np.add.at(weight, i, np.abs(t) * (K0 + K1 * b + K2 * b * l2)[:, None])
        np.add.at(abs_sum, i, np.abs(t))

    add(*_terms(Y[i] - Yref[idx[i, j]], b, lambda d2, pw: -2.0 * a * b * (pw / d2) / (a * pw + 1.0)))
    for s in range(negative_sample_rate):
        m = ((fmix32_array(e ^ np.uint64(key(n, s, seed))) * np.uint64(Nr)) >> np.uint64(32)).astype(np.int64)
        add(*_terms(Y[i] - Yref[m], b, lambda d2, pw: 2.0 * gamma * b / ((0.001 + d2) * (a * pw + 1.0))))
    B = alpha * U * (weight + depth(k, negative_sample_rate) * abs_sum) + 2.0 * U * np.abs(Y)
    return Epoch(Y + alpha * total, B, int(i.size))


def transform(idx, weights, Yref, n_epochs, a, b, gamma=1.0, alpha0=0.25, negative_sample_rate=5, seed=0, Y0=None, epochs=None, snapshots=()):
    """epochs [begin, end) of the schedule from Y0 (None: `init`), positions kept in fp64 -> (Y, firings, {n: the positions epoch n starts from})"""
    begin, end = (0, n_epochs) if epochs is None else epochs
    Y = init(idx, weights, Yref) if Y0 is None else np.asarray(Y0, dtype=np.float64).copy()
    wmax = rates(weights)[1]
    fired, snap = 0, {}
    for n in range(begin, end):
        if n in snapshots:
            snap[n] = Y.copy()
        step = epoch(idx, weights, Yref, Y, n, n_epochs, a, b, gamma, alpha0, negative_sample_rate, seed, wmax=wmax)
        Y, fired = step.Y, fired + step.fired
    return Y, fired, snap


# ---- umap-learn's loop on one thread: the quality bar's other side ---------------------------------------------------------------------------
def sequential(idx, weights, Yref, Y0, n_epochs, a, b, gamma=1.0, alpha0=0.25, negative_sample_rate=5, seed=0):
    """optimize_layout_euclidean(move_other=False) as umap-learn's transform runs it without numba's threads: every kept entry in order,
    applied at once to the query cell's position; entries below wmax / n_epochs dropped, epochs_per_sample = wmax / w, negative samples from
    a generator (a draw whose index equals the query cell's is skipped, as that loop does)"""
    idx = np.asarray(idx, dtype=np.int64)
    Nq, k = idx.shape
    r = rates(weights)[0].ravel()
    ref = [list(map(float, row)) for row in np.asarray(Yref, dtype=np.float64)]
    Y = [list(map(float, row)) for row in np.asarray(Y0, dtype=np.float64)]
    Nr, dim = len(ref), len(ref[0])
    keep = np.nonzero(r >= 1.0 / n_epochs)[0]
    head, tail = (keep // k).tolist(), idx.ravel()[keep].tolist()
    eps = (1.0 / r[keep]).tolist()
    eps_neg = [x / negative_sample_rate if negative_sample_rate else float("inf") for x in eps]
    nxt, nxt_neg = list(eps), list(eps_neg)
    rng = np.random.RandomState(seed)

    def clip(v):
        return 4.0 if v > 4.0 else -4.0 if v < -4.0 else v

    for n in range(n_epochs):
        alpha = alpha0 * (1.0 - n / n_epochs)
        draws = rng.randint(0, Nr, size=(len(head), negative_sample_rate + 1)).tolist() if negative_sample_rate else None
        for e in range(len(head)):
            if nxt[e] > n + 1:                               # (umap-learn counts epochs from 1)
                continue
            cur, oth = Y[head[e]], ref[tail[e]]
            d2 = sum((cur[c] - oth[c]) ** 2 for c in range(dim))
            if d2 > 0.0:
                coef = -2.0 * a * b * d2 ** (b - 1.0) / (a * d2 ** b + 1.0)
                for c in range(dim):
                    cur[c] += clip(coef * (cur[c] - oth[c])) * alpha
            nxt[e] += eps[e]
            if negative_sample_rate:
                n_neg = min(int((n + 1 - nxt_neg[e]) / eps_neg[e]), negative_sample_rate)
                for p in range(max(n_neg, 0)):
                    m = draws[e][p]
                    if m == head[e]:
                        continue
                    oth = ref[m]
                    d2 = sum((cur[c] - oth[c]) ** 2 for c in range(dim))
                    if d2 > 0.0:
                        coef = 2.0 * gamma * b / ((0.001 + d2) * (a * d2 ** b + 1.0))
                        for c in range(dim):
                            cur[c] += clip(coef * (cur[c] - oth[c])) * alpha
                nxt_neg[e] += max(n_neg, 0) * eps_neg[e]
    return np.array(Y)


# ---- what the tests measure -------------------------------------------------------------------------------------------------------------------
def spread_to_neighbours(Y, idx, Yref):
    """D: the mean layout distance from a query cell to its k listed reference cells"""
    diff = np.asarray(Y, dtype=np.float64)[:, None, :] - np.asarray(Yref, dtype=np.float64)[np.asarray(idx, dtype=np.int64)]
    return float(np.sqrt((diff * diff).sum(axis=2)).mean())


def vote(Y, Yref, ref_labels, k=15):
    """the majority label among the k reference cells nearest to a query cell in the layout (ties to the smallest label)"""
    Y, Yref = np.asarray(Y, dtype=np.float64), np.asarray(Yref, dtype=np.float64)
    d = ((Y * Y).sum(axis=1)[:, None] + (Yref * Yref).sum(axis=1)[None, :]) - 2.0 * (Y @ Yref.T)
    near = np.argsort(d, axis=1, kind="stable")[:, :k]
    lab = np.asarray(ref_labels)[near]
    return np.array([np.bincount(row).argmax() for row in lab])


def problem(N, Nq, G, k, seed=0):
    """planted groups split into a reference and a query: (Xref, lab_ref, Xq, lab_q, idx int32, dist float32): the query's k nearest
    reference cells by exact search in fp64, ties to the smaller index"""
    from umap_ref import groups
    X, lab = groups(N, G, seed=seed)
    Xr, Xq = X[:N - Nq].astype(np.float64), X[N - Nq:].astype(np.float64)
    d2 = ((Xq * Xq).sum(axis=1)[:, None] + (Xr * Xr).sum(axis=1)[None, :]) - 2.0 * (Xq @ Xr.T)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    dist = np.sqrt(np.maximum(np.take_along_axis(d2, idx, axis=1), 0.0))
    return X[:N - Nq], lab[:N - Nq], X[N - Nq:], lab[N - Nq:], idx.astype(np.int32), dist.astype(np.float32)

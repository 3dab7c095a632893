"""kmeans_centers (the reference's src/utils.cpp:10-64, as oracle/harmony_oracle.cpp::kmeans_centers walks it) in plain numpy fp64, with the margins that
say whether an fp32 implementation must reach the same discrete decisions.  Not a test module.

  anchors   cell floor(u01(seed, 0, i) * float(N - 1)) for cluster i (the product is the fp32 one: it IS the index)
  race      cluster i takes the cell n with the smallest -log(u01(seed, 1 + i, n)) / |2 (1 - y_i . x_n)|, y_i its anchor's row; a cell an earlier cluster
            took is passed over (its value raised to the largest, the smallest taken again)
  Lloyd     ten iterations: every cell goes to the first smallest |y_k|^2 - 2 y_k . x_n, a centre becomes the mean of its cells, an empty cluster keeps its centre

The uniforms are the documented counter generator (include/harmony_mi355x.h), vectorised here and held to the oracle's orc_u01 by tests/test_kmeans_ref_cpu.py.
Rounding bound of one fp32 score against its exact value: e(x, y) = (2 d + 4) 2^-24 (|x|^2 + |y|^2), the form tests/test_gpu_metrics.py uses for |x - y|^2
(2 (1 - y . x) of the race and |y|^2 - 2 y . x of Lloyd are that quantity less |x|^2 (+ |y|^2): the same products and sums).  The race divides by it: a
candidate's value L / D moves by at most (L / D) (e / D + 4 * 2^-24) to first order (4 ulps for logf and the division)."""
import numpy as np

U24 = 2.0 ** -24
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15)) & M64
    x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & M64
    x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & M64
    return x ^ (x >> np.uint64(31))


def u01(seed, stream, idx):
    """the generator's uniforms in (0, 1) for an array of indices, as float32"""
    with np.errstate(over="ignore"):
        idx = np.asarray(idx, dtype=np.uint64)
        key = np.uint64(seed) ^ (np.uint64(stream) * np.uint64(0xD1342543DE82EF95))
        h = _splitmix64(_splitmix64(np.asarray(key, dtype=np.uint64)) + idx)
    return ((h >> np.uint64(40)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def _race_clearance(L, D, e, Lw, Dw, ew, cap=64.0):
    """the largest f <= cap for which the winner stays in front when every candidate's denominator moves by f times its bound and the quotient by 4 f ulps: the
    others as low as they can get, L / (D + f e) (1 - 4 f u), the winner as high, Lw / (Dw - f ew) (1 + 4 f u).  (Not linearised: a candidate whose D is of the
    size of e -- the anchor's own cell and its near-duplicates -- can come down to L / e.)"""
    def holds(f):
        if Dw <= f * ew:
            return False
        return bool((L / (D + f * e) * (1 - 4 * f * U24)).min() >= Lw / (Dw - f * ew) * (1 + 4 * f * U24))
    if holds(cap):
        return cap
    lo, hi = 0.0, cap
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if holds(mid) else (lo, mid)
    return lo


def kmeans_centers(X, K, seed, iters=10):
    """X: N x d rows (the handle's cosine-normalised fp32 cells, as float64).  Returns a dict:
    seed_cells [K]; centers K x d (not normalised); anchors [K];
    race_gap [K]: (second smallest - smallest) / smallest of the candidates the cluster chose among; race_bound [K]: the rounding bound of that quotient;
    race_clear [K]: how many times their bounds the winner and any other candidate may move before they meet (capped at 64) -- >= 2 is clear;
    lloyd_gap [iters], lloyd_bound [iters], lloyd_clear [iters]: the same for the cell whose two best scores lie closest in units of their bounds;
    empty: clusters that were empty in some iteration; last_centers, last_assign, last_second: the centres the last iteration started from, every cell's
    centre in it and its second-best one (centers_after rebuilds the result from them)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    N, d = X.shape
    n2 = np.einsum("nd,nd->n", X, X)
    anchors = np.floor(u01(seed, 0, np.arange(K)) * np.float32(N - 1)).astype(np.int64)
    taken = np.zeros(N, dtype=bool)
    seed_cells = np.empty(K, dtype=np.int64)
    race_gap, race_bound, race_clear = np.empty(K), np.empty(K), np.empty(K)
    cells = np.arange(N)
    for i in range(K):
        y = X[anchors[i]]
        dis = np.abs(2.0 * (1.0 - X @ y))
        L = -np.log(u01(seed, 1 + i, cells).astype(np.float64))
        e = (2 * d + 4) * U24 * (n2 + n2[anchors[i]])
        with np.errstate(divide="ignore"):
            prob = L / dis
            err = prob * (e / dis + 4 * U24)
        prob[np.isnan(prob)] = np.inf
        err[~np.isfinite(err)] = 0.0            # (the anchor's own cell: an infinite value never wins)
        p = prob.copy()
        best = int(np.argmin(p))
        while taken[best]:
            p[best] = p.max()
            best = int(np.argmin(p))
        cand = ~taken
        cand[best] = False
        others, oerr = prob[cand], err[cand]
        j = int(np.argmin(others))
        with np.errstate(divide="ignore", invalid="ignore"):      # (a uniform that rounds to 1.0f gives the value 0: it wins by any margin)
            race_gap[i] = (others[j] - prob[best]) / prob[best]
            race_bound[i] = (oerr[j] + err[best]) / prob[best]
        race_clear[i] = _race_clearance(L[cand], dis[cand], e[cand], L[best], dis[best], e[best])
        taken[best] = True
        seed_cells[i] = best
    Y = X[seed_cells].copy()
    lloyd_gap, lloyd_bound, lloyd_clear = np.empty(iters), np.empty(iters), np.empty(iters)
    empty = set()
    for it in range(iters):
        y2 = np.einsum("kd,kd->k", Y, Y)
        S = y2[None, :] - 2.0 * (X @ Y.T)
        if K > 1:
            two = np.argpartition(S, 1, axis=1)[:, :2]
            s2 = np.take_along_axis(S, two, axis=1)
            lo, hi = s2.min(axis=1), s2.max(axis=1)
            e = (2 * d + 4) * U24 * (2 * n2 + np.take_along_axis(np.broadcast_to(y2, S.shape), two, axis=1).sum(axis=1))
            w = int(np.argmin((hi - lo) / e))
            lloyd_gap[it], lloyd_bound[it], lloyd_clear[it] = hi[w] - lo[w], e[w], (hi[w] - lo[w]) / e[w]
        else:
            lloyd_gap[it], lloyd_bound[it], lloyd_clear[it] = np.inf, 0.0, np.inf
        a = np.argmin(S, axis=1)
        if it == iters - 1:
            Y_before, second = Y.copy(), np.argsort(S, axis=1)[:, 1] if K > 1 else a
        cnt = np.bincount(a, minlength=K)
        sums = np.zeros((K, d))
        np.add.at(sums, a, X)
        full = cnt > 0
        Y[full] = sums[full] / cnt[full, None]
        empty |= set(np.where(~full)[0].tolist())
    return dict(seed_cells=seed_cells, centers=Y, anchors=anchors, race_gap=race_gap, race_bound=race_bound, race_clear=race_clear,
                lloyd_gap=lloyd_gap, lloyd_bound=lloyd_bound, lloyd_clear=lloyd_clear, empty=sorted(empty),
                last_centers=Y_before, last_assign=a, last_second=second)


def is_clear(s):
    """every discrete decision of the run lies at least twice its rounding bound away from the next one"""
    return bool(s["race_clear"].min() >= 2.0 and s["lloyd_clear"].min() >= 2.0)


def normalised(Y):
    """K x d centres with unit rows"""
    return Y / np.linalg.norm(Y, axis=1, keepdims=True)


def centers_after(X, s, assign):
    """the centres the last iteration ends on when its cells go to `assign` instead of s["last_assign"]"""
    X = np.asarray(X, dtype=np.float64)
    Y = s["last_centers"].copy()
    cnt = np.bincount(assign, minlength=Y.shape[0])
    sums = np.zeros_like(Y)
    np.add.at(sums, assign, X)
    Y[cnt > 0] = sums[cnt > 0] / cnt[cnt > 0, None]
    return Y

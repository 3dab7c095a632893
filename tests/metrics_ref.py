"""The fp64 spec of the integration metrics (harmony_amd/metrics.py): exact brute-force k nearest neighbours and LISI, the local inverse
Simpson's index of the Harmony paper (immunogenomics/LISI, compute_lisi), restated in NumPy.  The spec reads fp32-rounded inputs, as the
device does, and computes everything else in float64."""
import numpy as np


def as_f32_f64(X):
    """the fp32 rounding of X, held in float64"""
    return np.ascontiguousarray(X, dtype=np.float32).astype(np.float64)


def sqdist_block(Q, X):
    """direct sum (q - x)^2 of every row of Q (b x d) against every row of X (N x d), float64, PC by PC (no b x N x d temporary)"""
    D = np.zeros((Q.shape[0], X.shape[0]))
    for j in range(X.shape[1]):
        t = Q[:, j:j + 1] - X[None, :, j]
        D += t * t
    return D


def knn(X, k, Q=None, extra=0, block=512):
    """Exact kNN of the rows of Q (None: the rows of X, self excluded by index) among the rows of X: (idx, d2), each Nq x (k + extra),
    sorted ascending by (d2, index) with a stable sort.  `extra` more neighbours serve the tests' gap rule."""
    X = as_f32_f64(X)
    self_excl = Q is None
    Q = X if self_excl else as_f32_f64(Q)
    kk = k + extra
    N = X.shape[0]
    idx = np.empty((Q.shape[0], kk), dtype=np.int64)
    d2 = np.empty((Q.shape[0], kk))
    n2x = (X * X).sum(axis=1)
    pad = min(N, kk + 32)
    for s in range(0, Q.shape[0], block):
        Qb = Q[s:s + block]
        r = np.arange(Qb.shape[0])
        # Preselection only (never a result): the fp64 GEMM form is within 1e-12 (|q|^2 + |x|^2) of the direct sum, so every row whose
        # (kk)-th and (pad)-th preselected distances are further apart than that holds its kk nearest among the `pad` preselected ones;
        # the other rows (long tie runs) take the direct sum against all of X.
        n2q = (Qb * Qb).sum(axis=1)
        G = n2q[:, None] + n2x[None, :] - 2.0 * (Qb @ X.T)
        if self_excl:
            G[r, s + r] = np.inf
        if pad < N:
            part = np.argpartition(G, (kk - 1, pad - 1), axis=1)[:, :pad]
            g = np.take_along_axis(G, part, axis=1)
            safe = g[:, pad - 1] - g[:, :kk].max(axis=1) > 1e-11 * (n2q + n2x.max())
        else:
            part = np.broadcast_to(np.arange(N), (Qb.shape[0], N))
            safe = np.ones(Qb.shape[0], bool)
        part = np.sort(part, axis=1)                                   # ascending index: the stable sort below then breaks ties by index
        D = np.zeros(part.shape)
        for j in range(X.shape[1]):
            t = Qb[:, j:j + 1] - X[part, j]
            D += t * t
        if self_excl:
            D[part == (s + r)[:, None]] = np.inf
        o = np.argsort(D, axis=1, kind="stable")[:, :kk]
        idx[s:s + block] = np.take_along_axis(part, o, axis=1)
        d2[s:s + block] = np.take_along_axis(D, o, axis=1)
        for i in np.nonzero(~safe)[0]:
            Di = sqdist_block(Qb[i:i + 1], X)[0]
            if self_excl:
                Di[s + i] = np.inf
            oi = np.argsort(Di, kind="stable")[:kk]
            idx[s + i], d2[s + i] = oi, Di[oi]
    return idx, d2


def hbeta(D, beta):
    P = np.exp(-D * beta)
    S = P.sum()
    if S == 0:
        return 0.0, np.zeros_like(P)
    H = np.log(S) + beta * np.sum(D * P) / S
    return H, P / S


def lisi_row(D, labels, perplexity, tol=1e-5):
    """One cell: D (m,) Euclidean distances to its neighbours, labels (n_cols, m) their codes -> (n_cols,) LISI."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        logU = np.log(perplexity)
        beta, bmin, bmax = 1.0, -np.inf, np.inf
        H, P = hbeta(D, beta)
        tries = 0
        while abs(H - logU) > tol and tries < 50:
            if H - logU > 0:
                bmin = beta
                beta = beta * 2 if np.isinf(bmax) else (beta + bmax) / 2
            else:
                bmax = beta
                beta = beta / 2 if np.isinf(bmin) else (beta + bmin) / 2
            H, P = hbeta(D, beta)
            tries += 1
    if H == 0:
        return np.full(labels.shape[0], -1.0)
    return np.array([1.0 / np.sum(np.bincount(lab, weights=P) ** 2) for lab in labels])


def lisi_from_knn(idx, dist, label_codes, perplexity):
    """idx, dist: Nq x m neighbour lists (dist Euclidean, read as fp32); label_codes: (n_cols, N) integer codes -> Nq x n_cols"""
    idx = np.asarray(idx)
    dist = as_f32_f64(dist)
    label_codes = np.atleast_2d(np.asarray(label_codes))
    out = np.empty((idx.shape[0], label_codes.shape[0]))
    for i in range(idx.shape[0]):
        out[i] = lisi_row(dist[i], label_codes[:, idx[i]], perplexity)
    return out


def compute_lisi(X, label_codes, perplexity=30):
    """LISI of every row of X over each label column, from the m = 3 perplexity - 1 nearest neighbours with self excluded"""
    m = int(3 * perplexity) - 1
    idx, d2 = knn(X, m)
    return lisi_from_knn(idx, np.sqrt(d2), label_codes, perplexity)


def knn_predict(idx, ref_codes, n_levels):
    """majority vote over the neighbours' codes, ties to the smallest code: (codes, share)"""
    votes = np.stack([np.bincount(r, minlength=n_levels) for r in np.asarray(ref_codes)[np.asarray(idx)]])
    win = votes.argmax(axis=1)
    return win, votes[np.arange(len(win)), win] / float(idx.shape[1])

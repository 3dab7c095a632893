"""NumPy fp64 restatement of the query mapping (DESIGN "Query mapping"; Symphony's mapQuery, Kang et al. 2021): the oracle of the GPU tests.
Not a test module."""
import numpy as np


def reference_summary(R, Zcorr):
    """R: K x N, Z_corr: d x N -> (Nr (K,), C (K x d))"""
    R = np.asarray(R, dtype=np.float64)
    return R.sum(axis=1), R @ np.asarray(Zcorr, dtype=np.float64).T


def assign(Zq, C, sigma):
    """R (K x Nq) of the query against the normalised rows of C"""
    Zq = np.asarray(Zq, dtype=np.float64)
    n = np.linalg.norm(Zq, axis=0)
    Zn = Zq / np.where(n > 0, n, 1.0)
    cn = np.linalg.norm(C, axis=1, keepdims=True)
    Y = C / np.where(cn > 0, cn, 1.0)
    L = -2.0 * (1.0 - Y @ Zn) / np.asarray(sigma, dtype=np.float64)[:, None]
    L -= L.max(axis=0, keepdims=True)
    E = np.exp(L)
    return E / E.sum(axis=0, keepdims=True)


def design(codes, n_levels):
    """one-hot rows of every covariate's levels: B x Nq"""
    rows = []
    for c, n in zip(codes, n_levels):
        rows.append((np.asarray(c)[None, :] == np.arange(n)[:, None]).astype(np.float64))
    return np.vstack(rows)


def map_query(Zq, codes, n_levels, Nr, C, sigma, lambda_=None, alpha=0.2, cutoff=1e-5):
    """Zq: d x Nq; codes: per covariate, the 0-based level of every cell; lambda_: None (alpha * E), or B values (one per level).
    Returns (Z_corr d x Nq, R K x Nq)."""
    Zq = np.asarray(Zq, dtype=np.float64)
    Nq = Zq.shape[1]
    R = assign(Zq, C, sigma)
    Phi = design(codes, n_levels)
    B = Phi.shape[0]
    Nb = Phi.sum(axis=1)
    X = np.vstack([np.ones((1, Nq)), Phi])
    Zc = Zq.copy()
    for k in range(R.shape[0]):
        Rk = R[k]
        tot = Rk.sum()
        with np.errstate(invalid="ignore", divide="ignore"):
            kept = np.where((Phi @ Rk) / Nb > cutoff)[0]
        rows = np.concatenate([[0], 1 + kept]).astype(int)
        Xk = X[rows]
        lam = np.zeros(len(rows))
        if lambda_ is None:
            lam[1:] = alpha * tot * Nb[kept] / Nq
        else:
            lam[1:] = np.asarray(lambda_, dtype=np.float64)[kept]
        A = (Xk * Rk) @ Xk.T + np.diag(lam)
        A[0, 0] += Nr[k]
        G = (Xk * Rk) @ Zq.T
        G[0] += C[k]
        W = np.linalg.solve(A, G)
        W[0] = 0.0
        Zc -= W.T @ (Xk * Rk)
    return Zc, R

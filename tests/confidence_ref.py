"""The mapping confidence restated in fp64 NumPy (the spec of include/harmony_mi355x_confidence.h; not a test module).

Reference moments, per soft cluster k of a fitted reference with R (K x N) and rows z_i (the columns of Z, d x N):
    S0 = sum_i R[k,i],  w_i = R[k,i] / S0,  mu_k = sum_i w_i z_i,
    Sigma_k = sum_i w_i (z_i - mu_k)(z_i - mu_k)^T / (1 - sum_i w_i^2)
-- R's cov.wt(method = "unbiased"), numpy's cov(aweights = R[k]) (asserted below at import, on a small case).

Per-cell score of a mapped query with its own soft assignment R (K x Nq) and rows z_i:
    Sigma_k + ridge I = L_k L_k^T,  U_k = L_k^-1 (lower triangular),
    dist[i,k] = || U_k (z_i - mu_k) ||_2,  score[i] = sum_k R[k,i] dist[i,k].
The whitening form is the contract: the error bars below rest on it.

Error bars (u = 2^-24), derived, not tuned:
    moments:    |mu_gpu - mu|_j <= 270 u sum_i w_i |z_ij|;  |Sigma_gpu - Sigma|_jj' <= 270 u sqrt(Sigma_jj Sigma_j'j')
                (a product passes at most 256 fp32 additions before it reaches an fp64 sum, plus the operand roundings; Cauchy-Schwarz on
                sum w |y_j| |y_j'|);
    distances:  |dist_gpu - dist|_ik <= (2 zs + 8) u || |U_k| (|z_i| + |mu_k|) ||_2,  zs = d rounded up to 4
                (one rounding of mu, U and of the difference, an fp32 dot product of at most zs terms, the sum of squares, the root).
"""
import numpy as np

U24 = 2.0 ** -24
MOMENT_FACTOR = 270.0


def reference_moments(R, Z):
    """R: K x N, Z: d x N -> mean (K x d), cov (K x d x d); ValueError naming the cluster where S0 = 0 or 1 - sum w^2 <= 0"""
    R = np.asarray(R, dtype=np.float64)
    Z = np.asarray(Z, dtype=np.float64)
    K, d = R.shape[0], Z.shape[0]
    mean = np.empty((K, d))
    cov = np.empty((K, d, d))
    for k in range(K):
        S0 = R[k].sum()
        if not S0 > 0:
            raise ValueError("cluster %d holds no mass" % k)
        w = R[k] / S0
        den = 1.0 - np.sum(w * w)
        if not den > 0:
            raise ValueError("cluster %d has no unbiased covariance" % k)
        mu = Z @ w
        Y = Z - mu[:, None]
        mean[k] = mu
        cov[k] = (Y * w) @ Y.T / den
    return mean, cov


def moment_bars(R, Z, cov):
    """(bar of the mean K x d, bar of the covariance K x d x d)"""
    R = np.asarray(R, dtype=np.float64)
    w = R / R.sum(axis=1, keepdims=True)
    mean_bar = MOMENT_FACTOR * U24 * (w @ np.abs(np.asarray(Z, dtype=np.float64)).T)
    sd = np.sqrt(np.einsum("kjj->kj", cov))
    return mean_bar, MOMENT_FACTOR * U24 * sd[:, :, None] * sd[:, None, :]


def whitening(cov, ridge=0.0):
    """U (K x d x d), U_k = L_k^-1 lower triangular; numpy.linalg.LinAlgError where cov_k + ridge I is not positive definite"""
    cov = np.asarray(cov, dtype=np.float64)
    K, d = cov.shape[0], cov.shape[1]
    U = np.empty_like(cov)
    for k in range(K):
        L = np.linalg.cholesky(cov[k] + ridge * np.eye(d))
        U[k] = np.tril(np.linalg.solve(L, np.eye(d)))
    return U


def distances(Z, mean, cov, ridge=0.0):
    """Z: d x Nq -> dist (Nq x K)"""
    Z = np.asarray(Z, dtype=np.float64)
    U = whitening(cov, ridge)
    out = np.empty((Z.shape[1], U.shape[0]))
    for k in range(U.shape[0]):
        out[:, k] = np.linalg.norm(U[k] @ (Z - np.asarray(mean, dtype=np.float64)[k][:, None]), axis=0)
    return out


def score(R, dist):
    """R: K x Nq, dist: Nq x K -> score (Nq,)"""
    return np.sum(np.asarray(R, dtype=np.float64).T * np.asarray(dist, dtype=np.float64), axis=1)


def distance_bars(Z, mean, cov, ridge=0.0):
    """delta (Nq x K)"""
    Z = np.abs(np.asarray(Z, dtype=np.float64))
    d = Z.shape[0]
    zs = (d + 3) // 4 * 4
    U = np.abs(whitening(cov, ridge))
    out = np.empty((Z.shape[1], U.shape[0]))
    for k in range(U.shape[0]):
        out[:, k] = np.linalg.norm(U[k] @ (Z + np.abs(np.asarray(mean, dtype=np.float64)[k])[:, None]), axis=0)
    return (2 * zs + 8) * U24 * out


def distances_fp32(Z, mean, cov, ridge=0.0):
    """a plain fp32 NumPy evaluation of the whitening form (fp64 factorisation, everything after it in float32): what honest fp32 gives"""
    Z = np.asarray(Z, dtype=np.float32)
    U = whitening(cov, ridge).astype(np.float32)
    mu = np.asarray(mean, dtype=np.float32)
    out = np.empty((Z.shape[1], U.shape[0]), dtype=np.float32)
    for k in range(U.shape[0]):
        T = U[k] @ (Z - mu[k][:, None])
        out[:, k] = np.sqrt(np.sum(T * T, axis=0, dtype=np.float32))
    return out


def _assert_equals_numpy_cov():
    rng = np.random.default_rng(0)
    R = rng.random((3, 40))
    Z = rng.standard_normal((4, 40))
    mean, cov = reference_moments(R, Z)
    for k in range(3):
        assert np.allclose(cov[k], np.cov(Z, aweights=R[k]), rtol=1e-12, atol=1e-14)
        assert np.allclose(mean[k], np.average(Z, axis=1, weights=R[k]), rtol=1e-12, atol=1e-14)


_assert_equals_numpy_cov()

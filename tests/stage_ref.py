"""NumPy fp64 restatement of the reference's three stages -- the clustering head, one update_R round and the ridge correction -- plus
compute_objective: the spec the stage tests compare the CPU oracle and the HIP library with.  Not a test module.

Every function takes the arrays it needs from the caller (the state a handle exposes through its getters) and returns fp64 arrays.
Phi is the B x N one-hot design (a dense array or any scipy.sparse matrix), B_vec the levels per covariate.
"""
import numpy as np
import scipy.sparse as sp


def _csc(Phi):
    return sp.csc_matrix(Phi, dtype=np.float64)


def my_ceil(num):
    """src/utils.cpp:102-108 on an fp32 argument"""
    num = np.float32(num)
    inum = int(num)
    return inum if num == np.float32(inum) else inum + 1


def block_partition(N, block_size):
    """(n_blocks, cells_per_block, [(lo, hi), ...]) of update_R (src/harmony.cpp:280-301): n_blocks = my_ceil(1.0 / block_size), cells_per_block
    = unsigned(N * block_size) with the product in fp32, the last block takes the remainder (empty blocks are dropped)."""
    bs = np.float32(block_size)
    nb = my_ceil(np.float32(1.0 / np.float64(bs)))
    cpb = int(np.float32(N) * bs)
    bounds = []
    for i in range(nb):
        lo, hi = i * cpb, ((i + 1) * cpb if i < nb - 1 else N)
        hi = min(hi, N)
        if lo < hi:
            bounds.append((lo, hi))
    return nb, cpb, bounds


def normalise_cols(Z):
    Z = np.asarray(Z, dtype=np.float64)
    n = np.linalg.norm(Z, axis=0)
    return Z / np.where(n > 0, n, 1.0)


def _assign(Y, Zc, sigma):
    """column softmax of -dist / sigma (src/harmony.cpp:144-147) and dist = 2 (1 - Y^T Z)"""
    dist = 2.0 * (1.0 - np.asarray(Y, dtype=np.float64).T @ Zc)
    L = -dist / np.asarray(sigma, dtype=np.float64)[:, None]
    L -= L.max(axis=0, keepdims=True)
    R = np.exp(L)
    return R / R.sum(axis=0, keepdims=True), dist


def head(Y, Zc, sigma, Phi, Pr_b, cold=False):
    """init_cluster_cpp's assignment (src/harmony.cpp:139-150) with Y already normalised; cold=True: the cold start of cluster_cpp
    (:214-228), which normalises Z_corr first.  Returns (R, dist, O, E)."""
    Zc = normalise_cols(Zc) if cold else np.asarray(Zc, dtype=np.float64)
    R, dist = _assign(Y, Zc, sigma)
    E = R.sum(axis=1)[:, None] * np.asarray(Pr_b, dtype=np.float64)[None, :]
    O = np.asarray((_csc(Phi) @ R.T).T)
    return R, dist, O, E


def _penalised(Y, Zc, sigma, theta, O, E, Phi_cells):
    """one block's new R (src/harmony.cpp:318-323): L1(L1(exp(-dist / sigma)) % (harmony_pow((2E + 1) / (O + E + 1), theta) * Phi))"""
    dist = 2.0 * (1.0 - Y.T @ Zc)
    L = -dist / sigma[:, None]
    L -= L.max(axis=0, keepdims=True)
    X = np.exp(L)
    X /= X.sum(axis=0, keepdims=True)
    pen = ((2.0 * E + 1.0) / (O + E + 1.0)) ** theta[None, :]      # harmony_pow: column b to the power theta[b] (src/utils.cpp:84-90)
    X *= np.asarray((Phi_cells.T @ pen.T).T)                        # a matrix product: the covariates' penalties add
    return X / X.sum(axis=0, keepdims=True)


def update_round(R_prev, R_next, Y, Zc, Phi, Pr_b, sigma, theta, order, n_blocks, cells_per_block):
    """One update_R round (src/harmony.cpp:269-342, harmony_pow src/utils.cpp:84-90), teacher-forced: block i sees the O / E tables built
    from R_next (the observed result) on the blocks before it and from R_prev on the blocks after it, so every block's spec is a one-step
    function of observed values.  order[p] = the cell at position p of the round's shuffle; Zc: the normalised Z_corr of the last head.
    Returns the spec R (K x N)."""
    Y = np.asarray(Y, dtype=np.float64)
    sigma = np.asarray(sigma, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    Pr_b = np.asarray(Pr_b, dtype=np.float64)
    Phi = _csc(Phi)
    order = np.asarray(order, dtype=np.int64)
    N = order.size
    bounds = []
    for i in range(n_blocks):
        lo, hi = i * cells_per_block, (min((i + 1) * cells_per_block, N) if i < n_blocks - 1 else N)
        if lo < hi:
            bounds.append(order[lo:hi])
    K, B = np.shape(R_prev)[0], Phi.shape[0]

    def contrib(R, cells):      # one block's O and row sums
        Rc = np.asarray(R[:, cells], dtype=np.float64)
        return np.asarray((Phi[:, cells] @ Rc.T).T), Rc.sum(axis=1)

    prev = [contrib(R_prev, c) for c in bounds]
    nxt = [contrib(R_next, c) for c in bounds]
    O_after = np.zeros((K, B))       # sum over j > i of the old contributions
    r_after = np.zeros(K)
    for o, r in prev:
        O_after += o
        r_after += r
    O_before, r_before = np.zeros((K, B)), np.zeros(K)
    out = np.empty((K, N))
    for i, cells in enumerate(bounds):
        O_after -= prev[i][0]
        r_after -= prev[i][1]
        O = O_before + O_after
        E = (r_before + r_after)[:, None] * Pr_b[None, :]
        out[:, cells] = _penalised(Y, np.asarray(Zc[:, cells], dtype=np.float64), sigma, theta, O, E, Phi[:, cells])
        O_before += nxt[i][0]
        r_before += nxt[i][1]
    return out


def _update_round_direct(R_prev, Y, Zc, Phi, Pr_b, sigma, theta, order, n_blocks, cells_per_block, R_next=None):
    """the reference's own loop (remove the block's old cells, recompute them, put them back) on dense fp64 arrays; R_next given: put back the
    observed values instead of the recomputed ones (the teacher-forced form).  For checking update_round at a few hundred cells."""
    Phi = np.asarray(_csc(Phi).todense())
    R = np.array(R_prev, dtype=np.float64)
    Y, sigma, theta, Pr_b = (np.asarray(a, dtype=np.float64) for a in (Y, sigma, theta, Pr_b))
    O = R @ Phi.T
    E = R.sum(axis=1)[:, None] * Pr_b[None, :]
    N = len(order)
    out = np.empty_like(R)
    for i in range(n_blocks):
        lo, hi = i * cells_per_block, (min((i + 1) * cells_per_block, N) if i < n_blocks - 1 else N)
        if lo >= hi:
            continue
        c = np.asarray(order[lo:hi])
        E -= R[:, c].sum(axis=1)[:, None] * Pr_b[None, :]
        O -= R[:, c] @ Phi[:, c].T
        for j, cell in enumerate(c):
            dist = 2.0 * (1.0 - Y.T @ np.asarray(Zc[:, cell], dtype=np.float64))
            x = np.exp(-dist / sigma)
            x /= x.sum()
            x *= (((2 * E + 1) / (O + E + 1)) ** theta[None, :]) @ Phi[:, cell]
            out[:, cell] = x / x.sum()
        R[:, c] = out[:, c] if R_next is None else np.asarray(R_next[:, c], dtype=np.float64)
        E += R[:, c].sum(axis=1)[:, None] * Pr_b[None, :]
        O += R[:, c] @ Phi[:, c].T
    return out


def objective(R, dist, O, E, Phi, sigma, theta, N):
    """compute_objective (src/harmony.cpp:157-170): (kmeans_error, entropy, cross_entropy), each scaled by 2000 / N (fp32 constant).
    safe_entropy is R % trunc_log(R) (src/utils.cpp:78-81): 0 where R = 0."""
    R = np.asarray(R, dtype=np.float64)
    sigma = np.asarray(sigma, dtype=np.float64)
    norm = float(np.float32(2000) / np.float32(N))
    km = float(np.sum(R * np.asarray(dist, dtype=np.float64)))
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = float(np.sum(np.where(R > 0, R * np.log(np.where(R > 0, R, 1.0)), 0.0).sum(axis=1) * sigma))
    L = np.asarray(theta, dtype=np.float64)[None, :] * np.log((O + E + 1.0) / (2.0 * E + 1.0))
    RPhi = np.asarray((_csc(Phi) @ R.T).T)
    cross = float(np.sum(sigma[:, None] * L * RPhi))
    return km * norm, ent * norm, cross * norm


def _combinations(Phi, B_vec):
    """(q_of_cell (N,), levels (Q x C)): the distinct level combinations of a one-hot design with C covariates"""
    Phi = _csc(Phi)
    Phi.sort_indices()
    C = len(B_vec)
    nnz = np.diff(Phi.indptr)
    assert np.all(nnz == C), "every cell needs one level of every covariate"
    codes = Phi.indices.reshape(-1, C)
    levels, q = np.unique(codes, axis=0, return_inverse=True)
    return q.ravel(), levels


def kept_levels(O, N_b, B_vec, cutoff):
    """(keep (K x B bool), active (K x C)): a level enters cluster k's system when float(O[k, b]) / N_b > cutoff in fp32 (src/harmony.cpp:368-380)
    and its covariate has at least two such levels (:389-402)"""
    rep = np.asarray(O, dtype=np.float32) / np.asarray(N_b, dtype=np.float32)[None, :]
    over = rep > np.float32(cutoff)
    cov = np.repeat(np.arange(len(B_vec)), B_vec)
    cnt = np.stack([over[:, cov == c].sum(axis=1) for c in range(len(B_vec))], axis=1)
    active = cnt > 1
    return over & active[:, cov], active


def cutoff_margin(O, N_b, cutoff):
    """smallest |rep / cutoff - 1| over the table: the keep decisions are comparable between two backends when it is well above fp32 rounding"""
    rep = np.asarray(O, dtype=np.float64) / np.asarray(N_b, dtype=np.float64)[None, :]
    return float(np.min(np.abs(rep / cutoff - 1.0)))


def moe_correct_ridge(R, Z_orig, O, E, Phi, B_vec, lambda_vec, alpha, cutoff, Y_prev):
    """moe_correct_ridge_cpp (src/harmony.cpp:345-633, find_lambda_cpp src/utils.cpp:159-163) in fp64 with np.linalg.solve.
    lambda_vec: None (estimated: alpha * E[k, kept]) or the B + 1 fixed values.  A cluster whose kept levels are not all B levels takes the subset
    path (the intercept and every sum over the union of the kept levels' cells, only those cells corrected); with no active covariate it is
    skipped and keeps Y_prev[:, k].  The systems come from per-combination sums (one K x d x N pass).
    Returns a dict: Z_corr, Y (normalised), W (the last non-skipped cluster's, row 0 zeroed), subset, skipped (K bools), kept (K index arrays),
    lam (K arrays of the kept levels' Lambda), cond (K 1-norm condition numbers, nan when skipped)."""
    R = np.asarray(R, dtype=np.float64)
    Zo = np.asarray(Z_orig, dtype=np.float64)
    K, B = R.shape[0], np.shape(O)[1]
    d = Zo.shape[0]
    N_b = np.asarray(_csc(Phi).sum(axis=1)).ravel()
    q_of, levels = _combinations(Phi, B_vec)
    Q = levels.shape[0]
    order = np.argsort(q_of, kind="stable")
    starts = np.searchsorted(q_of[order], np.arange(Q + 1))
    nq = np.empty((Q, K))
    Sq = np.empty((Q, K, d))
    for q in range(Q):
        c = order[starts[q]:starts[q + 1]]
        nq[q] = R[:, c].sum(axis=1)
        Sq[q] = R[:, c] @ Zo[:, c].T
    keep, _active = kept_levels(O, N_b, B_vec, cutoff)
    Y = np.array(Y_prev, dtype=np.float64)
    Wq = np.zeros((Q, K, d))        # the correction row of a cell of combination q from cluster k
    res = dict(subset=np.zeros(K, bool), skipped=np.zeros(K, bool), kept=[], lam=[], cond=np.full(K, np.nan), W=None)
    for k in range(K):
        kept = np.where(keep[k])[0]
        res["kept"].append(kept)
        res["subset"][k] = kept.size != B
        if kept.size == 0:
            res["skipped"][k] = True
            res["lam"].append(np.zeros(0))
            continue
        m = kept.size + 1
        row = np.full(B, -1)
        row[kept] = np.arange(1, m)
        rows_q = row[levels]                         # Q x C: the kept rows of every combination (-1: not kept)
        inq = (rows_q >= 0).any(axis=1)              # combinations in the union of the kept levels' cells
        A = np.zeros((m, m))
        G = np.zeros((m, d))
        for q in np.where(inq)[0]:
            rr = np.concatenate([[0], rows_q[q][rows_q[q] >= 0]])
            A[np.ix_(rr, rr)] += nq[q, k]
            G[rr] += Sq[q, k]
        lam = (alpha * np.asarray(E, dtype=np.float64)[k, kept]) if lambda_vec is None else np.asarray(lambda_vec, dtype=np.float64)[kept + 1]
        res["lam"].append(lam)
        A[np.arange(1, m), np.arange(1, m)] += lam
        W = np.linalg.solve(A, G)
        res["cond"][k] = np.linalg.norm(A, 1) * np.linalg.norm(np.linalg.inv(A), 1)
        Y[:, k] = W[0]
        W[0] = 0.0
        res["W"] = W
        for q in np.where(inq)[0]:
            Wq[q, k] = W[rows_q[q][rows_q[q] >= 0]].sum(axis=0)
    Zc = Zo.copy()
    for q in range(Q):
        c = order[starts[q]:starts[q + 1]]
        Zc[:, c] -= Wq[q].T @ R[:, c]
    res["Z_corr"] = Zc
    res["Y"] = normalise_cols(Y)
    return res


def _moe_correct_ridge_direct(R, Z_orig, O, E, Phi, B_vec, lambda_vec, alpha, cutoff, Y_prev):
    """the per-cell dense form of moe_correct_ridge (the reference's own products on the subset of cells): for checking it at a few hundred cells"""
    R = np.asarray(R, dtype=np.float64)
    Zo = np.asarray(Z_orig, dtype=np.float64)
    Phi = np.asarray(_csc(Phi).todense())
    K, B = R.shape[0], Phi.shape[0]
    N_b = Phi.sum(axis=1)
    keep, _ = kept_levels(O, N_b, B_vec, cutoff)
    Zc = Zo.copy()
    Y = np.array(Y_prev, dtype=np.float64)
    W_last = None
    for k in range(K):
        kept = np.where(keep[k])[0]
        if kept.size == 0:
            continue
        cells = np.where(Phi[kept].sum(axis=0) > 0)[0]
        X = np.vstack([np.ones((1, cells.size)), Phi[np.ix_(kept, cells)]])
        XR = X * R[k, cells]
        lam = alpha * np.asarray(E, dtype=np.float64)[k, kept] if lambda_vec is None else np.asarray(lambda_vec)[kept + 1]
        A = XR @ X.T + np.diag(np.concatenate([[0.0], lam]))
        W = np.linalg.inv(A) @ (XR @ Zo[:, cells].T)
        Y[:, k] = W[0]
        W[0] = 0.0
        W_last = W
        Zc[:, cells] -= W.T @ XR
    return Zc, normalise_cols(Y), W_last

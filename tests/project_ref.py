"""The count projection restated in fp64 NumPy (the spec of include/harmony_mi355x_project.h; not a test module).

A query is a CSR matrix of Nq cells x G_all genes; slot[g] is the row j of the reference's tables (U G x d, mean, sd) gene g corresponds to,
or -1.  Per cell i with library size T_i (the row sum over ALL columns, or a caller's value), in the DENSE form of the definition:
    y_ig = log1p(x_ig scale / T_i) for every query gene g with slot[g] = j >= 0, zeros included (T_i = 0: y = 0),
    s_ij = (y_ig - mean_j) / sd_j, min(s_ij, clip) with a clip;  reference genes absent from the query: s_ij = 0,
    P[i,:] = sum_j s_ij U[j,:].
`project` evaluates exactly that on a dense matrix, so it does not rest on the identity the kernel uses; `project_sparse` is that identity,
    P[i,:] = b + sum over the stored entries with slot >= 0 of w U[j,:],  b = sum_{j present} (-mean_j / sd_j) U[j,:],
    w = min(y, mean_j + clip sd_j) / sd_j,
and `project_fp32` its sequential float32 evaluation (b in fp64): what honest fp32 gives.

Error bar (u = 2^-24, n_i the contributing entries of cell i), derived, not tuned:
    |P_gpu - P|_ij <= (n_i + 16) u sum_g |w_ig| |U_gj| + 2 u |b_j|
n_i u from the fma chain; the 16 covers the roundings of x scale / T, log1pf, 1 / sd, the cap, the fp32 U and the final add.
"""
import numpy as np

U24 = 2.0 ** -24


def row_totals(data, indptr):
    data = np.asarray(data, dtype=np.float64)
    Nq = len(indptr) - 1
    return np.array([data[indptr[i]:indptr[i + 1]].sum() for i in range(Nq)], dtype=np.float64)


def dense(data, indices, indptr, G_all):
    Nq = len(indptr) - 1
    X = np.zeros((Nq, G_all), dtype=np.float64)
    for i in range(Nq):
        X[i, np.asarray(indices[indptr[i]:indptr[i + 1]], dtype=np.int64)] = data[indptr[i]:indptr[i + 1]]
    return X


def project(data, indices, indptr, G_all, slot, U, mean, sd, scale=1e4, clip=None, totals=None):
    """the dense form -> P (Nq x d) in fp64"""
    X = dense(data, indices, indptr, G_all)
    T = row_totals(data, indptr) if totals is None else np.asarray(totals, dtype=np.float64)
    U, mean, sd, slot = np.asarray(U, np.float64), np.asarray(mean, np.float64), np.asarray(sd, np.float64), np.asarray(slot)
    Y = np.zeros_like(X)
    pos = T > 0
    Y[pos] = np.log1p(X[pos] * scale / T[pos, None])
    S = np.zeros((X.shape[0], U.shape[0]))                 # reference genes the query lacks stay 0
    g = np.nonzero(slot >= 0)[0]
    j = slot[g]
    S[:, j] = (Y[:, g] - mean[j]) / sd[j]
    if clip is not None:
        S[:, j] = np.minimum(S[:, j], clip)
    return S @ U


def _weights(data, indices, indptr, slot, mean, sd, scale, clip, totals):
    """per stored entry: (row of the tables or -1, w) in fp64"""
    data = np.asarray(data, dtype=np.float64)
    T = row_totals(data, indptr) if totals is None else np.asarray(totals, dtype=np.float64)
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    j = np.asarray(slot)[np.asarray(indices, dtype=np.int64)]
    Tr = T[rows]
    y = np.where(Tr > 0, np.log1p(data * scale / np.where(Tr > 0, Tr, 1.0)), 0.0)
    jj = np.maximum(j, 0)
    mean, sd = np.asarray(mean, np.float64), np.asarray(sd, np.float64)
    cap = mean[jj] + clip * sd[jj] if clip is not None else np.full(j.shape, np.inf)
    w = np.where(j >= 0, np.minimum(y, cap) / sd[jj], 0.0)
    return rows, j, w, y, cap


def offset(slot, U, mean, sd):
    slot = np.asarray(slot)
    j = slot[slot >= 0]
    return (-(np.asarray(mean, np.float64)[j] / np.asarray(sd, np.float64)[j])) @ np.asarray(U, np.float64)[j]


def project_sparse(data, indices, indptr, G_all, slot, U, mean, sd, scale=1e4, clip=None, totals=None):
    """the sparse identity in fp64"""
    rows, j, w, _, _ = _weights(data, indices, indptr, slot, mean, sd, scale, clip, totals)
    U = np.asarray(U, np.float64)
    P = np.tile(offset(slot, U, mean, sd), (len(indptr) - 1, 1))
    keep = j >= 0
    np.add.at(P, rows[keep], w[keep, None] * U[j[keep]])
    return P


def clipped_entries(data, indices, indptr, slot, mean, sd, scale=1e4, clip=None, totals=None):
    """how many stored entries the clip actually lowers"""
    if clip is None:
        return 0
    _, j, _, y, cap = _weights(data, indices, indptr, slot, mean, sd, scale, clip, totals)
    return int(np.sum((j >= 0) & (y > cap)))


def bars(data, indices, indptr, G_all, slot, U, mean, sd, scale=1e4, clip=None, totals=None):
    """delta (Nq x d): the error bound of the docstring"""
    rows, j, w, _, _ = _weights(data, indices, indptr, slot, mean, sd, scale, clip, totals)
    Nq = len(indptr) - 1
    Ua = np.abs(np.asarray(U, np.float64))
    keep = j >= 0
    n = np.bincount(rows[keep], minlength=Nq).astype(np.float64)
    A = np.zeros((Nq, Ua.shape[1]))
    np.add.at(A, rows[keep], np.abs(w[keep, None]) * Ua[j[keep]])
    return (n[:, None] + 16.0) * U24 * A + 2.0 * U24 * np.abs(offset(slot, U, mean, sd))[None, :]


def project_fp32(data, indices, indptr, G_all, slot, U, mean, sd, scale=1e4, clip=None, totals=None):
    """a sequential float32 NumPy evaluation of the sparse form (totals and b in fp64): what honest fp32 gives"""
    f = np.float32
    data64 = np.asarray(data, dtype=np.float64)
    T = row_totals(data64, indptr) if totals is None else np.asarray(totals, dtype=np.float64)
    U32 = np.asarray(U, np.float64).astype(f)
    mean, sd = np.asarray(mean, np.float64), np.asarray(sd, np.float64)
    inv_sd = (1.0 / sd).astype(f)
    cap = (mean + clip * sd).astype(f) if clip is not None else np.full(sd.shape, np.inf, dtype=f)
    b = offset(slot, U, mean, sd)
    slot = np.asarray(slot)
    P = np.empty((len(indptr) - 1, U32.shape[1]), dtype=f)
    for i in range(len(indptr) - 1):
        r = f(scale / T[i]) if T[i] > 0 else f(0)
        acc = np.zeros(U32.shape[1], dtype=f)
        for e in range(indptr[i], indptr[i + 1]):
            j = slot[indices[e]]
            if j < 0:
                continue
            y = np.log1p(f(data64[e]) * r, dtype=f)
            w = f(min(y, cap[j]) * inv_sd[j])
            acc = (w * U32[j] + acc).astype(f)
        P[i] = (acc.astype(np.float64) + b).astype(f)
    return P


def random_case(Nq, G_all, G, d, seed, row_lengths=(), integer=True, shared=None, density=0.1):
    """A synthetic query and reference tables.  The first rows get the stored-entry counts of `row_lengths` (capped at G_all); the others
    about density G_all.  `shared` reference genes (default: all that fit but one in eight) are present in the query, in permuted order; the
    remaining query genes are unknown to the reference.  Rows are unsorted.
    -> dict(data, indices, indptr, G_all, slot, U, mean, sd)"""
    rng = np.random.default_rng(seed)
    if shared is None:
        shared = max(1, min(G, G_all) - min(G, G_all) // 8)
    shared = min(shared, G, G_all)
    slot = np.full(G_all, -1, dtype=np.int32)
    slot[rng.permutation(G_all)[:shared]] = rng.permutation(G)[:shared].astype(np.int32)
    lens = [min(int(n), G_all) for n in row_lengths][:Nq]
    while len(lens) < Nq:
        lens.append(int(min(G_all, rng.binomial(G_all, density))))
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([rng.permutation(G_all)[:n] for n in lens] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    vals = rng.geometric(0.4, size=int(indptr[-1])).astype(np.float64)
    if not integer:
        vals = vals * rng.uniform(0.25, 1.75, size=vals.size)
    U = rng.standard_normal((G, d)) / np.sqrt(G)
    mean = rng.uniform(0.0, 1.5, size=G)
    sd = rng.uniform(0.2, 1.5, size=G)
    return dict(data=vals, indices=indices, indptr=indptr, G_all=G_all, slot=slot, U=U, mean=mean, sd=sd)

"""The spec of Seurat's shared-nearest-neighbour graph (include/harmony_mi355x_snn.h): integers until the last step.

idx [N][m]: a neighbour list with self excluded, -1 an unfilled slot; k = m + 1.  A is the 0/1 matrix of N+(i) = {i} and the valid idx[i][.];
S = A A^T holds the shared counts; an entry is kept iff s >= s_min, the smallest s in 1 .. k + 1 with s / (2k - s) >= prune in fp64; its weight
is s / (2k - s) formed in fp64 and rounded once to fp32.  Rows ascending; the diagonal is an entry like any other.
"""
import numpy as np
import scipy.sparse as sp


def nn_matrix(idx):
    """A as int32 CSR with ascending rows: self added, -1 skipped"""
    idx = np.asarray(idx)
    N, m = idx.shape
    valid = idx >= 0
    rows = np.concatenate([np.arange(N), np.repeat(np.arange(N), m)[valid.ravel()]])
    cols = np.concatenate([np.arange(N), idx[valid]])
    A = sp.csr_matrix((np.ones(rows.size, dtype=np.int32), (rows, cols)), shape=(N, N))
    A.sort_indices()
    return A


def s_min(k, prune):
    for s in range(1, k + 2):
        if float(s) / float(2 * k - s) >= float(prune):
            return s
    raise AssertionError("s = k + 1 passes every prune <= 1")


def weights_of(s, k):
    s = np.asarray(s, dtype=np.float64)
    return (s / (2.0 * k - s)).astype(np.float32)


def candidates(idx):
    """C_i = sum over j in N+(i) of in-degree(j) + 1: the candidates of row i with multiplicity"""
    A = nn_matrix(idx)
    col = np.asarray(A.sum(axis=0)).ravel().astype(np.int64)      # in-degree(j) + 1 (the diagonal)
    return np.asarray(A.astype(np.int64) @ col).ravel()


def snn(idx, prune=1.0 / 15.0):
    """(indptr int64, indices int32, weights float32, shared counts int32) of the pruned graph"""
    idx = np.asarray(idx)
    N, m = idx.shape
    k = m + 1
    A = nn_matrix(idx)
    S = (A @ A.T).tocsr().astype(np.int32)
    S.sort_indices()
    keep = S.data >= s_min(k, prune)
    rows = np.repeat(np.arange(N), np.diff(S.indptr))[keep]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=N))]).astype(np.int64)
    s = S.data[keep]
    return indptr, S.indices[keep].astype(np.int32), weights_of(s, k), s

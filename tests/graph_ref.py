"""The fp64 / integer spec of the neighbour graph (harmony_amd/graph.py, include/harmony_mi355x_graph.h): umap-learn's fuzzy simplicial set as
scanpy builds it (local_connectivity = 1, set_op_mix_ratio = 1) restated in NumPy, the connected components of a symmetric pattern, and scib's
graph connectivity.  The input is a neighbour list with SELF EXCLUDED: idx [N][m] (-1: an unfilled slot, its distance is ignored), dist [N][m]
Euclidean, read as fp32 and held in float64; scanpy's n_neighbors is m + 1 (its column 0 is the cell itself at distance 0)."""
import numpy as np

TOL = 1e-5
STEPS = 64
MIN_SCALE = 1e-3


def as_f32_f64(X):
    return np.ascontiguousarray(X, dtype=np.float32).astype(np.float64)


def _lists(idx, dist):
    idx = np.asarray(idx).astype(np.int64)
    dist = as_f32_f64(dist)
    if idx.ndim != 2 or idx.shape != dist.shape:
        raise ValueError("idx and dist must be N x m matrices of one shape")
    valid = idx >= 0
    return idx, np.where(valid, dist, 0.0), valid


def psum(dist, valid, rho, mid):
    """sum_j (d_ij - rho_i > 0 ? exp(-(d_ij - rho_i) / mid_i) : 1) over the valid entries of every row"""
    r = dist - rho[:, None]
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        t = np.where(r > 0, np.exp(-np.where(r > 0, r, 0.0) / mid[:, None]), 1.0)
    return np.where(valid, t, 0.0).sum(axis=1)


def smooth_knn(idx, dist):
    """-> rho [N], sigma [N] (float64)"""
    idx, dist, valid = _lists(idx, dist)
    N, m = idx.shape
    target = np.log2(m + 1.0)
    pos = valid & (dist > 0)
    rho = np.where(pos.any(axis=1), np.where(pos, dist, np.inf).min(axis=1), 0.0)
    lo, hi, mid = np.zeros(N), np.full(N, np.inf), np.ones(N)
    live = valid.any(axis=1)
    for _ in range(STEPS):
        p = psum(dist, valid, rho, mid)
        live = live & ~(np.abs(p - target) < TOL)
        if not live.any():
            break
        up = live & (p > target)
        dn = live & ~(p > target)
        hi = np.where(up, mid, hi)
        lo = np.where(dn, mid, lo)
        with np.errstate(invalid="ignore", over="ignore"):
            half = (lo + hi) / 2
        mid = np.where(up, half, np.where(dn, np.where(np.isinf(hi), mid * 2, half), mid))
    mean_i = dist.sum(axis=1) / (m + 1.0)
    mean_all = dist.sum() / (float(N) * (m + 1.0))
    sigma = np.maximum(mid, MIN_SCALE * np.where(rho > 0, mean_i, mean_all))
    none = ~valid.any(axis=1)
    return np.where(none, 0.0, rho), np.where(none, 0.0, sigma)


def memberships(idx, dist, rho=None, sigma=None):
    """-> w [N][m] float64, the membership of every directed edge (0 at the unfilled slots)"""
    if rho is None:
        rho, sigma = smooth_knn(idx, dist)
    idx, dist, valid = _lists(idx, dist)
    r = dist - rho[:, None]
    one = (r <= 0) | (sigma[:, None] == 0)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        w = np.where(one, 1.0, np.exp(-np.where(one, 0.0, r) / np.where(sigma == 0, 1.0, sigma)[:, None]))
    return np.where(valid, w, 0.0)


def connectivities(idx, dist):
    """-> (indptr int64 [N + 1], indices int32, weights float32): row i is the union of {j in idx[i]} and {j : i in idx[j]}, ascending, with
    a + b - a b of the two directed memberships formed in float64 and rounded once"""
    w = memberships(idx, dist)
    idx, _, valid = _lists(idx, dist)
    N, m = idx.shape
    r = np.repeat(np.arange(N, dtype=np.int64), m)[valid.ravel()]
    c = idx.ravel()[valid.ravel()]
    wv = w.ravel()[valid.ravel()]
    fwd, bwd = r * N + c, c * N + r
    keys = np.unique(np.concatenate([fwd, bwd]))
    a, b = np.zeros(keys.size), np.zeros(keys.size)
    a[np.searchsorted(keys, fwd)] = wv
    b[np.searchsorted(keys, bwd)] = wv
    rows = keys // N
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=N))]).astype(np.int64)
    return indptr, (keys % N).astype(np.int32), (a + b - a * b).astype(np.float32)


def components(indptr, indices, labels=None):
    """comp[i] = the smallest cell index of i's connected component (union-find over the edges); with labels only edges whose two ends carry the
    same label count, and cells labelled -1 are singletons"""
    indptr, indices = np.asarray(indptr), np.asarray(indices)
    N = indptr.size - 1
    parent = list(range(N))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    lab = None if labels is None else np.asarray(labels)
    rows = np.repeat(np.arange(N), np.diff(indptr))
    keep = np.ones(rows.size, bool) if lab is None else (lab[rows] == lab[indices]) & (lab[rows] >= 0)
    for u, v in zip(rows[keep].tolist(), indices[keep].tolist()):
        ru, rv = find(u), find(v)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    return np.array([find(i) for i in range(N)], dtype=np.int32)


def graph_connectivity(indptr, indices, labels, n_levels):
    """scib's graph connectivity: per level, the share of its cells in its largest same-label component; the mean over the levels with cells"""
    labels = np.asarray(labels)
    comp = components(indptr, indices, labels)
    shares = []
    for lev in range(n_levels):
        cells = np.nonzero(labels == lev)[0]
        if cells.size:
            shares.append(np.bincount(comp[cells]).max() / cells.size)
    return float(np.mean(shares))

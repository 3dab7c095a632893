"""The spec of the rank sums per group (include/harmony_mi355x_ranksum.h; DESIGN "Rank sums per group"), not a test module.

The keys are formed in NumPy float32 exactly as defined -- key = fl32(fl32(x) r), r = fl32(scale / T) capped at 3e38 (one fp64 division rounded
to fp32, one fp32 product) -- and everything after them is integer arithmetic (NumPy int64 and Python integers): the library's n_obs, n_pos,
rank2 and tie3 must EQUAL what `rank_sums` returns.  The row total T is the caller's totals[i] or the fp64 sum of the row: the cases here use
integer counts (every order of additions gives the same total) or give the totals.  With totals = scale the rate is 1 and key = fl32(x): a
case then chooses the key bits itself (`csr_of_dense` of float32 values)."""
import numpy as np


def entry_keys(data, indices, indptr, scale=1e4, totals=None):
    """-> (float32 key of every stored entry, bool: the entry is positive, int64 row of every entry)"""
    data = np.asarray(data)
    indptr = np.asarray(indptr, dtype=np.int64)
    N = indptr.size - 1
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(indptr))
    x32 = data.astype(np.float32)
    xd = data.astype(np.float64) if data.dtype == np.float64 else x32.astype(np.float64)
    if totals is None:
        T = np.zeros(N)
        np.add.at(T, rows, np.where((xd >= 0) & (xd <= 3.0e38), xd, 0.0))
    else:
        T = np.asarray(totals, dtype=np.float64)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        r = np.where(T > 0, np.minimum((scale / np.where(T > 0, T, 1.0)).astype(np.float32), np.float32(3.0e38)), np.float32(0)).astype(np.float32)
        key = (x32 * r[rows]).astype(np.float32)
    assert key.dtype == np.float32
    return key, (xd > 0) & (key > 0), rows


def dense_keys(data, indices, indptr, G_all, scale=1e4, totals=None):
    """[N, G_all] float32: the key of every (cell, gene) pair, 0 where no positive entry is stored"""
    key, pos, rows = entry_keys(data, indices, indptr, scale, totals)
    K = np.zeros((len(indptr) - 1, G_all), dtype=np.float32)
    K[rows[pos], np.asarray(indices)[pos]] = key[pos]
    return K


def rank_sums(data, indices, indptr, G_all, codes, B, scale=1e4, totals=None, gene_slot=None, G=None):
    """the library's outputs: dict(n_obs [B] int64, n_pos, rank2 [B, G] int64, tie3 [G] Python integers)"""
    codes = np.asarray(codes, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    slot = np.arange(G_all, dtype=np.int64) if gene_slot is None else np.asarray(gene_slot, dtype=np.int64)
    G = G_all if gene_slot is None else int(G)
    key, pos, rows = entry_keys(data, indices, indptr, scale, totals)
    kept = codes >= 0
    Nk = int(kept.sum())
    n_obs = np.bincount(codes[kept], minlength=B).astype(np.int64)
    use = pos & kept[rows] & (slot[indices] >= 0)
    key, grp, out = key[use], codes[rows[use]], slot[indices[use]]
    by = np.argsort(out, kind="stable")
    key, grp, out = key[by], grp[by], out[by]
    cut = np.searchsorted(out, np.arange(G + 1))
    n_pos, rank2 = np.zeros((B, G), dtype=np.int64), np.zeros((B, G), dtype=np.int64)
    tie3 = np.empty(G, dtype=object)
    for j in range(G):
        k, g = key[cut[j]:cut[j + 1]], grp[cut[j]:cut[j + 1]]
        z = Nk - int(k.size)
        _, inv, cnt = np.unique(k, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        less = (np.cumsum(cnt) - cnt).astype(np.int64)               # positive keys below a tie block
        r2 = 2 * z + 2 * less[inv] + cnt[inv].astype(np.int64) + 1      # #(keys <) + #(keys <=) + 1 over the kept cells
        np.add.at(n_pos[:, j], g, 1)
        np.add.at(rank2[:, j], g, r2)
        rank2[:, j] += (n_obs - n_pos[:, j]) * (z + 1)
        tie3[j] = sum(int(c) ** 3 for c in cnt)
    return dict(n_obs=n_obs, n_pos=n_pos, rank2=rank2, tie3=tie3)


def rank_sums_brute(K, codes, B):
    """the same integers by counting pairs on the dense keys [N, G] (small N): -> (n_obs, n_pos, rank2, tie3)"""
    codes = np.asarray(codes, dtype=np.int64)
    kept = codes >= 0
    K, c = K[kept], codes[kept]
    G = K.shape[1]
    n_obs = np.bincount(c, minlength=B).astype(np.int64)
    n_pos, rank2 = np.zeros((B, G), dtype=np.int64), np.zeros((B, G), dtype=np.int64)
    tie3 = np.empty(G, dtype=object)
    for g in range(G):
        k = K[:, g]
        r2 = (k[None, :] < k[:, None]).sum(1) + (k[None, :] <= k[:, None]).sum(1) + 1
        t3 = 0
        for i in range(k.size):
            rank2[c[i], g] += int(r2[i])
            n_pos[c[i], g] += int(k[i] > 0)
            if k[i] > 0 and not np.any(k[:i] == k[i]):      # the first cell of a tie block of positive keys
                t3 += int((k == k[i]).sum()) ** 3
        tie3[g] = t3
    return n_obs, n_pos, rank2, tie3


def csr_of_dense(X, dtype=np.float64, reverse_rows=False):
    """dense values (0: not stored) -> (data, indices, indptr, G_all); reverse_rows stores every row's entries in descending gene order"""
    X = np.asarray(X)
    nz = X != 0
    indptr = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int64)
    data, indices = X[nz].astype(dtype), np.nonzero(nz)[1].astype(np.int32)
    if reverse_rows:
        for i in range(X.shape[0]):
            data[indptr[i]:indptr[i + 1]] = data[indptr[i]:indptr[i + 1]][::-1].copy()
            indices[indptr[i]:indptr[i + 1]] = indices[indptr[i]:indptr[i + 1]][::-1].copy()
    return data, indices, indptr, X.shape[1]


def wilcoxon(n_obs, n_pos, rank2, tie3, tie_correct=True):
    """the test from the integers in Python arithmetic, entry by entry: -> (u, auc, score) [B, G] fp64"""
    B, G = np.asarray(n_pos).shape
    Nk = int(np.sum(n_obs))
    u, auc, score = np.zeros((B, G)), np.zeros((B, G)), np.zeros((B, G))
    for b in range(B):
        n1 = int(n_obs[b])
        n2 = Nk - n1
        for g in range(G):
            P = int(np.asarray(n_pos)[:, g].sum())
            z = Nk - P
            tie = (int(tie3[g]) - P) + (z ** 3 - z)
            u[b, g] = (int(rank2[b][g]) - n1 * (n1 + 1)) / 2.0
            if n1 == 0 or n2 == 0:
                auc[b, g] = score[b, g] = np.nan
                continue
            auc[b, g] = u[b, g] / (n1 * n2)
            var = n1 * n2 / 12.0 * ((Nk + 1.0) - (tie / (Nk * (Nk - 1.0)) if tie_correct else 0.0))
            score[b, g] = (u[b, g] - n1 * n2 / 2.0) / np.sqrt(var) if var > 0 else 0.0
    return u, auc, score

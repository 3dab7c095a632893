"""The spec of the Louvain clustering (include/harmony_mi355x_louvain.h): integers and fp64 only, so that the library agrees bit for bit.

Input: a symmetric CSR (indptr int64, indices int32 ascending within a row, weights float32 in [0, 1], w_ij == w_ji).  The diagonal is
dropped; every other stored entry is an edge, also one of weight 0.  q_ij = rint(w_ij * 2^24) as int64 (half to even, C's llrint);
k_i = sum_j q_ij; M = sum_i k_i.  One level: comm[i] = i, tot[c] = k_c; sweep t is 8 sub-rounds, node i is active in sub-round
fmix32(i ^ fmix32(64 t + level + 1)) & 7; a sub-round decides every active node's move from the comm / tot of its start (score(c) =
dbl(w_ic) - (dbl(k_i) g) dbl(tot_c - [c == a] k_i), g = resolution / dbl(M); target: the c != a of largest score, ties to the smallest c; the
node moves iff score(target) > score(a)), then applies all moves.  A level ends after a sweep without a move or after max_sweeps; a level
without any move ends the call and is not recorded.  Aggregation renumbers the non-empty communities in ascending order of their id.
Q = sum_c (dbl(in_c) / dbl(M) - (resolution (dbl(tot_c) / dbl(M))) (dbl(tot_c) / dbl(M))), added in ascending c.  The call returns the first
level of the largest Q, the singletons when no level beats theirs.

`sequential` is a plain one-node-at-a-time Louvain (ascending node order) on the same integers: what the hashed sub-rounds are measured
against, not part of the spec.
"""
import collections

import numpy as np

SCALE = float(1 << 24)
SUBROUNDS = 8
M32 = 0xFFFFFFFF

Result = collections.namedtuple("Result", "labels n_clusters modularity level_clusters level_sweeps level_modularity best_level sweeps")


def fmix32(x):
    """murmur3's 32-bit finaliser of a Python int"""
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def fmix32_array(x):
    x = np.asarray(x, dtype=np.uint64) & M32                # (64-bit words, masked: no reliance on wrap-around)
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def buckets(n, t, level):
    key = fmix32(64 * t + level + 1)
    return (fmix32_array(np.arange(n, dtype=np.uint64) ^ key) & 7).astype(np.int64)


def quantise(indptr, indices, weights):
    """the edges without the diagonal as (src, dst, q) in row order, and k"""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    N = indptr.size - 1
    src = np.repeat(np.arange(N, dtype=np.int64), np.diff(indptr))
    q = np.rint(np.asarray(weights, dtype=np.float32).astype(np.float64) * SCALE).astype(np.int64)
    keep = src != indices
    src, dst, q = src[keep], indices[keep], q[keep]
    k = np.zeros(N, dtype=np.int64)
    np.add.at(k, src, q)
    return src, dst, q, k


def run_sums(key, q):
    """key ascending-sortable int64, q int64 -> (the distinct keys ascending, the sum of q per key)"""
    order = np.argsort(key, kind="stable")
    key, q = key[order], q[order]
    if key.size == 0:
        return key, q
    starts = np.nonzero(np.concatenate([[True], key[1:] != key[:-1]]))[0]
    return key[starts], np.add.reduceat(q, starts)


def modularity(inn, tot, M, resolution):
    if inn.size == 0:
        return 0.0
    dM = np.float64(M)
    a = inn.astype(np.float64) / dM
    t = tot.astype(np.float64) / dM
    terms = a - (np.float64(resolution) * t) * t
    return float(np.cumsum(terms)[-1])


def local_move(src, dst, q, k, n, g, level, max_sweeps):
    """-> (comm, sweeps run, nodes moved in all of them)"""
    comm = np.arange(n, dtype=np.int64)
    tot = k.copy()
    sweeps = moved_total = 0
    for t in range(max_sweeps):
        bk = buckets(n, t, level)
        moved = 0
        for b in range(SUBROUNDS):
            act = bk == b
            nodes = np.nonzero(act)[0]
            e = act[src]
            pi = np.concatenate([src[e], nodes])            # (the node's own community is always scored: weight 0 when no neighbour is in it)
            pc = np.concatenate([comm[dst[e]], comm[nodes]])
            pq = np.concatenate([q[e], np.zeros(nodes.size, dtype=np.int64)])
            key, w = run_sums((pi << 32) | pc, pq)
            pi, pc = key >> 32, key & M32
            own = pc == comm[pi]
            kg = k[pi].astype(np.float64) * np.float64(g)
            score = w.astype(np.float64) - kg * (tot[pc] - np.where(own, k[pi], 0)).astype(np.float64)
            stay = np.zeros(n, dtype=np.float64)
            stay[pi[own]] = score[own]
            oi, osc, oc = pi[~own], score[~own], pc[~own]
            o = np.lexsort((oc, -osc, oi))                   # per node: the largest score first, ties by the smallest community
            oi, osc, oc = oi[o], osc[o], oc[o]
            first = np.concatenate([[True], oi[1:] != oi[:-1]]) if oi.size else np.zeros(0, dtype=bool)
            ti, ts, tc = oi[first], osc[first], oc[first]
            mv = ts > stay[ti]
            mi, mc = ti[mv], tc[mv]
            np.subtract.at(tot, comm[mi], k[mi])
            np.add.at(tot, mc, k[mi])
            comm[mi] = mc
            moved += mi.size
        sweeps += 1
        moved_total += moved
        if moved == 0:
            break
    return comm, sweeps, moved_total


def aggregate(src, dst, q, k, inn, comm, n):
    """-> (new id of every node, C, coarse src, dst, q, k, in)"""
    present = np.zeros(n, dtype=bool)
    present[comm] = True
    new = (np.cumsum(present) - 1)[comm]
    C = int(present.sum())
    ck, cin = np.zeros(C, dtype=np.int64), np.zeros(C, dtype=np.int64)
    np.add.at(ck, new, k)
    np.add.at(cin, new, inn)
    cs, cd = new[src], new[dst]
    same = cs == cd
    np.add.at(cin, cs[same], q[same])
    key, w = run_sums((cs[~same] << 32) | cd[~same], q[~same])
    return new, C, key >> 32, key & M32, w, ck, cin


def louvain(indptr, indices, weights, resolution=1.0, max_levels=10, max_sweeps=32):
    src, dst, q, k = quantise(indptr, indices, weights)
    N = k.size
    M = int(k.sum())
    lab = np.arange(N, dtype=np.int64)
    if M == 0:
        return Result(lab.astype(np.int32), N, 0.0, [], [], [], 0, 0)
    g = np.float64(resolution) / np.float64(M)
    inn = np.zeros(N, dtype=np.int64)
    best_lab, best_q, best_level, best_c = lab, modularity(inn, k, M, resolution), 0, N
    lc, ls, lq = [], [], []
    n, total = N, 0
    for level in range(max_levels):
        comm, sweeps, moved = local_move(src, dst, q, k, n, g, level, max_sweeps)
        total += sweeps
        if moved == 0:
            break
        new, n, src, dst, q, k, inn = aggregate(src, dst, q, k, inn, comm, n)
        lab = new[lab]
        Q = modularity(inn, k, M, resolution)
        lc.append(n), ls.append(sweeps), lq.append(Q)
        if Q > best_q:
            best_lab, best_q, best_level, best_c = lab, Q, level + 1, n
    return Result(best_lab.astype(np.int32), best_c, best_q, lc, ls, lq, best_level, total)


def seurat_order(labels):
    """clusters renumbered by decreasing size, ties by the smallest member cell"""
    labels = np.asarray(labels)
    ids, first, counts = np.unique(labels, return_index=True, return_counts=True)
    rank = np.empty(ids.size, dtype=np.int32)
    rank[np.lexsort((first, -counts))] = np.arange(ids.size, dtype=np.int32)
    return rank[np.searchsorted(ids, labels)]


def partition_modularity(indptr, indices, weights, labels, resolution=1.0):
    """Q of any partition of the cells, by the spec's expression"""
    src, dst, q, k = quantise(indptr, indices, weights)
    labels = np.asarray(labels, dtype=np.int64)
    ids, lab = np.unique(labels, return_inverse=True)
    tot, inn = np.zeros(ids.size, dtype=np.int64), np.zeros(ids.size, dtype=np.int64)
    np.add.at(tot, lab, k)
    same = lab[src] == lab[dst]
    np.add.at(inn, lab[src[same]], q[same])
    M = int(k.sum())
    return modularity(inn, tot, M, resolution) if M else 0.0


# ---- a plain sequential Louvain on the same integers: the yardstick of quality -------------------------------------------------------------------
def sequential(indptr, indices, weights, resolution=1.0, max_levels=20, max_sweeps=100):
    """-> (labels, Q): nodes visited one after the other in ascending order, each move applied at once; levels until nothing moves"""
    src, dst, q, k = quantise(indptr, indices, weights)
    N = k.size
    M = int(k.sum())
    lab = np.arange(N, dtype=np.int64)
    if M == 0:
        return lab, 0.0
    inn = np.zeros(N, dtype=np.int64)
    n = N
    for _ in range(max_levels):
        ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))])
        comm, tot = list(range(n)), k.tolist()
        dl, ql, kl = dst.tolist(), q.tolist(), k.tolist()
        any_move = False
        for _ in range(max_sweeps):
            moved = 0
            for i in range(n):
                a, ki = comm[i], kl[i]
                w = {a: 0}
                for e in range(ptr[i], ptr[i + 1]):
                    c = comm[dl[e]]
                    w[c] = w.get(c, 0) + ql[e]
                # the gain of joining c, times M: w_ic M - resolution k_i tot_c (integers but for the resolution)
                best, best_gain = a, w[a] * M - resolution * ki * (tot[a] - ki)
                for c in sorted(w):
                    gain = w[c] * M - resolution * ki * (tot[c] - (ki if c == a else 0))
                    if gain > best_gain:
                        best, best_gain = c, gain
                if best != a:
                    tot[a] -= ki
                    tot[best] += ki
                    comm[i] = best
                    moved += 1
            any_move = any_move or moved > 0
            if moved == 0:
                break
        if not any_move:
            break
        new, n, src, dst, q, k, inn = aggregate(src, dst, q, k, inn, np.asarray(comm, dtype=np.int64), n)
        lab = new[lab]
    return lab, modularity(inn, k, M, resolution)


def adjusted_rand(a, b):
    a, b = np.unique(np.asarray(a), return_inverse=True)[1], np.unique(np.asarray(b), return_inverse=True)[1]
    table = np.zeros((a.max() + 1, b.max() + 1), dtype=np.int64)
    np.add.at(table, (a, b), 1)

    def pairs(x):
        return (x * (x - 1) // 2).sum()
    n = a.size
    sij, sa, sb = pairs(table), pairs(table.sum(axis=1)), pairs(table.sum(axis=0))
    expected = sa * sb / (n * (n - 1) / 2)
    return float((sij - expected) / ((sa + sb) / 2 - expected))


# ---- the hand-checkable graphs ---------------------------------------------------------------------------------------------------------------------
def csr_of_edges(N, edges, weight=1.0, diagonal=False):
    """a symmetric CSR of undirected edges (i, j) or (i, j, w): (indptr int64, indices int32, weights float32)"""
    rows = [dict() for _ in range(N)]
    for e in edges:
        i, j = int(e[0]), int(e[1])
        w = np.float32(e[2] if len(e) > 2 else weight)
        rows[i][j] = w
        rows[j][i] = w
    if diagonal:
        for i in range(N):
            rows[i][i] = np.float32(1.0)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.array([j for r in rows for j in sorted(r)], dtype=np.int32)
    weights = np.array([r[j] for r in rows for j in sorted(r)], dtype=np.float32)
    return indptr, indices, weights


def ring(n):
    return csr_of_edges(n, [(i, (i + 1) % n) for i in range(n)])


def path(n):
    return csr_of_edges(n, [(i, i + 1) for i in range(n - 1)])


def star(n):
    return csr_of_edges(n, [(0, i) for i in range(1, n)])


def complete(n):
    return csr_of_edges(n, [(i, j) for i in range(n) for j in range(i + 1, n)])


def two_cliques():
    """two 6-cliques joined by one edge, and 2 isolated cells"""
    edges = [(i, j) for i in range(6) for j in range(i + 1, 6)] + [(6 + i, 6 + j) for i in range(6) for j in range(i + 1, 6)] + [(5, 6)]
    return csr_of_edges(14, edges)


def planted(N, groups, d=10, seed=0):
    """N points around `groups` well separated centres: (X, the planted labels)"""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(groups, d)) * 8.0
    lab = np.arange(N) % groups
    return centres[lab] + rng.normal(size=(N, d)), lab

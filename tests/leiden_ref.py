"""The spec of the Leiden clustering (include/harmony_mi355x_leiden.h): integers and fp64 only, so that the library agrees bit for bit.

Input: Louvain's (louvain_ref.py): a symmetric CSR, q_ij = rint(w_ij * 2^24).  The diagonal and the entries with q_ij == 0 are dropped: they are
not edges.  k_i = sum_j q_ij, M = sum_i k_i, g = resolution / dbl(M).  One level on n nodes that start in the partition comm (comm[i] = i at
level 0):
  1. local moves: Louvain's hashed sub-rounds (key fmix32(64 t + level + 1)), with one more candidate for node i: community i itself with
     w = 0 ("alone") when comm[i] != i and tot[i] == 0;
  2. the level is recorded: C communities, Q added over them in ascending id;
  3. C == n: converged, the call ends with comm;
  4. refinement inside the communities (key fmix32((64 t + level + 1) ^ 0xFFFFFFFF)): ref[i] = i; a singleton i with
     dbl(P_i) >= (dbl(k_i) g) dbl(ctot - k_i) (P_i: its weight inside its community) that is active joins the refined community r of largest
     score dbl(w_ir) - (dbl(k_i) g) dbl(rtot_r), ties to the smallest r, iff the score is > 0; r must hold an inner neighbour that does not move
     in this sub-round and pass dbl(cut_r) >= (dbl(rtot_r) g) dbl(ctot - rtot_r).  A joiner has positive weight to a member that stays and
     a joined node never moves again, so every refined community is connected through edges of positive weight;
  5. aggregation by ref (Louvain's); the new nodes of one community start the next level together under the smallest new id among them.
The call returns the partition of the last level.
"""
import collections

import numpy as np

import louvain_ref as lr
from louvain_ref import (M32, SUBROUNDS, adjusted_rand, aggregate, buckets, fmix32, fmix32_array, modularity, quantise, run_sums,  # noqa: F401
                         seurat_order)

Result = collections.namedtuple("Result", "labels n_clusters modularity converged level_clusters level_nodes level_sweeps level_refine_sweeps "
                                          "level_modularity")


def refine_key(t, level):
    return fmix32((64 * t + level + 1) ^ M32)


def refine_buckets(n, t, level):
    return (fmix32_array(np.arange(n, dtype=np.uint64) ^ refine_key(t, level)) & 7).astype(np.int64)


def edges(indptr, indices, weights):
    """the edges (src, dst, q) in row order without the diagonal and without q == 0, and k"""
    src, dst, q, k = quantise(indptr, indices, weights)
    keep = q != 0
    return src[keep], dst[keep], q[keep], k


def _targets(pi, pc, w, score):
    """per node of pi: the candidate of largest score, ties to the smallest id -> (node, score, id)"""
    o = np.lexsort((pc, -score, pi))
    pi, pc, score = pi[o], pc[o], score[o]
    first = np.concatenate([[True], pi[1:] != pi[:-1]]) if pi.size else np.zeros(0, dtype=bool)
    return pi[first], score[first], pc[first]


def local_move(src, dst, q, k, comm, g, level, max_sweeps):
    """local moves from the partition comm -> (comm, tot, sweeps run, nodes moved in all of them)"""
    n = k.size
    comm = np.asarray(comm, dtype=np.int64).copy()
    tot = np.zeros(n, dtype=np.int64)
    np.add.at(tot, comm, k)
    sweeps = moved_total = 0
    for t in range(max_sweeps):
        bk = buckets(n, t, level)
        moved = 0
        for b in range(SUBROUNDS):
            act = bk == b
            nodes = np.nonzero(act)[0]
            e = act[src]
            alone = nodes[(comm[nodes] != nodes) & (tot[nodes] == 0)]
            pi = np.concatenate([src[e], nodes, alone])         # (the own community is always scored; alone: id i, empty, weight 0)
            pc = np.concatenate([comm[dst[e]], comm[nodes], alone])
            pq = np.concatenate([q[e], np.zeros(nodes.size + alone.size, dtype=np.int64)])
            key, w = run_sums((pi << 32) | pc, pq)
            pi, pc = key >> 32, key & M32
            own = pc == comm[pi]
            kg = k[pi].astype(np.float64) * np.float64(g)
            score = w.astype(np.float64) - kg * (tot[pc] - np.where(own, k[pi], 0)).astype(np.float64)
            stay = np.zeros(n, dtype=np.float64)
            stay[pi[own]] = score[own]
            ti, ts, tc = _targets(pi[~own], pc[~own], w[~own], score[~own])
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
    return comm, tot, sweeps, moved_total


def refine(src, dst, q, k, comm, tot, g, level, max_sweeps):
    """the refined partition inside the communities of comm -> (ref, sweeps run)"""
    n = k.size
    inner = comm[src] == comm[dst]
    src, dst, q = src[inner], dst[inner], q[inner]
    ctot = tot[comm]
    P = np.zeros(n, dtype=np.int64)
    np.add.at(P, src, q)
    dg = np.float64(g)
    kg = k.astype(np.float64) * dg
    node_ok = P.astype(np.float64) >= kg * (ctot - k).astype(np.float64)
    ref = np.arange(n, dtype=np.int64)
    rtot = k.copy()
    size = np.ones(n, dtype=np.int64)
    sweeps = 0
    for t in range(max_sweeps):
        bk = refine_buckets(n, t, level)
        moved = blocked = 0
        for b in range(SUBROUNDS):
            mover = (bk == b) & (size[ref] == 1) & node_ok
            cut = np.zeros(n, dtype=np.int64)
            leave = ref[src] != ref[dst]
            np.add.at(cut, ref[src[leave]], q[leave])
            cut_ok = cut.astype(np.float64) >= (rtot.astype(np.float64) * dg) * (tot[comm] - rtot).astype(np.float64)      # (indexed by r: ctot of r's own community, r is a node of it)
            e = mover[src]
            blocked += int((e & mover[dst]).sum())
            e &= ~mover[dst] & cut_ok[ref[dst]]
            key, w = run_sums((src[e] << 32) | ref[dst[e]], q[e])
            pi, pr = key >> 32, key & M32
            score = w.astype(np.float64) - kg[pi] * rtot[pr].astype(np.float64)
            ti, ts, tr = _targets(pi, pr, w, score)
            mv = ts > 0.0
            mi, mr = ti[mv], tr[mv]
            ref[mi] = mr
            np.add.at(rtot, mr, k[mi])
            rtot[mi] = 0
            np.add.at(size, mr, 1)
            size[mi] = 0
            moved += mi.size
        sweeps += 1
        if moved == 0 and blocked == 0:
            break
    return ref, sweeps


def level_sums(src, dst, q, inn, comm):
    """-> (the ids in use ascending, in per id: the members' in and both directions of every edge inside)"""
    n = comm.size
    cin = np.zeros(n, dtype=np.int64)
    np.add.at(cin, comm, inn)
    same = comm[src] == comm[dst]
    np.add.at(cin, comm[src[same]], q[same])
    return np.unique(comm), cin


def leiden(indptr, indices, weights, resolution=1.0, max_levels=20, max_sweeps=32):
    src, dst, q, k = edges(indptr, indices, weights)
    N = k.size
    M = int(k.sum())
    lab = np.arange(N, dtype=np.int64)
    if M == 0:
        return Result(lab.astype(np.int32), N, 0.0, True, [], [], [], [], [])
    g = np.float64(resolution) / np.float64(M)
    inn = np.zeros(N, dtype=np.int64)
    comm = np.arange(N, dtype=np.int64)
    lc, ln, ls, lrs, lq = [], [], [], [], []
    converged = False
    for level in range(max_levels):
        n = k.size
        comm, tot, sweeps, moved = local_move(src, dst, q, k, comm, g, level, max_sweeps)
        used, cin = level_sums(src, dst, q, inn, comm)
        Q = modularity(cin[used], tot[used], M, resolution)
        lc.append(int(used.size)), ls.append(sweeps), lq.append(Q), ln.append(n), lrs.append(0)
        if used.size == n:
            converged = True
            break
        if level == max_levels - 1:
            break
        ref, rs = refine(src, dst, q, k, comm, tot, g, level, max_sweeps)
        new, n2, src, dst, q, k, inn = aggregate(src, dst, q, k, inn, ref, n)
        ln[-1], lrs[-1] = n2, rs
        if n2 == n and moved == 0:                           # a guard: nothing merged and nothing moved
            break
        parent = np.full(n, n2, dtype=np.int64)
        np.minimum.at(parent, comm, new)                     # per community: the smallest new id among its refined parts
        nxt = np.zeros(n2, dtype=np.int64)
        nxt[new] = parent[comm]
        lab = new[lab]
        comm = nxt
    final = np.unique(comm, return_inverse=True)[1][lab]
    return Result(final.astype(np.int32), lc[-1], lq[-1], converged, lc, ln, ls, lrs, lq)


def components_within(graph, labels):
    """components over the edges of positive (quantised) weight inside the labels, minus the number of labels: 0 iff every label is connected"""
    import scipy.sparse as sp
    import scipy.sparse.csgraph as csg
    src, dst, q, k = edges(*graph)
    labels = np.asarray(labels)
    same = labels[src] == labels[dst]
    N = k.size
    A = sp.csr_matrix((np.ones(int(same.sum())), (src[same].copy(), dst[same].copy())), shape=(N, N))
    return int(csg.connected_components(A, directed=False)[0]) - int(np.unique(labels).size)


def er(N, deg, seed, weighted):
    """a sparse random graph with weights in {0, 1/16, .., 1} (explicit zeros included) or all 1"""
    rng = np.random.default_rng(seed)
    m = int(N * deg / 2)
    e = rng.integers(0, N, size=(m, 2))
    e = e[e[:, 0] != e[:, 1]]
    w = rng.integers(0, 17, size=len(e)) / 16.0 if weighted else np.ones(len(e))
    return lr.csr_of_edges(N, [(a, b, x) for (a, b), x in zip(e, w)])

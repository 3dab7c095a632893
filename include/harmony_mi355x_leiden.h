/* harmony_mi355x_leiden.h -- Leiden clustering of a neighbour graph on the GPU: scanpy's default clustering (sc.tl.leiden on the
 * connectivities) and Seurat's FindClusters(algorithm = 4), as a deterministic algorithm whose result is a pure function of the input and
 * whose clusters are connected.  Python: harmony_amd/leiden.py (leiden, Harmony.leiden, Harmony.clusters(algorithm = "leiden")).
 * Companion of harmony_mi355x.h (handles, status codes) and of harmony_mi355x_louvain.h, whose input, integers, score and sub-rounds it shares.
 *
 * The graph: hmx_louvain's (a symmetric CSR on the host, indptr [N + 1] int64, indices int32 strictly ascending within a row, weights float
 * with w_ij == w_ji bit for bit, finite and in [0, 1]; fewer than 2^31 stored entries).  q_ij = llrint((double)w_ij * 2^24).  The diagonal is
 * dropped, and so is every entry with q_ij == 0: it is not an edge (hmx_louvain keeps those).  k_i = sum_j q_ij, M = sum_i k_i,
 * g = resolution / (double)M.  M = 0 returns every cell as its own cluster, modularity 0, no level, converged.
 *   bucket(i, key) = fmix32(i ^ key) & 7.  One level on n nodes that start in the partition comm (comm[i] = i at level 0):
 *   1. local moves.  tot[c] = the sum of k_i over the members of c.  Sweep t is 8 sub-rounds, key = fmix32(64 t + level + 1); a sub-round
 *      decides on the comm and tot of its start.  Candidates of the active node i in community a: a, the community of every neighbour, and
 *      "alone" -- c = i with w = 0 -- when comm[i] != i and tot[i] == 0.  score(c) = dbl(w_ic) - (dbl(k_i) g) dbl(tot_c - (c == a ? k_i : 0))
 *      in three rounded fp64 operations that are never fused.  The target is the c != a of largest score, ties to the smallest c; i moves iff
 *      score(target) > score(a).  Then the moves are applied.  The phase ends after a sweep without a move or after max_sweeps.
 *   2. the level is recorded: C = the communities in use; Q = sum_c (dbl(in_c) / dbl(M) - (resolution (dbl(tot_c) / dbl(M))) (dbl(tot_c) /
 *      dbl(M))), added in ascending id of c, in_c = the members' in plus both directions of every edge inside c.
 *   3. C == n: converged; the call ends with this level's partition.  Level max_levels - 1 ends the call as well, not converged.
 *   4. refinement inside the communities ("inner": an edge whose ends share a community).  ctot = the community's tot, P_i = the sum of the
 *      inner q_ij, node_ok[i] = dbl(P_i) >= (dbl(k_i) g) dbl(ctot - k_i); ref[i] = i, rtot[r] = k_r, size[r] = 1.  Sweep t is 8 sub-rounds,
 *      key = fmix32((64 t + level + 1) ^ 0xFFFFFFFF).  i is a mover iff it is active, size[ref[i]] == 1 and node_ok[i].  From the state of the
 *      sub-round's start, with cut_r = the sum of q over the inner edges that leave r: r is a candidate of the mover i iff i has an inner
 *      neighbour in r that is no mover of this sub-round and dbl(cut_r) >= (dbl(rtot_r) g) dbl(ctot - rtot_r); score(r) = dbl(w_ir) -
 *      (dbl(k_i) g) dbl(rtot_r); the target is the largest score, ties to the smallest r; i joins it iff score > 0.  The refinement ends after
 *      a sweep without a move and without an inner edge between two movers of one sub-round, or after max_sweeps.
 *   5. aggregation by ref, as hmx_louvain aggregates by comm; the new nodes of one community start the next level together:
 *      comm'[new(r)] = the smallest new(r') over the r' refined from r's community.  If nothing merged and nothing had moved the call ends,
 *      not converged (a guard).
 * The call returns the partition of the last level: labels [N] in 0 .. *n_clusters - 1 in ascending order of the communities' ids,
 * *modularity its Q, *converged 1 or 0.  When converged, every cluster is connected through edges of positive q: a joiner of step 4 has such an
 * edge to a member that stays, and a node that has been joined never moves again.  level_clusters, level_nodes (the nodes after the
 * refinement; of a level that ended the call, its own nodes), level_sweeps, level_refine_sweeps, level_modularity: optional, max_levels
 * entries each, of which the recorded levels ("leiden:levels") are written.  Two calls give the same bits; tests/leiden_ref.py is the same
 * algorithm in NumPy and agrees bit for bit.
 *
 * Argument checks, limits and statuses: hmx_louvain's (a null pointer but the five optional ones, N < 1, resolution outside (0, 100],
 * max_levels outside 1 .. 64, max_sweeps outside 1 .. 4096, a malformed indptr: HMX_ERR_ARG before a device is touched; a malformed pattern or
 * weight: HMX_ERR_ARG from the device before anything else runs, no output written; HMX_ERR_LIMIT: N > 2e9, 2^31 stored entries or more).
 * Wall time: "timer:leiden" (its parts: "timer:leiden_moves" with the levels' records, "timer:leiden_refine", "timer:leiden_aggregate").
 * hmx_get, of the last call: "leiden:levels", "leiden:sweeps" and "leiden:refine_sweeps" (of all levels), "leiden:clusters",
 * "leiden:converged", "leiden:long_rows" (the rows of level 0 with more edges than "louvain:short_cap", which the test switch
 * "louvain_short_cap" sets for this call too). */
#ifndef HARMONY_MI355X_LEIDEN_H
#define HARMONY_MI355X_LEIDEN_H

#include "harmony_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int hmx_leiden(hmx_ctx* ctx, const int64_t* indptr, const int32_t* indices, const float* weights, int64_t N, double resolution,
               int32_t max_levels, int32_t max_sweeps, int32_t* labels, int32_t* n_clusters, double* modularity, int32_t* converged,
               int32_t* level_clusters, int32_t* level_nodes, int32_t* level_sweeps, int32_t* level_refine_sweeps, double* level_modularity);

#ifdef __cplusplus
}
#endif
#endif

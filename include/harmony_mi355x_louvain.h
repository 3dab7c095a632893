/* harmony_mi355x_louvain.h -- Louvain clustering of a neighbour graph on the GPU: what Seurat's FindClusters does with the SNN graph, as a
 * deterministic algorithm whose result is a pure function of the input.  Python: harmony_amd/louvain.py (louvain, Harmony.clusters).
 * Companion of harmony_mi355x.h (handles, status codes), of harmony_mi355x_snn.h and harmony_mi355x_graph.h, whose graphs it reads.
 *
 * The graph: a symmetric CSR on the host, indptr [N + 1] int64, indices int32 strictly ascending within a row, weights float with
 * w_ij == w_ji bit for bit, finite and in [0, 1] (other callers divide by their largest weight).  Fewer than 2^31 stored entries.  The diagonal
 * may be stored and is ignored; every other stored entry is an edge, also one of weight 0.
 *   q_ij   = llrint((double)w_ij * 2^24), an int64; k_i = sum_j q_ij; M = sum_i k_i.  Every sum is an integer sum: its order does not matter.
 *            M = 0 returns every cell as its own cluster, modularity 0, no level.
 *   level  comm[i] = i, tot[c] = k_c, g = resolution / (double)M.  Sweep t = 0, 1, .. is 8 sub-rounds; node i is active in sub-round
 *            fmix32(i ^ fmix32(64 t + level + 1)) & 7 (murmur3's 32-bit finaliser).  A sub-round first decides, from the comm and tot of its
 *            start alone: for the active node i in community a and every community c of a neighbour and a itself, w_ic = the sum of q_ij
 *            over the neighbours in c, score(c) = dbl(w_ic) - (dbl(k_i) g) dbl(tot_c - (c == a ? k_i : 0)) in three correctly rounded fp64
 *            operations that are never fused; the target is the c != a of largest score, ties to the smallest c; i moves iff
 *            score(target) > score(a).  Then it applies the moves.  The level ends after a sweep without a move or after max_sweeps.
 *   next   the non-empty communities are renumbered 0 .. C - 1 in ascending order of their id; W_cc' = the sum of q_ij over i in c, j in c';
 *            in_c = sum in_i + the q_ij inside c; k_c = sum k_i.  A level in which nothing moved ends the call and is not recorded.
 *   Q      = sum_c (dbl(in_c) / dbl(M) - (resolution (dbl(tot_c) / dbl(M))) (dbl(tot_c) / dbl(M))), added in ascending c in fp64.
 * The call returns the labels of the first recorded level with the largest Q -- synchronous moves can lower Q --, the singletons if no level
 * beats theirs: labels [N] in 0 .. *n_clusters - 1 in the order of the renumbering, *modularity its Q.  level_clusters, level_sweeps,
 * level_modularity: optional, max_levels entries each, of which the recorded levels ("louvain:levels") are written.  Two calls give the same
 * bits; tests/louvain_ref.py is the same algorithm in NumPy and agrees bit for bit.
 *
 * HMX_ERR_ARG: a null pointer (but the optional ones), N < 1, resolution outside (0, 100] or NaN, max_levels outside 1 .. 64, max_sweeps
 * outside 1 .. 4096, indptr not ascending from 0 or a row longer than N -- all checked before a device is touched --, an index out of range,
 * a row not ascending, an edge without its mirror or with another weight, a weight outside [0, 1] or not finite -- checked on the device
 * before anything else runs.  HMX_ERR_LIMIT: N > 2e9, 2^31 stored entries or more.
 * Wall time: "timer:louvain".  hmx_get, of the last call: "louvain:levels" the recorded levels; "louvain:best_level" the level returned (1 the
 * first, 0 the singletons); "louvain:sweeps" the sweeps of all levels, the last one's included; "louvain:clusters"; "louvain:long_rows" the
 * rows of level 0 with more than "louvain:short_cap" entries, which one workgroup walks in windows of community ids instead of one wave
 * sorting them in LDS. */
#ifndef HARMONY_MI355X_LOUVAIN_H
#define HARMONY_MI355X_LOUVAIN_H

#include "harmony_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int hmx_louvain(hmx_ctx* ctx, const int64_t* indptr, const int32_t* indices, const float* weights, int64_t N, double resolution,
                int32_t max_levels, int32_t max_sweeps, int32_t* labels, int32_t* n_clusters, double* modularity,
                int32_t* level_clusters, int32_t* level_sweeps, double* level_modularity);

#ifdef __cplusplus
}
#endif
#endif

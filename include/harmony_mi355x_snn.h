/* harmony_mi355x_snn.h -- Seurat's shared-nearest-neighbour graph of an embedding on the GPU: what FindNeighbors builds and FindClusters
 * reads, the Jaccard overlap of the k-nearest-neighbour sets, pruned.  Python: harmony_amd/snn.py (snn, snn_from_knn, Harmony.snn).
 * Companion of harmony_mi355x.h (handles, status codes), of harmony_mi355x_metrics.h, whose hmx_knn produces the lists this header reads,
 * and of harmony_mi355x_graph.h, whose `capacity` rule it follows.
 *
 * The neighbour lists: idx [N][m] int32, SELF EXCLUDED, as hmx_knn(Q = NULL) returns them; idx -1 marks an unfilled slot.  A row lists a
 * cell at most once and never itself.  Seurat's k.param is k = m + 1: it counts the cell itself, so 2 <= k <= 129.
 *   N+(i)   = {i} and the valid idx[i][.]; A is the N x N 0/1 matrix of these sets (Seurat's `nn` graph, diagonal included);
 *   s_il    = |N+(i) & N+(l)| = (A A^T)_il, an integer in 0 .. k; s_ii = 1 + (valid entries of row i);
 *   J(s)    = s / (2k - s), formed in fp64 on the host for s = 0 .. k and rounded once to fp32: a table the kernels look up.  k stays m + 1
 *             in the denominator even for a row with unfilled slots;
 *   prune   an entry is dropped when J(s) < prune in fp64 (0 <= prune <= 1; Seurat's default 1 / 15).  The host turns this into one integer,
 *             s_min = the smallest s in 1 .. k + 1 with (double)s / (double)(2k - s) >= prune, and an entry is kept iff s >= s_min: prune = 0
 *             keeps every s >= 1; k = 20 with 1 / 15 keeps s >= 3; k = 8 with 1 / 15 keeps s = 1 (the two doubles are equal, the test is <).
 * The graph: CSR, indptr [N + 1] int64, indices int32 ascending within a row, weights float, all on the host.  The diagonal is kept unless
 * it is pruned, as Seurat keeps it.  The matrix is symmetric bit for bit, since s is.  There is no O(N m) bound on the number of entries: a
 * cell listed by D others makes those D rows mutually adjacent before pruning.  `capacity`: the entries `indices` and `weights` hold;
 * capacity < indptr[N] returns HMX_ERR_LIMIT with indptr written and nothing else, so that a caller can size exactly and call again.
 * The kernels do no floating-point arithmetic and use integer atomics only: two calls give the same bits.
 *
 * hmx_snn_from_knn   the SNN graph of lists on the host.  HMX_ERR_ARG: a null pointer, N < 1, m < 1, an index outside [-1, N), a row that
 *                    lists itself or a cell twice, prune outside [0, 1] or NaN, capacity < 0.  HMX_ERR_LIMIT: m > 128, N > 2e9.
 * hmx_snn_graph      exact kNN (hmx_knn, self excluded, m = k - 1) and the SNN graph in one call; the lists stay in HBM.  X: N x d rows of
 *                    x_dtype at x_location, or NULL: the handle's current Z_corr (N must be the handle's cell count; d is ignored;
 *                    HMX_ERR_STATE on a handle without an embedding).  knn_idx, knn_dist: optional outputs (host, [N][m]).
 *                    HMX_ERR_LIMIT: k outside 2 .. 129 or above N, d > 128, N > 2e9.
 * Arguments are checked before a device is touched.  The calls need no fitted state (but X == NULL) and leave none but timers and counters.
 * Wall time: "timer:knn" and "timer:snn" (hmx_snn_graph), "timer:snn" (hmx_snn_from_knn).  hmx_get, of the last call: "snn:s_min" the
 * integer pruning threshold; "snn:short_cap" the largest candidate count (sum over j in N+(i) of in-degree(j) + 1) a row may have to be
 * sorted by one wave in LDS; "snn:window" the cells of the dense counter window that longer rows are walked in; "snn:long_rows" the rows
 * that took that long path. */
#ifndef HARMONY_MI355X_SNN_H
#define HARMONY_MI355X_SNN_H

#include "harmony_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int hmx_snn_from_knn(hmx_ctx* ctx, const int32_t* idx, int64_t N, int32_t m, double prune,
                     int64_t* indptr, int32_t* indices, float* weights, int64_t capacity);

int hmx_snn_graph(hmx_ctx* ctx, const void* X, int32_t x_dtype, int32_t x_location, int64_t N, int32_t d, int32_t k, double prune,
                  int32_t* knn_idx, float* knn_dist,
                  int64_t* indptr, int32_t* indices, float* weights, int64_t capacity);

#ifdef __cplusplus
}
#endif
#endif

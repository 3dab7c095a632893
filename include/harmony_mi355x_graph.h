/* harmony_mi355x_graph.h -- the neighbour graph of an embedding on the GPU, in the form scanpy stores it: `connectivities`, UMAP's fuzzy
 * simplicial set of the exact k nearest neighbours, as a CSR matrix, next to the neighbour lists that are scanpy's `distances`; and the
 * connected components of a symmetric graph, optionally restricted to the edges whose two ends carry one label (scib's graph connectivity).
 * Python: harmony_amd/graph.py (neighbors, graph_from_knn, connected_components, graph_connectivity).  Companion of harmony_mi355x.h (handles,
 * status codes) and of harmony_mi355x_metrics.h, whose hmx_knn produces the lists this header reads.
 *
 * The neighbour lists: idx [N][m] int32 and dist [N][m] float (Euclidean), SELF EXCLUDED, as hmx_knn(Q = NULL) returns them; idx -1 marks an
 * unfilled slot whose dist is ignored.  A row lists a cell at most once.  scanpy's n_neighbors is m + 1 (its column 0 is the cell itself).
 * local_connectivity = 1 and set_op_mix_ratio = 1, scanpy's values, are fixed.  Per cell i over its valid entries, in fp64:
 *   rho_i    the smallest positive distance of the row, 0 if it has none;
 *   sigma_i  the bisection of umap-learn's smooth_knn_dist for target = log2(m + 1): lo = 0, hi = inf, mid = 1, at most 64 steps of
 *            psum = sum_j (d_ij - rho_i > 0 ? exp(-(d_ij - rho_i) / mid) : 1); stop when |psum - target| < 1e-5; psum > target: hi = mid,
 *            mid = (lo + hi) / 2; else lo = mid and mid = 2 mid while hi is infinite, (lo + hi) / 2 after; sigma_i = mid, floored at
 *            1e-3 mean_i when rho_i > 0 (mean_i = sum_j d_ij / (m + 1): the self zero counts), else at 1e-3 mean_all (all rows' mean);
 *   w_ij     1 where d_ij - rho_i <= 0 or sigma_i = 0, else exp(-(d_ij - rho_i) / sigma_i): the membership of the directed edge i -> j.
 * A row without a valid entry has rho = sigma = 0.
 * The graph: row i of the CSR holds the UNION of {j in idx[i]} and {j : i in idx[j]}, ascending in j, no self loop, with the weight
 * a + b - a b (a = w_ij, 0 if i does not list j; b = w_ji likewise), formed in fp64 and rounded once to fp32.  The pattern is a function of
 * idx alone: a weight that underflows stays as an explicit 0.  indptr [N + 1] int64, indices int32, weights float, all on the host;
 * indptr[N] <= 2 N m entries.  `capacity`: the entries `indices` and `weights` hold; capacity < indptr[N] returns HMX_ERR_LIMIT with indptr
 * written and nothing else, so that a caller can size exactly and call again.  rho, sigma: optional outputs (host, double [N]).
 * Integer atomics only and fixed summation orders: two calls give the same bits.
 *
 * hmx_graph_from_knn    the graph of lists on the host.  HMX_ERR_ARG: an index outside [-1, N), idx[i][j] == i, a NaN distance of a valid
 *                       entry, a row that lists a cell twice (found on the device), a null pointer, N < 1, m < 1, capacity < 0.
 *                       HMX_ERR_LIMIT: m > 128, N > 2e9.
 * hmx_neighbor_graph    exact kNN (hmx_knn, self excluded, m = n_neighbors - 1) and the graph in one call; the lists stay in HBM.  X: N x d rows
 *                       of x_dtype at x_location, or NULL: the handle's current Z_corr (N must be the handle's cell count; d is ignored).
 *                       knn_idx, knn_dist: optional outputs (host, [N][m]), scanpy's `distances` row by row.  HMX_ERR_LIMIT: n_neighbors
 *                       outside 2 .. 129 or above N, d > 128, N > 2e9.
 * hmx_graph_components  comp[i] (host, int32 [N]) = the smallest cell index of i's connected component in the symmetric CSR pattern
 *                       (indptr, indices: host; rows strictly ascending; self loops are allowed and ignored).  labels (host, int32 [N], or
 *                       NULL): only edges whose two ends carry the same label >= 0 count; a cell labelled -1 is a component of its own.
 *                       n_components (optional): the number of components.  HMX_ERR_ARG: indptr not ascending from 0 or a row longer
 *                       than N (checked on the host), a label below -1, an index outside [0, N), an unsorted row or an edge without its
 *                       mirror (checked on the device before anything else runs).  HMX_ERR_INTERNAL: 64 hook-and-jump rounds did not
 *                       suffice (they halve the number of trees: this cannot happen below 2^63 cells).  hmx_get "graph:cc_rounds": the rounds
 *                       of the last call.
 * Arguments are checked before a device is touched.  The calls need no fitted state (but X == NULL) and leave none.
 * Wall time: "timer:knn" and "timer:graph" (hmx_neighbor_graph), "timer:graph" (hmx_graph_from_knn), "timer:components". */
#ifndef HARMONY_MI355X_GRAPH_H
#define HARMONY_MI355X_GRAPH_H

#include "harmony_mi355x.h"

/* a status of this header's own, behind harmony_mi355x.h's: a bound the algorithm guarantees was hit (a defect of the library, not of the call) */
#define HMX_ERR_INTERNAL 9

#ifdef __cplusplus
extern "C" {
#endif

int hmx_graph_from_knn(hmx_ctx* ctx, const int32_t* idx, const float* dist, int64_t N, int32_t m,
                       int64_t* indptr, int32_t* indices, float* weights, int64_t capacity,
                       double* rho, double* sigma);

int hmx_neighbor_graph(hmx_ctx* ctx, const void* X, int32_t x_dtype, int32_t x_location, int64_t N, int32_t d, int32_t n_neighbors,
                       int32_t* knn_idx, float* knn_dist,
                       int64_t* indptr, int32_t* indices, float* weights, int64_t capacity,
                       double* rho, double* sigma);

int hmx_graph_components(hmx_ctx* ctx, int64_t N, const int64_t* indptr, const int32_t* indices, const int32_t* labels,
                         int32_t* comp, int64_t* n_components);

#ifdef __cplusplus
}
#endif
#endif

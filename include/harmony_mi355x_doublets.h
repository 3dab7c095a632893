/* harmony_mi355x_doublets.h -- doublet detection on the GPU in the manner of Scrublet (Wolock, Lopez & Klein, Cell Systems 2019): synthetic
 * doublets are the summed raw counts of random pairs of observed cells, pushed through the same normalisation and loadings as the observed
 * cells; every cell is then scored by the share of synthetic cells among its nearest neighbours in the combined set.  Companion of
 * harmony_mi355x.h (handles, status codes) in the way harmony_mi355x_project.h and harmony_mi355x_metrics.h are; the same library exports these
 * entry points.  The scores themselves (Scrublet's Bayesian likelihood, the threshold between the two modes of the simulated scores) are
 * closed-form functions of the neighbour counts: harmony_amd.doublets. */
#ifndef HARMONY_MI355X_DOUBLETS_H
#define HARMONY_MI355X_DOUBLETS_H

#include "harmony_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* P = n_sim synthetic doublets in the d PCs of the reference, straight from the CSR matrix of the N observed cells x G_all genes.
 *   The matrix, slot, U, mean, sd, G, d, scale, clip and totals are those of the count projection (harmony_mi355x_project.h) with the same
 *   checks: indptr [N + 1] int64, indices [nnz] int32, data [nnz] of data_dtype, all three on the host or all three in HBM (csr_location);
 *   values finite and >= 0, no column twice in a row, rows need not be sorted.
 *   pairs [n_sim][2] int64 (host): the two parents of every synthetic cell, each in [0, N); a == b is allowed (Scrublet draws with replacement).
 * Synthetic cell s with parents (a, b): T_s = T_a + T_b (the library sizes over ALL G_all columns, fp64, or the caller's totals);
 * x_sj = x_aj + x_bj for every reference slot j either parent stores; y = log1p(x_sj scale / T_s), w = min(y, mean_j + clip sd_j) / sd_j;
 * P[s,:] = b + sum_j w U[j,:] with the projection's b.  T_s = 0: y = 0.  The counts are added BEFORE the log: this is not the projection of
 * either parent, nor their mean.  x_a + x_b, w and the sum are fp32; the sum runs over j in ASCENDING slot order, so the result is a function
 * of the two rows as sets: a permutation of the entries inside a CSR row, (a, b) against (b, a), two calls, a host- against a device-resident
 * matrix and the position of a pair in `pairs` all give the same bits.  With u = 2^-24 and n_s distinct contributing slots
 *   |P - exact|_sj <= (n_s + 18) u sum_g |w_sg| |U_gj| + 2 u |b_j|.
 *   out: d x n_sim column-major float (cells x PCs row-major), the layout hmx_project_counts writes, on the host or in HBM (out_location).
 *
 * Needs no fitted state and leaves none: any handle serves.  Checked before the device is touched -- HMX_ERR_ARG: what hmx_project_counts
 * refuses, n_sim < 1, a parent outside [0, N); HMX_ERR_LIMIT: d > 128, G above 16128 (a wave keeps one fp32 word per reference gene in LDS:
 * 4 waves per workgroup up to G = 3840, 2 up to 7936, 1 up to 16128), G_all > 2^24.  A host-resident matrix is validated as in
 * hmx_project_counts and uploaded WHOLE in chunked copies into buffers that live for the call (the parents of a pair are arbitrary rows); one
 * that does not fit the free HBM is refused with HMX_ERR_LIMIT and its size in the text.  A device-resident matrix is guarded by the kernel
 * as in hmx_project_counts: HMX_ERR_ARG, the output then undefined.  No device: HMX_ERR_DEVICE.  Wall time of the last call:
 * "timer:simulate_doublets". */
int hmx_simulate_doublets(hmx_ctx* ctx, int64_t N, int32_t G_all,
                          const int64_t* indptr, const int32_t* indices, const void* data, int32_t data_dtype, int32_t csr_location,
                          const int32_t* slot,
                          const double* U, const double* mean, const double* sd, int32_t G, int32_t d,
                          double scale, double clip, const double* totals,
                          int64_t n_sim, const int64_t* pairs,
                          void* out, int32_t out_location);

/* n_sim_neighbors_out [n_obs + n_sim] (host): for every row of X, how many of its k_adj nearest OTHER rows are synthetic (index >= n_obs).
 *   X [n_obs + n_sim][d] row-major of x_dtype, on the host or in HBM (x_location): the observed cells first, then the synthetic ones.
 *   The neighbours are hmx_knn's (exact, Euclidean, self excluded, ties to the smaller index); the counts are integers: the same in every call.
 *   knn_idx_out / knn_dist_out [n_obs + n_sim][k_adj] (host) or NULL: the lists themselves, as hmx_knn returns them.
 * HMX_ERR_ARG: a null or non-positive argument; HMX_ERR_LIMIT: outside 1 <= k_adj <= 128, k_adj >= n_obs + n_sim, d > 128.
 * Wall time of the last call: "timer:knn" (the search) and "timer:doublet_neighbors" (the counts behind it). */
int hmx_doublet_neighbors(hmx_ctx* ctx, const void* X, int32_t x_dtype, int32_t x_location, int64_t n_obs, int64_t n_sim, int32_t d, int32_t k_adj,
                          int32_t* n_sim_neighbors_out, int32_t* knn_idx_out, float* knn_dist_out);

#ifdef __cplusplus
}
#endif
#endif

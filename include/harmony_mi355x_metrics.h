/* harmony_mi355x_metrics.h -- scoring an integration on the GPU: exact k nearest neighbours, LISI (the local inverse Simpson's index
 * of the Harmony paper, immunogenomics/LISI) and what kNN label transfer needs.  Companion of harmony_mi355x.h (handles, status codes,
 * HMX_F64 / HMX_F32, HMX_HOST / HMX_DEVICE); the same library exports these entry points.
 *
 * The handle supplies the device (hmx_set_int "device"), the stream and the error text; the calls need no fitted state and leave none:
 * they work on a fresh handle, a fitted one or a query handle.  Arguments are checked before the device is touched (HMX_ERR_ARG /
 * HMX_ERR_LIMIT); without a HIP device the calls fail with HMX_ERR_DEVICE -- there is no CPU fallback.  Wall time of the last call:
 * "timer:knn" / "timer:lisi" through the scalar getter.
 *
 * Matrices are cells x PCs row-major (= d x N column-major, the layout of the embedding everywhere else in this interface). */
#ifndef HARMONY_MI355X_METRICS_H
#define HARMONY_MI355X_METRICS_H

#include "harmony_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Exact k nearest neighbours of the Nq rows of Q among the N rows of X (Euclidean; fp32 storage, squared distances as
 * |q|^2 + |x|^2 - 2 q.x with the dot product on the fp32 matrix cores).  Q == NULL: the rows of X themselves with self excluded -- row i
 * never returns index i (by index, not by distance: duplicates of a cell are returned); q_dtype / q_location / Nq are then ignored.
 * Per query row, sorted ascending by (computed squared distance, data index): idx[Nq][k] (0-based) and dist[Nq][k] = sqrt(max(d2, 0)),
 * both on the host or both in HBM (out_location).  Ties go to the smaller index; two calls on the same input are bit-identical.
 * Envelope: 1 <= d <= 128, 1 <= k <= 128, k <= N (k <= N - 1 with self excluded), N, Nq <= 2e9.  Rows with non-finite values have no
 * defined neighbours (slots that cannot be filled hold index -1 and distance +inf). */
int hmx_knn(hmx_ctx* ctx, const void* X, int32_t x_dtype, int32_t x_location, int64_t N,
            const void* Q, int32_t q_dtype, int32_t q_location, int64_t Nq,
            int32_t d, int32_t k, int32_t* idx, float* dist, int32_t out_location);

/* LISI of Nq cells from their neighbour lists (host arrays): idx[Nq][m] indices into the N labelled cells, dist[Nq][m] Euclidean distances
 * (not squared), labels[n_cols][N] 0-based level codes with n_levels[c] levels in column c, 1 <= m <= 128.  Per cell the weights
 * P_j = exp(-D_j beta) / sum are searched for entropy ln(perplexity) (beta from 1, doubling / halving, then bisection; tolerance 1e-5, at
 * most 50 steps), once for all columns; out[Nq][n_cols] = 1 / sum over levels of (sum of P_j with that label)^2, or -1 where the entropy
 * is exactly 0 (every weight underflowed), as the LISI package returns.  fp64 on the device. */
int hmx_lisi(hmx_ctx* ctx, const int32_t* idx, const float* dist, int64_t Nq, int32_t m,
             const int32_t* labels, int64_t N, int32_t n_cols, const int32_t* n_levels, double perplexity, double* out);

/* Both stages without the neighbour lists leaving HBM: the m = floor(3 perplexity) - 1 nearest neighbours of every row of X with self
 * excluded, then the LISI of every cell over every label column into out[N][n_cols] (host).  X == NULL: the handle's current Z_corr
 * (a fitted or a query handle; x_dtype / x_location / d are ignored, N must be the handle's cell count, labels in the order the cells were
 * given in).  HMX_ERR_LIMIT when m > 128 or m > N - 1. */
int hmx_compute_lisi(hmx_ctx* ctx, const void* X, int32_t x_dtype, int32_t x_location, int64_t N, int32_t d,
                     const int32_t* labels, int32_t n_cols, const int32_t* n_levels, double perplexity, double* out);

#ifdef __cplusplus
}
#endif
#endif

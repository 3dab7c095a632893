/* harmony_mi355x_confidence.h -- mapping confidence on the GPU: the soft clusters' moments of a fitted reference, and the per-cell
 * Mahalanobis score of a mapped query against them (Symphony's calcPerCellMappingMetric, Kang et al., Nat. Commun. 2021).  Companion of
 * harmony_mi355x.h (handles, status codes) in the way harmony_mi355x_metrics.h and harmony_mi355x_silhouette.h are; the same library
 * exports these entry points.
 *
 * Arguments and state are checked before the device is touched (HMX_ERR_ARG / HMX_ERR_STATE / HMX_ERR_SOLVE); there is no CPU
 * fallback.  Both calls leave the handle as it was.  Wall time of the last call: "timer:reference_moments" / "timer:mapping_confidence"
 * through the scalar getter. */
#ifndef HARMONY_MI355X_CONFIDENCE_H
#define HARMONY_MI355X_CONFIDENCE_H

#include "harmony_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* which rows of a handle a call measures on: its Z_orig rows or its Z_corr rows.  Reference and query must use the same space. */
#define HMX_SPACE_ORIG 0
#define HMX_SPACE_CORR 1

/* The R-weighted moments of every soft cluster of a fitted handle, from its current R (K x N; R must be valid, as for hmx_get "ref_Nr") and
 * the rows z_i of `space`.  Per cluster k, with S0 = sum_i R[k,i] and w_i = R[k,i] / S0:
 *   mean[k + K j]        mu_k = sum_i w_i z_i                                              (K x d, column-major like "ref_C")
 *   cov[(k d + j) d + j'] sum_i w_i (z_i - mu_k)(z_i - mu_k)^T / (1 - sum_i w_i^2)          ([K][d][d], symmetric)
 * -- R's cov.wt(method = "unbiased"), numpy's cov(aweights = R[k]).  A cluster with S0 = 0 or 1 - sum w^2 <= 0 fails the call with
 * HMX_ERR_SOLVE; the error text names it.  Products are added in fp32 for at most 128 terms before they reach an fp64 sum; no atomics: two
 * calls on the same state are bit-identical.  On a sharded handle the call is COLLECTIVE: every rank calls, every rank gets the global
 * moments.  A query handle: HMX_ERR_STATE. */
int hmx_reference_moments(hmx_ctx* ctx, int32_t space, double* mean, double* cov);

/* The mapping confidence of a query handle (after hmx_map_query; HMX_ERR_STATE otherwise) against the moments of its reference.  With
 * cov_k + ridge I = L_k L_k^T (Cholesky in fp64 on the host; a failure: HMX_ERR_SOLVE, the error text names the cluster), U_k = L_k^-1:
 *   dist[i K + k] = || U_k (z_i - mu_k) ||_2                  (float, row-major [Nq][K]; dist may be NULL)
 *   score[i]      = sum_k R[k,i] dist[i,k]                    (fp64 sum in cluster order)
 * both in the order the cells were given in; R is the query's own soft assignment, exactly what hmx_get_matrix "R" returns, z_i its row of
 * `space`.  K and d must equal the handle's (HMX_ERR_ARG); mean / cov as hmx_reference_moments lays them out, finite (HMX_ERR_ARG);
 * ridge >= 0 (HMX_ERR_ARG).  Two calls on the same input are bit-identical, with or without dist. */
int hmx_mapping_confidence(hmx_ctx* ctx, int32_t space, const double* mean, const double* cov, int32_t K, int32_t d,
                           double ridge, double* score, float* dist);

#ifdef __cplusplus
}
#endif
#endif

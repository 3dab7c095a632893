/* harmony_mi355x_project.h -- raw query counts into the reference's PC space on the GPU: the first three steps of Symphony's mapQuery
 * (Kang et al., Nat. Commun. 2021): library-size normalise and log1p, scale every variable gene by the REFERENCE's mean and standard
 * deviation, multiply by the reference's gene loadings.  Companion of harmony_mi355x.h (handles, status codes) in the way
 * harmony_mi355x_metrics.h, harmony_mi355x_silhouette.h and harmony_mi355x_confidence.h are; the same library exports this entry point.
 *
 * The loadings, means and standard deviations come from whatever produced the reference's PCs: harmony_mi355x_pca.h's operator driven by
 * harmony_amd.pca.fit_loadings, or another package (scanpy: varm["PCs"], var["mean"], var["std"]; Seurat: Loadings). */
#ifndef HARMONY_MI355X_PROJECT_H
#define HARMONY_MI355X_PROJECT_H

#include "harmony_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* P = the Nq query cells in the d PCs of the reference, from a CSR matrix of Nq cells x G_all query genes.
 *   indptr [Nq + 1] int64, indices [nnz] int32, data [nnz] of data_dtype (HMX_F32 | HMX_F64); all three on the host or all three in HBM
 *     (csr_location).  Values are finite and >= 0, no column twice in a row; rows need not be sorted; nnz may exceed 2^31.
 *   slot [G_all] (host): -1, or the row j in [0, G) of the reference's tables the query gene corresponds to; every j at most once.
 *   U [G][d] row-major (the loadings), mean [G] >= 0, sd [G] > 0 (host).
 *   scale > 0 (Symphony / scanpy: 1e4); clip: scanpy's max_value, <= 0: none; totals [Nq] (host) or NULL: the row sums over all G_all columns.
 * Per cell i with library size T_i, for every stored entry x of a gene with slot j >= 0: y = log1p(x scale / T_i), s_ij = (y - mean_j) / sd_j,
 * min(s_ij, clip) with a clip; a reference gene that the query has (j in the image of slot) but row i does not store: s_ij = -mean_j / sd_j;
 * a reference gene the query lacks contributes nothing (Symphony fills it with zero after scaling).  P[i,:] = sum_j s_ij U[j,:].  T_i = 0: y = 0.
 * Evaluated as P[i,:] = b + sum over the stored entries of w U[j,:], b = sum_{j present} (-mean_j / sd_j) U[j,:] in fp64 on the host,
 * w = min(y, mean_j + clip sd_j) / sd_j in fp32, added in CSR order in fp32: with u = 2^-24 and n_i contributing entries
 *   |P - exact|_ij <= (n_i + 16) u sum_g |w_ig| |U_gj| + 2 u |b_j|.
 * No atomics on results: two calls, host- or device-resident, are bit-identical, and a row's result does not depend on the other rows.
 *   out: d x Nq column-major float (cells x PCs row-major), the layout hmx_map_query takes, on the host or in HBM (out_location).
 *
 * Needs no fitted state and leaves none: any handle serves.  Checked before the device is touched -- HMX_ERR_ARG: a null or non-positive
 * argument, slot out of range or two genes on one row, sd <= 0 or non-finite, mean < 0, scale <= 0, totals negative; HMX_ERR_LIMIT: d > 128,
 * G or G_all > 2^24.  A host-resident matrix is validated before anything is launched (indptr monotone from 0, columns within [0, G_all)):
 * HMX_ERR_ARG.  A device-resident one cannot be: the kernel checks every indptr pair against nnz = indptr[Nq] and every column, treats an
 * offending entry (also a negative or non-finite value, wherever the matrix lives) as absent, and the call returns HMX_ERR_ARG with the first
 * kind of violation in the error text; the output is then undefined.  No device: HMX_ERR_DEVICE.  A host-resident matrix is uploaded in
 * slabs of whole cells (capped by bytes) through two staging sets, the copy of one slab beside the kernel of the one before.
 * Wall time of the last call: "timer:project". */
int hmx_project_counts(hmx_ctx* ctx, int64_t Nq, int32_t G_all,
                       const int64_t* indptr, const int32_t* indices, const void* data, int32_t data_dtype, int32_t csr_location,
                       const int32_t* slot,
                       const double* U, const double* mean, const double* sd, int32_t G, int32_t d,
                       double scale, double clip, const double* totals,
                       void* out, int32_t out_location);

#ifdef __cplusplus
}
#endif
#endif

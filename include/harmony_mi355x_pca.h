/* harmony_mi355x_pca.h -- the reference side of the count workflow on the GPU: per-gene statistics of the log-normalised counts and the
 * standardised cells x variable-genes matrix S as an operator (P = S V, W = S^T P), from which a caller fits the reference's PCA loadings by
 * subspace iteration without ever forming S (harmony_amd/pca.py: gene_stats, fit_loadings).  Companion of harmony_mi355x.h (handles, status
 * codes) and of harmony_mi355x_project.h, whose count-matrix contract, guards and definition of S these entry points share: the PCs that
 * hmx_pca_apply gives for a cell are, bit for bit, the ones hmx_project_counts gives for it with the same tables.
 *
 * The count matrix: CSR of N cells x G_all genes, indptr [N + 1] int64, indices [nnz] int32, data [nnz] of data_dtype (HMX_F32 | HMX_F64), all
 * three on the host or all three in HBM (csr_location).  Values finite and >= 0, no column twice in a row, rows need not be sorted.  A
 * host-resident matrix is validated on the host and uploaded in slabs of whole cells ("project_slab_bytes"); a device-resident one is guarded
 * by the kernels (an offending entry is treated as absent, the call returns HMX_ERR_ARG and names the first kind of violation).
 * y_ig = log1p(x_ig scale / T_i), T_i = totals[i] or the row sum over all G_all columns (fp64); T_i = 0: y = 0. */
#ifndef HARMONY_MI355X_PCA_H
#define HARMONY_MI355X_PCA_H

#include "harmony_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per gene g of all G_all: n[g] = the stored entries > 0, s1[g] = sum_i y_ig, s2[g] = sum_i y_ig^2 (host, fp64); mean = s1 / N,
 * var = (s2 - s1^2 / N) / (N - 1).  N >= 2.  y is formed in fp32 as hmx_project_counts forms it, clamped to ymax = 1.001 log1p(scale) (with
 * caller-given totals, which do not bound x / T: 89), and y, y^2 are rounded to the steps step[0] = 2^-F1, step[1] = 2^-F2 and added as 64-bit
 * integers: F1 = min(40, floor(62 - log2(N ymax))), F2 likewise with ymax^2, so N <= 2e9 cannot overflow.  Integer addition does not
 * depend on the order: two calls, host- or device-resident input, any slab cap and any order of the cells give the same bits.
 *   |s1 - exact| <= u sum_i c_i y_i + n step[0],  |s2 - exact| <= 2 u sum_i c_i y_i^2 + n step[1],  u = 2^-24, c_i = 3 kappa_i + 4 <= 7 with kappa the
 *   condition of log1p at the entry's argument (three roundings in the argument, log1pf to 2 ulp; DESIGN "Fitting the loadings").
 * step: [2] (host) or NULL.  Needs no fitted state and leaves none.  Wall time: "timer:gene_stats". */
int hmx_gene_stats(hmx_ctx* ctx, int64_t N, int32_t G_all,
                   const int64_t* indptr, const int32_t* indices, const void* data, int32_t data_dtype, int32_t csr_location,
                   double scale, const double* totals,
                   int64_t* n, double* s1, double* s2, double* step);

/* S (N x G) over the G chosen genes: slot [G_all] (host; -1 or the column j in [0, G), every j at most once), mean [G] >= 0, sd [G] > 0,
 * scale, clip (<= 0: none), totals [N] or NULL -- all as for hmx_project_counts.  Stored entry: s_ij = min((y - mean_j) / sd_j, clip); entry
 * not stored: s_ij = -mean_j / sd_j; a column no gene maps to is zero.
 * Reads the raw matrix twice (count, fill) and leaves on the handle, in HBM: per cell its contributing (j, w) in CSR order,
 * w = min(y, mean_j + clip sd_j) / sd_j by hmx_project_counts' fp32 expression; and the same entries per gene as (cell, w) in ascending cell
 * order (a stable counting sort over tiles of 256 cells; no atomics on results).  16 bytes per contributing entry, hmx_get "pca_entries"
 * reports their number.  A second call replaces the state; hmx_pca_release and hmx_destroy free it.
 * HMX_ERR_LIMIT: G > 16384, N > 2e9.  Wall time: "timer:pca_prepare". */
int hmx_pca_prepare(hmx_ctx* ctx, int64_t N, int32_t G_all,
                    const int64_t* indptr, const int32_t* indices, const void* data, int32_t data_dtype, int32_t csr_location,
                    const int32_t* slot, const double* mean, const double* sd, int32_t G,
                    double scale, double clip, const double* totals);

/* V [G][k] row-major fp64 (host), k <= 128.  P = S V: N x k row-major fp32 to the host or HBM (P_location), NULL: not returned;
 *   P[i,:] = b + sum over cell i's list of w V32[j,:] in fp32 in CSR order, b = sum_j (-mean_j / sd_j) V[j,:] in fp64:
 *   |P - exact|_ic <= (n_i + 16) u sum_j |w_ij| |V_jc| + 2 u |b_c|  (harmony_mi355x_project.h's bound).
 * W = S^T P: G x k row-major fp64 (host), of the fp32 P above:
 *   W[j,:] = sum over gene j's list of w P[i,:] - (mean_j / sd_j) colsum(P); the list in order, runs of 256 entries in fp32 added up in fp64,
 *   colsum in fp64 over ranges of 1024 rows in order:
 *   |W - exact|_jc <= (min(n_j, 256) + 10) u sum_i |w_ij| |P_ic| + (mean_j / sd_j) (N + 2) 2^-53 sum_i |P_ic|  (n_j the entries of gene j's list).
 * Two applies give the same bits, whatever the residence of the matrix the state was prepared from.
 * HMX_ERR_STATE without a prepared state.  Wall time: "timer:pca_apply". */
int hmx_pca_apply(hmx_ctx* ctx, const double* V, int32_t k, double* W, void* P, int32_t P_location);

int hmx_pca_release(hmx_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif

/* harmony_mi355x_groups.h -- gene statistics per group of cells on the GPU: per (group, gene) the number of cells that store a positive count
 * and the sums of y and y^2 of the log-normalised expression, from which a caller ranks variable genes within each batch and marker genes of
 * each label (harmony_amd/group_stats.py: gene_stats_by_group, variable_genes, rank_genes_groups).  Companion of harmony_mi355x.h (handles,
 * status codes) and of harmony_mi355x_pca.h, whose count-matrix contract, guards, arithmetic and fixed-point steps this entry point shares: the
 * group sums of a gene add up, bit for bit, to what hmx_gene_stats returns for it.
 *
 * The count matrix: CSR of N cells x G_all genes, indptr [N + 1] int64, indices [nnz] int32, data [nnz] of data_dtype (HMX_F32 | HMX_F64), all
 * three on the host or all three in HBM (csr_location).  Values finite and >= 0, no column twice in a row, rows need not be sorted.  A
 * host-resident matrix is validated on the host and uploaded in slabs of whole cells ("project_slab_bytes"); a device-resident one is guarded
 * by the kernel (an offending entry is treated as absent, the call returns HMX_ERR_ARG and names the first kind of violation; the rows of
 * cells labelled -1 are not read, so not guarded).
 * y_ig = log1p(x_ig scale / T_i), T_i = totals[i] or the row sum over all G_all columns (fp64); T_i = 0: y = 0. */
#ifndef HARMONY_MI355X_GROUPS_H
#define HARMONY_MI355X_GROUPS_H

#include "harmony_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* labels [N] (host): the group of every cell in [0, B), or -1: the cell belongs to no group and is left out.  Per group b and gene g:
 *   n_obs[b] = the cells of the group,  n[b G_all + g] = those of them that store an entry > 0,
 *   s1[b G_all + g] = sum over the group's cells of y_ig,  s2[b G_all + g] = the same of y_ig^2   (host; int64, int64, fp64, fp64);
 *   mean = s1 / n_obs, var = (s2 - s1^2 / n_obs) / (n_obs - 1) are the caller's (N >= 1 here; a group may be empty).
 * Per entry the arithmetic is hmx_gene_stats': y in fp32 as hmx_project_counts forms it, clamped to ymax = 1.001 log1p(scale) (with
 * caller-given totals: 89), y and y^2 rounded to the steps step[0] = 2^-F1, step[1] = 2^-F2 and added as 64-bit integers.  F1 and F2 are
 * hmx_gene_stats' for the WHOLE N -- F1 = min(40, floor(62 - log2(N ymax))), F2 likewise with ymax^2 -- so group sums and ungrouped sums are
 * multiples of the same step: with every cell in a group, sum_b s1[b G_all + g] is hmx_gene_stats' s1[g] exactly (the integers are; the
 * doubles while the integers stay below 2^53), and "all other cells" is total - group, an exact subtraction.
 * Integer addition does not depend on the order: two calls, host- or device-resident input, any slab cap, any order of the cells (with their
 * labels) give the same bits, and renumbering the groups permutes the rows.
 *   |s1 - exact| <= u sum_(i in b) c_i y_i + n step[0],  |s2 - exact| <= 2 u sum_(i in b) c_i y_i^2 + n step[1],  u = 2^-24, c_i = 3 kappa_i + 4 <= 7
 *   (harmony_mi355x_pca.h's bound with the sums restricted to the group; n = n[b G_all + g]).
 * How it runs: the host sorts the kept cells stably by label and cuts them into chunks of at most 256 cells of one group (and one slab); a
 * workgroup keeps the tables of 7680 genes in LDS for one group at a time and adds the touched genes into the [B][G_all] accumulators in HBM
 * where the group changes between two of its chunks.  A group of only a few cells therefore costs up to one global atomic per stored entry:
 * many tiny groups are slow, never wrong.
 * HMX_ERR_ARG: a label outside [-1, B) (the message names the first such cell), B < 1, a null pointer, the count matrix out of contract.
 * HMX_ERR_LIMIT: B > 4096 or B G_all > 2^25 (three 64-bit accumulators per (group, gene): 805 MB of HBM at the limit, and as much on the
 * host while they are converted); G_all > 2^24, N > 2e9.
 * step: [2] (host) or NULL.  Needs no fitted state and leaves none.  Wall time: "timer:gene_stats_grouped". */
int hmx_gene_stats_grouped(hmx_ctx* ctx, int64_t N, int32_t G_all,
                           const int64_t* indptr, const int32_t* indices, const void* data, int32_t data_dtype, int32_t csr_location,
                           double scale, const double* totals,
                           const int32_t* labels, int32_t B,
                           int64_t* n_obs, int64_t* n, double* s1, double* s2, double* step);

#ifdef __cplusplus
}
#endif
#endif

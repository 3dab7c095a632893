/* harmony_mi355x_ranksum.h -- Wilcoxon rank sums per group of cells on the GPU: per (group, gene) the exact doubled midrank sum of the group's
 * cells among all kept cells, and per gene the tie term, from which a caller forms U, the AUC and the normal-approximation score of the
 * rank-sum test (harmony_amd/rank_sums.py: rank_sums_by_group, wilcoxon_from_rank_sums, rank_genes_groups with method="wilcoxon").  Companion
 * of harmony_mi355x.h (handles, status codes) and of harmony_mi355x_groups.h, whose count-matrix contract, guards and labels this entry point shares.
 *
 * The count matrix: CSR of N cells x G_all genes, indptr [N + 1] int64, indices [nnz] int32, data [nnz] of data_dtype (HMX_F32 | HMX_F64), all
 * three on the host or all three in HBM (csr_location).  Values finite and >= 0, rows need not be sorted.  PRECONDITION: a row stores a gene at
 * most once (the counts of expressing cells assume it as well); a gene with more positive entries than kept cells is refused, other
 * repetitions are not detected.  A host-resident matrix is validated on the host and uploaded in slabs of whole cells ("project_slab_bytes"),
 * once for the count sweep and once per gene block; a device-resident one is guarded by the kernels (an offending entry is treated as absent,
 * the call returns HMX_ERR_ARG and names the first kind of violation; the rows of cells labelled -1 are not read, so not guarded).
 *
 * labels [N] (host): the group of every cell in [0, B), or -1: the cell is left out.  The KEPT cells are those with a label >= 0, N_k of them.
 * The key of a stored entry of cell i: key = fl32(fl32(x) r_i), r_i = fl32(scale / T_i) capped at 3e38 (0 where T_i = 0), T_i = totals[i] or
 * the row sum over all G_all columns (fp64): the argument of the log-normalised expression, one fp64 division and one fp32 product.  The
 * entry is POSITIVE when x > 0 and key > 0; every other (cell, gene) pair of a kept cell has key 0.  Keys are compared by value (+inf is a
 * legal key).  The test ranks the key, not log1p(key): the logarithm is monotone, so the order is the same, and the key can be reproduced
 * bit for bit on a host while a device's log1pf cannot; two keys that differ before the logarithm are therefore never tied here.
 *
 * gene_slot [G_all] (host): the output row in [0, G) of every gene, or -1: the gene is not ranked; no two genes share a row.  NULL: every
 * gene, row = gene, and G must be G_all.  Per selected gene g, P_g its positive entries among the kept cells and z_g = N_k - P_g:
 *   n_obs[b]           the kept cells of group b                                                            (host, int64 [B])
 *   n_pos[b G + g]     those of them with a positive entry                                                  (host, int64 [B][G])
 *   rank2[b G + g]     the DOUBLED midrank sum of group b over all its cells: a cell's doubled midrank is
 *                      #(keys < its key) + #(keys <= its key) + 1 over the kept cells; a zero cell has z_g + 1  (host, int64 [B][G])
 *   tie3[2 g], [2 g + 1]  sum of t^3 over the tie blocks of the POSITIVE keys as an unsigned 128-bit integer: low, high word   (host, uint64 [G][2])
 * sum_b rank2[b G + g] = N_k (N_k + 1).  Everything is integer arithmetic: two calls, host- or device-resident input, any slab cap, any
 * "ranksum_list_bytes", any order of the cells (with their labels) give the same bits, and renumbering the groups permutes the rows.
 *
 * How it runs: one sweep counts P_g; the selected genes are cut into gene blocks whose lists (8 bytes per positive entry, and as much for the
 * sort's second buffer) fit "ranksum_list_bytes" (default 8 GiB; hmx_get "ranksum_blocks": the blocks of the last call); per block one more
 * sweep writes key bits << 32 | group gene-major, then one workgroup per gene sorts its list (in LDS up to hmx_get "ranksum_sort_lds" entries,
 * by a radix sort in chunks of hmx_get "ranksum_chunk" beyond) and ranks it.  A host-resident matrix is therefore uploaded 1 + blocks times.
 * HMX_ERR_ARG: a label outside [-1, B) (the message names the first such cell), B < 1, G < 1, a gene_slot entry outside [-1, G) or a row
 * taken twice, NULL gene_slot with G != G_all, a null pointer, the count matrix out of contract.
 * HMX_ERR_LIMIT: B > 4096, B G > 2^25, N_k > 2^30; G_all > 2^24, N > 2e9.
 * Needs no fitted state and leaves none.  Wall time: "timer:rank_sums", of which "timer:rank_sums_count" (the count sweep),
 * "timer:rank_sums_fill" (the fill sweeps) and "timer:rank_sums_sort" (sorting and ranking). */
#ifndef HARMONY_MI355X_RANKSUM_H
#define HARMONY_MI355X_RANKSUM_H

#include "harmony_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int hmx_rank_sums(hmx_ctx* ctx, int64_t N, int32_t G_all,
                  const int64_t* indptr, const int32_t* indices, const void* data, int32_t data_dtype, int32_t csr_location,
                  double scale, const double* totals,
                  const int32_t* labels, int32_t B,
                  const int32_t* gene_slot, int32_t G,
                  int64_t* n_obs, int64_t* n_pos, int64_t* rank2, uint64_t* tie3);

#ifdef __cplusplus
}
#endif
#endif

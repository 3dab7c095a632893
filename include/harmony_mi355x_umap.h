/* harmony_mi355x_umap.h -- the UMAP layout of a neighbour graph on the GPU: the stochastic gradient descent that umap-learn runs over the fuzzy
 * simplicial set, as a deterministic algorithm whose result is a pure function of the input.  Python: harmony_amd/umap.py (umap_layout, umap,
 * Harmony.umap).  Companion of harmony_mi355x.h (handles, status codes) and of harmony_mi355x_graph.h, whose connectivities it reads.
 *
 * The graph: a symmetric CSR on the host, indptr [N + 1] int64, indices int32 strictly ascending within a row, weights float with
 * w_ij == w_ji bit for bit, finite and in [0, 1].  Fewer than 2^31 stored entries.  A stored diagonal is ignored; an explicit 0 never fires.
 * Y0 [N][dim]: the float starting positions, dim 2 or 3.  The schedule has n_epochs epochs, of which the call runs [epoch_begin, epoch_end).
 *   wmax   the largest off-diagonal weight; wmax == 0 returns Y0.
 *   fire   entry e (its position in the CSR, a uint32) has r_e = (double)w_e / (double)wmax, one IEEE division, and fires in epoch n iff
 *            floor((double)(n + 1) r_e) > floor((double)n r_e): umap-learn's epochs_per_sample = wmax / w in closed form.  An entry and its
 *            mirror fire in the same epochs.
 *   epoch  n reads the positions the epoch before left (a snapshot) and writes the next: alpha = (float)(learning_rate (1 - n / n_epochs)),
 *            formed in fp64; for cell i the sum over the fired entries (i, j) of its row, j != i, of
 *              2 clip(c_a (y_i - y_j)),  c_a = -2ab d2^(b-1) / (a d2^b + 1) if d2 = |y_i - y_j|^2 > 0, else 0  (the 2: umap-learn moves both
 *              ends of an edge, and the mirror entry pushes i by the same amount), and for s = 0 .. negative_sample_rate - 1 of
 *              clip(c_r (y_i - y_k)),    c_r = 2 gamma b / ((0.001 + d2)(a d2^b + 1)) if d2 > 0 and k != i, else 0,
 *              k = ((uint64)fmix32(e ^ key(n, s)) N) >> 32,  key(n, s) = fmix32(fmix32(seed) + 32 n + s + 1) in uint32 arithmetic (fmix32:
 *              murmur3's 32-bit finaliser); clip to [-4, 4] per coordinate; y_i_new = y_i + alpha sum.  A negative sample moves only i.
 * Positions are float.  The terms are computed in fp32 with d2^b = exp2(b log2 d2); a row's sum has one fixed shape (lane accumulators over
 * the row's entries in steps of 64 -- 256 above "umap:short_cap" --, an xor butterfly, the waves' partials as (0 + 1) + (2 + 3)): two calls
 * give the same bits.  tests/umap_ref.py is the same map in NumPy fp64 with the bound a device's fp32 terms stay within.
 *
 * HMX_ERR_ARG: a null pointer, N < 1, dim not 2 or 3, n_epochs outside 1 .. 2^20, epoch_begin / epoch_end not 0 <= begin <= end <= n_epochs,
 * a or b or learning_rate not positive and finite, gamma negative or not finite, negative_sample_rate outside 0 .. 31, indptr not ascending
 * from 0 or a row longer than N, a value of Y0 that is not finite -- all checked before a device is touched --, an index out of range, a row
 * not ascending, an edge without its mirror or with another weight, a weight outside [0, 1] or not finite -- checked on the device before any
 * epoch runs; Y is not written.  HMX_ERR_LIMIT: N > 2e9, 2^31 stored entries or more.
 * Wall time: "timer:umap".  hmx_get, of the last call: "umap:fired" the directed firings of its epochs; "umap:epochs" the epochs it ran;
 * "umap:long_rows" the rows with more than "umap:short_cap" entries, which one workgroup walks instead of one wave. */
#ifndef HARMONY_MI355X_UMAP_H
#define HARMONY_MI355X_UMAP_H

#include "harmony_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int hmx_umap_layout(hmx_ctx* ctx, const int64_t* indptr, const int32_t* indices, const float* weights, int64_t N, int32_t dim,
                    const float* Y0, int32_t n_epochs, int32_t epoch_begin, int32_t epoch_end, double a, double b, double gamma,
                    double learning_rate, int32_t negative_sample_rate, uint32_t seed, float* Y);

#ifdef __cplusplus
}
#endif
#endif

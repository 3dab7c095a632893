/* harmony_mi355x_umap_transform.h -- query cells put into a fitted UMAP layout on the GPU: what umap-learn's transform, Symphony's
 * mapQuery(do_umap = TRUE) and Seurat's MapQuery(reduction.model = "umap") do after a query has been mapped onto a reference.  The reference's
 * positions stay where they are; a query cell is attracted and repelled by reference cells alone, so the result is a pure function of the
 * arguments and every cell is independent of every other one.  Python: harmony_amd/umap_transform.py (umap_query_weights,
 * umap_transform_from_knn, umap_transform, Harmony.umap_transform).  Companion of harmony_mi355x.h (handles, status codes), of
 * harmony_mi355x_metrics.h, whose search gives the lists, and of harmony_mi355x_umap.h, whose layout is projected into.
 *
 * The lists: host arrays idx [Nq][k] int32 and dist [Nq][k] float, the k = n_neighbors nearest reference cells of every query cell ascending by
 * distance, as the search of the reference with the query returns them: every slot filled, no self column, 1 <= k <= 128, k <= Nr.
 *
 * Stage 1, the weights -- umap-learn's transform as written, local_connectivity - 1 = 0 included:
 *   rho    0 for every row.
 *   sigma  the bisection of the neighbour graph's search (lo 0, hi infinite, mid 1, at most 64 steps, doubling while hi is infinite, stop at
 *            |psum - log2 k| < 1e-5) over psum = sum_{j = 1 .. k-1} (d_j > 0 ? exp(-d_j / mid) : 1): THE FIRST ENTRY OF THE LIST IS LEFT OUT OF
 *            THE SUM, as umap-learn's smooth_knn_dist leaves out column 0 (it was written for lists whose column 0 is the cell itself);
 *            sigma = max(mid, 1e-3 sum_all d / (Nq k)).
 *   w_j    (d_j <= 0 || sigma == 0) ? 1 : exp(-d_j / sigma) for all k entries, column 0 included; fp64, rounded to float once.
 *
 * Stage 2, the epochs.  Yref [Nr][dim]: the reference's float positions, dim 2 or 3.
 *   start  Yq0 [Nq][dim] when given; else y_i = sum_j w_ij yref_j / sum_j w_ij in fp64 over the list's entries in their order, rounded to float
 *            once, and the plain mean of the k listed positions where every weight of the row is 0.  Yinit, when given, receives the start.
 *   fire   entry e = i k + j (a uint32) has r_e = (double)w_e / (double)wmax, wmax the largest weight of the call, one IEEE division, and fires
 *            in epoch n iff floor((double)(n + 1) r_e) > floor((double)n r_e): umap-learn zeroing every weight below wmax / n_epochs and giving
 *            the others epochs_per_sample = wmax / w, in closed form.  wmax == 0 or an empty epoch range returns the start.
 *   epoch  n of cell i, from y_i as the epoch found it: over the fired entries in their order the sum of
 *              clip(c_a (y_i - yref_j)),   c_a = -2ab d2^(b-1) / (a d2^b + 1) if d2 = |y_i - yref_j|^2 > 0, else 0, and for
 *              s = 0 .. negative_sample_rate - 1 of
 *              clip(c_r (y_i - yref_m)),   c_r = 2 gamma b / ((0.001 + d2)(a d2^b + 1)) if d2 > 0, else 0,
 *              m = ((uint64)fmix32(e ^ key(n, s)) Nr) >> 32,  key(n, s) = fmix32(fmix32(seed) + 32 n + s + 1) in uint32 arithmetic;
 *            clip to [-4, 4] per coordinate; y_i <- y_i + alpha_n sum with alpha_n = (float)(alpha0 (1 - n / n_epochs)), formed in fp64.  A cell
 *            of which nothing fired in an epoch keeps its bits.  (The attraction carries no factor 2 and no sample is skipped for being the
 *            cell itself: a query cell moves alone and is not in the reference.  umap-learn passes alpha0 = learning_rate / 4.)
 * The terms are fp32 with d2^b = exp2(b log2 d2), the layout's expressions; a cell's sum has one fixed shape (lane accumulators over a group of 16
 * lanes for k <= 16, of 64 lanes with two entries per lane above, then an xor butterfly): two calls give the same bits, and the epochs
 * [0, a) then [a, n) from the first call's result equal [0, n).  tests/umap_transform_ref.py is the same map in NumPy fp64 with the bound a
 * device's fp32 terms stay within.
 *
 * Everything is checked on the host before a device is touched.  HMX_ERR_ARG: a null pointer (sigma, Yq0 and Yinit may be null), Nq < 1,
 * k outside 1 .. 128, k > Nr, an index outside [0, Nr), a distance that is NaN, negative or infinite, a weight outside [0, 1] or not finite,
 * dim not 2 or 3, n_epochs outside 1 .. 2^20, epoch_begin / epoch_end not 0 <= begin <= end <= n_epochs, a or b or alpha0 not positive and
 * finite, gamma negative or not finite, negative_sample_rate outside 0 .. 31, a value of Yref or Yq0 that is not finite; Y is not written.
 * HMX_ERR_LIMIT: Nq k >= 2^31, Nr > 2e9.
 * Wall time: "timer:umap_query_weights", "timer:umap_transform"; "timer:umap_transform_epochs": the GPU time of the epochs' one kernel launch,
 * between two events (0 when no epoch ran).  hmx_get, of the last transform: "umap_transform:fired" the firings of its
 * epochs over all cells; "umap_transform:epochs" the epochs it ran. */
#ifndef HARMONY_MI355X_UMAP_TRANSFORM_H
#define HARMONY_MI355X_UMAP_TRANSFORM_H

#include "harmony_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int hmx_umap_query_weights(hmx_ctx* ctx, const int32_t* idx, const float* dist, int64_t Nq, int32_t k, int64_t Nr, float* weights,
                           double* sigma);

int hmx_umap_transform(hmx_ctx* ctx, const int32_t* idx, const float* weights, int64_t Nq, int32_t k, const float* Yref, int64_t Nr,
                       int32_t dim, const float* Yq0, int32_t n_epochs, int32_t epoch_begin, int32_t epoch_end, double a, double b,
                       double gamma, double alpha0, int32_t negative_sample_rate, uint32_t seed, float* Yinit, float* Y);

#ifdef __cplusplus
}
#endif
#endif

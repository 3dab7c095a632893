/* harmony_mi355x_silhouette.h -- silhouette widths on the GPU: per cell, per label, optionally within groups (the average silhouette
 * width of integration benchmarks: over the cell type, and over the batch within each cell type).  Companion of harmony_mi355x.h (handles,
 * status codes, HMX_F64 / HMX_F32, HMX_HOST / HMX_DEVICE) and harmony_mi355x_metrics.h; the same library exports this entry point.
 *
 * The handle supplies the device, the stream and the error text; the call needs no fitted state and leaves none.  Arguments are checked
 * before the device is touched (HMX_ERR_ARG / HMX_ERR_LIMIT / HMX_ERR_STATE); without a HIP device the call fails with HMX_ERR_DEVICE --
 * there is no CPU fallback.  Wall time of the last call: "timer:silhouette" through the scalar getter. */
#ifndef HARMONY_MI355X_SILHOUETTE_H
#define HARMONY_MI355X_SILHOUETTE_H

#include "harmony_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The silhouette width of every row of X (cells x PCs row-major, host or HBM), Euclidean, as sklearn.metrics.silhouette_samples defines it,
 * extended by groups: only cells of one group see each other (groups == NULL: one group; n_groups is then ignored).  labels[N] are 0-based
 * codes below n_levels, groups[N] below n_groups (host arrays).  Per cell i, into host arrays in the order the cells were given in:
 *   a[i]  the mean distance to the OTHER cells of its group with its label (self excluded by index; duplicates count, at distance 0);
 *   b[i]  the smallest, over the other labels present in its group, of the mean distance to that label's cells;
 *   s[i]  (b - a) / max(a, b); 0 where max(a, b) = 0; 0 with a = 0 where i is the only cell of its label in its group;
 *         s = a = b = NaN where the group holds fewer than two labels.
 * a and b may be NULL.  Every distance is computed (fp32 storage, |q|^2 + |x|^2 - 2 q.x with the dot product on the fp32 matrix cores, as
 * hmx_knn does), none is sampled; a distance passes at most 64 fp32 additions before it reaches an fp64 sum.  No atomics: two calls on the
 * same input are bit-identical.  X == NULL: the handle's current Z_corr (a fitted or a query handle; x_dtype / x_location / d are ignored,
 * N must be the handle's cell count, labels and groups in the order the cells were given in); the handle is left as it was.
 * Envelope: 1 <= d <= 128, N <= 2e9. */
int hmx_silhouette(hmx_ctx* ctx, const void* X, int32_t x_dtype, int32_t x_location, int64_t N, int32_t d,
                   const int32_t* labels, int32_t n_levels, const int32_t* groups, int32_t n_groups,
                   double* s, double* a, double* b);

#ifdef __cplusplus
}
#endif
#endif

// hmx_query_tile.h -- the soft assignment of a 16-cell query tile, shared by the kernels of the query mapping (hmx_query.hip) and of the mapping
// confidence (hmx_confidence.hip): ONE copy of the code, so that every kernel that recomputes R of a mapped query gets the same bits.
#pragma once
#include "hmx_internal.h"

namespace hmx {
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int QT = 16;          // cells per tile
constexpr int QZS = 128;        // largest row stride (d <= 128)
constexpr int QKP = 256;        // largest K

__device__ __forceinline__ float qwmax(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

// rows s .. s + cnt - 1 of Z into zt (pads and missing cells 0) and their inverse norms
__device__ __forceinline__ void q_load_tile(const QueryDev& Q, const float* __restrict__ Z, int s, int cnt, float (*zt)[QZS], float* inv) {
  const int zs = Q.zs;
  for (int i = threadIdx.x; i < QT * zs; i += blockDim.x) {
    const int c = i / zs, j = i - c * zs;
    zt[c][j] = c < cnt ? Z[(size_t)(s + c) * zs + j] : 0.f;
  }
  __syncthreads();
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  for (int c = w; c < QT; c += blockDim.x >> 6) {
    float ss = 0.f;
    for (int j = l; j < zs; j += 64) ss += zt[c][j] * zt[c][j];
    ss = wave_sum(ss);
    if (l == 0) inv[c] = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
  }
  __syncthreads();
}

// R of the tile into lg[c][k] (0 for missing cells): dot of the normalised row with every normalised centroid on the matrix cores
// (wave w takes the cluster tiles w, w + 4, ...), logits (dot - 1) * 2 / sigma_k, column maximum subtracted, exp, normalised.
__device__ __forceinline__ void q_assign(const QueryDev& Q, int cnt, float (*zt)[QZS], const float* inv, float (*lg)[QKP]) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int r = l & 15, g = l >> 4;
  const int nct = Q.KP16 >> 4;
  for (int ct = w; ct < nct; ct += nw) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float* yrow = Q.yhat + (size_t)(16 * ct + r) * Q.zs;
    const float iv = inv[r];
    for (int j0 = 0; j0 < Q.zs; j0 += 4) {
      const float a = zt[r][j0 + g] * iv;             // A[cell r][step g]
      const float b = yrow[j0 + g];                   // B[step g][cluster 16 ct + r]
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    }
    const int k = 16 * ct + r;
    if (k < Q.K) {
      const float s2 = Q.sig2[k];
#pragma unroll
      for (int i = 0; i < 4; i++) lg[4 * g + i][k] = (acc[i] - 1.0f) * s2;     // D[cell 4 g + i][cluster k]
    }
  }
  __syncthreads();
  for (int c = w; c < QT; c += nw) {
    if (c >= cnt) {
      for (int k = l; k < Q.K; k += 64) lg[c][k] = 0.f;
      continue;
    }
    float m = -INFINITY;
    for (int k = l; k < Q.K; k += 64) m = fmaxf(m, lg[c][k]);
    m = qwmax(m);
    float s = 0.f;
    for (int k = l; k < Q.K; k += 64) { const float e = expf(lg[c][k] - m); lg[c][k] = e; s += e; }
    s = wave_sum(s);
    const float is = 1.0f / s;
    for (int k = l; k < Q.K; k += 64) lg[c][k] *= is;
  }
  __syncthreads();
}

}  // namespace hmx

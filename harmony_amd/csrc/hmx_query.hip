// hmx_query.hip -- gfx950 kernels of the query mapping (hmx_map_query) and of the reference summary ("ref_Nr" / "ref_C").
//
// A query is mapped in two streaming passes over its rows (internal, combination-sorted order), 16-cell tiles:
//   k_query_stats<0>  normalise the tile's rows in LDS, distance GEMM against the normalised centroid image on
//                     v_mfma_f32_16x16x4_f32, per-cluster-sigma softmax -> R of the tile (LDS only), then the per-chunk sums
//                     n[k] = sum R and S[k][:] = sum R z (fp32 within a tile, fp64 across tiles, fixed order) into a private
//                     partial slot of the chunk;
//   k_query_fold      adds the slots of every combination in chunk order (fp64): no atomics, bit-reproducible;
//   k_query_apply     recomputes R of the tile the same way and writes Z_corr = Z - sum_k R_k Wq[q][k][:] (or, on request, R).
// k_query_stats<1> is the same accumulation with R read from a fitted handle's rows: Nr = sum R, Cref = sum R Z_corr.
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
__device__ __forceinline__ float qwsum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
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
    ss = qwsum(ss);
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
    s = qwsum(s);
    const float is = 1.0f / s;
    for (int k = l; k < Q.K; k += 64) lg[c][k] *= is;
  }
  __syncthreads();
}

// SUMMARY = 0: query statistics (R from the assignment, z = the query rows); 1: reference summary (R and z = the fitted handle's rows).
// Workgroup (x, y) = (chunk, slice of the K (d + 1) entries [k][0..d) = sum R z, [k][d] = sum R); fp64 accumulators in LDS.
template <int SUMMARY>
__global__ __launch_bounds__(256) void k_query_stats(QueryDev Q) {
  extern __shared__ double qacc[];
  __shared__ float zt[QT][QZS];
  __shared__ float lg[QT][QKP];
  __shared__ float inv[QT];
  const int W1 = Q.d + 1, total = Q.K * W1;
  const int e0 = blockIdx.y * Q.slice, e1 = min(total, e0 + Q.slice);
  for (int e = e0 + threadIdx.x; e < e1; e += blockDim.x) qacc[e - e0] = 0.0;
  const Item it = Q.chunks[blockIdx.x];
  const float* Z = SUMMARY ? Q.Zsum : Q.Z;
  for (int s = it.start; s < it.start + it.cnt; s += QT) {
    const int cnt = min(QT, it.start + it.cnt - s);
    __syncthreads();
    q_load_tile(Q, Z, s, cnt, zt, inv);
    if (SUMMARY) {
      for (int i = threadIdx.x; i < QT * Q.K; i += blockDim.x) {
        const int c = i / Q.K, k = i - c * Q.K;
        lg[c][k] = c < cnt ? Q.Rsum[(size_t)(s + c) * Q.K + k] : 0.f;
      }
      __syncthreads();
    } else {
      q_assign(Q, cnt, zt, inv, lg);
    }
    for (int e = e0 + threadIdx.x; e < e1; e += blockDim.x) {
      const int k = e / W1, j = e - k * W1;
      float t = 0.f;
      if (j < Q.d) {
#pragma unroll
        for (int c = 0; c < QT; c++) t += lg[c][k] * zt[c][j];
      } else {
#pragma unroll
        for (int c = 0; c < QT; c++) t += lg[c][k];
      }
      qacc[e - e0] += (double)t;
    }
  }
  __syncthreads();
  for (int e = e0 + threadIdx.x; e < e1; e += blockDim.x) Q.part[(size_t)blockIdx.x * total + e] = qacc[e - e0];
}

// out[q][e] = sum of the partial slots of combination q's chunks, in chunk order
__global__ void k_query_fold(const double* __restrict__ part, const int* __restrict__ qchunk, int nq, int total, double* __restrict__ out) {
  const size_t n = (size_t)nq * total;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int q = (int)(i / total), e = (int)(i - (size_t)q * total);
    double s = 0.0;
    for (int ch = qchunk[q]; ch < qchunk[q + 1]; ch++) s += part[(size_t)ch * total + e];
    out[i] = s;
  }
}

// pass 2: Z_corr rows (Q.out != nullptr) and / or R rows (Q.Rout != nullptr) of every tile of the workgroup's chunk
__global__ __launch_bounds__(256) void k_query_apply(QueryDev Q) {
  extern __shared__ float wl[];      // Wq[q] staged when it fits (Q.w_lds)
  __shared__ float zt[QT][QZS];
  __shared__ float lg[QT][QKP];
  __shared__ float inv[QT];
  const Item it = Q.chunks[blockIdx.x];
  const int Kd = Q.K * Q.d;
  const float* W = Q.Wq + (size_t)it.q * Kd;
  if (Q.out && Q.w_lds) {
    for (int i = threadIdx.x; i < Kd; i += blockDim.x) wl[i] = W[i];
    W = wl;
  }
  for (int s = it.start; s < it.start + it.cnt; s += QT) {
    const int cnt = min(QT, it.start + it.cnt - s);
    __syncthreads();
    q_load_tile(Q, Q.Z, s, cnt, zt, inv);
    q_assign(Q, cnt, zt, inv, lg);
    if (Q.Rout)
      for (int i = threadIdx.x; i < cnt * Q.K; i += blockDim.x) {
        const int c = i / Q.K, k = i - c * Q.K;
        Q.Rout[(size_t)(s + c) * Q.K + k] = lg[c][k];
      }
    if (Q.out)
      for (int i = threadIdx.x; i < cnt * Q.zs; i += blockDim.x) {
        const int c = i / Q.zs, j = i - c * Q.zs;
        float v = 0.f;
        if (j < Q.d) {
          float t = 0.f;
          for (int k = 0; k < Q.K; k++) t += lg[c][k] * W[(size_t)k * Q.d + j];
          v = zt[c][j] - t;
        }
        Q.out[(size_t)(s + c) * Q.zs + j] = v;
      }
  }
}

size_t query_stats_lds(const QueryDev& Q) { return (size_t)Q.slice * sizeof(double); }

void l_query_stats(const Launch& L, const QueryDev& Q, int summary) {
  const int total = Q.K * (Q.d + 1), nsl = (total + Q.slice - 1) / Q.slice;
  const dim3 grid((unsigned)Q.nchunks, (unsigned)nsl);
  if (summary) hipLaunchKernelGGL(k_query_stats<1>, grid, dim3(256), query_stats_lds(Q), L.stream, Q);
  else hipLaunchKernelGGL(k_query_stats<0>, grid, dim3(256), query_stats_lds(Q), L.stream, Q);
}
void l_query_fold(const Launch& L, const double* part, const int* qchunk, int nq, int total, double* out) {
  const size_t n = (size_t)nq * total;
  hipLaunchKernelGGL(k_query_fold, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, L.stream, part, qchunk, nq, total, out);
}
void l_query_apply(const Launch& L, const QueryDev& Q) {
  hipLaunchKernelGGL(k_query_apply, dim3((unsigned)Q.nchunks), dim3(256), (Q.out && Q.w_lds) ? (size_t)Q.K * Q.d * sizeof(float) : 0, L.stream, Q);
}

}  // namespace hmx

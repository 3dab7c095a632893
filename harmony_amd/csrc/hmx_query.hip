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
#include "hmx_query_tile.h"      // q_load_tile / q_assign: the tile's rows and its soft assignment

namespace hmx {
// SUMMARY = 0: query statistics (R from the assignment, z = the query rows); 1: reference summary (R and z = the fitted handle's rows);
// 2: the summary with one more column, [k][d + 1] = sum R^2 (pass A of the reference moments, hmx_confidence.hip).
// Workgroup (x, y) = (chunk, slice of the K (d + 1) entries [k][0..d) = sum R z, [k][d] = sum R); fp64 accumulators in LDS.
template <int SUMMARY>
__global__ __launch_bounds__(256) void k_query_stats(QueryDev Q) {
  extern __shared__ double qacc[];
  __shared__ float zt[QT][QZS];
  __shared__ float lg[QT][QKP];
  __shared__ float inv[QT];
  const int W1 = query_stats_width(Q.d, SUMMARY), total = Q.K * W1;
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
      } else if (j == Q.d) {
#pragma unroll
        for (int c = 0; c < QT; c++) t += lg[c][k];
      } else {
#pragma unroll
        for (int c = 0; c < QT; c++) t += lg[c][k] * lg[c][k];
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
  const int total = Q.K * query_stats_width(Q.d, summary), nsl = (total + Q.slice - 1) / Q.slice;
  const dim3 grid((unsigned)Q.nchunks, (unsigned)nsl);
  if (summary == 2) hipLaunchKernelGGL(k_query_stats<2>, grid, dim3(256), query_stats_lds(Q), L.stream, Q);
  else if (summary) hipLaunchKernelGGL(k_query_stats<1>, grid, dim3(256), query_stats_lds(Q), L.stream, Q);
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

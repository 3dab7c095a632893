// hmx_confidence.hip -- gfx950 kernels of the mapping confidence (include/harmony_mi355x_confidence.h; DESIGN "Mapping confidence").
//
// Reference side (hmx_reference_moments), after pass A (k_query_stats<2>, hmx_query.hip: S0 = sum R, sum R^2, sum R z per cluster):
//   k_conf_moments<NP>  workgroup (x, y) = (chunk of cells, cluster k).  With c_k = fl32(mu_k) of pass A and y = z - c_k the centred second
//                       moment sum_i R[k,i] y y^T runs on v_mfma_f32_16x16x4_f32: output rows and columns are PCs, the reduction dimension is
//                       cells, the A operand is R y.  Only the upper triangle of the grid of 16 x 16 tiles is computed, its tile pairs dealt
//                       over the four waves (NP per wave, accumulators in registers).  A product is added in fp32 for CONF_FLUSH tiles
//                       (128 additions), then the tile goes into fp64 registers; the chunk's sums land in a private slot -- no atomics --
//                       that k_query_fold adds in chunk order.  The centred first moment sum R y rides along on the vector ALU.
// Query side (hmx_mapping_confidence):
//   k_conf_score<MG>    workgroup = one chunk of the mapping, 64 cells at a time: R of four 16-cell tiles with the mapping's own q_load_tile /
//                       q_assign (LDS only), then every wave takes one tile, keeps its rows in registers as A operands and runs over the
//                       clusters: T = (Z_tile - mu_k) U_k^T on the fp32 MFMA (the 16-column groups wholly above the diagonal are skipped),
//                       row sums of T^2 over 16 lanes, square root, score += (double) R * (double) dist in cluster order.
#include "hmx_internal.h"
#include "hmx_query_tile.h"

namespace hmx {

constexpr int CONF_LDS = 144;          // row stride of the staged cells in floats: 144 % 64 = 16, the four rows of an MFMA step fall into four bank groups

// pair p of the upper triangle (row-major) -> (a, b), a <= b
__device__ __forceinline__ void conf_pair(int NG, int p, int& a, int& b) {
  a = 0;
  while (p >= NG - a) { p -= NG - a; a++; }
  b = a + p;
}

template <int NP>
__global__ __launch_bounds__(256) void k_conf_moments(ConfMomDev P) {
  __shared__ __attribute__((aligned(16))) float zb[CONF_BLOCK][CONF_LDS];
  __shared__ float rb[CONF_BLOCK];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, r = l & 15, g = l >> 4;
  const int k = blockIdx.y, zs = P.zs, NG = P.NG, nf4 = zs >> 2;
  const Item it = P.chunks[blockIdx.x];
  const int end = it.start + it.cnt;
  const float* ck = P.c + (size_t)k * zs;

  // this wave's tile pairs w, w + 4, ...: LDS columns of the lane's A and B values and the centre's components there
  int ja[NP], jb[NP];
  float ca[NP], cb[NP];
  bool has[NP];
#pragma unroll
  for (int n = 0; n < NP; n++) {
    const int p = w + 4 * n;
    has[n] = p < P.npairs;
    int a = 0, b = 0;
    if (has[n]) conf_pair(NG, p, a, b);
    ja[n] = 16 * a + r; jb[n] = 16 * b + r;
    ca[n] = ja[n] < zs ? ck[ja[n]] : 0.f;
    cb[n] = jb[n] < zs ? ck[jb[n]] : 0.f;
  }
  // ... and its groups w, w + 4 of the first moment
  int jm[2]; float cm[2]; bool hm[2];
#pragma unroll
  for (int u = 0; u < 2; u++) {
    hm[u] = w + 4 * u < NG;
    jm[u] = hm[u] ? 16 * (w + 4 * u) + r : r;
    cm[u] = jm[u] < zs ? ck[jm[u]] : 0.f;
  }
  for (int i = tid; i < CONF_BLOCK * CONF_LDS; i += 256) (&zb[0][0])[i] = 0.f;      // (the columns behind zs stay 0)

  f32x4 acc[NP];
  double dacc[NP][4];
  float fm[2] = {0.f, 0.f};
  double dm[2] = {0.0, 0.0};
#pragma unroll
  for (int n = 0; n < NP; n++) {
    acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; i++) dacc[n][i] = 0.0;
  }
  auto flush = [&]() {
#pragma unroll
    for (int n = 0; n < NP; n++) {
#pragma unroll
      for (int i = 0; i < 4; i++) dacc[n][i] += (double)acc[n][i];
      acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < 2; u++) { dm[u] += (double)fm[u]; fm[u] = 0.f; }
  };

  int blocks = 0;
  for (int s0 = it.start; s0 < end; s0 += CONF_BLOCK) {
    __syncthreads();                                  // the previous block has been read by every wave
    for (int i = tid; i < CONF_BLOCK * nf4; i += 256) {
      const int row = i / nf4, col = i - row * nf4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (s0 + row < end) v = *(const f32x4*)(P.Z + (size_t)(s0 + row) * zs + 4 * col);
      *(f32x4*)&zb[row][4 * col] = v;
    }
    if (tid < CONF_BLOCK) rb[tid] = s0 + tid < end ? P.R[(size_t)(s0 + tid) * P.K + k] : 0.f;      // (a missing cell weighs 0)
    __syncthreads();
#pragma unroll 4
    for (int st = 0; st < CONF_BLOCK / 4; st++) {
      const int cell = 4 * st + g;                    // the lane's cell of this reduction step
      const float rr = rb[cell];
#pragma unroll
      for (int n = 0; n < NP; n++) {
        if (has[n]) {
          const float a = (zb[cell][ja[n]] - ca[n]) * rr;      // A[PC 16 a + r][cell]
          const float b = zb[cell][jb[n]] - cb[n];             // B[cell][PC 16 b + r]
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[n], 0, 0, 0);
        }
      }
#pragma unroll
      for (int u = 0; u < 2; u++)
        if (hm[u]) fm[u] += (zb[cell][jm[u]] - cm[u]) * rr;
    }
    if (++blocks == CONF_FLUSH * 16 / CONF_BLOCK) { flush(); blocks = 0; }
  }
  flush();

  double* slot = P.part + ((size_t)blockIdx.x * P.K + k) * P.E;
#pragma unroll
  for (int n = 0; n < NP; n++) {
    if (has[n]) {
#pragma unroll
      for (int i = 0; i < 4; i++) slot[(size_t)(w + 4 * n) * 256 + 4 * l + i] = dacc[n][i];      // D[PC 16 a + 4 g + i][PC 16 b + r]
    }
  }
#pragma unroll
  for (int u = 0; u < 2; u++) {
    double v = dm[u];                                 // the four cell residues of a column, in a fixed order
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (hm[u] && g == 0) slot[(size_t)P.npairs * 256 + jm[u]] = v;
  }
}

void l_conf_moments(const Launch& L, const ConfMomDev& P) {
  const dim3 grid((unsigned)P.nchunks, (unsigned)P.K);
  const int np = (P.npairs + 3) / 4;
  if (np <= 1) hipLaunchKernelGGL(k_conf_moments<1>, grid, dim3(256), 0, L.stream, P);
  else if (np <= 3) hipLaunchKernelGGL(k_conf_moments<3>, grid, dim3(256), 0, L.stream, P);
  else if (np <= 6) hipLaunchKernelGGL(k_conf_moments<6>, grid, dim3(256), 0, L.stream, P);
  else hipLaunchKernelGGL(k_conf_moments<9>, grid, dim3(256), 0, L.stream, P);
}

// MG: PC groups of 16 the kernel is built for (ceil(zs / 16) <= MG of them are run)
template <int MG>
__global__ __launch_bounds__(256) void k_conf_score(ConfDev P) {
  __shared__ float zt[QT][QZS];
  __shared__ float lg[CONF_TILES][QT][QKP];
  __shared__ float inv[QT];
  const QueryDev& Q = P.Q;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, r = l & 15, g = l >> 4;
  const int zs = Q.zs, K = Q.K, NG = (zs + 15) >> 4;
  const Item it = Q.chunks[blockIdx.x];
  const int end = it.start + it.cnt;
  for (int s0 = it.start; s0 < end; s0 += QT * CONF_TILES) {
    for (int t = 0; t < CONF_TILES; t++) {            // R of the four tiles, exactly as the mapping computes it
      const int s = s0 + QT * t, cnt = max(0, min(QT, end - s));
      __syncthreads();
      q_load_tile(Q, Q.Z, s, cnt, zt, inv);
      q_assign(Q, cnt, zt, inv, lg[t]);
    }
    const int s = s0 + QT * w, cnt = min(QT, end - s);
    if (cnt <= 0) continue;                           // (wave-uniform; the barriers above are passed by every wave of every block of 64)
    f32x4 a[MG];                                      // the wave's rows: cell s + r, PCs 16 t + 4 g + {0..3}
#pragma unroll
    for (int t = 0; t < MG; t++) {
      a[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t < NG && r < cnt && 16 * t + 4 * g < zs) a[t] = *(const f32x4*)(P.Zs + (size_t)(s + r) * zs + 16 * t + 4 * g);
    }
    int dst[4];                                       // the lane's rows of the result tile: cells s + 4 g + i, in the order they were given in
#pragma unroll
    for (int i = 0; i < 4; i++) dst[i] = 4 * g + i < cnt ? P.perm[s + 4 * g + i] : -1;
    double sc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < K; k++) {
      const float* Uk = P.U + (size_t)k * zs * zs;
      const float* mk = P.mu + (size_t)k * zs;
      f32x4 y[MG], acc[MG];
#pragma unroll
      for (int t = 0; t < MG; t++) {
        y[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (t < NG && 16 * t + 4 * g < zs) y[t] = a[t] - *(const f32x4*)(mk + 16 * t + 4 * g);
      }
#pragma unroll
      for (int b = 0; b < MG; b++) {
        if (b < NG) {
          const int j = 16 * b + r;                   // output column: row j of U_k
#pragma unroll
          for (int t = 0; t <= b; t++) {              // (the groups t > b lie wholly above the diagonal)
            f32x4 u = {0.f, 0.f, 0.f, 0.f};
            if (j < zs && 16 * t + 4 * g < zs) u = *(const f32x4*)(Uk + (size_t)j * zs + 16 * t + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; i++) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(y[t][i], u[i], acc[b], 0, 0, 0);
          }
        }
      }
      // acc[b][i] = T[cell 4 g + i][PC 16 b + r]
#pragma unroll
      for (int i = 0; i < 4; i++) {
        float ss = 0.f;
#pragma unroll
        for (int b = 0; b < MG; b++) if (b < NG) ss = fmaf(acc[b][i], acc[b][i], ss);
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
        const float dist = sqrtf(ss);
        sc[i] += (double)lg[w][4 * g + i][k] * (double)dist;
        if (P.dist && r == 0 && dst[i] >= 0) P.dist[(size_t)dst[i] * K + k] = dist;
      }
    }
    if (r == 0) {
#pragma unroll
      for (int i = 0; i < 4; i++) if (dst[i] >= 0) P.score[dst[i]] = sc[i];
    }
  }
}

void l_conf_score(const Launch& L, const ConfDev& P) {
  if (P.Q.zs <= 64) hipLaunchKernelGGL(k_conf_score<4>, dim3((unsigned)P.Q.nchunks), dim3(256), 0, L.stream, P);
  else hipLaunchKernelGGL(k_conf_score<8>, dim3((unsigned)P.Q.nchunks), dim3(256), 0, L.stream, P);
}

}  // namespace hmx

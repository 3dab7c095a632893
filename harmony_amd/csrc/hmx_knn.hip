// hmx_knn.hip -- gfx950 kernels of the integration metrics (include/harmony_mi355x_metrics.h): exact brute-force k nearest neighbours
// and LISI, the local inverse Simpson's index (DESIGN "Scoring an integration").
//
//   k_knn_ingest   rows of either element type -> fp32 rows of stride zs (pads 0) and their squared norms (one fmaf chain per row);
//   k_knn<MG, KP>  workgroup (x, y) = (64 query rows, chunk y of the data rows): every wave owns 16 query rows (A operand in registers)
//                  and all four stream the chunk in 64-row slabs staged through LDS; d2 = |q|^2 + |x|^2 - 2 q.x with the dot product
//                  on v_mfma_f32_16x16x4_f32; per query row a sorted list of KP (distance, index) keys in LDS, two positions per lane,
//                  filtered by the current k-th distance; the result of a chunk is its k smallest keys;
//   k_knn_merge    more than one chunk: one wave per query row merges the chunks' lists in chunk order;
//   k_lisi         one wave per cell: the perplexity search of the neighbour weights and the Simpson index of every label column, fp64.
// A key is (order-preserving bits of d2) << 32 | data index, so that one 64-bit comparison orders by (d2, index): ties go to the smaller
// index, keys are unique, and the k smallest of a set do not depend on the order they were offered in -- no atomics, bit-reproducible.
#include "hmx_dist_tile.h"

namespace hmx {
typedef unsigned long long u64;

constexpr u64 KNN_EMPTY = ~0ull;      // above every key of a real distance (NaN included)

__device__ __forceinline__ u64 knn_key(float d2, int idx) {
  d2 += 0.0f;                                          // -0 -> +0: equal distances must have equal bits
  unsigned b = __float_as_uint(d2);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((u64)b << 32) | (unsigned)idx;
}
__device__ __forceinline__ float knn_key_d2(u64 key) {
  unsigned b = (unsigned)(key >> 32);
  b = (b & 0x80000000u) ? (b & 0x7fffffffu) : ~b;
  return __uint_as_float(b);
}
// the sorted list of a wave, position p in lane p & 63, slot p >> 6 (e0 / e1): number of keys below `key`
__device__ __forceinline__ int knn_rank(u64 e0, u64 e1, u64 key) {
  return __popcll(__ballot(e0 < key)) + __popcll(__ballot(e1 < key));
}
// ... and `key` put at that position, the keys behind it moved up by one (the last one leaves)
__device__ __forceinline__ void knn_insert(u64& e0, u64& e1, u64 key, int rank, int l) {
  const u64 p0 = __shfl_up(e0, 1, 64), w = __shfl(e0, 63, 64);
  u64 p1 = __shfl_up(e1, 1, 64);
  if (l == 0) p1 = w;
  e0 = l < rank ? e0 : (l == rank ? key : p0);
  e1 = l + 64 < rank ? e1 : (l + 64 == rank ? key : p1);
}
__device__ __forceinline__ void knn_store_result(const KnnDev& P, long long qi, int p, u64 key) {
  const bool have = key != KNN_EMPTY;                 // (a list is short only when the rows hold NaN)
  P.idx[(size_t)qi * P.k + p] = have ? (int)(unsigned)key : -1;
  P.dist[(size_t)qi * P.k + p] = have ? sqrtf(fmaxf(knn_key_d2(key), 0.f)) : INFINITY;
}

// one thread per row
__global__ __launch_bounds__(256) void k_knn_ingest(const void* __restrict__ src, int f32, long long n, int d, int zs, float* __restrict__ dst,
                                                    float* __restrict__ nrm) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  float s = 0.f;
  for (int j = 0; j < zs; j++) {
    float v = 0.f;
    if (j < d) v = f32 ? ((const float*)src)[(size_t)r * d + j] : (float)((const double*)src)[(size_t)r * d + j];
    dst[(size_t)r * zs + j] = v;
    s = fmaf(v, v, s);
  }
  nrm[r] = s;
}

// MG: PC groups of 16 the kernel is built for (P.NG <= MG of them are run); KP: list positions per query row (64 | 128, P.k <= KP)
template <int MG, int KP>
__global__ __launch_bounds__(256) void k_knn(KnnDev P) {
  typedef DistTile<MG> Tile;                          // hmx_dist_tile.h: the A operand, the slab staging and the MFMA loop
  __shared__ __attribute__((aligned(16))) float slab[KNN_SLAB][Tile::S];
  __shared__ float sxn[KNN_SLAB];
  __shared__ u64 lists[4][16][KP];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, c = l & 15, g = l >> 4;
  const long long q0 = (long long)blockIdx.x * KNN_QROWS + 16 * w;
  const long long c0 = (long long)blockIdx.y * P.chunk, c1 = min(P.N, c0 + P.chunk);
  const int zs = P.zs, NG = P.NG, k = P.k;

  Tile DT;
  DT.init(q0 + c < P.Nq ? P.Q + (size_t)(q0 + c) * zs : nullptr, zs, NG, slab);
  float qn[4], thr[4];                                // the lane's rows of the result tile: query rows q0 + 4 g + i
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const long long qi = q0 + 4 * g + i;
    qn[i] = qi < P.Nq ? P.qn[qi] : NAN;               // (a missing row's distances are NaN: never below a threshold)
    thr[i] = INFINITY;
  }
  for (int q = 0; q < 16; q++)
    for (int p = l; p < KP; p += 64) lists[w][q][p] = KNN_EMPTY;

  DT.fetch(P.X, P.xn, c0, c1, zs);
  for (long long base = c0; base < c1; base += KNN_SLAB) {
    __syncthreads();                                  // the previous slab has been read by every wave
    DT.stage(slab, sxn, zs);
    __syncthreads();
    if (base + KNN_SLAB < c1) DT.fetch(P.X, P.xn, base + KNN_SLAB, c1, zs);

    f32x4 acc[4];                                     // acc[tt][i] = q . x of (query row q0 + 4 g + i, data row base + 16 tt + c)
    DT.dots(slab, NG, acc);
    float d2[4][4];
    bool any = false;
#pragma unroll
    for (int tt = 0; tt < 4; tt++) {
      const long long x = base + 16 * tt + c;
      const float xn = sxn[16 * tt + c];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        float v = fmaf(-2.0f, acc[tt][i], qn[i] + xn);
        if (x >= c1 || (P.excl && x == q0 + 4 * g + i)) v = NAN;
        d2[tt][i] = v;
        any |= v <= thr[i];
      }
    }
    if (__ballot(any) == 0) continue;
#pragma unroll
    for (int tt = 0; tt < 4; tt++) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        u64 m = __ballot(d2[tt][i] <= thr[i]);
        while (m) {
          const int src = __ffsll(m) - 1;
          m &= m - 1;
          const float v = __shfl(d2[tt][i], src, 64);
          const u64 key = knn_key(v, (int)(base + 16 * tt + (src & 15)));
          u64* L = lists[w][4 * (src >> 4) + i];
          u64 e0 = L[l], e1 = KP > 64 ? L[(l + 64) & (KP - 1)] : KNN_EMPTY;
          const int rank = knn_rank(e0, e1, key);
          if (rank >= k) continue;                    // (the threshold moved since the mask was taken, or a tie with the k-th at a larger index)
          knn_insert(e0, e1, key, rank, l);
          L[l] = e0;
          if (KP > 64) L[(l + 64) & (KP - 1)] = e1;
          const u64 kth = __shfl(k > 64 ? e1 : e0, (k - 1) & 63, 64);
          const float nt = kth == KNN_EMPTY ? INFINITY : knn_key_d2(kth);
          if (g == (src >> 4)) thr[i] = nt;
        }
      }
    }
  }
  for (int q = 0; q < 16; q++) {
    const long long qi = q0 + q;
    if (qi >= P.Nq) break;
    for (int p = l; p < k; p += 64) {
      const u64 key = lists[w][q][p];
      if (P.nchunks > 1) P.part[((size_t)qi * P.nchunks + blockIdx.y) * k + p] = key;
      else knn_store_result(P, qi, p, key);
    }
  }
}

// the k smallest keys of a query row's chunk lists (each sorted): chunk after chunk, key after key, until one does not enter
__global__ __launch_bounds__(256) void k_knn_merge(KnnDev P) {
  const int l = threadIdx.x & 63, k = P.k;
  const long long qi = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qi >= P.Nq) return;
  u64 e0 = KNN_EMPTY, e1 = KNN_EMPTY;
  for (int ch = 0; ch < P.nchunks; ch++) {
    const u64* src = P.part + ((size_t)qi * P.nchunks + ch) * k;
    bool done = false;
    for (int j0 = 0; j0 < k && !done; j0 += 64) {
      const u64 mine = j0 + l < k ? src[j0 + l] : KNN_EMPTY;
      const int n = min(64, k - j0);
      for (int j = 0; j < n; j++) {
        const u64 key = __shfl(mine, j, 64);
        const int rank = key == KNN_EMPTY ? k : knn_rank(e0, e1, key);
        if (rank >= k) { done = true; break; }
        knn_insert(e0, e1, key, rank, l);
      }
    }
  }
  if (l < k) knn_store_result(P, qi, l, e0);
  if (l + 64 < k) knn_store_result(P, qi, l + 64, e1);
}

// LISI of cell (wave) over every label column.  Lane l holds neighbours l and l + 64 (m <= 128).  The weights P_j = exp(-D_j beta) / S are
// found once per cell (binary search of beta for entropy ln(perplexity), as immunogenomics/LISI's compute_simpson_index does), then
// every column's index is 1 / sum_j P_j (sum_j' P_j' [label_j' = label_j]) -- the sum over levels of the squared level masses, without a table of levels.
__global__ __launch_bounds__(256) void k_lisi(const int* __restrict__ idx, const float* __restrict__ dist, long long Nq, int m,
                                              const int* __restrict__ labels, long long N, int ncols, double logU, double tol, double* __restrict__ out) {
  const int l = threadIdx.x & 63;
  const long long cell = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (cell >= Nq) return;
  const bool h0 = l < m, h1 = l + 64 < m;
  const double D0 = h0 ? (double)dist[(size_t)cell * m + l] : 0.0, D1 = h1 ? (double)dist[(size_t)cell * m + l + 64] : 0.0;
  int i0 = h0 ? idx[(size_t)cell * m + l] : -1, i1 = h1 ? idx[(size_t)cell * m + l + 64] : -1;
  if (i0 >= N) i0 = -1;
  if (i1 >= N) i1 = -1;
  double P0 = 0.0, P1 = 0.0, H = 0.0;
  auto hbeta = [&](double beta) {
    P0 = h0 ? exp(-D0 * beta) : 0.0;
    P1 = h1 ? exp(-D1 * beta) : 0.0;
    const double S = wave_sum(P0 + P1);
    if (S == 0.0) { H = 0.0; P0 = P1 = 0.0; return; }
    const double DP = wave_sum(D0 * P0 + D1 * P1);
    H = log(S) + beta * DP / S;
    P0 /= S; P1 /= S;
  };
  double beta = 1.0, bmin = -INFINITY, bmax = INFINITY;
  hbeta(beta);
  for (int tries = 0; fabs(H - logU) > tol && tries < 50; tries++) {
    if (H - logU > 0) { bmin = beta; beta = isinf(bmax) ? beta * 2 : (beta + bmax) / 2; }
    else { bmax = beta; beta = isinf(bmin) ? beta / 2 : (beta + bmin) / 2; }
    hbeta(beta);
  }
  for (int col = 0; col < ncols; col++) {
    double r = -1.0;                                  // H == 0: what the LISI package returns, 1 / (-1)
    if (H != 0.0) {
      const int a0 = i0 >= 0 ? labels[(size_t)col * N + i0] : -1 - l, a1 = i1 >= 0 ? labels[(size_t)col * N + i1] : -65 - l;
      double s0 = 0.0, s1 = 0.0;
      for (int j = 0; j < m; j++) {
        const int aj = __shfl(j < 64 ? a0 : a1, j & 63, 64);
        const double pj = __shfl(j < 64 ? P0 : P1, j & 63, 64);
        s0 += a0 == aj ? pj : 0.0;
        s1 += a1 == aj ? pj : 0.0;
      }
      r = 1.0 / wave_sum(P0 * s0 + P1 * s1);
    }
    if (l == 0) out[(size_t)cell * ncols + col] = r;
  }
}

void l_knn_ingest(const Launch& L, const void* src, int f32, long long n, int d, int zs, float* dst, float* nrm) {
  hipLaunchKernelGGL(k_knn_ingest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, L.stream, src, f32, n, d, zs, dst, nrm);
}
template <int MG>
static void knn_launch(const Launch& L, const KnnDev& P, dim3 grid) {
  if (P.k > 64) hipLaunchKernelGGL((k_knn<MG, 128>), grid, dim3(256), 0, L.stream, P);
  else hipLaunchKernelGGL((k_knn<MG, 64>), grid, dim3(256), 0, L.stream, P);
}
void l_knn(const Launch& L, const KnnDev& P) {
  const dim3 grid((unsigned)((P.Nq + KNN_QROWS - 1) / KNN_QROWS), (unsigned)P.nchunks);
  if (P.NG <= 2) knn_launch<2>(L, P, grid);
  else if (P.NG <= 4) knn_launch<4>(L, P, grid);
  else knn_launch<8>(L, P, grid);
  if (P.nchunks > 1) hipLaunchKernelGGL(k_knn_merge, dim3((unsigned)((P.Nq + 3) / 4)), dim3(256), 0, L.stream, P);
}
void l_lisi(const Launch& L, const int* idx, const float* dist, long long Nq, int m, const int* labels, long long N, int ncols, double perplexity,
            double* out) {
  hipLaunchKernelGGL(k_lisi, dim3((unsigned)((Nq + 3) / 4)), dim3(256), 0, L.stream, idx, dist, Nq, m, labels, N, ncols, log(perplexity), 1e-5, out);
}

}  // namespace hmx

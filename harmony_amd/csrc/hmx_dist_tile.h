// hmx_dist_tile.h -- the streamed distance tile, shared by the exact kNN (hmx_knn.hip) and the silhouette widths (hmx_silhouette.hip): ONE copy
// of the staging and of the MFMA loop, so that a change to either reaches every kernel that streams data rows past 64 query rows.
//
// A workgroup of 256 threads holds 64 query rows, 16 per wave (A operand in registers), and streams data rows in slabs of KNN_SLAB = 64
// through LDS, register-staged one slab ahead: fetch(next) is issued right behind the second barrier of a step and lands while the step's
// MFMAs run.  The kernel declares the LDS arrays (slab[KNN_SLAB][S], sxn[KNN_SLAB]) and keeps the loop over `base` with its two barriers:
//
//   DT.init(...); DT.fetch(.., c0, ..);
//   for (base = c0; base < c1; base += KNN_SLAB) {
//     __syncthreads(); DT.stage(slab, sxn, zs); __syncthreads();
//     if (base + KNN_SLAB < c1) DT.fetch(.., base + KNN_SLAB, ..);
//     DT.dots(slab, NG, acc);      // acc[tt][i] = q . x of (query row q0 + 4 g + i, data row base + 16 tt + c), c = lane & 15, g = lane >> 4
//     ...
//   }
#pragma once
#include "hmx_internal.h"

namespace hmx {
typedef float f32x4 __attribute__((ext_vector_type(4)));

// MG: PC groups of 16 the kernel is built for (NG <= MG of them are run)
template <int MG>
struct DistTile {
  static constexpr int S = 16 * MG + 4;               // slab row stride in floats: S / 4 odd, so that the 16 rows of a b128 read spread over the banks
  f32x4 a[MG];                                        // A operand: the wave's query row c, PCs 16 t + 4 g + {0..3}
  f32x4 pre[8];                                       // staging: thread (row = tid >> 2, s = tid & 3) moves the float4 columns s, s + 4, ... of its slab row
  float prexn;

  // the A operand from `qrow` (the lane's query row q0 + c; nullptr: no such row, zeros) and the slab zeroed (the columns behind zs stay 0)
  __device__ __forceinline__ void init(const float* qrow, int zs, int NG, float (*slab)[S]) {
    const int tid = threadIdx.x, g = (tid & 63) >> 4;
#pragma unroll
    for (int t = 0; t < MG; t++) {
      a[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t < NG && qrow && 16 * t + 4 * g < zs) a[t] = *(const f32x4*)(qrow + 16 * t + 4 * g);
    }
    for (int i = tid; i < KNN_SLAB * S; i += 256) (&slab[0][0])[i] = 0.f;
    prexn = 0.f;
  }
  // rows base .. base + 63 of X (behind c1: zeros) and their norms into registers
  __device__ __forceinline__ void fetch(const float* X, const float* xn, long long base, long long c1, int zs) {
    const int tid = threadIdx.x, nf4 = zs >> 2;
    const long long r = base + (tid >> 2);
#pragma unroll
    for (int f = 0; f < 8; f++) {
      const int col = (tid & 3) + 4 * f;
      if (col < nf4) pre[f] = r < c1 ? *(const f32x4*)(X + (size_t)r * zs + 4 * col) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (tid < KNN_SLAB) prexn = base + tid < c1 ? xn[base + tid] : 0.f;
  }
  // ... and from the registers into LDS, between the two barriers of a step
  __device__ __forceinline__ void stage(float (*slab)[S], float* sxn, int zs) const {
    const int tid = threadIdx.x, nf4 = zs >> 2;
#pragma unroll
    for (int f = 0; f < 8; f++) {
      const int col = (tid & 3) + 4 * f;
      if (col < nf4) *(f32x4*)&slab[tid >> 2][4 * col] = pre[f];
    }
    if (tid < KNN_SLAB) sxn[tid] = prexn;
  }
  __device__ __forceinline__ void dots(const float (*slab)[S], int NG, f32x4 (&acc)[4]) const {
    const int c = threadIdx.x & 15, g = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int tt = 0; tt < 4; tt++) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < MG; t++) {
      if (t < NG) {
#pragma unroll
        for (int tt = 0; tt < 4; tt++) {
          const f32x4 b = *(const f32x4*)&slab[16 * tt + c][16 * t + 4 * g];      // B operand: data row base + 16 tt + c, the same PCs
#pragma unroll
          for (int i = 0; i < 4; i++) acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][i], b[i], acc[tt], 0, 0, 0);
        }
      }
    }
  }
};

}  // namespace hmx

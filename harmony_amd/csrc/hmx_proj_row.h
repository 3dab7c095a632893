// hmx_proj_row.h -- what the kernels that walk a CSR row of raw counts share (hmx_project.hip: k_project; hmx_pca.hip: the gene statistics, the
// compact list and both products of the standardised matrix): the library size of a row, the normalisation rate, the weight of a stored entry
// and the drain of queued (row of the table, weight) pairs.  One arithmetic for the reference and the query: a cell's PCs from hmx_pca_apply
// and from hmx_project_counts with the same tables are the same bits because both run THESE expressions in the same order.
#pragma once
#include "hmx_internal.h"

namespace hmx {

__device__ __forceinline__ void proj_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the sum of the row's entries [lo, hi) in fp64: lanes stride the row, a butterfly adds the partials (anything but a finite value >= 0 is skipped)
template <bool F64>
__device__ __forceinline__ double proj_row_total(const void* data, long long lo, long long hi, int lane) {
  double t = 0.0;
#pragma unroll 4
  for (long long e = lo + lane; e < hi; e += 64) {
    const double x = F64 ? ((const double*)data)[e] : (double)((const float*)data)[e];
    if (x >= 0 && x <= 3.0e38) t += x;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
  return t;
}

// scale / T in fp32 (T = 0: an empty row or stored zeros, y = 0)
__device__ __forceinline__ float proj_rate(double scale, double T) { return T > 0 ? fminf((float)(scale / T), 3.0e38f) : 0.f; }

// y = log1p(x scale / T) and w = min(y, mean_j + clip sd_j) / sd_j of a stored entry
__device__ __forceinline__ float proj_log(float x, float r) { return log1pf(x * r); }
__device__ __forceinline__ float proj_weight(float x, float r, float cap, float inv_sd) { return fminf(proj_log(x, r), cap) * inv_sd; }

// n <= 64 queued entries, lane l holding entry l (w = 0, j = 0 behind n), eight at a time in queue order
template <int NC>
__device__ __forceinline__ void proj_drain(const float* __restrict__ U, int zs, int lane, int jj, float ww, int n, float (&acc)[NC]) {
  for (int g = 0; g < n; g += 8) {
    int j[8]; float w[8], u[8][NC];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      j[k] = __builtin_amdgcn_readlane(jj, g + k);
      w[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ww), g + k));
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
#pragma unroll
      for (int c = 0; c < NC; c++) u[k][c] = U[(size_t)j[k] * zs + lane + 64 * c];
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
#pragma unroll
      for (int c = 0; c < NC; c++) acc[c] = fmaf(w[k], u[k][c], acc[c]);
    }
  }
}

// The wave's queue of contributing (row of the table, weight) pairs in LDS (qj, qw: 128 entries each), shared by k_project and
// k_doublet_project.  push: the lanes with keep append their (j, w) behind the qn waiting entries in lane order (ballot + prefix count; below =
// the mask of the lanes under this one); once 64 wait they are drained and the rest moves to the front.  flush: the drain of what is left.
template <int NC>
__device__ __forceinline__ void proj_queue_push(int* qj, float* qw, int& qn, unsigned long long below, int lane, bool keep, int j, float w,
                                                const float* __restrict__ U, int zs, float (&acc)[NC]) {
  const unsigned long long mask = __ballot(keep);
  if (keep) {
    const int at = qn + __popcll(mask & below);
    qj[at] = j; qw[at] = w;
  }
  qn += __popcll(mask);
  proj_wave_sync();
  if (qn >= 64) {
    const int jj = qj[lane]; const float ww = qw[lane];
    const int rj = qj[64 + lane]; const float rw = qw[64 + lane];
    proj_wave_sync();
    qj[lane] = rj; qw[lane] = rw;      // the entries behind the first 64 move to the front
    qn -= 64;
    proj_drain<NC>(U, zs, lane, jj, ww, 64, acc);
    proj_wave_sync();
  }
}
template <int NC>
__device__ __forceinline__ void proj_queue_flush(const int* qj, const float* qw, int qn, int lane, const float* __restrict__ U, int zs, float (&acc)[NC]) {
  const int jj = lane < qn ? qj[lane] : 0; const float ww = lane < qn ? qw[lane] : 0.f;
  proj_wave_sync();
  proj_drain<NC>(U, zs, lane, jj, ww, qn, acc);
}

}  // namespace hmx

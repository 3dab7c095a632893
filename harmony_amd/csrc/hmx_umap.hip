// hmx_umap.hip -- gfx950 kernels of the UMAP layout (include/harmony_mi355x_umap.h; DESIGN "The UMAP layout") on a symmetric CSR with float
// weights in [0, 1].  An epoch reads a snapshot of the positions and writes the next one: everything that moves cell i stands in row i, so
// there is no scatter and no floating-point atomic.  Which entries fire is decided in fp64 (one division, one product, one floor), the terms
// are fp32 with one fixed expression, the row's sum has one fixed shape: two calls give the same bits.
//
//   k_um_wmax             one wave per row: the largest off-diagonal weight (an integer atomicMax on the float's bits: non-negative floats
//                         order as unsigned integers); the rows above the short path's cap listed; the rows' firing counters zeroed;
//   k_um_epoch<DIM>       one wave per row of at most short_cap entries: lane l takes entries l, l + 64, ..; per fired entry the attraction
//                         to y_j and negative_sample_rate hashed repulsions, gathered from the snapshot four terms at a time and added in
//                         their order; xor butterfly; lane 0 writes;
//   k_um_epoch_long<DIM>  one workgroup per listed row: thread t takes entries t, t + 256, ..; butterfly per wave, the four waves' partials
//                         added as (0 + 1) + (2 + 3);
//   k_um_fired            the rows' firing counters added up (integers).
// Every loop has a bound known on entry; no kernel waits for another workgroup; integer atomics only; no LDS but the long path's partials.
#include "hmx_umap.h"
#include "hmx_um_device.h"      // um_fmix32, um_load, um_clip, um_term: shared with hmx_umap_transform.hip

namespace hmx {

// entry e of row i: 1 if it fired.  r = dbl(w) / dbl(wmax); fires iff floor(dbl(n + 1) r) > floor(dbl(n) r)
template <int DIM>
__device__ __forceinline__ unsigned um_entry(const UmDev& D, long long i, long long e, float xi, float yi, float zi, float& ax, float& ay, float& az) {
  const int j = D.indices[e];
  if (j == (int)i) return 0u;
  const double r = __ddiv_rn((double)D.weights[e], D.wmax);
  if (!(floor(__dmul_rn((double)(D.n + 1), r)) > floor(__dmul_rn((double)D.n, r)))) return 0u;
  // term 0 is the attraction to y_j, term s >= 1 the negative sample s - 1.  The other ends are gathered four terms at a time, ahead of the
  // arithmetic, so that a step waits for one round of loads and not for four; the terms are added in their order either way.
  const int terms = D.g2b != 0.0f ? 1 + D.nneg : 1;
  for (int s0 = 0; s0 < terms; s0 += 4) {
    long long o[4];
    float xo[4], yo[4], zo[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int s = s0 + u;
      long long k = i;                                           // no term: the cell itself, skipped below
      if (s == 0) k = j;
      else if (s < terms)
        k = (long long)(((unsigned long long)um_fmix32((unsigned)e ^ um_fmix32(D.kbase + (unsigned)(s - 1))) * (unsigned long long)D.N) >> 32);
      o[u] = k;
      um_load<DIM>(D.yold, k, xo[u], yo[u], zo[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if (o[u] == i) continue;                                   // a sample that drew the cell itself, or no term
      if (s0 + u == 0) um_term<DIM, true>(D, xi - xo[u], yi - yo[u], zi - zo[u], ax, ay, az);
      else um_term<DIM, false>(D, xi - xo[u], yi - yo[u], zi - zo[u], ax, ay, az);
    }
  }
  return 1u;
}
template <int DIM>
__device__ __forceinline__ void um_write(const UmDev& D, long long i, unsigned cnt, float xi, float yi, float zi, float sx, float sy, float sz) {
  float* o = D.ynew + DIM * i;
  if (cnt == 0u) { o[0] = xi; o[1] = yi; if (DIM == 3) o[2] = zi; return; }      // nothing fired: the position is copied
  o[0] = xi + D.alpha * sx;
  o[1] = yi + D.alpha * sy;
  if (DIM == 3) o[2] = zi + D.alpha * sz;
  D.fired[i] += cnt;                                             // (the row has one writer per epoch, and the epochs follow each other)
}

__global__ __launch_bounds__(256) void k_um_wmax(UmDev D) {
  const int l = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= D.N) return;
  const long long b = D.indptr[i], e1 = D.indptr[i + 1];
  unsigned m = 0u;
  for (long long e = b + l; e < e1; e += 64) {
    const float w = D.weights[e];
    if (D.indices[e] != (int)i && w > 0.0f && w <= 1.0f) m = max(m, __float_as_uint(w));      // (a weight the check refuses is never used)
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, s, 64));
  if (l != 0) return;
  // (most rows of a kNN graph hold the largest weight: the word only grows, so a row at or below what it reads there has nothing to add, and a
  // stale read costs one atomic more, never a wrong maximum)
  if (m > *(volatile unsigned*)D.wbits) atomicMax(D.wbits, m);
  D.fired[i] = 0ull;
  if (e1 - b > D.short_cap) {
    const unsigned at = atomicAdd(D.nlong, 1u);
    if ((long long)at < D.N) D.longrows[at] = (int)i;
  }
}

template <int DIM>
__global__ __launch_bounds__(256) void k_um_epoch(UmDev D) {
  const int l = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= D.N) return;
  const long long b = D.indptr[i], len = D.indptr[i + 1] - b;
  if (len > D.short_cap) return;                                 // a long row
  float xi, yi, zi, ax = 0.0f, ay = 0.0f, az = 0.0f;
  um_load<DIM>(D.yold, i, xi, yi, zi);
  unsigned cnt = 0u;
  for (long long t = l; t < len; t += 64) cnt += um_entry<DIM>(D, i, b + t, xi, yi, zi, ax, ay, az);
  cnt = wave_sum(cnt);
  ax = wave_sum(ax);
  ay = wave_sum(ay);
  if (DIM == 3) az = wave_sum(az);
  if (l == 0) um_write<DIM>(D, i, cnt, xi, yi, zi, ax, ay, az);
}

template <int DIM>
__global__ __launch_bounds__(256) void k_um_epoch_long(UmDev D) {
  __shared__ float ps[4][3];
  __shared__ unsigned pc[4];
  const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
  const unsigned nlong = (unsigned)min((long long)*D.nlong, D.N);
  for (unsigned r = blockIdx.x; r < nlong; r += gridDim.x) {
    const long long i = D.longrows[r];
    const long long b = D.indptr[i], len = D.indptr[i + 1] - b;
    float xi, yi, zi, ax = 0.0f, ay = 0.0f, az = 0.0f;
    um_load<DIM>(D.yold, i, xi, yi, zi);
    unsigned cnt = 0u;
    for (long long t = tid; t < len; t += 256) cnt += um_entry<DIM>(D, i, b + t, xi, yi, zi, ax, ay, az);
    cnt = wave_sum(cnt);
    ax = wave_sum(ax);
    ay = wave_sum(ay);
    if (DIM == 3) az = wave_sum(az);
    if (l == 0) { ps[wv][0] = ax; ps[wv][1] = ay; ps[wv][2] = az; pc[wv] = cnt; }
    __syncthreads();
    if (tid == 0)
      um_write<DIM>(D, i, (pc[0] + pc[1]) + (pc[2] + pc[3]), xi, yi, zi, (ps[0][0] + ps[1][0]) + (ps[2][0] + ps[3][0]),
                    (ps[0][1] + ps[1][1]) + (ps[2][1] + ps[3][1]), (ps[0][2] + ps[1][2]) + (ps[2][2] + ps[3][2]));
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_um_fired(UmDev D) {
  __shared__ unsigned long long part[4];
  unsigned long long s = 0ull;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < D.N; i += (long long)gridDim.x * 256) s += D.fired[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(D.total, part[0] + part[1] + part[2] + part[3]);
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------------------
static dim3 um_waves4(long long n) { return dim3((unsigned)((n + 3) / 4)); }

void l_um_wmax(const Launch& L, const UmDev& D) { hipLaunchKernelGGL(k_um_wmax, um_waves4(D.N), dim3(256), 0, L.stream, D); }
void l_um_epoch(const Launch& L, const UmDev& D, int dim, bool with_long) {
  if (dim == 2) {
    hipLaunchKernelGGL(k_um_epoch<2>, um_waves4(D.N), dim3(256), 0, L.stream, D);
    if (with_long) hipLaunchKernelGGL(k_um_epoch_long<2>, dim3(UM_LONG_WGS), dim3(256), 0, L.stream, D);
  } else {
    hipLaunchKernelGGL(k_um_epoch<3>, um_waves4(D.N), dim3(256), 0, L.stream, D);
    if (with_long) hipLaunchKernelGGL(k_um_epoch_long<3>, dim3(UM_LONG_WGS), dim3(256), 0, L.stream, D);
  }
}
void l_um_fired(const Launch& L, const UmDev& D) {
  hipLaunchKernelGGL(k_um_fired, dim3((unsigned)std::min<long long>((D.N + 255) / 256, 1024)), dim3(256), 0, L.stream, D);
}

}  // namespace hmx

// hmx_umap_transform.hip -- gfx950 kernels that put query cells into a fitted UMAP layout (include/harmony_mi355x_umap_transform.h; DESIGN
// "Query cells in a fitted layout").  The reference's positions are fixed and a query cell is pulled and pushed by reference cells alone, so
// every cell is independent of every other one: all its epochs run in one launch with its position in registers.
//
//   k_ut_weights          one wave per list, lane l holds entries l and l + 64 (k_smooth_knn's layout): rho = 0, the search of sigma over the
//                         entries behind the first, the floor from the global mean distance, the k weights exp(-d / sigma) in fp64;
//   k_ut_init<DIM>        one thread per cell: the weighted mean of the listed positions in fp64, entry by entry; the plain mean where every
//                         weight is 0;
//   k_ut_transform<DIM, G>  a group of G lanes per cell (16: four cells to a wave, lists of up to 16 entries; 64: two entries per lane): a lane
//                         loads its entry's index, firing rate and reference position once; per epoch the fired entries' attraction and hashed
//                         repulsions, the samples gathered four at a time ahead of the arithmetic and added in their order; an xor butterfly
//                         over the group leaves the same bits in every lane, each of which updates its own copy of the position; lane 0 of the
//                         group writes the position and the cell's firing count once, at the end.
// Every loop has a bound known on entry; no kernel waits for another workgroup; no LDS, no scratch, no atomics.
#include "hmx_umap_transform.h"
#include "hmx_um_device.h"

namespace hmx {

// ---- the weights of the lists ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ut_weights(UqDev Q) {
  const int l = threadIdx.x & 63, k = Q.k;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= Q.Nq) return;                                     // (the whole wave)
  const bool h0 = l < k, h1 = l + 64 < k;
  const size_t at = (size_t)row * k + l;
  const double d0 = h0 ? (double)Q.dist[at] : 0.0, d1 = h1 ? (double)Q.dist[at + 64] : 0.0;
  // the search leaves the list's first entry out (umap-learn's smooth_knn_dist walks columns 1 .. k - 1); the weights below do not
  const bool s0 = h0 && l != 0;
  const double target = log2((double)k);
  double lo = 0.0, hi = INFINITY, mid = 1.0;
  for (int step = 0; step < 64; step++) {
    const double t0 = s0 ? (d0 > 0.0 ? exp(-d0 / mid) : 1.0) : 0.0, t1 = h1 ? (d1 > 0.0 ? exp(-d1 / mid) : 1.0) : 0.0;
    const double psum = wave_sum(t0 + t1);
    if (fabs(psum - target) < 1e-5) break;
    if (psum > target) { hi = mid; mid = (lo + hi) / 2; }
    else { lo = mid; mid = isinf(hi) ? mid * 2 : (lo + hi) / 2; }
  }
  const double sigma = fmax(mid, 1e-3 * (Q.total[0] / ((double)Q.Nq * (double)k)));      // (rho = 0: always the global mean)
  if (h0) Q.w[at] = (float)((d0 <= 0.0 || sigma == 0.0) ? 1.0 : exp(-d0 / sigma));
  if (h1) Q.w[at + 64] = (float)((d1 <= 0.0 || sigma == 0.0) ? 1.0 : exp(-d1 / sigma));
  if (l == 0) Q.sigma[row] = sigma;
}

// ---- the start: the weighted mean of the listed positions ---------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(256) void k_ut_init(UtDev D) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= D.Nq) return;
  const size_t at = (size_t)i * D.k;
  double sw = 0.0, sx = 0.0, sy = 0.0, sz = 0.0, mx = 0.0, my = 0.0, mz = 0.0;
  for (int t = 0; t < D.k; t++) {
    const double w = (double)D.w[at + t];
    float x, y, z;
    um_load<DIM>(D.yref, D.idx[at + t], x, y, z);
    sw += w;
    sx += w * (double)x; sy += w * (double)y; sz += w * (double)z;
    mx += (double)x; my += (double)y; mz += (double)z;
  }
  const bool none = !(sw > 0.0);                               // every weight underflowed: the plain mean
  const double den = none ? (double)D.k : sw;
  float* o = D.y0 + DIM * i;
  o[0] = (float)((none ? mx : sx) / den);
  o[1] = (float)((none ? my : sy) / den);
  if (DIM == 3) o[2] = (float)((none ? mz : sz) / den);
}

// ---- every epoch of every cell -------------------------------------------------------------------------------------------------------------------
template <int DIM, int G>
__global__ __launch_bounds__(256) void k_ut_transform(UtDev D) {
  constexpr int EPL = G == 64 ? 2 : 1;                         // entries per lane
  const int lane = threadIdx.x & 63, lg = lane & (G - 1);
  const long long cell = ((long long)blockIdx.x * 256 + threadIdx.x) / G;
  // a group behind the last cell walks the last cell again and writes nothing: every lane of a wave reaches every ballot and shuffle
  const long long i = min(cell, D.Nq - 1);
  float xi, yi, zi;
  um_load<DIM>(D.y0, i, xi, yi, zi);
  unsigned e[EPL];
  double r[EPL], fl[EPL];
  float xj[EPL], yj[EPL], zj[EPL];
#pragma unroll
  for (int u = 0; u < EPL; u++) {
    const int slot = lg + 64 * u;
    const bool have = slot < D.k;
    e[u] = (unsigned)((long long)i * D.k + (have ? slot : 0));
    const int j = D.idx[e[u]];
    r[u] = have ? __ddiv_rn((double)D.w[e[u]], D.wmax) : 0.0;      // (no entry: a rate of 0 never fires)
    um_load<DIM>(D.yref, j, xj[u], yj[u], zj[u]);
    fl[u] = floor(__dmul_rn((double)D.n0, r[u]));
  }
  const int nneg = D.g2b != 0.0f ? D.nneg : 0;
  unsigned cnt = 0u;
  for (int n = D.n0; n < D.n1; n++) {
    const unsigned kb = D.kbase0 + 32u * (unsigned)n;
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    unsigned nf = 0u;
#pragma unroll
    for (int u = 0; u < EPL; u++) {
      // fires iff floor(dbl(n + 1) r) > floor(dbl(n) r); the right side is the left side of the epoch before
      const double fn = floor(__dmul_rn((double)(n + 1), r[u]));
      const bool fired = fn > fl[u];
      fl[u] = fn;
      const unsigned long long bal = __ballot(fired);
      nf += G == 64 ? (unsigned)__popcll(bal) : (unsigned)__popc((unsigned)(bal >> (lane & ~(G - 1))) & ((1u << (G & 31)) - 1u));
      if (!fired) continue;
      um_term<DIM, true, false>(D, xi - xj[u], yi - yj[u], zi - zj[u], ax, ay, az);
      // the samples' addresses do not depend on y: four loads are issued ahead of the arithmetic; the terms are added in their order
      for (int s0 = 0; s0 < nneg; s0 += 4) {
        float xo[4], yo[4], zo[4];
#pragma unroll
        for (int v = 0; v < 4; v++) {
          const int s = s0 + v;
          long long o = 0;                                     // (no term: cell 0's position is read and skipped below)
          if (s < nneg) o = (long long)(((unsigned long long)um_fmix32(e[u] ^ um_fmix32(kb + (unsigned)s)) * (unsigned long long)D.Nr) >> 32);
          um_load<DIM>(D.yref, o, xo[v], yo[v], zo[v]);
        }
#pragma unroll
        for (int v = 0; v < 4; v++)
          if (s0 + v < nneg) um_term<DIM, false>(D, xi - xo[v], yi - yo[v], zi - zo[v], ax, ay, az);
      }
    }
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) {
      ax += __shfl_xor(ax, m, 64);
      ay += __shfl_xor(ay, m, 64);
      if (DIM == 3) az += __shfl_xor(az, m, 64);
    }
    if (nf != 0u) {                                            // (the same in every lane of the group; nothing fired: the bits are kept)
      const float alpha = D.alpha[n - D.n0];
      xi = xi + alpha * ax;
      yi = yi + alpha * ay;
      if (DIM == 3) zi = zi + alpha * az;
      cnt += nf;
    }
  }
  if (lg != 0 || cell >= D.Nq) return;
  float* o = D.y + DIM * cell;
  o[0] = xi; o[1] = yi;
  if (DIM == 3) o[2] = zi;
  D.fired[cell] = (unsigned long long)cnt;
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------------
void l_ut_weights(const Launch& L, const UqDev& Q) {
  hipLaunchKernelGGL(k_ut_weights, dim3((unsigned)((Q.Nq + 3) / 4)), dim3(256), 0, L.stream, Q);
}
void l_ut_init(const Launch& L, const UtDev& D, int dim) {
  const dim3 grid((unsigned)((D.Nq + 255) / 256));
  if (dim == 2) hipLaunchKernelGGL(k_ut_init<2>, grid, dim3(256), 0, L.stream, D);
  else hipLaunchKernelGGL(k_ut_init<3>, grid, dim3(256), 0, L.stream, D);
}
void l_ut_transform(const Launch& L, const UtDev& D, int dim) {
  const int g = D.k <= UT_SMALL_K ? 16 : 64;
  const dim3 grid((unsigned)((D.Nq * g + 255) / 256));
  if (dim == 2) {
    if (g == 16) hipLaunchKernelGGL((k_ut_transform<2, 16>), grid, dim3(256), 0, L.stream, D);
    else hipLaunchKernelGGL((k_ut_transform<2, 64>), grid, dim3(256), 0, L.stream, D);
  } else {
    if (g == 16) hipLaunchKernelGGL((k_ut_transform<3, 16>), grid, dim3(256), 0, L.stream, D);
    else hipLaunchKernelGGL((k_ut_transform<3, 64>), grid, dim3(256), 0, L.stream, D);
  }
}

}  // namespace hmx

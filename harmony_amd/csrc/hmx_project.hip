// hmx_project.hip -- gfx950 kernel of the count projection (include/harmony_mi355x_project.h; DESIGN "Projecting query counts").
//
//   k_project<NC, F64>  one wave per cell, four waves per workgroup, cells in a grid-stride loop.  A cell is a CSR row of raw counts; the result
//                       is its row of PCs, P = b + sum over the stored entries whose gene has a slot j >= 0 of w U[j,:], w = min(log1p(x scale / T),
//                       cap_j) inv_sd_j.  The centring lives in b (host, fp64): the zeros of the row are never touched.
//       phase 1         T = the row's sum in fp64 (skipped when the caller gave totals): lanes stride the row, a butterfly adds the partials.
//       phase 2         the row again, 64 entries a sweep, PROJ_SWEEPS sweeps in flight (a row is a few KB: L2).  Every lane looks its entry's slot up and forms w; the contributing
//                       (j, w) of the sweep are appended, in CSR order, to the wave's queue in LDS (ballot + prefix count).  Only about G / G_all
//                       of the entries contribute, so a sweep rarely fills a register's worth: the queue is drained 64 at a time, and once at the
//                       end of the row.  A drain takes eight wave-uniform (j, w) at a time (readlane), issues their eight U row fetches -- lanes
//                       are PCs, U is G x zs fp32 with zs = 64 NC, served from L2 -- and then runs the eight dependent fmaf.
//                       The accumulation order of a cell is its CSR order whatever the grid, the slab or the residence of the matrix: no atomics
//                       on results, two calls are bit-identical.
//   Out-of-contract input never leaves the arrays: an indptr pair outside 0 <= lo <= hi <= nnz empties the row, a column outside [0, G_all) or a
//   negative / non-finite value makes the entry non-contributing, and the kind of violation is or-ed into one flag word the host reads back.
#include "hmx_proj_row.h"      // (proj_wave_sync, proj_row_total, proj_rate, proj_weight, proj_drain: shared with hmx_pca.hip; the queue: with hmx_doublets.hip)

namespace hmx {

template <int NC, bool F64>
__global__ __launch_bounds__(256) void k_project(ProjDev P) {
  __shared__ int qj[PROJ_WAVES][128];
  __shared__ float qw[PROJ_WAVES][128];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int zs = 64 * NC;
  const unsigned long long below = lane ? ~0ull >> (64 - lane) : 0ull;
  unsigned bad = 0;
  for (long long i = (long long)blockIdx.x * PROJ_WAVES + wv; i < P.nrows; i += (long long)gridDim.x * PROJ_WAVES) {
    long long lo = P.indptr[i] - P.base, hi = P.indptr[i + 1] - P.base;
    if (lo < 0 || hi < lo || hi > P.nnz) { bad |= PROJ_BAD_INDPTR; lo = hi = 0; }
    // ---- phase 1: the library size
    const double T = P.totals ? P.totals[P.row0 + i] : proj_row_total<F64>(P.data, lo, hi, lane);
    const float r = proj_rate(P.scale, T);      // (T = 0: an empty row or stored zeros, y = 0 and P = b)
    // ---- phase 2
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.f;
    int qn = 0;
    for (long long p = lo; p < hi; p += 64 * PROJ_SWEEPS) {      // (hi > lo here)
      // PROJ_SWEEPS sweeps of 64 entries at a time, every load unconditional (clamped addresses): the three dependent fetches of an entry --
      // column and value, slot, cap and 1 / sd -- are in flight for all the sweeps at once
      int col[PROJ_SWEEPS], j[PROJ_SWEEPS]; float x[PROJ_SWEEPS], w[PROJ_SWEEPS]; bool in[PROJ_SWEEPS];
#pragma unroll
      for (int s = 0; s < PROJ_SWEEPS; s++) {
        const long long e = p + 64 * s + lane;
        in[s] = e < hi;
        const long long ee = in[s] ? e : hi - 1;
        col[s] = P.indices[ee];
        x[s] = F64 ? (float)((const double*)P.data)[ee] : ((const float*)P.data)[ee];
      }
#pragma unroll
      for (int s = 0; s < PROJ_SWEEPS; s++) {
        const bool okc = (unsigned)col[s] < (unsigned)P.G_all;
        const bool okx = x[s] >= 0.f && x[s] <= 3.0e38f;
        if (in[s] && !okc) bad |= PROJ_BAD_COLUMN;
        if (in[s] && !okx) bad |= x[s] < 0.f ? PROJ_BAD_NEGATIVE : PROJ_BAD_NONFINITE;
        j[s] = P.slot[okc ? col[s] : 0];
        if (!(in[s] && okc && okx) || (unsigned)j[s] >= (unsigned)P.G) j[s] = -1;
      }
#pragma unroll
      for (int s = 0; s < PROJ_SWEEPS; s++) {
        const int jc = j[s] >= 0 ? j[s] : 0;
        w[s] = proj_weight(x[s], r, P.cap[jc], P.inv_sd[jc]);
      }
#pragma unroll
      for (int s = 0; s < PROJ_SWEEPS; s++)      // (a sweep behind the row's end: no lane)
        proj_queue_push<NC>(qj[wv], qw[wv], qn, below, lane, j[s] >= 0, j[s], w[s], P.U, zs, acc);
    }
    proj_queue_flush<NC>(qj[wv], qw[wv], qn, lane, P.U, zs, acc);
#pragma unroll
    for (int c = 0; c < NC; c++) {
      const int pc = lane + 64 * c;
      if (pc < P.d) P.out[(size_t)(P.row0 + i) * P.d + pc] = (float)((double)acc[c] + P.b[pc]);
    }
  }
  if (bad) atomicOr(P.flag, bad);
}

void l_project(const Launch& L, const ProjDev& P, hipStream_t stream) {
  if (P.nrows <= 0) return;
  const long long want = (P.nrows + PROJ_WAVES - 1) / PROJ_WAVES;
  const dim3 grid((unsigned)std::min<long long>(want, 256 * 8));
  const int nc = (P.d + 63) / 64;
  (void)L;
  if (nc == 1) {
    if (P.f64) hipLaunchKernelGGL((k_project<1, true>), grid, dim3(64 * PROJ_WAVES), 0, stream, P);
    else hipLaunchKernelGGL((k_project<1, false>), grid, dim3(64 * PROJ_WAVES), 0, stream, P);
  } else {
    if (P.f64) hipLaunchKernelGGL((k_project<2, true>), grid, dim3(64 * PROJ_WAVES), 0, stream, P);
    else hipLaunchKernelGGL((k_project<2, false>), grid, dim3(64 * PROJ_WAVES), 0, stream, P);
  }
}

}  // namespace hmx

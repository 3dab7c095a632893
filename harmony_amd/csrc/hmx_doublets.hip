// hmx_doublets.hip -- gfx950 kernels of the doublet detection (include/harmony_mi355x_doublets.h; DESIGN "Doublet detection").
//
//   k_doublet_project<NC, F64>  one wave per synthetic cell, cells in a grid-stride loop, 4 / 2 / 1 waves per workgroup by G (hmx_doublet_plan.h).
//                       A synthetic cell is the SUM of the raw counts of two observed cells (its parents, rows a and b of the CSR matrix) taken
//                       before the log; the result is its row of PCs, P = b + sum over the reference slots j either parent stores of w U[j,:],
//                       w = min(log1p((x_aj + x_bj) scale / (T_a + T_b)), cap_j) inv_sd_j -- k_project's arithmetic (hmx_proj_row.h) on the merged row.
//       phase 1         T_a and T_b in fp64 as in k_project (skipped when the caller gave totals), T = T_a + T_b.
//       phase 2         row a, then row b: 64 entries a sweep, PROJ_SWEEPS sweeps in flight, clamped addresses.  An entry whose gene has a slot
//                       j >= 0 adds its value into word j of the wave's OWN table in LDS (gp fp32 words).  No column twice in a row and the rows
//                       one after the other: no two lanes of a pass target one word, plain read-add-write, no atomics.  A scatter: of the 32
//                       lanes of a half about 32 G / G_all carry a slot, on 32 banks -- a 2-way conflict in one instruction of three at
//                       G / G_all = 1 / 4, rarer below; each costs one LDS cycle beside the three dependent global loads of the sweep.
//       phase 3         the table in ascending order, 64 slots a sweep (stride 1: conflict-free), every word zeroed as it is read -- the table is
//                       clean for the wave's next cell.  w from the per-slot tables; the non-zero slots are compacted (ballot) into k_project's
//                       queue and drained exactly as there: eight wave-uniform (j, w), their U rows fetched ahead of the eight fmaf, lanes = PCs.
//                       The accumulation order is the ascending slot order: a function of the two rows as SETS.  The order of the entries
//                       inside a CSR row, of the two parents, the grid and the residence of the matrix do not reach the bits.
//   Out-of-contract input never leaves the arrays (as in k_project): an indptr pair outside 0 <= lo <= hi <= nnz empties that parent, a column
//   outside [0, G_all) or a negative / non-finite value makes the entry non-contributing, the kind of violation is or-ed into one flag word.
//
//   k_doublet_count     one thread per row of the neighbour lists [N][m]: the entries >= n_obs.  An integer per row, no atomics.
#include "hmx_proj_row.h"
#include "hmx_doublets.h"

namespace hmx {

// the entries [lo, hi) of one parent into the wave's table
template <bool F64>
__device__ __forceinline__ void dbl_scatter(const ProjDev& P, long long lo, long long hi, int lane, float* tab, unsigned& bad) {
  for (long long p = lo; p < hi; p += 64 * PROJ_SWEEPS) {      // (hi > lo here)
    int col[PROJ_SWEEPS], j[PROJ_SWEEPS]; float x[PROJ_SWEEPS]; bool in[PROJ_SWEEPS];
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
    for (int s = 0; s < PROJ_SWEEPS; s++)
      if (j[s] >= 0) tab[j[s]] += x[s];      // (j < G <= gp)
  }
}

template <int NC, bool F64>
__global__ __launch_bounds__(256) void k_doublet_project(DoubletDev D) {
  extern __shared__ float dbl_lds[];      // [waves][gp] slot tables | [waves][DBL_QUEUE] queued slots | [waves][DBL_QUEUE] queued weights
  const ProjDev& P = D.C;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const int zs = 64 * NC;
  const unsigned long long below = lane ? ~0ull >> (64 - lane) : 0ull;
  float* tab = dbl_lds + (size_t)wv * D.gp;
  int* qj = (int*)(dbl_lds + (size_t)waves * D.gp) + wv * DBL_QUEUE;
  float* qw = dbl_lds + (size_t)waves * D.gp + (size_t)waves * DBL_QUEUE + wv * DBL_QUEUE;
  for (int t = lane; t < D.gp; t += 64) tab[t] = 0.f;
  proj_wave_sync();
  unsigned bad = 0;
  for (long long s = (long long)blockIdx.x * waves + wv; s < D.n_sim; s += (long long)gridDim.x * waves) {
    const long long pa = D.pairs[2 * s], pb = D.pairs[2 * s + 1];
    long long alo = P.indptr[pa], ahi = P.indptr[pa + 1], blo = P.indptr[pb], bhi = P.indptr[pb + 1];
    if (alo < 0 || ahi < alo || ahi > P.nnz) { bad |= PROJ_BAD_INDPTR; alo = ahi = 0; }
    if (blo < 0 || bhi < blo || bhi > P.nnz) { bad |= PROJ_BAD_INDPTR; blo = bhi = 0; }
    // ---- phase 1: the library size of the sum
    const double Ta = P.totals ? P.totals[pa] : proj_row_total<F64>(P.data, alo, ahi, lane);
    const double Tb = P.totals ? P.totals[pb] : proj_row_total<F64>(P.data, blo, bhi, lane);
    const float r = proj_rate(P.scale, Ta + Tb);      // (T = 0: y = 0 and P = b)
    // ---- phase 2: x_a + x_b by slot
    dbl_scatter<F64>(P, alo, ahi, lane, tab, bad);
    proj_wave_sync();
    dbl_scatter<F64>(P, blo, bhi, lane, tab, bad);
    proj_wave_sync();
    // ---- phase 3: the table in ascending slot order
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.f;
    int qn = 0;
    for (int base = 0; base < D.gp; base += 64 * PROJ_SWEEPS) {
      float v[PROJ_SWEEPS], w[PROJ_SWEEPS], cp[PROJ_SWEEPS], is[PROJ_SWEEPS];
#pragma unroll
      for (int k = 0; k < PROJ_SWEEPS; k++) {
        const int j = base + 64 * k + lane;
        v[k] = 0.f;
        if (base + 64 * k < D.gp) { v[k] = tab[j]; tab[j] = 0.f; }      // (wave-uniform; gp is a multiple of 64)
        const int jc = j < P.G ? j : P.G - 1;
        cp[k] = P.cap[jc]; is[k] = P.inv_sd[jc];
      }
#pragma unroll
      for (int k = 0; k < PROJ_SWEEPS; k++) w[k] = proj_weight(v[k], r, cp[k], is[k]);
#pragma unroll
      for (int k = 0; k < PROJ_SWEEPS; k++)      // (only slots below G were written: v > 0 implies j < G)
        proj_queue_push<NC>(qj, qw, qn, below, lane, v[k] > 0.f, base + 64 * k + lane, w[k], P.U, zs, acc);
    }
    proj_queue_flush<NC>(qj, qw, qn, lane, P.U, zs, acc);
    proj_wave_sync();
#pragma unroll
    for (int c = 0; c < NC; c++) {
      const int pc = lane + 64 * c;
      if (pc < P.d) P.out[(size_t)s * P.d + pc] = (float)((double)acc[c] + P.b[pc]);
    }
  }
  if (bad) atomicOr(P.flag, bad);
}

__global__ __launch_bounds__(256) void k_doublet_count(const int* __restrict__ idx, long long N, int m, long long n_obs, int* __restrict__ cnt) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
    const int* row = idx + (size_t)i * m;
    int c = 0;
    for (int k = 0; k < m; k++) c += row[k] >= n_obs ? 1 : 0;
    cnt[i] = c;
  }
}

void l_doublet_project(const Launch& L, const DoubletDev& D, const DoubletPlan& plan, hipStream_t stream) {
  (void)L;
  if (D.n_sim <= 0 || plan.waves <= 0) return;
  const dim3 grid(plan.grid), block(64 * plan.waves);
  const size_t lds = (size_t)plan.lds_bytes;
  if (plan.nc == 1) {
    if (D.C.f64) hipLaunchKernelGGL((k_doublet_project<1, true>), grid, block, lds, stream, D);
    else hipLaunchKernelGGL((k_doublet_project<1, false>), grid, block, lds, stream, D);
  } else {
    if (D.C.f64) hipLaunchKernelGGL((k_doublet_project<2, true>), grid, block, lds, stream, D);
    else hipLaunchKernelGGL((k_doublet_project<2, false>), grid, block, lds, stream, D);
  }
}

void l_doublet_count(const Launch& L, const int* idx, long long N, int m, long long n_obs, int* cnt, hipStream_t stream) {
  (void)L;
  if (N <= 0) return;
  const dim3 grid((unsigned)std::min<long long>((N + 255) / 256, 256 * 8));
  hipLaunchKernelGGL(k_doublet_count, grid, dim3(256), 0, stream, idx, N, m, n_obs, cnt);
}

}  // namespace hmx

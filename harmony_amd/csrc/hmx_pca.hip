// hmx_pca.hip -- gfx950 kernels of the reference's PCA from raw counts (include/harmony_mi355x_pca.h; DESIGN "Fitting the loadings").
//
//   k_gene_stats<F64>        per gene: stored positive entries, sum of y and of y^2, y = log1p(x scale / T) in k_project's fp32 arithmetic.  y and y^2 are
//                            quantised to a power-of-two step and added as 64-bit INTEGERS: a workgroup (16 waves, one cell per wave at a time) keeps the
//                            tables of PCA_STAT_GENES genes in LDS (ds atomics), grid.y sweeps the gene ranges, and at the end every touched gene costs one
//                            global integer add per workgroup.  Integer sums do not depend on the order: any grid, slab split or cell order gives the same bits.
//   k_gene_stats_grouped<F64> the same sums per (group, gene): the cells arrive as chunks of one group each (hmx_group_plan.h), a workgroup's tables belong
//                            to one group at a time and are flushed where the group changes (include/harmony_mi355x_groups.h; DESIGN "Gene statistics per group").
//   k_pca_compact<F64, FILL> the raw CSR once to count (FILL = false) and once to fill: per cell its contributing (j, w) in CSR order (ballot prefix),
//                            w by proj_weight -- the expression k_project uses.
//   k_pca_hist / k_pca_scan / k_pca_place   the same entries gene-major, (cell, w) per gene in ascending cell order: a stable counting sort by gene over tiles of
//                            PCA_TILE cells.  Histogram per tile (LDS), exclusive scan over the tiles per gene, then ONE wave per tile walks its cells in order
//                            and places every entry at its gene's running offset for that tile (LDS; a gene occurs once per row, so lanes never collide).
//   k_pca_p<NC>              P = S V over the compact list: one wave per cell, lanes are columns, proj_drain's fmaf chain in CSR order, b added in fp64.
//   k_pca_colsum1 / 2        the column sums of P in fp64: ranges of PCA_COLSUM_ROWS rows one after the other, then the ranges one after the other.
//   k_pca_w<NC> / k_pca_wred W = S^T P over the gene-major list: one wave per chunk of <= PCA_CHUNK entries of ONE gene, proj_drain over the rows of P the list names,
//                            runs of PCA_RUN entries in fp32 flushed into fp64; then per gene the chunks in order and - (mean / sd) colsum.
//   No float atomics anywhere; every order of additions is fixed by the lists alone.
#include "hmx_proj_row.h"

namespace hmx {

// one cell of the gene statistics, one wave: the stored entries of row i whose gene lies in [g0, g0 + ng) into the workgroup's LDS tables
template <bool F64>
__device__ __forceinline__ void stat_row(const PcaStatDev& S, long long i, int lane, int g0, int ng, unsigned long long* t1, unsigned long long* t2,
                                         unsigned* tn, unsigned& bad) {
  const ProjDev& P = S.C;
  long long lo = P.indptr[i] - P.base, hi = P.indptr[i + 1] - P.base;
  if (lo < 0 || hi < lo || hi > P.nnz) { bad |= PROJ_BAD_INDPTR; lo = hi = 0; }
  const double T = P.totals ? P.totals[P.row0 + i] : proj_row_total<F64>(P.data, lo, hi, lane);
  const float r = proj_rate(P.scale, T);
  for (long long e = lo + lane; e < hi; e += 64) {
    const int col = P.indices[e];
    const double xd = F64 ? ((const double*)P.data)[e] : (double)((const float*)P.data)[e];
    const float x = (float)xd;
    const bool okc = (unsigned)col < (unsigned)P.G_all;
    const bool okx = x >= 0.f && x <= 3.0e38f;
    if (!okc) bad |= PROJ_BAD_COLUMN;
    if (!okx) bad |= x < 0.f ? PROJ_BAD_NEGATIVE : PROJ_BAD_NONFINITE;
    const int g = col - g0;
    if (okc && okx && xd > 0 && g >= 0 && g < ng) {
      const double y = (double)fminf(proj_log(x, r), S.ymax);
      atomicAdd(&t1[g], (unsigned long long)__double2ll_rn(y * S.q1));
      atomicAdd(&t2[g], (unsigned long long)__double2ll_rn(y * y * S.q2));
      atomicAdd(&tn[g], 1u);
    }
  }
}

template <bool F64>
__global__ __launch_bounds__(1024) void k_gene_stats(PcaStatDev S) {
  __shared__ unsigned long long t1[PCA_STAT_GENES], t2[PCA_STAT_GENES];
  __shared__ unsigned tn[PCA_STAT_GENES];
  const ProjDev& P = S.C;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int g0 = blockIdx.y * PCA_STAT_GENES, ng = min(P.G_all - g0, PCA_STAT_GENES);
  for (int g = threadIdx.x; g < ng; g += 1024) { t1[g] = 0; t2[g] = 0; tn[g] = 0; }
  __syncthreads();
  unsigned bad = 0;
  for (long long i = (long long)blockIdx.x * 16 + wv; i < P.nrows; i += (long long)gridDim.x * 16) stat_row<F64>(S, i, lane, g0, ng, t1, t2, tn, bad);
  __syncthreads();
  for (int g = threadIdx.x; g < ng; g += 1024)
    if (tn[g]) {
      atomicAdd(&S.s1[g0 + g], t1[g]); atomicAdd(&S.s2[g0 + g], t2[g]); atomicAdd(&S.n[g0 + g], (unsigned long long)tn[g]);
    }
  if (bad) atomicOr(P.flag, bad);
}

void l_gene_stats(const PcaStatDev& S, hipStream_t stream) {
  const ProjDev& P = S.C;
  if (P.nrows <= 0) return;
  const dim3 grid((unsigned)std::min<long long>((P.nrows + 15) / 16, 256), (unsigned)((P.G_all + PCA_STAT_GENES - 1) / PCA_STAT_GENES));
  if (P.f64) hipLaunchKernelGGL((k_gene_stats<true>), grid, dim3(1024), 0, stream, S);
  else hipLaunchKernelGGL((k_gene_stats<false>), grid, dim3(1024), 0, stream, S);
}

// The same sums per (group, gene).  A workgroup walks a contiguous run of the launch's chunks (hmx_group_plan.h: <= GROUP_CHUNK cells of ONE group
// each; the run is cut from the chunk count and the grid, the chunks themselves from the labels alone); its LDS tables belong to one group at a
// time.  Where the group changes between two of its chunks it adds the touched genes into acc[group G_all + g] and clears them, a barrier on
// either side (the chunk loop's bounds and every chunk's group are uniform over the workgroup).  Integer adds: the grid, the cut of the runs and
// the order of the cells do not reach the bits.  Cost accepted: a group of a few cells touches few genes more than once, so it pays up to one
// global atomic per stored entry -- many tiny groups are slow, never wrong.
template <bool F64>
__global__ __launch_bounds__(1024) void k_gene_stats_grouped(GroupStatDev Q) {
  __shared__ unsigned long long t1[PCA_STAT_GENES], t2[PCA_STAT_GENES];
  __shared__ unsigned tn[PCA_STAT_GENES];
  const PcaStatDev& S = Q.S;
  const ProjDev& P = S.C;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int g0 = blockIdx.y * PCA_STAT_GENES, ng = min(P.G_all - g0, PCA_STAT_GENES);
  for (int g = threadIdx.x; g < ng; g += 1024) { t1[g] = 0; t2[g] = 0; tn[g] = 0; }
  const long long c0 = Q.nchunks * blockIdx.x / gridDim.x, c1 = Q.nchunks * (blockIdx.x + 1) / gridDim.x;
  auto flush = [&](int group) {      // between two barriers: every wave's ds atomics of `group` have landed, none of the next group has begun
    const size_t at = (size_t)group * P.G_all + g0;
    for (int g = threadIdx.x; g < ng; g += 1024)
      if (tn[g]) {
        atomicAdd(&S.s1[at + g], t1[g]); atomicAdd(&S.s2[at + g], t2[g]); atomicAdd(&S.n[at + g], (unsigned long long)tn[g]);
        t1[g] = 0; t2[g] = 0; tn[g] = 0;
      }
  };
  int cur = c0 < c1 ? Q.chunks[c0].group : 0;
  unsigned bad = 0;
  __syncthreads();
  for (long long c = c0; c < c1; c++) {
    const GroupChunk ch = Q.chunks[c];
    if (ch.group != cur) {
      __syncthreads();
      flush(cur);
      __syncthreads();
      cur = ch.group;
    }
    for (int k = wv; k < ch.len; k += 16) {
      const long long i = (long long)Q.perm[ch.start + k] - P.row0;
      if (i >= 0 && i < P.nrows) stat_row<F64>(S, i, lane, g0, ng, t1, t2, tn, bad);      // (the plan keeps a launch's chunks inside its rows)
    }
  }
  __syncthreads();
  flush(cur);
  if (bad) atomicOr(P.flag, bad);
}

void l_gene_stats_grouped(const GroupStatDev& Q, hipStream_t stream) {
  const ProjDev& P = Q.S.C;
  if (P.nrows <= 0 || Q.nchunks <= 0) return;
  const dim3 grid((unsigned)std::min<long long>(Q.nchunks, 256), (unsigned)((P.G_all + PCA_STAT_GENES - 1) / PCA_STAT_GENES));
  if (P.f64) hipLaunchKernelGGL((k_gene_stats_grouped<true>), grid, dim3(1024), 0, stream, Q);
  else hipLaunchKernelGGL((k_gene_stats_grouped<false>), grid, dim3(1024), 0, stream, Q);
}

template <bool F64, bool FILL>
__global__ __launch_bounds__(256) void k_pca_compact(PcaCompactDev S) {
  const ProjDev& P = S.C;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long below = lane ? ~0ull >> (64 - lane) : 0ull;
  unsigned bad = 0;
  for (long long i = (long long)blockIdx.x * PROJ_WAVES + wv; i < P.nrows; i += (long long)gridDim.x * PROJ_WAVES) {
    long long lo = P.indptr[i] - P.base, hi = P.indptr[i + 1] - P.base;
    if (lo < 0 || hi < lo || hi > P.nnz) { bad |= PROJ_BAD_INDPTR; lo = hi = 0; }
    float r = 0.f;
    long long at0 = 0;
    if (FILL) {
      const double T = P.totals ? P.totals[P.row0 + i] : proj_row_total<F64>(P.data, lo, hi, lane);
      r = proj_rate(P.scale, T);
      at0 = S.cptr[P.row0 + i];
    }
    long long n = 0;
    for (long long p = lo; p < hi; p += 64) {
      const long long e = p + lane;
      const bool in = e < hi;
      const long long ee = in ? e : hi - 1;
      const int col = P.indices[ee];
      const float x = F64 ? (float)((const double*)P.data)[ee] : ((const float*)P.data)[ee];
      const bool okc = (unsigned)col < (unsigned)P.G_all;
      const bool okx = x >= 0.f && x <= 3.0e38f;
      if (in && !okc) bad |= PROJ_BAD_COLUMN;
      if (in && !okx) bad |= x < 0.f ? PROJ_BAD_NEGATIVE : PROJ_BAD_NONFINITE;
      int j = P.slot[okc ? col : 0];
      if (!(in && okc && okx) || (unsigned)j >= (unsigned)P.G) j = -1;
      const unsigned long long mask = __ballot(j >= 0);
      if (FILL && j >= 0) {
        const long long at = at0 + n + __popcll(mask & below);
        if (at < S.entries) { S.cj[at] = j; S.cw[at] = proj_weight(x, r, P.cap[j], P.inv_sd[j]); }
      }
      n += __popcll(mask);
    }
    if (!FILL && lane == 0) S.cnt[P.row0 + i] = n;
  }
  if (bad) atomicOr(P.flag, bad);
}

void l_pca_compact(const PcaCompactDev& S, bool fill, hipStream_t stream) {
  const ProjDev& P = S.C;
  if (P.nrows <= 0) return;
  const dim3 grid((unsigned)std::min<long long>((P.nrows + PROJ_WAVES - 1) / PROJ_WAVES, 256 * 8)), block(64 * PROJ_WAVES);
  if (fill) {
    if (P.f64) hipLaunchKernelGGL((k_pca_compact<true, true>), grid, block, 0, stream, S);
    else hipLaunchKernelGGL((k_pca_compact<false, true>), grid, block, 0, stream, S);
  } else {
    if (P.f64) hipLaunchKernelGGL((k_pca_compact<true, false>), grid, block, 0, stream, S);
    else hipLaunchKernelGGL((k_pca_compact<false, false>), grid, block, 0, stream, S);
  }
}

// ---- the transposition: tile t = cells [t PCA_TILE, (t + 1) PCA_TILE), whatever the grid ----------------------------------------------------
__global__ __launch_bounds__(256) void k_pca_hist(PcaListDev T) {
  extern __shared__ int h_[];      // [G]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int g = threadIdx.x; g < T.G; g += 256) h_[g] = 0;
  __syncthreads();
  const long long c0 = (long long)blockIdx.x * PCA_TILE, c1 = min(c0 + PCA_TILE, T.N);
  for (long long i = c0 + wv; i < c1; i += 4)
    for (long long e = T.cptr[i] + lane; e < T.cptr[i + 1]; e += 64) atomicAdd(&h_[T.cj[e]], 1);
  __syncthreads();
  for (int g = threadIdx.x; g < T.G; g += 256) T.hist[(size_t)blockIdx.x * T.G + g] = h_[g];
}

// per gene: hist[t][g] becomes the entries of the tiles before t, glen[g] the gene's total
__global__ __launch_bounds__(256) void k_pca_scan(PcaListDev T) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= T.G) return;
  long long run = 0;
  for (long long t = 0; t < T.ntiles; t++) {
    const int v = T.hist[(size_t)t * T.G + g];
    T.hist[(size_t)t * T.G + g] = (int)run;
    run += v;
  }
  T.glen[g] = run;
}

__global__ __launch_bounds__(64) void k_pca_place(PcaListDev T) {
  extern __shared__ int h_[];      // [G] the running offset of every gene within this tile's part of its segment
  const int lane = threadIdx.x;
  for (int g = lane; g < T.G; g += 64) h_[g] = T.hist[(size_t)blockIdx.x * T.G + g];
  proj_wave_sync();
  const long long c0 = (long long)blockIdx.x * PCA_TILE, c1 = min(c0 + PCA_TILE, T.N);
  for (long long i = c0; i < c1; i++) {
    for (long long e = T.cptr[i] + lane; e < T.cptr[i + 1]; e += 64) {
      const int j = T.cj[e];
      const int k = h_[j];
      h_[j] = k + 1;
      const long long at = T.gptr[j] + k;
      if (at < T.gptr[j + 1]) { T.tcell[at] = (int)i; T.tw[at] = T.cw[e]; }
    }
    proj_wave_sync();
  }
}

void l_pca_transpose_count(const PcaListDev& T, hipStream_t stream) {
  if (T.ntiles <= 0) return;
  hipLaunchKernelGGL(k_pca_hist, dim3((unsigned)T.ntiles), dim3(256), (size_t)T.G * sizeof(int), stream, T);
  hipLaunchKernelGGL(k_pca_scan, dim3((unsigned)((T.G + 255) / 256)), dim3(256), 0, stream, T);
}
void l_pca_transpose_place(const PcaListDev& T, hipStream_t stream) {
  if (T.ntiles <= 0) return;
  hipLaunchKernelGGL(k_pca_place, dim3((unsigned)T.ntiles), dim3(64), (size_t)T.G * sizeof(int), stream, T);
}

// ---- P = S V ---------------------------------------------------------------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(256) void k_pca_p(PcaApplyDev A) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int zs = 64 * NC;
  for (long long i = (long long)blockIdx.x * PROJ_WAVES + wv; i < A.N; i += (long long)gridDim.x * PROJ_WAVES) {
    const long long lo = A.cptr[i], hi = A.cptr[i + 1];
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.f;
    for (long long p = lo; p < hi; p += 64) {
      const long long e = p + lane;
      const int jj = e < hi ? A.cj[e] : 0;
      const float ww = e < hi ? A.cw[e] : 0.f;
      proj_drain<NC>(A.V, zs, lane, jj, ww, (int)min((long long)64, hi - p), acc);
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
      const int pc = lane + 64 * c;
      const float v = pc < A.k ? (float)((double)acc[c] + A.b[pc]) : 0.f;
      A.Ppad[(size_t)i * zs + pc] = v;
      if (A.out && pc < A.k) A.out[(size_t)i * A.k + pc] = v;
    }
  }
}

// thread c: the sum of column c of P over rows [r PCA_COLSUM_ROWS, (r + 1) PCA_COLSUM_ROWS) one after the other
__global__ __launch_bounds__(128) void k_pca_colsum1(PcaApplyDev A) {
  const int c = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * PCA_COLSUM_ROWS, r1 = min(r0 + PCA_COLSUM_ROWS, A.N);
  double s = 0.0;
  for (long long i = r0; i < r1; i++) s += (double)A.Ppad[(size_t)i * A.zs + c];
  A.colpart[(size_t)blockIdx.x * A.zs + c] = s;
}
__global__ __launch_bounds__(128) void k_pca_colsum2(PcaApplyDev A) {
  const int c = threadIdx.x;
  double s = 0.0;
  for (long long r = 0; r < A.nranges; r++) s += A.colpart[(size_t)r * A.zs + c];
  A.colsum[c] = s;
}

// ---- W = S^T P -------------------------------------------------------------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(256) void k_pca_w(PcaApplyDev A) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int zs = 64 * NC;
  const long long ch = (long long)blockIdx.x * PROJ_WAVES + wv;
  if (ch >= A.nchunks) return;
  const PcaChunk C = A.chunk[ch];
  double sum[NC];
#pragma unroll
  for (int c = 0; c < NC; c++) sum[c] = 0.0;
  for (int q = 0; q < C.len; q += PCA_RUN) {
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.f;
    const int qe = min(q + PCA_RUN, C.len);
    for (int p = q; p < qe; p += 64) {
      const bool in = p + lane < qe;
      const int cell = in ? A.tcell[C.start + p + lane] : 0;
      const float w = in ? A.tw[C.start + p + lane] : 0.f;
      proj_drain<NC>(A.Ppad, zs, lane, cell, w, min(64, qe - p), acc);
    }
#pragma unroll
    for (int c = 0; c < NC; c++) sum[c] += (double)acc[c];
  }
#pragma unroll
  for (int c = 0; c < NC; c++) A.part[(size_t)ch * zs + lane + 64 * c] = sum[c];
}

// thread (g, c): the chunks of gene g in order, then the centring
__global__ __launch_bounds__(256) void k_pca_wred(PcaApplyDev A) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int g = (int)(t / A.zs), c = (int)(t % A.zs);
  if (g >= A.G || c >= A.k) return;
  double s = 0.0;
  for (int ch = A.cstart[g]; ch < A.cstart[g + 1]; ch++) s += A.part[(size_t)ch * A.zs + c];
  A.W[(size_t)g * A.k + c] = s - A.ratio[g] * A.colsum[c];
}

void l_pca_apply(const PcaApplyDev& A, hipStream_t stream) {
  if (A.N <= 0) return;
  const dim3 grid((unsigned)std::min<long long>((A.N + PROJ_WAVES - 1) / PROJ_WAVES, 256 * 8)), block(64 * PROJ_WAVES);
  const dim3 wgrid((unsigned)((A.nchunks + PROJ_WAVES - 1) / PROJ_WAVES));
  if (A.zs == 64) hipLaunchKernelGGL((k_pca_p<1>), grid, block, 0, stream, A);
  else hipLaunchKernelGGL((k_pca_p<2>), grid, block, 0, stream, A);
  hipLaunchKernelGGL(k_pca_colsum1, dim3((unsigned)A.nranges), dim3(A.zs), 0, stream, A);
  hipLaunchKernelGGL(k_pca_colsum2, dim3(1), dim3(A.zs), 0, stream, A);
  if (A.nchunks > 0) {
    if (A.zs == 64) hipLaunchKernelGGL((k_pca_w<1>), wgrid, block, 0, stream, A);
    else hipLaunchKernelGGL((k_pca_w<2>), wgrid, block, 0, stream, A);
  }
  hipLaunchKernelGGL(k_pca_wred, dim3((unsigned)(((long long)A.G * A.zs + 255) / 256)), dim3(256), 0, stream, A);
}

}  // namespace hmx

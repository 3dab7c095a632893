// hmx_ranksum.hip -- gfx950 kernels of the rank sums per group (include/harmony_mi355x_ranksum.h; DESIGN "Rank sums per group").
//
//   k_rank_sweep<F64, FILL>  the kept rows of a count matrix, one wave per cell at a time, a workgroup on a contiguous run of the launch's rows.  The key
//                            of a stored entry is fl32(fl32(x) r), r = proj_rate(scale, T): the entry is positive when stat_row's guards pass and key > 0.
//                            FILL = false counts the positive entries per selected gene in an LDS table (RS_GENES genes, grid.y sweeps the ranges) and adds
//                            every touched gene's count into count[] with one global integer add.  FILL = true builds the same table, reserves every touched
//                            gene's range of its segment with ONE global integer add, then walks the same rows again and places key bits << 32 | group
//                            through the LDS cursors.  Where an entry lands inside its segment depends on the order of arrival; nothing downstream does.
//   k_rank_sort              one workgroup per gene at a time, the genes drawn from a counter.  A list of at most RS_SORT_LDS entries is sorted in LDS by a
//                            bitonic network; a longer one by an LSD radix sort over the four key bytes between the list and the second buffer, RS_CHUNK
//                            entries at a time (per-wave digit tables, a scan over (digit, wave), in-wave ranks from ballots: stable).  Over the sorted list
//                            a forward scan gives every entry the first index of its tie block, a backward scan the index behind its last; both carry across
//                            the chunks.  Every entry adds first + behind + 1 + 2 z into its group's 64-bit LDS cell, the head of a block adds t^3 into a
//                            128-bit register pair.  The tables are stored once per gene into cells that belong to that gene alone.
//   Integer adds and plain stores are the only writes; no floating-point value is summed; no workgroup waits for another one.
#include "hmx_ranksum.h"
#include "hmx_proj_row.h"

namespace hmx {

// one cell, one wave: the positive entries of row i whose output row lies in [g0, g0 + ng) are counted in h (PLACE = false) or placed through it
template <bool F64, bool PLACE>
__device__ __forceinline__ void rank_row(const RankSweepDev& S, long long i, int lane, int g0, int ng, unsigned* h, unsigned& bad) {
  const ProjDev& P = S.C;
  const int grp = S.labels[P.row0 + i];
  if (grp < 0) return;      // (uniform over the wave: the row is not read)
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
    const float key = x * r;
    if (okc && okx && xd > 0 && key > 0.f) {
      const int j = (P.slot ? P.slot[col] : col) - g0;
      if ((unsigned)j < (unsigned)ng) {
        if (!PLACE) atomicAdd(&h[j], 1u);
        else {
          const long long at = S.seg[g0 + j] + (long long)atomicAdd(&h[j], 1u);
          if (at < S.seg[g0 + j + 1] && at - S.base < S.entries)
            S.list[at - S.base] = ((unsigned long long)__float_as_uint(key) << 32) | (unsigned long long)(unsigned)grp;
        }
      }
    }
  }
}

template <bool F64, bool FILL>
__global__ __launch_bounds__(1024) void k_rank_sweep(RankSweepDev S) {
  __shared__ unsigned h[RS_GENES];
  const ProjDev& P = S.C;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int g0 = S.j0 + blockIdx.y * RS_GENES, ng = min(S.j1 - g0, RS_GENES);
  for (int g = threadIdx.x; g < ng; g += 1024) h[g] = 0;
  const long long r0 = P.nrows * blockIdx.x / gridDim.x, r1 = P.nrows * (blockIdx.x + 1) / gridDim.x;      // this workgroup's run of cells
  unsigned bad = 0;
  __syncthreads();
  for (long long i = r0 + wv; i < r1; i += 16) rank_row<F64, false>(S, i, lane, g0, ng, h, bad);
  __syncthreads();
  if (!FILL) {
    for (int g = threadIdx.x; g < ng; g += 1024)
      if (h[g]) atomicAdd(&S.count[g0 + g], (unsigned long long)h[g]);
  } else {
    for (int g = threadIdx.x; g < ng; g += 1024)
      if (h[g]) h[g] = atomicAdd(&S.cursor[g0 + g], h[g]);      // the run's entries of gene g go to [old, old + h[g]) of its segment
    __syncthreads();
    for (long long i = r0 + wv; i < r1; i += 16) rank_row<F64, true>(S, i, lane, g0, ng, h, bad);
  }
  if (bad) atomicOr(P.flag, bad);
}

void l_rank_sweep(const RankSweepDev& S, bool fill, hipStream_t stream) {
  const ProjDev& P = S.C;
  if (P.nrows <= 0 || S.j1 <= S.j0) return;
  const dim3 grid((unsigned)std::min<long long>((P.nrows + 15) / 16, 256), (unsigned)((S.j1 - S.j0 + RS_GENES - 1) / RS_GENES));
  if (fill) {
    if (P.f64) hipLaunchKernelGGL((k_rank_sweep<true, true>), grid, dim3(1024), 0, stream, S);
    else hipLaunchKernelGGL((k_rank_sweep<false, true>), grid, dim3(1024), 0, stream, S);
  } else {
    if (P.f64) hipLaunchKernelGGL((k_rank_sweep<true, false>), grid, dim3(1024), 0, stream, S);
    else hipLaunchKernelGGL((k_rank_sweep<false, false>), grid, dim3(1024), 0, stream, S);
  }
}

// the lanes of the wave that hold the same 8-bit digit as this one (defined in the valid lanes)
__device__ __forceinline__ unsigned long long rank_peers(unsigned d, bool valid) {
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long v = __ballot(valid && bit);
    m &= bit ? v : ~v;
  }
  return m;
}

__global__ __launch_bounds__(1024) void k_rank_sort(RankSortDev R) {
  __shared__ unsigned long long sbuf[RS_SORT_LDS];      // the bitonic sort's list; the radix sort's per-wave digit tables [16][256]
  __shared__ unsigned long long racc[4096];             // per group: the doubled midrank sum of this gene's positive entries
  __shared__ unsigned rcnt[4096];                       // ... and their number
  __shared__ unsigned hist[4][256];                     // the digit counts of the four key bytes
  __shared__ int skip[4];                               // a byte that is the same in every key: its pass moves nothing
  __shared__ int wtot[16];
  __shared__ unsigned long long tlo[16], thi[16];
  __shared__ int draw;
  unsigned (*wh)[256] = (unsigned (*)[256])sbuf;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned long long below = lane ? ~0ull >> (64 - lane) : 0ull;
  const int INF = 0x7fffffff;
  for (int b = tid; b < R.B; b += 1024) { racc[b] = 0; rcnt[b] = 0; }
  for (;;) {
    __syncthreads();      // the tables of the previous gene are stored and cleared, its draw is read
    if (tid == 0) draw = (int)atomicAdd(R.next, 1u);
    __syncthreads();
    const int k = draw;
    if (k < 0 || k >= R.ngenes) break;
    const int j = R.order[k];
    if ((unsigned)j >= (unsigned)R.G) continue;
    const long long a = R.seg[j] - R.base, len64 = R.seg[j + 1] - R.seg[j];      // the segment's length, read once: every bound below
    if (a < 0 || len64 <= 0 || len64 > ((long long)1 << 30) || a + len64 > R.entries) continue;
    const int len = (int)len64;
    const unsigned long long z2 = 2ull * (unsigned long long)(R.Nk - len64) + 1ull;      // 2 z + 1
    unsigned long long* seg = R.list + a;
    const unsigned long long* src;

    if (len <= RS_SORT_LDS) {
      // ---- bitonic network over the next power of two, the pads above every key (+inf is 0x7f800000)
      int m = 64;
      while (m < len) m <<= 1;
      for (int i = tid; i < m; i += 1024) sbuf[i] = i < len ? seg[i] : ~0ull;
      __syncthreads();
      for (int k2 = 2; k2 <= m; k2 <<= 1)
        for (int jj = k2 >> 1; jj > 0; jj >>= 1) {
          for (int i = tid; i < m; i += 1024) {
            const int l = i ^ jj;
            if (l > i) {
              const unsigned long long x = sbuf[i], y = sbuf[l];
              const bool up = (i & k2) == 0;
              if ((x > y) == up) { sbuf[i] = y; sbuf[l] = x; }
            }
          }
          __syncthreads();
        }
      src = sbuf;
    } else {
      // ---- LSD radix sort over the four key bytes.  The digit counts of all four passes from one read: they do not depend on the order
      hist[tid >> 8][tid & 255] = 0;
      if (tid < 4) skip[tid] = 0;
      __syncthreads();
      for (int p0 = wv * 64; p0 < len; p0 += 1024) {
        const int p = p0 + lane;
        const bool valid = p < len;
        const unsigned key = valid ? (unsigned)(seg[p] >> 32) : 0u;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const unsigned d = (key >> (8 * q)) & 255u;
          const unsigned long long m = rank_peers(d, valid);
          if (valid && (m & below) == 0) atomicAdd(&hist[q][d], (unsigned)__popcll(m));
        }
      }
      __syncthreads();
      unsigned long long* in = seg;
      unsigned long long* out = R.other + a;
      for (int q = 0; q < 4; q++) {
        unsigned run = 0;      // thread d < 256: where the next entry of digit d goes
        if (tid < 256) {
          if (hist[q][tid] == (unsigned)len) skip[q] = 1;
          for (int d = 0; d < tid; d++) run += hist[q][d];
        }
        __syncthreads();
        if (skip[q]) continue;
        for (int c0 = 0; c0 < len; c0 += RS_CHUNK) {
          for (int i = tid; i < 16 * 256; i += 1024) ((unsigned*)wh)[i] = 0;
          __syncthreads();
          unsigned long long e[4];
          unsigned loc[4];
#pragma unroll
          for (int s = 0; s < 4; s++) {      // wave wv: entries [c0 + 256 wv, c0 + 256 wv + 256) in order, 64 at a time
            const int p = c0 + wv * 256 + s * 64 + lane;
            const bool valid = p < len;
            e[s] = valid ? in[p] : 0ull;
            const unsigned d = (unsigned)(e[s] >> (32 + 8 * q)) & 255u;
            const unsigned long long m = rank_peers(d, valid);
            const unsigned old = valid ? wh[wv][d] : 0u;
            proj_wave_sync();
            if (valid && (m & below) == 0) wh[wv][d] = old + (unsigned)__popcll(m);
            proj_wave_sync();
            loc[s] = old + (unsigned)__popcll(m & below);      // the entry's rank among the wave's entries of its digit in this chunk
          }
          __syncthreads();
          if (tid < 256) {      // (digit, wave) in order: the digit's running offset, then the waves before
            unsigned acc = run;
            for (int w = 0; w < 16; w++) { const unsigned t = wh[w][tid]; wh[w][tid] = acc; acc += t; }
            run = acc;
          }
          __syncthreads();
#pragma unroll
          for (int s = 0; s < 4; s++) {
            const int p = c0 + wv * 256 + s * 64 + lane;
            if (p < len) {
              const unsigned d = (unsigned)(e[s] >> (32 + 8 * q)) & 255u;
              const unsigned at = wh[wv][d] + loc[s];
              if (at < (unsigned)len) out[at] = e[s];
            }
          }
          __syncthreads();
        }
        unsigned long long* t = in; in = out; out = t;      // (the barrier above: the pass's stores are visible to the whole workgroup)
      }
      src = in;
    }

    // ---- forward: the first index of every entry's tie block (the last head at or before it), carried across the chunks
    int carry = -1;
    for (int c0 = 0; c0 < len; c0 += RS_CHUNK) {
      const int p0 = c0 + 4 * tid;
      unsigned long long w[4];
      int f[4];
      int last = -1;
      unsigned pk = (p0 > 0 && p0 < len) ? (unsigned)(src[p0 - 1] >> 32) : 0u;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int p = p0 + q;
        const bool valid = p < len;
        w[q] = valid ? src[p] : 0ull;
        const unsigned key = (unsigned)(w[q] >> 32);
        if (valid && (p == 0 || key != pk)) last = p;
        f[q] = last;
        pk = key;
      }
      int inc = last;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o, 64); if (lane >= o) inc = max(inc, v); }
      int ex = __shfl_up(inc, 1, 64);
      if (lane == 0) ex = -1;
      if (lane == 63) wtot[wv] = inc;
      __syncthreads();
      int tot = carry;
      for (int w2 = 0; w2 < 16; w2++) { if (w2 == wv) ex = max(ex, tot); tot = max(tot, wtot[w2]); }
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const unsigned grp = (unsigned)w[q];
        if (p0 + q < len && grp < (unsigned)R.B) {
          atomicAdd(&racc[grp], (unsigned long long)max(f[q], ex) + z2);
          atomicAdd(&rcnt[grp], 1u);
        }
      }
      carry = tot;
      __syncthreads();
    }
    // ---- backward: the index behind every entry's tie block (the next head after it, or len); a head adds t^3
    unsigned long long t3lo = 0, t3hi = 0;
    carry = len;
    for (int c0 = ((len - 1) / RS_CHUNK) * RS_CHUNK; c0 >= 0; c0 -= RS_CHUNK) {
      const int p0 = c0 + 4 * tid;
      unsigned key[4];
      unsigned grp[4];
      int l[4];
      const unsigned pk = (p0 > 0 && p0 < len) ? (unsigned)(src[p0 - 1] >> 32) : 0u;
      const unsigned nk = p0 + 4 < len ? (unsigned)(src[p0 + 4] >> 32) : 0u;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const unsigned long long w = p0 + q < len ? src[p0 + q] : 0ull;
        key[q] = (unsigned)(w >> 32);
        grp[q] = (unsigned)w;
      }
      int nxt = INF;
#pragma unroll
      for (int q = 3; q >= 0; q--) {
        const int p = p0 + q;
        if (p < len && (p + 1 == len || (q < 3 ? key[q + 1] : nk) != key[q])) nxt = p + 1;
        l[q] = nxt;
      }
      int inc = nxt;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_down(inc, o, 64); if (lane + o < 64) inc = min(inc, v); }
      int ex = __shfl_down(inc, 1, 64);
      if (lane == 63) ex = INF;
      if (lane == 0) wtot[wv] = inc;
      __syncthreads();
      int tot = carry;
      for (int w2 = 15; w2 >= 0; w2--) { if (w2 == wv) ex = min(ex, tot); tot = min(tot, wtot[w2]); }
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int p = p0 + q;
        if (p < len) {
          const int behind = min(l[q], ex);
          if (grp[q] < (unsigned)R.B) atomicAdd(&racc[grp[q]], (unsigned long long)behind);
          if (p == 0 || key[q] != (q ? key[q - 1] : pk)) {
            const unsigned long long t = (unsigned long long)(behind - p), t2 = t * t;
            const unsigned long long s = t3lo + t2 * t;
            t3hi += __umul64hi(t2, t) + (s < t3lo ? 1ull : 0ull);
            t3lo = s;
          }
        }
      }
      carry = tot;
      __syncthreads();
    }
    // ---- the 128-bit sums: a butterfly over the wave, then the sixteen waves one after the other
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const unsigned long long olo = __shfl_xor(t3lo, m, 64), ohi = __shfl_xor(t3hi, m, 64);
      const unsigned long long s = t3lo + olo;
      t3hi += ohi + (s < t3lo ? 1ull : 0ull);
      t3lo = s;
    }
    if (lane == 0) { tlo[wv] = t3lo; thi[wv] = t3hi; }
    __syncthreads();
    if (tid == 0) {
      unsigned long long lo = 0, hi = 0;
      for (int w2 = 0; w2 < 16; w2++) { const unsigned long long s = lo + tlo[w2]; hi += thi[w2] + (s < lo ? 1ull : 0ull); lo = s; }
      R.tie3[2 * (size_t)j] = lo; R.tie3[2 * (size_t)j + 1] = hi;
    }
    for (int b = tid; b < R.B; b += 1024) {      // the gene's cells of the outputs: plain stores
      R.rank2[(size_t)b * R.G + j] = racc[b]; R.npos[(size_t)b * R.G + j] = rcnt[b];
      racc[b] = 0; rcnt[b] = 0;
    }
  }
}

void l_rank_sort(const RankSortDev& R, hipStream_t stream) {
  if (R.ngenes <= 0) return;
  hipLaunchKernelGGL(k_rank_sort, dim3((unsigned)std::min(R.ngenes, 256)), dim3(1024), 0, stream, R);
}

}  // namespace hmx

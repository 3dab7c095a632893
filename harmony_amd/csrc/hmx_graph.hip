// hmx_graph.hip -- gfx950 kernels of the neighbour graph (include/harmony_mi355x_graph.h; DESIGN "The neighbour graph"): UMAP's fuzzy simplicial
// set of a neighbour list with self excluded, as a CSR matrix, and the connected components of a symmetric pattern.
//
//   k_graph_distsum / 2   the sum of all valid distances in fp64: workgroup partials in a fixed shape, then one workgroup;
//   k_smooth_knn          one wave per cell, lane l holds neighbours l and l + 64 (k_lisi's layout): rho, the search of sigma, the row's memberships
//                         w; it also counts the in-degrees (integer adds);
//   k_scan_*              exclusive scan of 32-bit counts into 64-bit offsets: workgroup sums, one workgroup over the sums, the final pass;
//   k_graph_place         the transposed lists (who lists me): entry source * m + slot through the row's integer cursor;
//   k_graph_sort_short    one wave per transposed row of <= 128 entries: rank sort in registers.  Longer rows are noted for
//   k_graph_sort_long     one workgroup per long row: 128-entry chunks by the same rank sort, then merge passes between two buffers;
//   k_graph_union<WRITE>  one wave per row: the out-list sorted by index in LDS, merged with the sorted in-list by ranks (binary searches);
//                         WRITE = false counts the row's length, WRITE = true writes indices / weights behind the scanned lengths;
//   k_snn_indegree / rowweight / short<WRITE> / long<WRITE>   Seurat's SNN graph (include/harmony_mi355x_snn.h; DESIGN "Seurat's SNN graph") over the
//                         same transposed lists: in-degrees alone, candidates per row, one wave sorting a row's candidates in LDS, one workgroup
//                         walking a long row's index range in dense windows of 8-bit counters;
//   k_cc_check / init / hook / jump   components: the pattern's checks, comp[i] = i, the hooks (integer atomicMin), bounded pointer jumping.
// Integer atomics only; every floating-point sum has a fixed order; after the segment sort nothing depends on the order of placement.
#include "hmx_graph.h"

namespace hmx {
typedef unsigned long long u64;

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m, 64));
  return v;
}
// the keys of a wave, position p in lane p & 63, slot p >> 6; the first n <= 128 positions are real and distinct: the rank of the lane's two keys
__device__ __forceinline__ void wave_ranks(u64 e0, u64 e1, int n, int& r0, int& r1) {
  r0 = r1 = 0;
  for (int j = 0; j < n; j++) {
    const u64 key = __shfl(j < 64 ? e0 : e1, j & 63, 64);
    r0 += key < e0 ? 1 : 0;
    r1 += key < e1 ? 1 : 0;
  }
}
// the n <= 128 keys at `seg`, sorted in place by one wave
__device__ __forceinline__ void wave_sort_keys(u64* seg, int n, int l) {
  const u64 e0 = l < n ? seg[l] : ~0ull, e1 = l + 64 < n ? seg[l + 64] : ~0ull;
  int r0, r1;
  wave_ranks(e0, e1, n, r0, r1);
  if (l < n) seg[r0] = e0;
  if (l + 64 < n) seg[r1] = e1;
}
// number of keys below `key` in the ascending keys[0 .. n)
__device__ __forceinline__ long long lower_bound_keys(const u64* keys, long long n, u64 key) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int lower_bound_int(const int* v, int n, int key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the sum of a workgroup's 256 values in a fixed tree, in thread 0
__device__ __forceinline__ double block_sum_256(double v, double* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (t < s) sh[t] += sh[t + s];
    __syncthreads();
  }
  return sh[0];
}

// ---- smooth kNN distances -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_graph_distsum(GraphDev G) {
  __shared__ double sh[256];
  const long long cnt = G.N * G.m, step = (long long)gridDim.x * 256;
  double s = 0.0;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < cnt; p += step)
    if (G.idx[p] >= 0) s += (double)G.dist[p];
  const double tot = block_sum_256(s, sh);
  if (threadIdx.x == 0) G.part[blockIdx.x] = tot;
}
__global__ __launch_bounds__(256) void k_graph_distsum2(GraphDev G) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int p = threadIdx.x; p < G.nparts; p += 256) s += G.part[p];
  const double tot = block_sum_256(s, sh);
  if (threadIdx.x == 0) G.total[0] = tot;
}

__global__ __launch_bounds__(256) void k_smooth_knn(GraphDev G) {
  const int l = threadIdx.x & 63, m = G.m;
  const long long cell = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (cell >= G.N) return;
  const bool h0 = l < m, h1 = l + 64 < m;
  const size_t at = (size_t)cell * m + l;
  const int i0 = h0 ? G.idx[at] : -1, i1 = h1 ? G.idx[at + 64] : -1;
  const bool v0 = i0 >= 0, v1 = i1 >= 0;
  const double d0 = v0 ? (double)G.dist[at] : 0.0, d1 = v1 ? (double)G.dist[at + 64] : 0.0;
  if (v0) atomicAdd(G.deg + i0, 1u);
  if (v1) atomicAdd(G.deg + i1, 1u);
  double rho = 0.0, sigma = 0.0;
  if (__ballot(v0 || v1) != 0) {
    const bool p0 = v0 && d0 > 0.0, p1 = v1 && d1 > 0.0;
    if (__ballot(p0 || p1) != 0) rho = wave_min(fmin(p0 ? d0 : INFINITY, p1 ? d1 : INFINITY));
    const double r0 = d0 - rho, r1 = d1 - rho, target = log2((double)(m + 1));
    double lo = 0.0, hi = INFINITY, mid = 1.0;
    for (int step = 0; step < 64; step++) {
      const double t0 = v0 ? (r0 > 0.0 ? exp(-r0 / mid) : 1.0) : 0.0, t1 = v1 ? (r1 > 0.0 ? exp(-r1 / mid) : 1.0) : 0.0;
      const double psum = wave_sum(t0 + t1);
      if (fabs(psum - target) < 1e-5) break;
      if (psum > target) { hi = mid; mid = (lo + hi) / 2; }
      else { lo = mid; mid = isinf(hi) ? mid * 2 : (lo + hi) / 2; }
    }
    const double floor_at = rho > 0.0 ? wave_sum(d0 + d1) / (double)(m + 1) : G.total[0] / ((double)G.N * (double)(m + 1));
    sigma = fmax(mid, 1e-3 * floor_at);
    if (v0) G.w[at] = (r0 <= 0.0 || sigma == 0.0) ? 1.0 : exp(-r0 / sigma);
    if (v1) G.w[at + 64] = (r1 <= 0.0 || sigma == 0.0) ? 1.0 : exp(-r1 / sigma);
  }
  if (l == 0) { G.rho[cell] = rho; G.sigma[cell] = sigma; }
}

// ---- exclusive scan of counts -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_scan_sums(const unsigned* __restrict__ cnt, long long n, long long* __restrict__ bsum) {
  __shared__ long long sh[256];
  const int t = threadIdx.x;
  const long long base = (long long)blockIdx.x * GR_SCAN_CHUNK + 8 * t;
  long long s = 0;
  for (int e = 0; e < 8; e++) if (base + e < n) s += cnt[base + e];
  sh[t] = s;
  __syncthreads();
  for (int k = 128; k >= 1; k >>= 1) {
    if (t < k) sh[t] += sh[t + k];
    __syncthreads();
  }
  if (t == 0) bsum[blockIdx.x] = sh[0];
}
// the workgroup's 1024 values -> their exclusive prefix (Hillis-Steele in LDS); *total: their sum
__device__ __forceinline__ long long block_exclusive_1024(long long v, long long* sh, long long* total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int k = 1; k < 1024; k <<= 1) {
    const long long add = t >= k ? sh[t - k] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const long long incl = sh[t];
  *total = sh[1023];
  __syncthreads();
  return incl - v;
}
__global__ __launch_bounds__(1024) void k_scan_top(long long* bsum, long long nb) {
  __shared__ long long sh[1024];
  long long carry = 0;
  for (long long base = 0; base < nb; base += 1024) {
    const long long i = base + threadIdx.x;
    const long long v = i < nb ? bsum[i] : 0;
    long long total;
    const long long ex = block_exclusive_1024(v, sh, &total);
    if (i < nb) bsum[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) bsum[nb] = carry;
}
__global__ __launch_bounds__(256) void k_scan_final(const unsigned* __restrict__ cnt, long long n, const long long* __restrict__ bsum, long long nb,
                                                    long long* __restrict__ off) {
  __shared__ long long sh[256];
  const int t = threadIdx.x;
  const long long base = (long long)blockIdx.x * GR_SCAN_CHUNK + 8 * t;
  unsigned c[8];
  long long s = 0;
  for (int e = 0; e < 8; e++) { c[e] = base + e < n ? cnt[base + e] : 0u; s += c[e]; }
  sh[t] = s;
  __syncthreads();
  for (int k = 1; k < 256; k <<= 1) {
    const long long add = t >= k ? sh[t - k] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  long long run = bsum[blockIdx.x] + sh[t] - s;
  for (int e = 0; e < 8; e++) {
    if (base + e < n) off[base + e] = run;
    run += c[e];
  }
  if (blockIdx.x == 0 && t == 0) off[n] = bsum[nb];
}

// ---- the transposed lists -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_graph_place(GraphDev G) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= G.N * G.m) return;
  const int j = G.idx[p];
  if (j < 0) return;
  const unsigned left = atomicSub(G.deg + j, 1u);      // (the in-degree counted by k_smooth_knn: 1 .. deg[j], every value once)
  G.tkey[G.toff[j] + (long long)left - 1] = (u64)p;
}

__global__ __launch_bounds__(256) void k_graph_sort_short(GraphDev G) {
  const int l = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= G.N) return;
  const long long b = G.toff[row], n = G.toff[row + 1] - b;
  if (n > GR_WAVE_KEYS) {
    if (l == 0) G.longrows[atomicAdd(G.nlong, 1u)] = (int)row;
    return;
  }
  if (n > 1) wave_sort_keys(G.tkey + b, (int)n, l);
}

__global__ __launch_bounds__(1024) void k_graph_sort_long(GraphDev G) {
  const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
  const unsigned nlong = *G.nlong;
  for (unsigned r = blockIdx.x; r < nlong; r += gridDim.x) {
    const long long row = G.longrows[r], b = G.toff[row], n = G.toff[row + 1] - b;
    u64* src = G.tkey + b;
    u64* dst = G.tother + b;
    for (long long c = wv; c * GR_WAVE_KEYS < n; c += 16)
      wave_sort_keys(src + c * GR_WAVE_KEYS, (int)min((long long)GR_WAVE_KEYS, n - c * GR_WAVE_KEYS), l);
    __syncthreads();
    // merge passes: runs of `width` sorted entries, two neighbours at a time; an entry lands at its place in its own run plus its rank in the other
    for (long long width = GR_WAVE_KEYS; width < n; width <<= 1) {
      for (long long t = tid; t < n; t += 1024) {
        const u64 key = src[t];
        const long long run = t / width, a0 = run * width, b0 = (run ^ 1) * width;
        const long long cnt = b0 < n ? lower_bound_keys(src + b0, min(width, n - b0), key) : 0;
        dst[min(a0, b0) + (t - a0) + cnt] = key;
      }
      __syncthreads();
      u64* x = src; src = dst; dst = x;
    }
    if (src != G.tkey + b)
      for (long long t = tid; t < n; t += 1024) dst[t] = src[t];
    __syncthreads();
  }
}

// ---- the union of the out-list and the in-list of a row ---------------------------------------------------------------------------------------
template <bool WRITE>
__global__ __launch_bounds__(256) void k_graph_union(GraphDev G) {
  __shared__ int sj[4][GR_WAVE_KEYS];
  __shared__ double sa[4][GR_WAVE_KEYS];
  __shared__ int smp[4][GR_WAVE_KEYS + 1];
  const int l = threadIdx.x & 63, wv = threadIdx.x >> 6, m = G.m;
  const long long i = (long long)blockIdx.x * 4 + wv;
  const bool active = i < G.N;
  const bool h0 = active && l < m, h1 = active && l + 64 < m;
  const size_t at = (size_t)(active ? i : 0) * m + l;
  const int j0 = h0 ? G.idx[at] : -1, j1 = h1 ? G.idx[at + 64] : -1;
  const double a0 = j0 >= 0 ? G.w[at] : 0.0, a1 = j1 >= 0 ? G.w[at + 64] : 0.0;
  // the out-list sorted by index (it arrives sorted by distance); unfilled slots go behind the real ones
  const u64 e0 = ((u64)(j0 >= 0 ? (unsigned)j0 : 0xffffffffu) << 32) | (unsigned)l;
  const u64 e1 = ((u64)(j1 >= 0 ? (unsigned)j1 : 0xffffffffu) << 32) | (unsigned)(l + 64);
  int r0, r1;
  wave_ranks(e0, e1, m, r0, r1);
  const int nout = __popcll(__ballot(j0 >= 0)) + __popcll(__ballot(j1 >= 0));
  if (h0) { sj[wv][r0] = j0; sa[wv][r0] = a0; }
  if (h1) { sj[wv][r1] = j1; sa[wv][r1] = a1; }
  __syncthreads();
  const long long tb = active ? G.toff[i] : 0, nin = active ? G.toff[i + 1] - tb : 0;
  const u64* keys = G.tkey + tb;
  // per out-entry q (sorted position): lb = in-entries of a smaller source; mutual: the in-list holds the entry's own index
  long long lb[2];
  bool mut[2];
  u64 mb[2];
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const int q = l + 64 * s;
    const bool have = q < nout;
    const int j = have ? sj[wv][q] : 0;
    lb[s] = have ? lower_bound_keys(keys, nin, (u64)j * (u64)m) : 0;
    mut[s] = have && lb[s] < nin && keys[lb[s]] < ((u64)j + 1) * (u64)m;
    if (have && q + 1 < nout && sj[wv][q + 1] == j) atomicOr(G.flag, GR_FLAG_DUP);
    mb[s] = __ballot(mut[s]);
  }
  const u64 below = (1ull << l) - 1;
  const int mp[2] = {(int)__popcll(mb[0] & below), (int)(__popcll(mb[0]) + __popcll(mb[1] & below))};      // mutual out-entries ahead of q
  const int nmut = __popcll(mb[0]) + __popcll(mb[1]);
  if (!WRITE) {
    if (active && l == 0) G.len[i] = (unsigned)((long long)nout + nin - nmut);
    return;
  }
  const long long ob = active ? G.indptr[i] : 0, rowlen = active ? G.indptr[i + 1] - ob : 0;
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const int q = l + 64 * s;
    if (q < nout) {
      smp[wv][q] = mp[s];
      const long long pos = q + lb[s] - mp[s];
      const double a = sa[wv][q], b = mut[s] ? G.w[keys[lb[s]]] : 0.0;
      if (pos < rowlen) { G.indices[ob + pos] = sj[wv][q]; G.weights[ob + pos] = (float)(a + b - a * b); }
    }
  }
  if (l == 0) smp[wv][nout] = nmut;
  __syncthreads();
  // the in-entries no out-entry mirrors: behind the out-entries of a smaller index and the earlier in-entries that are not mutual
  for (long long t = l; t < nin; t += 64) {
    const u64 p = keys[t];
    const int src = (int)(p / (u64)m);
    const int lo = lower_bound_int(sj[wv], nout, src);
    if (lo < nout && sj[wv][lo] == src) continue;
    const long long pos = lo + t - smp[wv][lo];
    if (pos < rowlen) { G.indices[ob + pos] = src; G.weights[ob + pos] = (float)G.w[p]; }
  }
}

// ---- Seurat's shared-nearest-neighbour graph -----------------------------------------------------------------------------------------------------
// s_il = |N+(i) & N+(l)| is the multiplicity of l among the candidates of row i: for every j in N+(i), the sources that list j and j itself.
// Integers throughout: the weight of s is looked up in S.jtab.
__global__ __launch_bounds__(256) void k_snn_indegree(GraphDev G) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= G.N * G.m) return;
  const int j = G.idx[p];
  if (j >= 0 && j < G.N) atomicAdd(G.deg + j, 1u);
}
__device__ __forceinline__ int snn_source(u64 key, int m) {
  return (key >> 32) == 0 ? (int)((unsigned)key / (unsigned)m) : (int)(key / (u64)m);
}
// entry q of N+(i): the list's slot q, then the cell itself; -1: an unfilled slot
__device__ __forceinline__ int snn_entry(const SnnDev& S, long long i, int q) {
  return q < S.m ? S.idx[(size_t)i * S.m + q] : q == S.m ? (int)i : -1;
}
__device__ __forceinline__ int wave_inclusive(int v, int l) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (l >= d) v += o;
  }
  return v;
}

__global__ __launch_bounds__(256) void k_snn_rowweight(SnnDev S) {
  const int l = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= S.N) return;
  long long c = 0;
  for (int q = l; q <= S.m; q += 64) {
    const int j = snn_entry(S, i, q);
    if (j >= 0) c += S.toff[j + 1] - S.toff[j] + 1;
  }
  c = wave_sum(c);
  if (l == 0) {
    S.cand[i] = (unsigned)min(c, 0xffffffffll);
    if (c > SNN_SHORT_CAP) {
      const unsigned at = atomicAdd(S.nlong, 1u);
      if ((long long)at < S.N) S.longrows[at] = (int)i;
    }
  }
}

// the bitonic sort of P = 128 IT keys in LDS by one wave (IT = 0: 64 keys, half the lanes).  IT is a template argument so that a step's
// compare-exchanges unroll: a lane issues all its reads before its first write instead of one dependent read-write pair after the other
template <int IT>
__device__ __forceinline__ void snn_bitonic(unsigned* sc, int l) {
  constexpr int PER = IT > 0 ? IT : 1, P = IT > 0 ? 128 * IT : 64;
  const bool on = IT > 0 || l < 32;
  for (int k2 = 2; k2 <= P; k2 <<= 1)
    for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
      int a[PER];
      unsigned x[PER], y[PER];
#pragma unroll
      for (int u = 0; u < PER; u++) {
        const int t = l + 64 * u;
        a[u] = ((t & ~(j2 - 1)) << 1) | (t & (j2 - 1));
        x[u] = on ? sc[a[u]] : 0u;
        y[u] = on ? sc[a[u] | j2] : 0u;
      }
#pragma unroll
      for (int u = 0; u < PER; u++)
        if (on && (x[u] > y[u]) == ((a[u] & k2) == 0)) { sc[a[u]] = y[u]; sc[a[u] | j2] = x[u]; }
      __syncthreads();
    }
}

// one wave per row of at most SNN_SHORT_CAP candidates: gathered into LDS, sorted (bitonic), run lengths, the survivors placed by ballot prefixes
template <bool WRITE>
__global__ __launch_bounds__(64) void k_snn_short(SnnDev S) {
  constexpr int SLOTS = 192;                             // three entries of N+(i) per lane
  __shared__ unsigned sc[SNN_SHORT_CAP];
  __shared__ long long eb[SLOTS];
  __shared__ int en[SLOTS], eo[SLOTS], ej[SLOTS];
  const int l = threadIdx.x, m = S.m;
  const long long i = blockIdx.x;
  if (i >= S.N || S.cand[i] > (unsigned)SNN_SHORT_CAP) return;      // (the whole workgroup: a long row)
  int run = 0;
#pragma unroll
  for (int s = 0; s < 3; s++) {
    const int q = l + 64 * s;
    const int j = snn_entry(S, i, q);
    long long b = 0;
    int cnt = 0;
    if (j >= 0) { b = S.toff[j]; cnt = (int)(S.toff[j + 1] - b) + 1; }
    const int inc = wave_inclusive(cnt, l);
    eb[q] = b; en[q] = cnt; eo[q] = run + inc - cnt; ej[q] = j;
    run += __shfl(inc, 63, 64);
  }
  const int n = min(run, SNN_SHORT_CAP);
  __syncthreads();
  for (int q = 0; q <= m; q++) {
    const int cnt = en[q], o = eo[q];
    const u64* keys = S.tkey + eb[q];
    for (int t = l; t < cnt; t += 64) {
      const unsigned v = t < cnt - 1 ? (unsigned)snn_source(keys[t], m) : (unsigned)ej[q];
      if (o + t < SNN_SHORT_CAP) sc[o + t] = v;
    }
  }
  int P = 64;
  while (P < n) P <<= 1;                                 // (n <= SNN_SHORT_CAP, a power of two)
  for (int t = n + l; t < P; t += 64) sc[t] = 0xffffffffu;
  __syncthreads();
  static_assert(SNN_SHORT_CAP == 2048, "the sort's variants end at 2048 keys");
  switch (P) {                                           // (the same branch in every lane)
    case 64: snn_bitonic<0>(sc, l); break;
    case 128: snn_bitonic<1>(sc, l); break;
    case 256: snn_bitonic<2>(sc, l); break;
    case 512: snn_bitonic<4>(sc, l); break;
    case 1024: snn_bitonic<8>(sc, l); break;
    default: snn_bitonic<16>(sc, l); break;
  }
  const long long ob = WRITE ? S.indptr[i] : 0, rowlen = WRITE ? S.indptr[i + 1] - ob : 0;
  int base = 0;
  for (int c = 0; c < n; c += 64) {
    const int p = c + l;
    bool keep = false;
    unsigned key = 0;
    int s = 0;
    if (p < n) {
      key = sc[p];
      if (p == 0 || sc[p - 1] != key) {                  // the head of a run: its length is the shared count
        int lo = p + 1, hi = n;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (sc[mid] <= key) lo = mid + 1; else hi = mid;
        }
        s = lo - p;
        keep = s >= S.s_min;
      }
    }
    const u64 bal = __ballot(keep);
    const long long pos = base + __popcll(bal & ((1ull << l) - 1));
    if (WRITE && keep && pos < rowlen) { S.indices[ob + pos] = (int)key; S.weights[ob + pos] = S.jtab[min(s, m + 1)]; }
    base += __popcll(bal);
  }
  if (!WRITE && l == 0) S.len[i] = (unsigned)base;
}

// one workgroup per long row: the index range in windows of SNN_WINDOW cells, an 8-bit counter per cell (s <= 129), swept in order
template <bool WRITE>
__global__ __launch_bounds__(256) void k_snn_long(SnnDev S) {
  __shared__ unsigned cnt[SNN_WINDOW / 4];
  __shared__ long long eb[SNN_MAX_K];
  __shared__ int en[SNN_MAX_K], ej[SNN_MAX_K];
  __shared__ int wtot[4];
  __shared__ int any;
  const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6, m = S.m;
  const unsigned nlong = (unsigned)min((long long)*S.nlong, S.N);
  for (unsigned r = blockIdx.x; r < nlong; r += gridDim.x) {
    const long long i = S.longrows[r];
    for (int q = tid; q <= m; q += 256) {
      const int j = snn_entry(S, i, q);
      eb[q] = j >= 0 ? S.toff[j] : 0;
      en[q] = j >= 0 ? (int)(S.toff[j + 1] - S.toff[j]) : 0;
      ej[q] = j;
    }
    const long long ob = WRITE ? S.indptr[i] : 0, rowlen = WRITE ? S.indptr[i + 1] - ob : 0;
    long long base = 0;
    for (long long w0 = 0; w0 < S.N; w0 += SNN_WINDOW) {
      const long long w1 = min(w0 + SNN_WINDOW, S.N);
      for (int t = tid; t < SNN_WINDOW / 4; t += 256) cnt[t] = 0u;
      if (tid == 0) any = 0;
      __syncthreads();
      for (int q = wv; q <= m; q += 4) {
        const int j = ej[q];
        if (j < 0) continue;
        const u64* keys = S.tkey + eb[q];
        const long long lo = lower_bound_keys(keys, en[q], (u64)w0 * (u64)m), hi = lower_bound_keys(keys, en[q], (u64)w1 * (u64)m);
        for (long long t = lo + l; t < hi; t += 64) {
          const unsigned off = (unsigned)((long long)snn_source(keys[t], m) - w0);
          if (off < (unsigned)SNN_WINDOW) atomicAdd(&cnt[off >> 2], 1u << (8 * (off & 3)));
        }
        const bool own = j >= w0 && j < w1;
        if (l == 0 && own) { const unsigned off = (unsigned)(j - w0); atomicAdd(&cnt[off >> 2], 1u << (8 * (off & 3))); }
        if (l == 0 && (own || hi > lo)) atomicOr(&any, 1);
      }
      __syncthreads();
      if (any) {                                         // (the same value in every thread: written before the barrier)
        for (int c = 0; c < SNN_WINDOW; c += 1024) {
          const unsigned word = cnt[(c >> 2) + tid];
          const long long cell0 = w0 + c + 4 * tid;
          int kept = 0;
#pragma unroll
          for (int b = 0; b < 4; b++) kept += ((int)((word >> (8 * b)) & 255u) >= S.s_min && cell0 + b < S.N) ? 1 : 0;
          const int inc = wave_inclusive(kept, l);
          if (l == 63) wtot[wv] = inc;
          __syncthreads();
          int before = 0, total = 0;
#pragma unroll
          for (int w = 0; w < 4; w++) { before += w < wv ? wtot[w] : 0; total += wtot[w]; }
          if (WRITE) {
            long long pos = base + before + inc - kept;
#pragma unroll
            for (int b = 0; b < 4; b++) {
              const int s = (int)((word >> (8 * b)) & 255u);
              if (s >= S.s_min && cell0 + b < S.N) {
                if (pos < rowlen) { S.indices[ob + pos] = (int)(cell0 + b); S.weights[ob + pos] = S.jtab[min(s, m + 1)]; }
                pos++;
              }
            }
          }
          base += total;
          __syncthreads();
        }
      }
      __syncthreads();
    }
    if (!WRITE && tid == 0) S.len[i] = (unsigned)base;
    __syncthreads();
  }
}

// ---- connected components ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cc_check(CcDev C) {
  const int l = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= C.N) return;
  const long long b = C.indptr[i], e1 = C.indptr[i + 1];
  int bad = 0;
  for (long long e = b + l; e < e1; e += 64) {
    const int j = C.indices[e];
    if (j < 0 || j >= C.N) { bad |= GR_FLAG_RANGE; continue; }
    if (e > b && C.indices[e - 1] >= j) bad |= GR_FLAG_ORDER;
    const long long jb = C.indptr[j], jn = C.indptr[j + 1] - jb;
    const int lo = lower_bound_int(C.indices + jb, (int)jn, (int)i);      // (a row holds fewer than 2^31 entries: its indices are distinct when it passes)
    if (lo >= jn || C.indices[jb + lo] != (int)i) bad |= GR_FLAG_ASYM;
  }
  if (bad) atomicOr(C.flag, bad);
}
__global__ __launch_bounds__(256) void k_cc_init(CcDev C) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < C.N) C.comp[i] = (int)i;
}
// every kept edge (each once, from its larger end): the larger root's entry is lowered to the smaller root
__global__ __launch_bounds__(256) void k_cc_hook(CcDev C) {
  const int l = threadIdx.x & 63;
  const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= C.N) return;
  const int lu = C.labels ? C.labels[u] : 0;
  if (lu < 0) return;
  const long long b = C.indptr[u], e1 = C.indptr[u + 1];
  bool changed = false;
  for (long long e = b + l; e < e1; e += 64) {
    const int v = C.indices[e];
    if (v >= u) break;                                   // (rows ascend: nothing smaller follows in this lane's stride)
    if (C.labels && C.labels[v] != lu) continue;
    const int cu = C.comp[u], cv = C.comp[v];
    if (cu == cv) continue;
    const int hi = max(cu, cv), lo = min(cu, cv);
    if (atomicMin(C.comp + hi, lo) > lo) changed = true;
  }
  if (changed) atomicOr(C.flag, GR_FLAG_CHANGED);
}
// up to GR_CC_HOPS parents up; every value read is an ancestor, so a tree's depth shrinks by that factor per launch
__global__ __launch_bounds__(256) void k_cc_jump(CcDev C, int check) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= C.N) return;
  int c = C.comp[i];
  for (int h = 0; h < GR_CC_HOPS; h++) {
    const int p = C.comp[c];
    if (p == c) break;
    c = p;
  }
  C.comp[i] = c;
  if (check && C.comp[c] != c) atomicOr(C.flag, GR_FLAG_DEEP);
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------------
static dim3 waves4(long long n) { return dim3((unsigned)((n + 3) / 4)); }
static dim3 threads256(long long n) { return dim3((unsigned)((n + 255) / 256)); }

long long graph_sum_parts(long long count) { return std::max<long long>(1, std::min<long long>(GR_SUM_PARTS, (count + 2047) / 2048)); }
void l_graph_distsum(const Launch& L, const GraphDev& G) {
  hipLaunchKernelGGL(k_graph_distsum, dim3((unsigned)G.nparts), dim3(256), 0, L.stream, G);
  hipLaunchKernelGGL(k_graph_distsum2, dim3(1), dim3(256), 0, L.stream, G);
}
void l_graph_smooth(const Launch& L, const GraphDev& G) { hipLaunchKernelGGL(k_smooth_knn, waves4(G.N), dim3(256), 0, L.stream, G); }
void l_graph_scan(const Launch& L, const unsigned* cnt, long long n, long long* off, long long* bsum) {
  const long long nb = (n + GR_SCAN_CHUNK - 1) / GR_SCAN_CHUNK;
  hipLaunchKernelGGL(k_scan_sums, dim3((unsigned)nb), dim3(256), 0, L.stream, cnt, n, bsum);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, L.stream, bsum, nb);
  hipLaunchKernelGGL(k_scan_final, dim3((unsigned)nb), dim3(256), 0, L.stream, cnt, n, (const long long*)bsum, nb, off);
}
void l_graph_place(const Launch& L, const GraphDev& G) { hipLaunchKernelGGL(k_graph_place, threads256(G.N * G.m), dim3(256), 0, L.stream, G); }
void l_graph_sort(const Launch& L, const GraphDev& G) {
  hipLaunchKernelGGL(k_graph_sort_short, waves4(G.N), dim3(256), 0, L.stream, G);
  hipLaunchKernelGGL(k_graph_sort_long, dim3(GR_LONG_WGS), dim3(1024), 0, L.stream, G);
}
void l_graph_union(const Launch& L, const GraphDev& G, bool write) {
  if (write) hipLaunchKernelGGL(k_graph_union<true>, waves4(G.N), dim3(256), 0, L.stream, G);
  else hipLaunchKernelGGL(k_graph_union<false>, waves4(G.N), dim3(256), 0, L.stream, G);
}
void l_snn_indegree(const Launch& L, const GraphDev& G) { hipLaunchKernelGGL(k_snn_indegree, threads256(G.N * G.m), dim3(256), 0, L.stream, G); }
void l_snn_rowweight(const Launch& L, const SnnDev& S) { hipLaunchKernelGGL(k_snn_rowweight, waves4(S.N), dim3(256), 0, L.stream, S); }
void l_snn_short(const Launch& L, const SnnDev& S, bool write) {
  if (write) hipLaunchKernelGGL(k_snn_short<true>, dim3((unsigned)S.N), dim3(64), 0, L.stream, S);
  else hipLaunchKernelGGL(k_snn_short<false>, dim3((unsigned)S.N), dim3(64), 0, L.stream, S);
}
void l_snn_long(const Launch& L, const SnnDev& S, bool write) {
  if (write) hipLaunchKernelGGL(k_snn_long<true>, dim3(SNN_LONG_WGS), dim3(256), 0, L.stream, S);
  else hipLaunchKernelGGL(k_snn_long<false>, dim3(SNN_LONG_WGS), dim3(256), 0, L.stream, S);
}
void l_cc_check(const Launch& L, const CcDev& C) { hipLaunchKernelGGL(k_cc_check, waves4(C.N), dim3(256), 0, L.stream, C); }
void l_cc_init(const Launch& L, const CcDev& C) { hipLaunchKernelGGL(k_cc_init, threads256(C.N), dim3(256), 0, L.stream, C); }
void l_cc_hook(const Launch& L, const CcDev& C) { hipLaunchKernelGGL(k_cc_hook, waves4(C.N), dim3(256), 0, L.stream, C); }
void l_cc_jump(const Launch& L, const CcDev& C, bool check) { hipLaunchKernelGGL(k_cc_jump, threads256(C.N), dim3(256), 0, L.stream, C, check ? 1 : 0); }

}  // namespace hmx

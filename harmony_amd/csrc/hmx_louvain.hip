// hmx_louvain.hip -- gfx950 kernels of the Louvain clustering (include/harmony_mi355x_louvain.h; DESIGN "Louvain clustering") on a symmetric CSR
// with float weights in [0, 1].  Weights become integers once (q = llrint(w 2^24)); from there every sum is an integer sum, the one
// floating-point expression is the three-operation score, and a sub-round's decisions read only what its start left: the result is a pure
// function of the input.
//
//   k_lv_check            one wave per row: every weight in [0, 1] and finite, every mirror entry of the same bits (one flag word);
//   k_lv_quantise         one wave per row: q per entry (0 on the diagonal), the row's degree k;
//   k_lv_init             comm[i] = i, tot[i] = k[i]; the rows above the short path's cap are listed;
//   k_lv_decide           one wave per active row of at most short_cap entries: keys comm << 32 | slot sorted in LDS (bitonic), run sums, score,
//                         arg-max with ties to the smallest community; writes target[i] or -1, never comm;
//   k_lv_decide_long      one workgroup per active long row: the community range of the row in windows of LV_WINDOW 64-bit LDS counters;
//   k_lv_apply            the movers of the sub-round: comm, tot (integer atomics), the count of moves;
//   k_lv_mark / count / place / reduce<WRITE> / compose   aggregation: the non-empty ids marked (then scanned), entries, degree and inner weight
//                         per community, keys c' << 32 | entry placed in the community's segment (then sorted by the graph stage's sort), run
//                         heads counted / coarse indices and sums written behind the scanned lengths, the cells' labels composed.
// Every loop has a bound known on entry; no kernel waits for another workgroup; integer atomics only.
#include "hmx_louvain.h"
#include "hmx_lv_device.h"

namespace hmx {

__device__ __forceinline__ int lv_lower_bound(const int* v, int n, int key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ long long wave_inclusive_ll(long long v, int l) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long o = __shfl_up(v, d, 64);
    if (l >= d) v += o;
  }
  return v;
}

// ---- the caller's graph ------------------------------------------------------------------------------------------------------------------------------
// (safe on a pattern that fails l_cc_check: an index out of range is skipped, a search in an unsorted row stays inside the row)
__global__ __launch_bounds__(256) void k_lv_check(LvIn I) {
  const int l = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= I.N) return;
  const long long b = I.indptr[i], e1 = I.indptr[i + 1];
  int bad = 0;
  for (long long e = b + l; e < e1; e += 64) {
    const float w = I.weights[e];
    if (!(w >= 0.0f && w <= 1.0f)) bad |= LV_FLAG_WEIGHT;      // (NaN fails both comparisons)
    const int j = I.indices[e];
    if (j < 0 || j >= I.N) continue;
    const long long jb = I.indptr[j], jn = I.indptr[j + 1] - jb;
    const int lo = lv_lower_bound(I.indices + jb, (int)jn, (int)i);
    if (lo < jn && I.indices[jb + lo] == (int)i && __float_as_uint(I.weights[jb + lo]) != __float_as_uint(w)) bad |= LV_FLAG_MIRROR;
  }
  if (bad) atomicOr(I.flag, bad);
}
__global__ __launch_bounds__(256) void k_lv_quantise(LvIn I) {
  const int l = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= I.N) return;
  const long long b = I.indptr[i], e1 = I.indptr[i + 1];
  long long s = 0;
  for (long long e = b + l; e < e1; e += 64) {
    const long long q = I.indices[e] == (int)i ? 0ll : __double2ll_rn((double)I.weights[e] * LV_SCALE);      // (the product is exact: 24 bits times a power of two)
    I.q[e] = q;
    s += q;
  }
  s = wave_sum(s);
  if (l == 0) I.k[i] = s;
}

// ---- local moves ---------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lv_init(LvDev D) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= D.n) return;
  D.comm[i] = (int)i;
  D.tot[i] = D.k[i];
  if (D.indptr[i + 1] - D.indptr[i] > D.short_cap) {
    const unsigned at = atomicAdd(D.nlong, 1u);
    if ((long long)at < D.n) D.longrows[at] = (int)i;
  }
}

__global__ __launch_bounds__(64) void k_lv_decide(LvDev D) {
  __shared__ u64 sk[LV_SHORT_CAP];
  __shared__ long long sq[LV_SHORT_CAP];
  const int l = threadIdx.x;
  const long long i = blockIdx.x;
  if (i >= D.n || lv_bucket(i, D.key) != D.bucket) return;      // (the whole workgroup)
  const long long b = D.indptr[i], len = D.indptr[i + 1] - b;
  if (len > D.short_cap || len > LV_SHORT_CAP) return;           // a long row
  const int n = (int)len;
  if (n == 0) { if (l == 0) D.target[i] = -1; return; }
  const int a = D.comm[i];
  const long long ki = D.k[i];
  const double kg = lv_kg(ki, D.g);
  int P = 64;
  while (P < n) P <<= 1;                                         // (n <= LV_SHORT_CAP, a power of two)
  for (int t = l; t < P; t += 64) {
    u64 key = ~0ull;
    if (t < n) {
      const int j = D.indices[b + t];
      if (j != (int)i) key = ((u64)(unsigned)D.comm[j] << 32) | (unsigned)t;      // (the diagonal sorts behind every community, with the padding)
    }
    sk[t] = key;
  }
  __syncthreads();
  for (int k2 = 2; k2 <= P; k2 <<= 1)
    for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
      for (int t = l; t < (P >> 1); t += 64) {
        const int x = ((t & ~(j2 - 1)) << 1) | (t & (j2 - 1));
        const u64 u = sk[x], v = sk[x | j2];
        if ((u > v) == ((x & k2) == 0)) { sk[x] = v; sk[x | j2] = u; }
      }
      __syncthreads();
    }
  for (int t = l; t < n; t += 64) {
    const u64 key = sk[t];
    sq[t] = key == ~0ull ? 0ll : D.q[b + (long long)(unsigned)key];
  }
  __syncthreads();
  bool has = false;
  double bs = 0.0;
  int bc = 0;
  long long wa = 0;
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int p = c0 + l;
    if (p >= n) continue;
    const u64 key = sk[p];
    if (key == ~0ull) continue;
    const unsigned c = (unsigned)(key >> 32);
    if (p > 0 && (unsigned)(sk[p - 1] >> 32) == c) continue;     // not the head of its run
    long long w = 0;
    for (int r = p; r < n && (unsigned)(sk[r] >> 32) == c; r++) w += sq[r];
    if ((int)c == a) wa = w;
    else lv_better(has, bs, bc, true, lv_score(w, kg, D.tot[c]), (int)c);
  }
  wa = wave_sum(wa);
  const double sa = lv_score(wa, kg, D.tot[a] - ki);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const int oh = __shfl_xor(has ? 1 : 0, m, 64);
    const double os = __shfl_xor(bs, m, 64);
    const int oc = __shfl_xor(bc, m, 64);
    lv_better(has, bs, bc, oh != 0, os, oc);
  }
  if (l == 0) D.target[i] = (has && bs > sa) ? bc : -1;
}

__global__ __launch_bounds__(256) void k_lv_decide_long(LvDev D) {
  __shared__ u64 cnt[LV_WINDOW];
  __shared__ unsigned pres[LV_WINDOW / 32];
  __shared__ double rs[256];
  __shared__ int rc[256], rh[256];
  __shared__ int s_mn, s_mx;
  __shared__ long long s_wa;
  const int tid = threadIdx.x;
  const unsigned nlong = (unsigned)min((long long)*D.nlong, D.n);
  for (unsigned r = blockIdx.x; r < nlong; r += gridDim.x) {
    const long long i = D.longrows[r];
    if (lv_bucket(i, D.key) != D.bucket) continue;               // (the same in every thread)
    const long long b = D.indptr[i], len = D.indptr[i + 1] - b;
    const int a = D.comm[i];
    const long long ki = D.k[i];
    const double kg = lv_kg(ki, D.g);
    if (tid == 0) { s_mn = a; s_mx = a; s_wa = 0; }
    __syncthreads();
    int mn = a, mx = a;
    for (long long t = tid; t < len; t += 256) {
      const int j = D.indices[b + t];
      if (j == (int)i) continue;
      const int c = D.comm[j];
      mn = min(mn, c); mx = max(mx, c);
    }
    atomicMin(&s_mn, mn);
    atomicMax(&s_mx, mx);
    __syncthreads();
    const long long first = (long long)(s_mn / LV_WINDOW) * LV_WINDOW, last = s_mx;
    bool has = false;
    double bs = 0.0;
    int bc = 0;
    for (long long w0 = first; w0 <= last; w0 += LV_WINDOW) {    // (at most n / LV_WINDOW + 1 windows)
      for (int t = tid; t < LV_WINDOW; t += 256) cnt[t] = 0ull;
      for (int t = tid; t < LV_WINDOW / 32; t += 256) pres[t] = 0u;
      __syncthreads();
      for (long long t = tid; t < len; t += 256) {
        const int j = D.indices[b + t];
        if (j == (int)i) continue;
        const long long off = (long long)D.comm[j] - w0;
        if (off >= 0 && off < LV_WINDOW) {
          atomicAdd(&cnt[off], (u64)D.q[b + t]);
          atomicOr(&pres[off >> 5], 1u << (off & 31));
        }
      }
      if (tid == 0 && a >= w0 && a < w0 + LV_WINDOW) atomicOr(&pres[(a - w0) >> 5], 1u << ((a - w0) & 31));
      __syncthreads();
      for (int off = tid; off < LV_WINDOW; off += 256) {
        if (!((pres[off >> 5] >> (off & 31)) & 1u)) continue;
        const int c = (int)(w0 + off);
        const long long w = (long long)cnt[off];
        if (c == a) s_wa = w;                                    // (one thread of one window)
        else lv_better(has, bs, bc, true, lv_score(w, kg, D.tot[c]), c);
      }
      __syncthreads();
    }
    rs[tid] = bs; rc[tid] = bc; rh[tid] = has ? 1 : 0;
    __syncthreads();
    if (tid == 0) {
      bool h = false;
      double s = 0.0;
      int c = 0;
      for (int t = 0; t < 256; t++) lv_better(h, s, c, rh[t] != 0, rs[t], rc[t]);
      const double sa = lv_score(s_wa, kg, D.tot[a] - ki);
      D.target[i] = (h && s > sa) ? c : -1;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_lv_apply(LvDev D) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= D.n || lv_bucket(i, D.key) != D.bucket) return;
  const int t = D.target[i];
  if (t < 0 || t >= D.n) return;
  const int a = D.comm[i];
  const long long ki = D.k[i];
  D.comm[i] = t;
  atomicAdd((u64*)(D.tot + t), (u64)ki);
  atomicAdd((u64*)(D.tot + a), (u64)(-ki));
  atomicAdd(D.moved, 1u);
}

// ---- aggregation ---------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lv_mark(LvAgg A) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < A.n) A.mark[A.comm[i]] = 1u;
}
__global__ __launch_bounds__(256) void k_lv_count(LvAgg A) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  const long long c = A.newid[A.comm[i]];
  if (c < 0 || c >= A.C) return;
  atomicAdd(A.ecount + c, (unsigned)(A.indptr[i + 1] - A.indptr[i]));
  atomicAdd((u64*)(A.ck + c), (u64)A.k[i]);
  if (A.in) atomicAdd((u64*)(A.cin + c), (u64)A.in[i]);
}
__global__ __launch_bounds__(256) void k_lv_place(LvAgg A) {
  const int l = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= A.n) return;
  const long long c = A.newid[A.comm[i]];
  if (c < 0 || c >= A.C) return;
  const long long b = A.indptr[i], len = A.indptr[i + 1] - b;
  if (len == 0) return;
  unsigned base = 0;
  if (l == 0) base = atomicAdd(A.cursor + c, (unsigned)len);
  base = __shfl(base, 0, 64);
  const long long sb = A.soff[c], sn = A.soff[c + 1] - sb;
  for (long long t = l; t < len; t += 64) {
    const long long cj = A.newid[A.comm[A.indices[b + t]]];
    if ((long long)base + t < sn) A.keys[sb + base + t] = ((u64)cj << 32) | (u64)(b + t);      // (fewer than 2^31 entries: the host refuses more)
  }
}
// one wave per community: its segment, sorted by the other end's community, in chunks of 64; a segmented scan gives every run's sum at its tail
template <bool WRITE>
__global__ __launch_bounds__(256) void k_lv_reduce(LvAgg A) {
  const int l = threadIdx.x & 63;
  const long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= A.C) return;
  const long long sb = A.soff[c], sn = A.soff[c + 1] - sb;
  const long long ob = WRITE ? A.cindptr[c] : 0, rowlen = WRITE ? A.cindptr[c + 1] - ob : 0;
  const u64 upto = l == 63 ? ~0ull : ((2ull << l) - 1);          // lanes 0 .. l
  long long base = 0, carry = 0, self = 0;
  for (long long p0 = 0; p0 < sn; p0 += 64) {
    const long long p = p0 + l;
    const bool valid = p < sn;
    const u64 key = valid ? A.keys[sb + p] : 0ull;
    const long long cj = (long long)(key >> 32);
    const bool head = valid && (p == 0 || (long long)(A.keys[sb + p - 1] >> 32) != cj);
    const u64 nonself = __ballot(head && cj != c);
    if (WRITE) {
      const bool tail = valid && (p == sn - 1 || (long long)(A.keys[sb + p + 1] >> 32) != cj);
      const long long v = valid ? A.q[(long long)(unsigned)key] : 0ll;
      const long long s = wave_inclusive_ll(v, l);
      const u64 hm = __ballot(head) & upto;
      const int start = hm ? 63 - __clzll((long long)hm) : 0;    // the head of the lane's run in this chunk; none: the run came in from the last chunk
      const long long before = __shfl(s, start > 0 ? start - 1 : 0, 64);
      long long seg = s - (start > 0 ? before : 0ll);
      if (!hm) seg += carry;
      if (tail) {
        if (cj == c) self += seg;
        else {
          const long long pos = base + __popcll(nonself & upto) - 1;
          if (pos >= 0 && pos < rowlen) { A.cindices[ob + pos] = (int)cj; A.cq[ob + pos] = seg; }
        }
      }
      carry = __shfl((valid && !tail) ? seg : 0ll, 63, 64);
    }
    base += __popcll(nonself);
  }
  if (!WRITE) {
    if (l == 0) A.len[c] = (unsigned)base;
    return;
  }
  self = wave_sum(self);
  if (l == 0) A.cin[c] += self;                                  // (k_lv_count's atomics ended with their kernel)
}
__global__ __launch_bounds__(256) void k_lv_compose(LvAgg A, int first) {
  const long long cell = (long long)blockIdx.x * 256 + threadIdx.x;
  if (cell >= A.cells) return;
  const long long node = first ? cell : (long long)A.lab[cell];
  if (node < 0 || node >= A.n) return;
  A.lab[cell] = (int)A.newid[A.comm[node]];
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------------------
static dim3 lv_waves4(long long n) { return dim3((unsigned)((n + 3) / 4)); }
static dim3 lv_threads256(long long n) { return dim3((unsigned)((n + 255) / 256)); }

void l_lv_check(const Launch& L, const LvIn& I) { hipLaunchKernelGGL(k_lv_check, lv_waves4(I.N), dim3(256), 0, L.stream, I); }
void l_lv_quantise(const Launch& L, const LvIn& I) { hipLaunchKernelGGL(k_lv_quantise, lv_waves4(I.N), dim3(256), 0, L.stream, I); }
void l_lv_init(const Launch& L, const LvDev& D) { hipLaunchKernelGGL(k_lv_init, lv_threads256(D.n), dim3(256), 0, L.stream, D); }
void l_lv_decide(const Launch& L, const LvDev& D, bool with_long) {
  hipLaunchKernelGGL(k_lv_decide, dim3((unsigned)D.n), dim3(64), 0, L.stream, D);
  if (with_long) hipLaunchKernelGGL(k_lv_decide_long, dim3(LV_LONG_WGS), dim3(256), 0, L.stream, D);
}
void l_lv_apply(const Launch& L, const LvDev& D) { hipLaunchKernelGGL(k_lv_apply, lv_threads256(D.n), dim3(256), 0, L.stream, D); }
void l_lv_mark(const Launch& L, const LvAgg& A) { hipLaunchKernelGGL(k_lv_mark, lv_threads256(A.n), dim3(256), 0, L.stream, A); }
void l_lv_count(const Launch& L, const LvAgg& A) { hipLaunchKernelGGL(k_lv_count, lv_threads256(A.n), dim3(256), 0, L.stream, A); }
void l_lv_place(const Launch& L, const LvAgg& A) { hipLaunchKernelGGL(k_lv_place, lv_waves4(A.n), dim3(256), 0, L.stream, A); }
void l_lv_reduce(const Launch& L, const LvAgg& A, bool write) {
  if (write) hipLaunchKernelGGL(k_lv_reduce<true>, lv_waves4(A.C), dim3(256), 0, L.stream, A);
  else hipLaunchKernelGGL(k_lv_reduce<false>, lv_waves4(A.C), dim3(256), 0, L.stream, A);
}
void l_lv_compose(const Launch& L, const LvAgg& A, bool first) { hipLaunchKernelGGL(k_lv_compose, lv_threads256(A.cells), dim3(256), 0, L.stream, A, first ? 1 : 0); }

}  // namespace hmx

// hmx_leiden.hip -- gfx950 kernels of the Leiden clustering (include/harmony_mi355x_leiden.h; DESIGN "Leiden clustering").  The integers, the
// score and the hashed sub-rounds are Louvain's (hmx_lv_device.h); the checks, the quantisation and the aggregation are hmx_louvain.hip's
// launchers.  What Louvain lacks is here:
//
//   k_ld_keep<WRITE>      one wave per row of the caller's graph: the entries with q != 0 (the diagonal has q = 0) counted, then written in
//                         their order behind the scanned counts: no later kernel sees a diagonal or an entry that is not an edge;
//   k_ld_iota / k_ld_parent_min / k_ld_parent_gather   a level's starting partition: the identity, or per community of the level before the
//                         smallest new id among its refined parts (an integer atomicMin), gathered per new node;
//   k_ld_start            tot[comm[i]] += k[i] (integer atomics); the rows above the short path's cap are listed;
//   k_ld_decide<REFINE> / k_ld_decide_long<REFINE>   k_lv_decide's two shapes.  Moves: the candidates are the neighbours' communities, the
//                         own one and "alone" (id i, weight 0, when comm[i] != i and tot[i] == 0).  Refinement: only a mover decides (active,
//                         a singleton, node_ok); a neighbour's key is ref[j], kept if j is inner, no mover of this sub-round and its refined
//                         community passes the cut test; staying scores 0.0; the (mover, mover) inner entries are counted in blocked;
//   k_ld_apply / k_ld_refine_apply   the movers of the sub-round: comm, tot / ref, rtot, size (integer atomics), the count of moves;
//   k_ld_refine_setup     one wave per row: P_i, node_ok, ref[i] = i, rtot[i] = k[i], size[i] = 1;
//   k_ld_cut              one wave per row: the inner q that leaves the row's refined community, added into cut[ref[i]];
//   k_ld_sums             one wave per row: in_i and the inner q added into cin[comm[i]], the id marked.
// Every loop has a bound known on entry; no kernel waits for another workgroup; integer atomics only.
#include "hmx_leiden.h"
#include "hmx_lv_device.h"

namespace hmx {

// dbl(x) >= (dbl(r) g) dbl(rest): two rounded products
__device__ __forceinline__ bool ld_holds(long long x, long long r, double g, long long rest) {
#pragma clang fp contract(off)
  const double rg = __dmul_rn(__ll2double_rn(r), g);
  return __ll2double_rn(x) >= __dmul_rn(rg, __ll2double_rn(rest));
}
// a mover of the refinement's sub-round: active, alone in its refined community, well connected to its community
__device__ __forceinline__ bool ld_mover(const LdDev& D, long long j) {
  return lv_bucket(j, D.key) == D.bucket && D.ok[j] != 0 && D.size[D.ref[j]] == 1;
}
// the key of entry j of a row whose node sits in community a: the community (moves) or the refined community (refinement) it votes for;
// -1: it does not vote.  mm: the entry joins two movers.
template <bool REFINE>
__device__ __forceinline__ int ld_key(const LdDev& D, int j, int a, long long ta, bool& mm) {
  mm = false;
  const int c = D.comm[j];
  if (!REFINE) return c;
  if (c != a) return -1;
  if (ld_mover(D, j)) { mm = true; return -1; }
  const int r = D.ref[j];
  const long long rt = D.rtot[r];
  return ld_holds(D.cut[r], rt, D.g, ta - rt) ? r : -1;
}

// ---- level 0: the edges ---------------------------------------------------------------------------------------------------------------------------------
template <bool WRITE>
__global__ __launch_bounds__(256) void k_ld_keep(LdKeep K) {
  const int l = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= K.N) return;
  const long long b = K.indptr[i], len = K.indptr[i + 1] - b;
  const long long ob = WRITE ? K.kptr[i] : 0, olen = WRITE ? K.kptr[i + 1] - ob : 0;
  const u64 below = (1ull << l) - 1;
  long long base = 0;
  for (long long t0 = 0; t0 < len; t0 += 64) {
    const long long t = t0 + l;
    const long long q = t < len ? K.q[b + t] : 0ll;
    const u64 m = __ballot(q != 0);
    if (WRITE && q != 0) {
      const long long pos = base + __popcll(m & below);
      if (pos < olen) { K.kindices[ob + pos] = K.indices[b + t]; K.kq[ob + pos] = q; }
    }
    base += __popcll(m);
  }
  if (!WRITE && l == 0) K.cnt[i] = (unsigned)base;
}

// ---- a level's start -----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ld_iota(LdDev D) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < D.n) D.comm[i] = (int)i;
}
__global__ __launch_bounds__(256) void k_ld_parent_min(LdNext X) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= X.n) return;
  const long long v = X.newid[X.ref[i]];
  if (v >= 0 && v < X.C) atomicMin(X.pmin + X.comm[i], (unsigned)v);
}
__global__ __launch_bounds__(256) void k_ld_parent_gather(LdNext X) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= X.n) return;
  const long long v = X.newid[X.ref[i]];
  if (v >= 0 && v < X.C) X.next[v] = (int)X.pmin[X.comm[i]];      // (the members of one refined community write the same value)
}
__global__ __launch_bounds__(256) void k_ld_start(LdDev D) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= D.n) return;
  const int c = D.comm[i];
  if (c >= 0 && c < D.n) atomicAdd((u64*)(D.tot + c), (u64)D.k[i]);
  if (D.indptr[i + 1] - D.indptr[i] > D.short_cap) {
    const unsigned at = atomicAdd(D.nlong, 1u);
    if ((long long)at < D.n) D.longrows[at] = (int)i;
  }
}

// ---- decisions: local moves and refinement --------------------------------------------------------------------------------------------------------------
template <bool REFINE>
__global__ __launch_bounds__(64) void k_ld_decide(LdDev D) {
  __shared__ u64 sk[LV_SHORT_CAP];
  __shared__ long long sq[LV_SHORT_CAP];
  const int l = threadIdx.x;
  const long long i = blockIdx.x;
  if (i >= D.n || lv_bucket(i, D.key) != D.bucket) return;      // (the whole workgroup)
  const long long b = D.indptr[i], len = D.indptr[i + 1] - b;
  if (len > D.short_cap || len > LV_SHORT_CAP) return;           // a long row
  const int n = (int)len;
  if (n == 0 || (REFINE && !ld_mover(D, i))) { if (l == 0) D.target[i] = -1; return; }
  const int a = D.comm[i];
  const long long ki = D.k[i], ta = D.tot[a];
  const double kg = lv_kg(ki, D.g);
  int P = 64;
  while (P < n) P <<= 1;                                         // (n <= LV_SHORT_CAP, a power of two)
  unsigned nmm = 0;
  for (int t = l; t < P; t += 64) {
    u64 key = ~0ull;
    if (t < n) {
      bool mm;
      const int c = ld_key<REFINE>(D, D.indices[b + t], a, ta, mm);
      if (c >= 0) key = ((u64)(unsigned)c << 32) | (unsigned)t;      // (an entry without a vote sorts behind every id, with the padding)
      nmm += mm ? 1u : 0u;
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
    if (REFINE) lv_better(has, bs, bc, true, lv_score(w, kg, D.rtot[c]), (int)c);
    else if ((int)c == a) wa = w;
    else lv_better(has, bs, bc, true, lv_score(w, kg, D.tot[c]), (int)c);
  }
  double sa = 0.0;                                               // staying: 0.0 in the refinement
  if (!REFINE) {
    wa = wave_sum(wa);
    sa = lv_score(wa, kg, ta - ki);
    if (l == 0 && a != (int)i && D.tot[i] == 0) lv_better(has, bs, bc, true, lv_score(0ll, kg, 0ll), (int)i);      // alone
  } else {
    nmm = wave_sum(nmm);
    if (l == 0 && nmm) atomicAdd(D.blocked, nmm);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const int oh = __shfl_xor(has ? 1 : 0, m, 64);
    const double os = __shfl_xor(bs, m, 64);
    const int oc = __shfl_xor(bc, m, 64);
    lv_better(has, bs, bc, oh != 0, os, oc);
  }
  if (l == 0) D.target[i] = (has && bs > sa) ? bc : -1;
}

template <bool REFINE>
__global__ __launch_bounds__(256) void k_ld_decide_long(LdDev D) {
  __shared__ u64 cnt[LV_WINDOW];
  __shared__ unsigned pres[LV_WINDOW / 32];
  __shared__ double rs[256];
  __shared__ int rc[256], rh[256];
  __shared__ int s_mn, s_mx;
  __shared__ unsigned s_mm;
  __shared__ long long s_wa;
  const int tid = threadIdx.x;
  const unsigned nlong = (unsigned)min((long long)*D.nlong, D.n);
  for (unsigned r = blockIdx.x; r < nlong; r += gridDim.x) {
    const long long i = D.longrows[r];
    if (lv_bucket(i, D.key) != D.bucket) continue;               // (the same in every thread, as the next test)
    if (REFINE && !ld_mover(D, i)) { if (tid == 0) D.target[i] = -1; continue; }
    const long long b = D.indptr[i], len = D.indptr[i + 1] - b;
    const int a = D.comm[i];
    const long long ki = D.k[i], ta = D.tot[a];
    const double kg = lv_kg(ki, D.g);
    if (tid == 0) { s_mn = REFINE ? 0x7fffffff : a; s_mx = REFINE ? -1 : a; s_wa = 0; s_mm = 0u; }
    __syncthreads();
    int mn = 0x7fffffff, mx = -1;
    unsigned nmm = 0;
    for (long long t = tid; t < len; t += 256) {
      bool mm;
      const int c = ld_key<REFINE>(D, D.indices[b + t], a, ta, mm);
      nmm += mm ? 1u : 0u;
      if (c < 0) continue;
      mn = min(mn, c); mx = max(mx, c);
    }
    atomicMin(&s_mn, mn);
    atomicMax(&s_mx, mx);
    if (REFINE && nmm) atomicAdd(&s_mm, nmm);
    __syncthreads();
    const long long first = (long long)(s_mn / LV_WINDOW) * LV_WINDOW, last = s_mx;
    bool has = false;
    double bs = 0.0;
    int bc = 0;
    for (long long w0 = first; w0 <= last; w0 += LV_WINDOW) {    // (at most n / LV_WINDOW + 1 windows; none when no entry votes)
      for (int t = tid; t < LV_WINDOW; t += 256) cnt[t] = 0ull;
      for (int t = tid; t < LV_WINDOW / 32; t += 256) pres[t] = 0u;
      __syncthreads();
      for (long long t = tid; t < len; t += 256) {
        bool mm;
        const int c = ld_key<REFINE>(D, D.indices[b + t], a, ta, mm);
        const long long off = (long long)c - w0;
        if (c >= 0 && off >= 0 && off < LV_WINDOW) {
          atomicAdd(&cnt[off], (u64)D.q[b + t]);
          atomicOr(&pres[off >> 5], 1u << (off & 31));
        }
      }
      if (!REFINE && tid == 0 && a >= w0 && a < w0 + LV_WINDOW) atomicOr(&pres[(a - w0) >> 5], 1u << ((a - w0) & 31));
      __syncthreads();
      for (int off = tid; off < LV_WINDOW; off += 256) {
        if (!((pres[off >> 5] >> (off & 31)) & 1u)) continue;
        const int c = (int)(w0 + off);
        const long long w = (long long)cnt[off];
        if (REFINE) lv_better(has, bs, bc, true, lv_score(w, kg, D.rtot[c]), c);
        else if (c == a) s_wa = w;                               // (one thread of one window)
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
      double sa = 0.0;
      if (!REFINE) {
        sa = lv_score(s_wa, kg, ta - ki);
        if (a != (int)i && D.tot[i] == 0) lv_better(h, s, c, true, lv_score(0ll, kg, 0ll), (int)i);      // alone
      } else if (s_mm) atomicAdd(D.blocked, s_mm);
      D.target[i] = (h && s > sa) ? c : -1;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_ld_apply(LdDev D) {
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
// (a mover's own refined community is no candidate of this sub-round: nothing else touches rtot[i] or size[i])
__global__ __launch_bounds__(256) void k_ld_refine_apply(LdDev D) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= D.n || lv_bucket(i, D.key) != D.bucket) return;
  const int t = D.target[i];
  if (t < 0 || t >= D.n) return;
  D.ref[i] = t;
  atomicAdd((u64*)(D.rtot + t), (u64)D.k[i]);
  atomicAdd(D.size + t, 1);
  D.rtot[i] = 0;
  D.size[i] = 0;
  atomicAdd(D.moved, 1u);
}

// ---- the refinement's and the level's sums ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ld_refine_setup(LdDev D) {
  const int l = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= D.n) return;
  const long long b = D.indptr[i], e1 = D.indptr[i + 1];
  const int a = D.comm[i];
  long long s = 0;
  for (long long e = b + l; e < e1; e += 64)
    if (D.comm[D.indices[e]] == a) s += D.q[e];
  s = wave_sum(s);
  if (l != 0) return;
  const long long ki = D.k[i];
  D.ok[i] = ld_holds(s, ki, D.g, D.tot[a] - ki) ? 1 : 0;
  D.ref[i] = (int)i;
  D.rtot[i] = ki;
  D.size[i] = 1;
}
__global__ __launch_bounds__(256) void k_ld_cut(LdDev D) {
  const int l = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= D.n) return;
  const long long b = D.indptr[i], e1 = D.indptr[i + 1];
  const int a = D.comm[i], r = D.ref[i];
  long long s = 0;
  for (long long e = b + l; e < e1; e += 64) {
    const int j = D.indices[e];
    if (D.comm[j] == a && D.ref[j] != r) s += D.q[e];
  }
  s = wave_sum(s);
  if (l == 0 && s) atomicAdd((u64*)(D.cut + r), (u64)s);
}
__global__ __launch_bounds__(256) void k_ld_sums(LdDev D) {
  const int l = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= D.n) return;
  const long long b = D.indptr[i], e1 = D.indptr[i + 1];
  const int a = D.comm[i];
  long long s = 0;
  for (long long e = b + l; e < e1; e += 64)
    if (D.comm[D.indices[e]] == a) s += D.q[e];
  s = wave_sum(s);
  if (l != 0) return;
  if (D.in) s += D.in[i];
  if (s) atomicAdd((u64*)(D.cin + a), (u64)s);
  D.mark[a] = 1u;
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------------------
static dim3 ld_waves4(long long n) { return dim3((unsigned)((n + 3) / 4)); }
static dim3 ld_threads256(long long n) { return dim3((unsigned)((n + 255) / 256)); }

void l_ld_keep(const Launch& L, const LdKeep& K, bool write) {
  if (write) hipLaunchKernelGGL(k_ld_keep<true>, ld_waves4(K.N), dim3(256), 0, L.stream, K);
  else hipLaunchKernelGGL(k_ld_keep<false>, ld_waves4(K.N), dim3(256), 0, L.stream, K);
}
void l_ld_iota(const Launch& L, const LdDev& D) { hipLaunchKernelGGL(k_ld_iota, ld_threads256(D.n), dim3(256), 0, L.stream, D); }
void l_ld_parent(const Launch& L, const LdNext& X) {
  hipLaunchKernelGGL(k_ld_parent_min, ld_threads256(X.n), dim3(256), 0, L.stream, X);
  hipLaunchKernelGGL(k_ld_parent_gather, ld_threads256(X.n), dim3(256), 0, L.stream, X);
}
void l_ld_start(const Launch& L, const LdDev& D) { hipLaunchKernelGGL(k_ld_start, ld_threads256(D.n), dim3(256), 0, L.stream, D); }
void l_ld_decide(const Launch& L, const LdDev& D, bool with_long) {
  hipLaunchKernelGGL(k_ld_decide<false>, dim3((unsigned)D.n), dim3(64), 0, L.stream, D);
  if (with_long) hipLaunchKernelGGL(k_ld_decide_long<false>, dim3(LV_LONG_WGS), dim3(256), 0, L.stream, D);
}
void l_ld_refine_decide(const Launch& L, const LdDev& D, bool with_long) {
  hipLaunchKernelGGL(k_ld_decide<true>, dim3((unsigned)D.n), dim3(64), 0, L.stream, D);
  if (with_long) hipLaunchKernelGGL(k_ld_decide_long<true>, dim3(LV_LONG_WGS), dim3(256), 0, L.stream, D);
}
void l_ld_apply(const Launch& L, const LdDev& D) { hipLaunchKernelGGL(k_ld_apply, ld_threads256(D.n), dim3(256), 0, L.stream, D); }
void l_ld_refine_apply(const Launch& L, const LdDev& D) { hipLaunchKernelGGL(k_ld_refine_apply, ld_threads256(D.n), dim3(256), 0, L.stream, D); }
void l_ld_refine_setup(const Launch& L, const LdDev& D) { hipLaunchKernelGGL(k_ld_refine_setup, ld_waves4(D.n), dim3(256), 0, L.stream, D); }
void l_ld_cut(const Launch& L, const LdDev& D) { hipLaunchKernelGGL(k_ld_cut, ld_waves4(D.n), dim3(256), 0, L.stream, D); }
void l_ld_sums(const Launch& L, const LdDev& D) { hipLaunchKernelGGL(k_ld_sums, ld_waves4(D.n), dim3(256), 0, L.stream, D); }

}  // namespace hmx

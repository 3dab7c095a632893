// hmx_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels for the Harmony
// clustering + correction loop.  MI355X only: no CUDA paths, no portability layer.
//
// Data layout (DESIGN.md "HBM layout"): cells are stored cell-major, exactly the
// reference's column-major d x N / K x N matrices (src/harmony.h:50), but in an
// internal order sorted by covariate-level combination so that every streaming pass sees
// long runs of cells sharing one combination.  "Cluster-lane" mapping: lane l of a wave
// owns clusters l, l+64, ... (KPL per lane); a cell's PCs are broadcast lane->SGPR with
// v_readlane.  Cross-cell sums (O, E, objective, ridge statistics) are accumulated per
// lane over a run and flushed with one coalesced atomic per run: 64-bit fixed point for
// R sums (exact, order-independent => bit-reproducible and shard-count independent),
// fp64 for the rest.
#include "hmx_internal.h"
#include "hmx_plan.h"
#include <float.h>
#include <hip/hip_ext.h>

#ifndef HMX_TILE_BF
#define HMX_TILE_BF 0         // 1 (hmx_tile_bf.hip): this translation unit builds ONLY k_tile, with the split-bf16 distance GEMM, and its dispatch
#endif

namespace hmx {
typedef float f32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) F3 { float x, y, z; };     // 12-byte row segment (global_store_dwordx3)
struct __attribute__((aligned(8))) F2 { float x, y; };

// --------------------------------------------------------------------------------------
// device helpers
// --------------------------------------------------------------------------------------
__device__ __forceinline__ float rlane(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ float wsum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ double wsumd(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wmin64(unsigned long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    unsigned lo = __shfl_xor((unsigned)(v & 0xffffffffu), m, 64);
    unsigned hi = __shfl_xor((unsigned)(v >> 32), m, 64);
    unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o < v ? o : v;
  }
  return v;
}
// UNCONDITIONAL load from a clamped (always valid) index, masked afterwards.  `cond ? p[i] : 0` makes hipcc branch
// around every load and wait vmcnt(0) at each join -- fully serialised memory latency (measured: 2-3x slower).
template <class T> __device__ __forceinline__ T ld_or(const T* __restrict__ p, size_t safe_idx, bool ok, T dflt) {
  const T v = p[safe_idx];
  return ok ? v : dflt;
}
__device__ __forceinline__ float trunc_logf_dev(float x) {  // arma::trunc_log (src/utils.cpp:78)
  return (x > 0.0f) ? logf(x) : logf(FLT_MIN);
}
// R in [0,1] -> fixed point: ONE function of the float for every kernel that adds or removes a cell's R (what a block update files is exactly what
// the next round takes out).  fma + truncating convert: two instructions (round half up; from 2^23 on r * 2^29 is an integer already).
__device__ __forceinline__ unsigned fx32_of(float r) { return (unsigned)__builtin_fmaf(r, FX_SCALE, 0.5f); }
__device__ __forceinline__ unsigned long long fx_of(float r) { return (unsigned long long)fx32_of(r); }

// diversity penalty ((2E+1)/(O+E+1))^theta (src/harmony.cpp:319-321) with a SHORT dependent chain: rcp, mul, log2, mul, exp2
// (~2e-7 relative; powf's ~100 dependent instructions cost >1 us in the serial prologue of every block step at gfx950's
// 26-cycle dependent-issue latency).  ONE definition for the fused and the stand-alone fold kernels: the sharded and the
// single-GPU paths must produce bit-identical penalty tables.
// one int64 of a K x B table into every peer's inbox: two self-validating granules {tag, half}, written through at system scope
// (par = plane * 8: the plane's first source slot)
__device__ __forceinline__ void p2p_send(const Dev& D, size_t par, int i, unsigned tag, long long v) {
  const unsigned long long tb = (unsigned long long)tag << 32;
  const unsigned long long lo = tb | ((unsigned long long)v & 0xffffffffull), hi = tb | ((unsigned long long)v >> 32);
#pragma unroll
  for (int gq = 0; gq < 8; gq++) if (gq < D.p2p_world && gq != D.p2p_rank) {
    unsigned long long* dst = D.p2p_inbox[gq] + ((par + D.p2p_rank) * P2P_CAP + i) * 2;
    __hip_atomic_store(dst, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(dst + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
__device__ __forceinline__ float pen_pow(float num, float den, float theta) {
  const float x = num * __builtin_amdgcn_rcpf(den);
  return __builtin_amdgcn_exp2f(theta * __builtin_amdgcn_logf(x));
}
#if !HMX_TILE_BF      // ---- peer inboxes beyond the chain's own exchanges: connection self-test and the small / large all-reduces ----
// Self-test of the peer-to-peer inboxes, run by every rank at the same time before the chain may use them: P2P_TEST_STEPS exchanges of
// a 2048-entry table with known contents through exactly the chain's code path (p2p_send, the same slots, parities and polls),
// every received value checked.  result[0] = wrong or missing values (0 = pass), result[1] = 100 MHz ticks of the steps after the
// first (the first absorbs the launch skew between the ranks; bounded at ~3 s).
constexpr int P2P_TEST_STEPS = 64;
__device__ __forceinline__ long long p2p_test_value(int rank, int step, int i) {
  const long long v = (long long)(rank + 1) * 0x100000001ll * (long long)(i + 1) + (long long)step * 7919;
  return ((i + step) & 1) ? -v : v;
}
__global__ void __launch_bounds__(512) k_p2p_selftest(Dev D, unsigned tag, int* result) {
  const int tid = threadIdx.x, G = D.p2p_world, me = D.p2p_rank;
  __shared__ int gave_up, bad;
  if (tid == 0) { gave_up = 0; bad = 0; }
  __syncthreads();
  int wrong = 0;
  unsigned long long t1 = 0;
  for (int step = 0; step < P2P_TEST_STEPS; step++) {
    if (step == 1) t1 = wall_clock64();
    const unsigned tagx = tag + (unsigned)step;
    const size_t par = (size_t)(step & 1) * 8;      // (the chain's two planes)
#pragma unroll
    for (int e = 0; e < 4; e++) p2p_send(D, par, tid + e * 512, tagx, p2p_test_value(me, step, tid + e * 512));
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int i = tid + e * 512;
#pragma unroll
      for (int gq = 0; gq < 8; gq++) if (gq < G && gq != me) {
        const unsigned long long* src = D.p2p_inbox_self() + ((par + gq) * P2P_CAP + i) * 2;
        unsigned long long lo = 0, hi = 0;
        bool got = false;
        for (int spins = 0; spins < (1 << 20); spins++) {
          lo = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          hi = __hip_atomic_load(src + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          if ((unsigned)(lo >> 32) == tagx && (unsigned)(hi >> 32) == tagx) { got = true; break; }
          if ((spins & 63) == 63 && __hip_atomic_load(&gave_up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
          if (step == 0) __builtin_amdgcn_s_sleep(100); else __builtin_amdgcn_s_sleep(2);
        }
        if (!got) { __hip_atomic_store(&gave_up, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); wrong++; }
        else if ((long long)((hi << 32) | (lo & 0xffffffffull)) != p2p_test_value(gq, step, i)) wrong++;
      }
    }
  }
  const unsigned long long t2 = wall_clock64();
  if (wrong) atomicAdd(&bad, wrong);
  __syncthreads();
  if (tid == 0) { result[0] = bad; result[1] = (int)(t2 - t1); }
}
// Generic all-reduce of a small buffer through the peers' inboxes (planes 2 / 3): the collectives of a run that are NOT block steps --
// O after a head, the objective's two sums, the Lloyd sums and counts, the seeding minima, small ridge statistics -- are a few KB each
// and latency-bound: as host-launched ncclAllReduce calls they cost a launch + a ring each (~50 per run).  Here: one workgroup, every
// rank writes its values straight into every peer's inbox (self-validating {tag, half} granules, as the chain does) and adds up what
// arrived in its own, in RANK ORDER (fp64 sums are then identical on every rank).  A rank can be at most one call ahead of a peer (it
// needs the peer's values of call n to finish call n), so two planes alternate.  Every spin is bounded; a timeout raises *err (the
// chain's error word: it reaches the host with the next objective snapshot).
__global__ void __launch_bounds__(1024) k_p2p_allreduce(Dev D, unsigned long long* __restrict__ buf, int n, int dtype, unsigned seq, int* err) {
  const int tid = threadIdx.x, G = D.p2p_world, me = D.p2p_rank;
  const unsigned tag = 0x40000000u + (seq & 0x3fffffffu);
  const size_t par = (size_t)(2 + (seq & 1u)) * 8;
  for (int base = 0; base < n; base += 1024 * 4) {
    unsigned long long mine[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int i = base + tid + e * 1024;
      mine[e] = (i < n) ? buf[i] : 0ull;
      if (i < n) p2p_send(D, par, i, tag, (long long)mine[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int i = base + tid + e * 1024;
      if (i >= n) continue;
      unsigned long long val[8];
#pragma unroll
      for (int gq = 0; gq < 8; gq++) {
        val[gq] = mine[e];
        if (gq < G && gq != me) {
          const unsigned long long* src = D.p2p_inbox_self() + ((par + gq) * P2P_CAP + i) * 2;
          unsigned long long lo = 0, hi = 0;
          bool got = false;
          for (int spins = 0; spins < (1 << 20); spins++) {
            lo = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            hi = __hip_atomic_load(src + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if ((unsigned)(lo >> 32) == tag && (unsigned)(hi >> 32) == tag) { got = true; break; }
            if ((spins & 255) == 255 && err && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
            __builtin_amdgcn_s_sleep(2);
          }
          if (!got && err) atomicExch(err, 7);
          val[gq] = (hi << 32) | (lo & 0xffffffffull);
        }
      }
      unsigned long long out;
      if (dtype == 1) { double a = 0.0; for (int gq = 0; gq < G; gq++) a += __longlong_as_double((long long)val[gq]); out = (unsigned long long)__double_as_longlong(a); }
      else if (dtype == 2) { long long a = (long long)val[0]; for (int gq = 1; gq < G; gq++) a = min(a, (long long)val[gq]); out = (unsigned long long)a; }
      else { long long a = 0; for (int gq = 0; gq < G; gq++) a += (long long)val[gq]; out = (unsigned long long)a; }
      buf[i] = out;
    }
  }
}
// LARGE buffers (the ridge statistics of many-level designs: Q K (d + 1) doubles, 10 MB at BASELINE configs[4]) through the same inboxes as
// reduce-scatter + all-gather: the one-shot form above would push every rank's WHOLE buffer over each of its links; here entry e of a
// window belongs to rank e / S (S = P2P_CAP / 2 entries per rank and window): (1) every rank sends its value of e to the owner only, (2) the owner
// adds the G values in RANK ORDER (fp64 sums identical on every rank) and sends the result to everybody, (3) the others pick it up -- 2 (G - 1) / G
// of the buffer per link instead of (G - 1) times it, many workgroups wide.  Inbox layout per (plane, source): entries [0, S) carry the
// scattered values, [S, 2 S) the gathered results; planes and tags as k_p2p_allreduce (one call = one window = one `seq`).  Three separate
// sweeps, so no thread waits while a peer still needs one of its sends; every spin is bounded (err = 7).
__device__ __forceinline__ void p2p_send_to(const Dev& D, int peer, size_t par, int i, unsigned tag, unsigned long long v) {
  const unsigned long long tb = (unsigned long long)tag << 32;
  const unsigned long long lo = tb | (v & 0xffffffffull), hi = tb | (v >> 32);
#pragma unroll
  for (int gq = 0; gq < 8; gq++) if (gq == peer) {       // (static indices only: a dynamic one would spill the kernarg copy)
    unsigned long long* dst = D.p2p_inbox[gq] + ((par + D.p2p_rank) * P2P_CAP + i) * 2;
    __hip_atomic_store(dst, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(dst + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
__device__ __forceinline__ unsigned long long p2p_wait(const Dev& D, size_t par, int src_rank, int i, unsigned tag, int* err) {
  const unsigned long long* src = D.p2p_inbox_self() + ((par + src_rank) * P2P_CAP + i) * 2;
  unsigned long long lo = 0, hi = 0;
  bool got = false;
  // bounded by the wall clock, not by a spin count: the windows of a large buffer follow rank-local phases of very different length (ridge
  // statistics of a 10M-cell shard), so a peer may legitimately arrive seconds late; wall_clock64 ticks at 100 MHz: 3 s, as the self-test
  const unsigned long long t_in = wall_clock64();
  for (int spins = 0;; spins++) {
    lo = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    hi = __hip_atomic_load(src + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if ((unsigned)(lo >> 32) == tag && (unsigned)(hi >> 32) == tag) { got = true; break; }
    if ((spins & 255) == 255) {
      if (err && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
      if (wall_clock64() - t_in > 300000000ull) break;
    }
    __builtin_amdgcn_s_sleep(2);
  }
  if (!got && err) atomicExch(err, 7);
  return (hi << 32) | (lo & 0xffffffffull);
}
__global__ void __launch_bounds__(1024) k_p2p_allreduce_big(Dev D, unsigned long long* __restrict__ buf, int n, int dtype, unsigned seq, int* err) {
  const int G = D.p2p_world, me = D.p2p_rank;
  constexpr int S = P2P_CAP / 2;
  const unsigned tag = 0x40000000u + (seq & 0x3fffffffu);
  const size_t par = (size_t)(2 + (seq & 1u)) * 8;
  const int t0 = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
  for (int e = t0; e < n; e += nt) {                       // (1) scatter: my value of every entry another rank owns
    const int owner = e / S;
    if (owner != me) p2p_send_to(D, owner, par, e - owner * S, tag, buf[e]);
  }
  for (int l = t0; l < S; l += nt) {                       // (2) my slice: reduce in rank order, gather out
    const int e = me * S + l;
    if (e >= n) break;
    unsigned long long val[8];
#pragma unroll
    for (int gq = 0; gq < 8; gq++) { val[gq] = buf[e]; if (gq < G && gq != me) val[gq] = p2p_wait(D, par, gq, l, tag, err); }
    unsigned long long out;
    if (dtype == 1) { double a = 0.0; for (int gq = 0; gq < G; gq++) a += __longlong_as_double((long long)val[gq]); out = (unsigned long long)__double_as_longlong(a); }
    else if (dtype == 2) { long long a = (long long)val[0]; for (int gq = 1; gq < G; gq++) a = min(a, (long long)val[gq]); out = (unsigned long long)a; }
    else { long long a = 0; for (int gq = 0; gq < G; gq++) a += (long long)val[gq]; out = (unsigned long long)a; }
    buf[e] = out;
#pragma unroll
    for (int gq = 0; gq < 8; gq++) if (gq < G && gq != me) p2p_send_to(D, gq, par, S + l, tag, out);
  }
  for (int e = t0; e < n; e += nt) {                       // (3) the other ranks' slices
    const int owner = e / S;
    if (owner != me) buf[e] = p2p_wait(D, par, owner, S + (e - owner * S), tag, err);
  }
}
#endif  // !HMX_TILE_BF

// counter-based generators -- same SPEC as include/harmony_mi355x.h documents
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}
struct FeistelKeys { uint32_t k[6]; int half; uint32_t mask; };
__host__ __device__ __forceinline__ uint64_t feistel_apply(const FeistelKeys& fk, uint64_t N, uint64_t g) {
  uint64_t x = g;
  do {
    uint32_t L = (uint32_t)(x >> fk.half), Rr = (uint32_t)(x & fk.mask);
#pragma unroll
    for (int r = 0; r < 6; r++) {
      uint32_t t = L ^ (fmix32(Rr * 0x9E3779B1u + fk.k[r]) & fk.mask);
      L = Rr; Rr = t;
    }
    x = ((uint64_t)L << fk.half) | Rr;
  } while (x >= N);
  return x;
}
static FeistelKeys make_keys(uint64_t seed, uint64_t round, uint64_t N) {
  FeistelKeys fk;
  int bits = 2;
  while (((uint64_t)1 << bits) < N) bits += 2;
  fk.half = bits / 2;
  fk.mask = (uint32_t)(((uint64_t)1 << fk.half) - 1);
  for (int r = 0; r < 6; r++)
    fk.k[r] = (uint32_t)(splitmix64(seed ^ (round * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)(r + 1) << 56)) >> 32);
  return fk;
}

// Stage the centroid table Yt[d][K] into LDS as [d][KP] (zero padded), k fastest:
// lane l then reads ldsY[j*KP + l + 64q] -- consecutive dwords, conflict-free.
__device__ __forceinline__ void stage_Y(float* ldsY, const float* __restrict__ Yt, int d, int K, int KP) {
  for (int i = threadIdx.x; i < d * KP; i += blockDim.x) {
    int j = i / KP, k = i - j * KP;
    ldsY[i] = ld_or(Yt, (size_t)j * K + min(k, K - 1), k < K, 0.0f);
  }
  __syncthreads();
}

// dots of CB cells (rows broadcast from lanes) with all clusters of this lane.
template <int KPL, int DPL, int CB>
__device__ __forceinline__ void group_dots(const float* __restrict__ ldsY, int d, int KP, int lane,
                                           const float (&z)[CB][DPL], float (&acc)[CB][KPL]) {
#pragma unroll
  for (int c = 0; c < CB; c++)
#pragma unroll
    for (int q = 0; q < KPL; q++) acc[c][q] = 0.0f;
  const int d0 = d < 64 ? d : 64;
  for (int j = 0; j < d0; ++j) {
    float y[KPL];
#pragma unroll
    for (int q = 0; q < KPL; q++) y[q] = ldsY[j * KP + lane + 64 * q];
#pragma unroll
    for (int c = 0; c < CB; c++) {
      const float zj = rlane(z[c][0], j);
#pragma unroll
      for (int q = 0; q < KPL; q++) acc[c][q] = fmaf(zj, y[q], acc[c][q]);
    }
  }
  if constexpr (DPL > 1) {
    for (int j = 64; j < d; ++j) {
      float y[KPL];
#pragma unroll
      for (int q = 0; q < KPL; q++) y[q] = ldsY[j * KP + lane + 64 * q];
#pragma unroll
      for (int c = 0; c < CB; c++) {
        const float zj = rlane(z[c][DPL - 1], j - 64);
#pragma unroll
        for (int q = 0; q < KPL; q++) acc[c][q] = fmaf(zj, y[q], acc[c][q]);
      }
    }
  }
}

template <int DPL>
__device__ __forceinline__ void load_row(const float* __restrict__ Z, size_t cell, int zs, int d, int lane, float (&z)[DPL]) {
  z[0] = ld_or(Z, cell * zs + min(lane, d - 1), lane < d, 0.0f);
  if constexpr (DPL > 1) z[DPL - 1] = ld_or(Z, cell * zs + min(64 + lane, d - 1), 64 + lane < d, 0.0f);
}

// flush a lane-private fixed-point run sum into a [B][K] table, once per covariate level
template <int KPL>
__device__ __forceinline__ void flush_fx(long long* __restrict__ tab, const int* __restrict__ qlev, int q, int C,
                                         int K, int lane, unsigned long long (&oacc)[KPL]) {
  for (int c = 0; c < C; c++) {
    const int b = qlev[q * C + c];
#pragma unroll
    for (int qq = 0; qq < KPL; qq++) {
      const int k = lane + 64 * qq;
      if (k < K && oacc[qq]) atomicAdd((unsigned long long*)&tab[(size_t)b * K + k], oacc[qq]);
    }
  }
#pragma unroll
  for (int qq = 0; qq < KPL; qq++) oacc[qq] = 0ull;
}

// --------------------------------------------------------------------------------------
// ingest / egress
// The kernels live in four include files (one translation unit: they share the helpers above and each other's device functions):
//   hmx_k_stream.inc   ingest / egress, shuffle and sort, old-contribution passes, fold / penalty, round tail, first-generation kernels
//   hmx_k_tile.inc     the MFMA tile machinery and k_tile (block update, head, Lloyd, seeding, persistent chain) -- also built by hmx_tile_bf.hip
//   hmx_k_correct.inc  objective tables / terms, MoE ridge correction (statistics, solve, apply), VALU fallbacks
//   hmx_k_launch.inc   launchers (no kernels; a k_tile launch is planned in hmx_plan.h) -- its dispatch_k_tile also built by hmx_tile_bf.hip (the peer-inbox kernels sit beside p2p_send above)
#include "hmx_k_stream.inc"
#include "hmx_k_tile.inc"
#include "hmx_k_correct.inc"
#include "hmx_k_launch.inc"
}  // namespace hmx

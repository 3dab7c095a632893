// hmx_k_tile.inc -- part of hmx_kernels.hip AND of hmx_tile_bf.hip (included inside namespace hmx): the MFMA tile machinery -- distance GEMM in its fp32 and
// split-bf16 forms, the contribution flush -- and k_tile itself: block update, head, Lloyd iteration, seeding race, persistent block chain (MODE 0..5).
// --------------------------------------------------------------------------------------
// MFMA tile variant of the block update (the dominant kernel).
//
// One wave owns tiles of 16 gathered cells.  dist(16 cells x 16 clusters) accumulates on the
// matrix cores with v_mfma_f32_16x16x4_f32 (exact fp32, k-ordered fma chain):
//   A = the cells' embedding rows   lane l supplies A[cell = l&15][k-slot = l>>4]
//   B = centroids                   lane l supplies B[k-slot = l>>4][cluster = l&15]
//   D                               lane l holds   D[cell = 4*(l>>4)+reg][cluster = l&15]
// PCs are assigned to k-slots so that every lane fetches its A operands with 16-byte loads:
// in float4 group t the lane with slot p holds PCs 16t+4p+{0..3}, used in steps 4t+{0..3};
// the centroid image D.Yimg is laid out on the host in exactly that order (and as float4 per
// lane per step -> conflict-free ds_read_b128).  The softmax normalisations are 16-lane DPP
// row reductions, the penalty is a per-run register vector, O is accumulated per lane in
// 64-bit fixed point and flushed once per run of equal covariate combination.
// --------------------------------------------------------------------------------------

__device__ __forceinline__ float dpp_f(float v, const int ctrl_id) {
  // ctrl_id: 0 quad_perm[1,0,3,2]  1 quad_perm[2,3,0,1]  2 row_half_mirror  3 row_mirror
  // (old = 0 + bound_ctrl: every source lane is in range, and this form lets hipcc fold the move into v_add_f32_dpp)
  const int x = __float_as_int(v);
  int r;
  switch (ctrl_id) {
    case 0: r = __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true); break;
    case 1: r = __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true); break;
    case 2: r = __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true); break;
    default: r = __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, true); break;
  }
  return __int_as_float(r);
}
// sum over the 16 lanes of a DPP row (lanes sharing l>>4); every lane gets the total
__device__ __forceinline__ float rowsum16(float v) {
  v += dpp_f(v, 0);
  v += dpp_f(v, 1);
  v += dpp_f(v, 2);
  v += dpp_f(v, 3);
  return v;
}

// arma::normalise(Z, 2, 0) with 16-byte accesses: 16 lanes per row (lane c: float4 c [and c + 16]), four rows per wave instruction, four
// instructions in flight; the row's sum of squares is a 16-lane DPP reduction.  Rows are zero beyond d (zs = d rounded up to 4).
template <int NF>
__global__ __launch_bounds__(TPB) void k_normalize4(const float* Zsrc, float* Z, int n, int nq) {   // Zsrc == Z: in place
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (long long base = (long long)wave * 16; base < n; base += (long long)nw * 16) {
    f32x4 v[4][NF];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const long long cell = min(base + 4 * u + g, (long long)n - 1);
      const f32x4* row = reinterpret_cast<const f32x4*>(Zsrc) + cell * nq;
#pragma unroll
      for (int f = 0; f < NF; f++) v[u][f] = row[min(c + 16 * f, nq - 1)];
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      float ss = 0.0f;
#pragma unroll
      for (int f = 0; f < NF; f++) {
        if (c + 16 * f >= nq) v[u][f] = zero4;
        ss += v[u][f][0] * v[u][f][0] + v[u][f][1] * v[u][f][1] + v[u][f][2] * v[u][f][2] + v[u][f][3] * v[u][f][3];
      }
      float nrm = sqrtf(rowsum16(ss));
      if (nrm == 0.0f) nrm = 1.0f;
      const long long cell = base + 4 * u + g;
      if (cell < n) {
        f32x4* row = reinterpret_cast<f32x4*>(Z) + cell * nq;
#pragma unroll
        for (int f = 0; f < NF; f++)
          if (c + 16 * f < nq) { f32x4 o; for (int e = 0; e < 4; e++) o[e] = v[u][f][e] / nrm; row[c + 16 * f] = o; }
      }
    }
  }
}

// N independent row sums, the DPP steps interleaved (ILP N: see epi_rows)
template <int N>
__device__ __forceinline__ void rowsum16xN(float (&v)[N]) {
#pragma unroll
  for (int st = 0; st < 4; st++) {
    float t[N];
#pragma unroll
    for (int i = 0; i < N; i++) t[i] = (st == 0) ? dpp_f(v[i], 0) : (st == 1) ? dpp_f(v[i], 1) : (st == 2) ? dpp_f(v[i], 2) : dpp_f(v[i], 3);
#pragma unroll
    for (int i = 0; i < N; i++) v[i] += t[i];
  }
}

template <int NCT>
__device__ __forceinline__ void tile_dots(const f32x4* __restrict__ ldsY4, const float* __restrict__ zrow, bool valid,
                                          int g, int lane, int NS, int NT4, int tail, f32x4 (&acc)[NCT],
                                          bool have_first = false, f32x4 zfirst = f32x4{0.f, 0.f, 0.f, 0.f}) {
  constexpr int NQ = (NCT + 3) / 4;
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  // zrow always points at a real row (row 0 for padding lanes): unconditional loads, masked afterwards
  f32x4 zt = zero4;
  if (have_first) zt = zfirst;                  // fetched by the caller before its LDS-staging barrier
  else if (NT4 > 0) zt = *reinterpret_cast<const f32x4*>(zrow + 4 * g);
  for (int t = 0; t < NT4; ++t) {
    const f32x4 zc = valid ? zt : zero4;
    if (t + 1 < NT4) zt = *reinterpret_cast<const f32x4*>(zrow + 16 * (t + 1) + 4 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int s = 4 * t + e;
#pragma unroll
      for (int qd = 0; qd < NQ; ++qd) {
        const f32x4 y = ldsY4[(qd * NS + s) * 64 + lane];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (4 * qd + i < NCT) acc[4 * qd + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(zc[e], y[i], acc[4 * qd + i], 0, 0, 0);
      }
    }
  }
  for (int u = 0; u < tail; ++u) {
    const int s = 4 * NT4 + u;
    const float zl = zrow[16 * NT4 + 4 * u + g];
    const float zv = valid ? zl : 0.0f;
#pragma unroll
    for (int qd = 0; qd < NQ; ++qd) {
      const f32x4 y = ldsY4[(qd * NS + s) * 64 + lane];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (4 * qd + i < NCT) acc[4 * qd + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(zv, y[i], acc[4 * qd + i], 0, 0, 0);
    }
  }
}

// LDS-DMA: every lane copies 16 bytes from its own global address to  lds_base + lane * 16  (wave-uniform base) without
// touching a VGPR; completion is counted by vmcnt like an ordinary load.
__device__ __forceinline__ void glds16(const float* gsrc, f32x4* lds_base) {
  // inline asm on purpose: with the builtin hipcc treats the DMA as a store to LDS and drains it (vmcnt(0)) in front of the next
  // LDS read -- the epilogue's penalty-table reads -- which exposes the whole copy latency.  The asm statement is invisible
  // to the wait-count pass; the caller waits with a counted s_waitcnt (the copies are older than everything it leaves in flight).
  // M0 = wave-uniform LDS byte address of the destination; written and restored inside the statement (compiler-reserved).
  const unsigned lds_dst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)(uintptr_t)lds_base));
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void glds4(const int* gsrc, int* lds_base) {   // 4 bytes per lane, same contract as glds16
  const unsigned lds_dst = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)(uintptr_t)lds_base));
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
// the MFMA chain of one tile with the A operands in an LDS image filled by glds16: group t < NT4 holds each lane's PCs
// 16t+4g..+3, group NT4+u the 16 bytes at PC 16*NT4+4u (the same for the four k-slot lanes of a cell: lane g uses component g)
template <int NCT>
__device__ __forceinline__ void tile_dots_lds(const f32x4* __restrict__ ldsY4, const f32x4* __restrict__ rows, bool valid, int g,
                                              int lane, int NS, int NT4, int tail, f32x4 (&acc)[NCT]) {
  constexpr int NQ = (NCT + 3) / 4;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) acc[ct] = zero4;
  for (int t = 0; t < NT4; ++t) {
    const f32x4 zl = rows[t * 64 + lane];
    const f32x4 zc = valid ? zl : zero4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int s = 4 * t + e;
#pragma unroll
      for (int qd = 0; qd < NQ; ++qd) {
        const f32x4 y = ldsY4[(qd * NS + s) * 64 + lane];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (4 * qd + i < NCT) acc[4 * qd + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(zc[e], y[i], acc[4 * qd + i], 0, 0, 0);
      }
    }
  }
  for (int u = 0; u < tail; ++u) {
    const int s = 4 * NT4 + u;
    const f32x4 zl = rows[(NT4 + u) * 64 + lane];
    const float zg = (g == 0) ? zl[0] : (g == 1) ? zl[1] : (g == 2) ? zl[2] : zl[3];
    const float zv = valid ? zg : 0.0f;
#pragma unroll
    for (int qd = 0; qd < NQ; ++qd) {
      const f32x4 y = ldsY4[(qd * NS + s) * 64 + lane];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (4 * qd + i < NCT) acc[4 * qd + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(zv, y[i], acc[4 * qd + i], 0, 0, 0);
    }
  }
}

// A-operand rows of one tile held in registers (d <= 76: at most 4 float4 groups + 3 single steps), so that the rows of
// tile i+1 can be requested while tile i is computed.  Loads are unconditional with clamped offsets (see ld_or).
struct RowRegs { f32x4 v[4]; float t[3]; };
__device__ __forceinline__ void load_rows(const float* __restrict__ zrow, int g, int NT4, int tail, RowRegs& r) {
  const int tmax = NT4 > 0 ? NT4 - 1 : 0, umax = tail > 0 ? tail - 1 : 0;
  if (NT4 > 0) {
#pragma unroll
    for (int t = 0; t < 4; t++) r.v[t] = *reinterpret_cast<const f32x4*>(zrow + 16 * min(t, tmax) + 4 * g);
  }
  if (tail > 0) {
#pragma unroll
    for (int u = 0; u < 3; u++) r.t[u] = zrow[16 * NT4 + 4 * min(u, umax) + g];
  }
}
template <int NCT>
__device__ __forceinline__ void tile_dots_regs(const f32x4* __restrict__ ldsY4, const RowRegs& r, bool valid, int lane,
                                               int NS, int NT4, int tail, f32x4 (&acc)[NCT]) {
  constexpr int NQ = (NCT + 3) / 4;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) acc[ct] = zero4;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t < NT4) {
      const f32x4 zc = valid ? r.v[t] : zero4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int s = 4 * t + e;
#pragma unroll
        for (int qd = 0; qd < NQ; ++qd) {
          const f32x4 y = ldsY4[(qd * NS + s) * 64 + lane];
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (4 * qd + i < NCT) acc[4 * qd + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(zc[e], y[i], acc[4 * qd + i], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    if (u < tail) {
      const int s = 4 * NT4 + u;
      const float zv = valid ? r.t[u] : 0.0f;
#pragma unroll
      for (int qd = 0; qd < NQ; ++qd) {
        const f32x4 y = ldsY4[(qd * NS + s) * 64 + lane];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (4 * qd + i < NCT) acc[4 * qd + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(zv, y[i], acc[4 * qd + i], 0, 0, 0);
      }
    }
  }
}

// ---- split-bf16 form of the distance GEMM ---------------------------------------------------------------------------------------
// v_mfma_f32_16x16x4_f32 runs at the fp32 VECTOR rate on gfx950 (32 cycles per SIMD, on the datapath the epilogue's VALU work needs);
// v_mfma_f32_16x16x32_bf16 takes ~17 cycles for 8x the products on the matrix cores proper.  With x = hi + mid + lo (three bf16 parts,
// exact: bf3_split) the 16 x 16 x 32 product of fp32 operands is six bf16 MFMAs (the three dropped cross terms are < 2^-21 |x||y| at worst, ~2^-24 typically: hmx_internal.h),
// fp32 accumulation: 12 NCT MFMAs per 64 PCs instead of 16 NCT per 64, at half the cycles each, and VALU work of the SIMD's other
// wave overlaps them.  A operand (cells): lane (c, g) holds PCs 32 s + 8 g + {0..7} of cell c in step s -- two 16-byte loads -- and
// splits them in registers (5.5 VALU per value); B operand (centroids): the three parts from the LDS image D.Yimg3, one ds_read_b128 each.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
struct Bf3 { u32x4 p[3]; };
__device__ __forceinline__ Bf3 bf3_split8(const f32x4 lo4, const f32x4 hi4) {
  Bf3 o;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float x0 = i < 2 ? lo4[2 * i] : hi4[2 * i - 4], x1 = i < 2 ? lo4[2 * i + 1] : hi4[2 * i - 3];
    const unsigned u0 = __float_as_uint(x0), u1 = __float_as_uint(x1);
    const float r0 = x0 - __uint_as_float(u0 & 0xffff0000u), r1 = x1 - __uint_as_float(u1 & 0xffff0000u);
    const unsigned v0 = __float_as_uint(r0), v1 = __float_as_uint(r1);
    const float s0 = r0 - __uint_as_float(v0 & 0xffff0000u), s1 = r1 - __uint_as_float(v1 & 0xffff0000u);
    o.p[0][i] = __builtin_amdgcn_perm(u1, u0, 0x07060302u);      // { bf16(x0), bf16(x1) }: the upper halves
    o.p[1][i] = __builtin_amdgcn_perm(v1, v0, 0x07060302u);
    o.p[2][i] = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), 0x07060302u);
  }
  return o;
}
// one step (32 PCs) of all cluster tiles: smallest terms first
template <int NCT>
__device__ __forceinline__ void bf_step(const u32x4* __restrict__ ldsB, const Bf3& a, int s, int NS2, int lane, f32x4 (&acc)[NCT]) {
  auto mf = [](const u32x4 A, const u32x4 B, const f32x4 C) __attribute__((always_inline)) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, A), __builtin_bit_cast(bf16x8, B), C, 0, 0, 0);
  };
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) {
    const u32x4* b = ldsB + ((size_t)(ct * NS2 + s) * 3) * 64 + lane;
    const u32x4 b0 = b[0], b1 = b[64], b2 = b[128];
    f32x4 v = acc[ct];
    v = mf(a.p[0], b2, v);
    v = mf(a.p[2], b0, v);
    v = mf(a.p[1], b1, v);
    v = mf(a.p[0], b1, v);
    v = mf(a.p[1], b0, v);
    v = mf(a.p[0], b0, v);
    acc[ct] = v;
  }
}
// rows in registers: r.v[2 s + h] = the 16 bytes at PC 32 s + 8 g + 4 h (clamped into the row; rowmask bit 2 s + h = inside the row)
__device__ __forceinline__ void load_rows_bf(const float* __restrict__ zrow, int g, int zs, RowRegs& r) {
#pragma unroll
  for (int t = 0; t < 4; t++) r.v[t] = *reinterpret_cast<const f32x4*>(zrow + min(32 * (t >> 1) + 8 * g + 4 * (t & 1), zs - 4));
}
__device__ __forceinline__ int rows_mask_bf(int g, int zs) {
  int m = 0;
#pragma unroll
  for (int t = 0; t < 8; t++) m |= (32 * (t >> 1) + 8 * g + 4 * (t & 1) < zs) ? (1 << t) : 0;
  return m;
}
template <int NCT>
__device__ __forceinline__ void tile_dots_bf_regs(const u32x4* __restrict__ ldsB, const RowRegs& r, bool valid, int rowmask, int lane,
                                                  int NS2, f32x4 (&acc)[NCT]) {
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) acc[ct] = zero4;
  const int m = valid ? rowmask : 0;
#pragma unroll
  for (int s = 0; s < 2; s++) {
    if (s < NS2) {
      const Bf3 a = bf3_split8((m >> (2 * s)) & 1 ? r.v[2 * s] : zero4, (m >> (2 * s + 1)) & 1 ? r.v[2 * s + 1] : zero4);
      bf_step<NCT>(ldsB, a, s, NS2, lane, acc);
    }
  }
}
// TWO tiles against ONE read of the centroid image (round 5, the chain's hoisted MFMA phase): a wave that owns two tiles of a block used to
// walk the 42 KB image twice -- the LDS operand reads of a SIMD's three tiles were 1.6 of the 5.4 us the workers need behind an arrival
// (DESIGN 7.1); with both tiles' rows in registers every (cluster tile, step) operand triple is read once and feeds twelve MFMAs, two
// independent accumulator chains.
template <int NCT>
__device__ __forceinline__ void tile_dots_bf_regs2(const u32x4* __restrict__ ldsB, const RowRegs& ra, bool valida, const RowRegs& rb, bool validb,
                                                   int rowmask, int lane, int NS2, f32x4 (&acca)[NCT], f32x4 (&accb)[NCT]) {
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto mf = [](const u32x4 A, const u32x4 B, const f32x4 C) __attribute__((always_inline)) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, A), __builtin_bit_cast(bf16x8, B), C, 0, 0, 0);
  };
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) { acca[ct] = zero4; accb[ct] = zero4; }
  const int ma = valida ? rowmask : 0, mb = validb ? rowmask : 0;
#pragma unroll
  for (int s = 0; s < 2; s++) {
    if (s < NS2) {
      const Bf3 a = bf3_split8((ma >> (2 * s)) & 1 ? ra.v[2 * s] : zero4, (ma >> (2 * s + 1)) & 1 ? ra.v[2 * s + 1] : zero4);
      const Bf3 b = bf3_split8((mb >> (2 * s)) & 1 ? rb.v[2 * s] : zero4, (mb >> (2 * s + 1)) & 1 ? rb.v[2 * s + 1] : zero4);
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) {
        const u32x4* y = ldsB + ((size_t)(ct * NS2 + s) * 3) * 64 + lane;
        const u32x4 y0 = y[0], y1 = y[64], y2 = y[128];
        f32x4 va = acca[ct], vb = accb[ct];          // (the same order of the six terms as bf_step: smallest first -- bit-identical to the one-tile form)
        va = mf(a.p[0], y2, va); vb = mf(b.p[0], y2, vb);
        va = mf(a.p[2], y0, va); vb = mf(b.p[2], y0, vb);
        va = mf(a.p[1], y1, va); vb = mf(b.p[1], y1, vb);
        va = mf(a.p[0], y1, va); vb = mf(b.p[0], y1, vb);
        va = mf(a.p[1], y0, va); vb = mf(b.p[1], y0, vb);
        va = mf(a.p[0], y0, va); vb = mf(b.p[0], y0, vb);
        acca[ct] = va; accb[ct] = vb;
      }
    }
  }
}
// rows streamed from memory one step ahead (any NS2 <= 4)
template <int NCT>
__device__ __forceinline__ void tile_dots_bf(const u32x4* __restrict__ ldsB, const float* __restrict__ zrow, bool valid, int rowmask, int g,
                                             int lane, int NS2, int zs, f32x4 (&acc)[NCT]) {
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) acc[ct] = zero4;
  const int m = valid ? rowmask : 0;
  f32x4 c0 = *reinterpret_cast<const f32x4*>(zrow + min(8 * g, zs - 4)), c1 = *reinterpret_cast<const f32x4*>(zrow + min(8 * g + 4, zs - 4));
  for (int s = 0; s < NS2; s++) {
    const f32x4 a0 = (m >> (2 * s)) & 1 ? c0 : zero4, a1 = (m >> (2 * s + 1)) & 1 ? c1 : zero4;
    if (s + 1 < NS2) {
      c0 = *reinterpret_cast<const f32x4*>(zrow + min(32 * (s + 1) + 8 * g, zs - 4));
      c1 = *reinterpret_cast<const f32x4*>(zrow + min(32 * (s + 1) + 8 * g + 4, zs - 4));
    }
    const Bf3 a = bf3_split8(a0, a1);
    bf_step<NCT>(ldsB, a, s, NS2, lane, acc);
  }
}

__device__ __forceinline__ unsigned long long shfl_u64(unsigned long long v, int srclane) {
  const unsigned lo = (unsigned)__shfl((int)(unsigned)v, srclane, 64), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), srclane, 64);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
  const unsigned lo = __shfl_xor((unsigned)(v & 0xffffffffu), m, 64);
  const unsigned hi = __shfl_xor((unsigned)(v >> 32), m, 64);
  return ((unsigned long long)hi << 32) | lo;
}
// The four 16-lane groups of a wave hold partial sums of the SAME clusters (different cells): add them
// first, then one atomic per cluster from group 0 -- into one of several table replicas, so that the
// hundreds of waves of a launch do not serialise on the same few L2 atomic addresses.
template <int NCT>
__device__ __forceinline__ void flush_tile_fx(long long* __restrict__ tab, long long* __restrict__ tab2, const int* __restrict__ qlev, int q, int C,
                                              int K, int KS, int c, int g, unsigned long long (&oacc)[NCT]) {      // (K: clusters this wave holds; KS: row stride of the tables)
  constexpr int NFULL = NCT >> 2, RT = NCT & 3, NG = NFULL + (RT ? 1 : 0);
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) {
    unsigned long long v = oacc[ct];
    v += shfl_xor_u64(v, 16);
    v += shfl_xor_u64(v, 32);
    oacc[ct] = v;
  }
  // Every lane now holds the sums of its clusters (kcol: 4c+{0..3} of a quad).  Redistribute so that lane (g, c) owns cluster
  // 64 G + 16 g + c of group G: ONE atomic instruction per group and level with all 64 lanes on consecutive addresses, instead of
  // one per cluster tile with 16 lanes.
  const int kk = 16 * g + c;
  unsigned long long mine[NG];
#pragma unroll
  for (int G = 0; G < NG; G++) {
    const int RG = (G < NFULL) ? 4 : RT;
    const int src = min(kk / RG, 15), jsel = kk - (kk / RG) * RG;
    unsigned long long v = 0ull;
#pragma unroll
    for (int jj = 0; jj < RG; jj++) {
      const unsigned long long t = shfl_u64(oacc[4 * G + jj], 16 * g + src);
      v = (jsel == jj) ? t : v;
    }
    mine[G] = (kk < 16 * RG) ? v : 0ull;
  }
  for (int cc = 0; cc < C; cc++) {
    const int b = qlev[q * C + cc];
#pragma unroll
    for (int G = 0; G < NG; G++) {
      const int k = 64 * G + kk;
      if (k < K && mine[G]) {
        atomicAdd((unsigned long long*)&tab[(size_t)b * KS + k], mine[G]);
        // the same sums are the cells' OLD contribution to their block of the NEXT round (tiles are keyed by it, D.Sold_next)
        if (tab2) atomicAdd((unsigned long long*)&tab2[(size_t)b * KS + k], mine[G]);
      }
    }
  }
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) oacc[ct] = 0ull;
}

// Instantiated cluster-tile counts are {1..8,10,12,13,14,16} (hmx_setup picks the smallest >= ceil(K/16)): cluster tiles
// below this index are always completely inside K, only the ones from it on can hold k >= K.
// (cluster tiles are grouped in quads by kcol: the tiles of the last group can hold k >= K)
constexpr int first_partial_ct(int nct) { return (nct & 3) ? 4 * (nct >> 2) : 4 * ((nct >> 2) - 1); }
// MODE 0: block update (cells gathered through lpair, penalty in the exponent, ONE normalisation)  update_R :318-330
// MODE 1: head (static 16-cell tiles of the internal order, plain softmax)                 :141-150 / :221-227
// Register budget: K > 64 runs 2 waves per SIMD (<= 256 VGPRs: row prefetch + two accumulator sets, K <= 112);
// K <= 64 with a uniform sigma runs the 128-VGPR variant (WPS = 4).
// MODE 2: one Lloyd iteration of kmeans_centers (nearest centre, fixed-point sums in LDS)  src/utils.cpp:56-61
// MODE 3: the seeding race of kmeans_centers: for every anchor k  argmin_n -log(u_kn) / |2(1 - y_k.x_n)|  src/utils.cpp:24-34
// MODE 4: the WHOLE block chain of one update_R round in ONE persistent launch (one workgroup per CU): the workers run MODE 0's
//         tile pipeline for block j, arrive on a counter, and -- while a dedicated folder workgroup folds the block's
//         contribution into O and publishes the next penalty table -- already gather the rows and run the MFMAs of their
//         first tile of block j+1.  Only  + log2 pen -> exp2 -> normalise -> store -> flush  stays on the chain's critical
//         path; the centroid image is staged once per round instead of once per block step.
// MODE 6: the block chain for 112 < K <= 224 (BASELINE configs[4]: K = 200) by WAVE PAIRS: waves 2p and 2p + 1 of a workgroup (two SIMDs) own
//         the same tiles, each runs MODE 4's worker on one half of the clusters ([0, KH) / [KH, K), NCT = cluster tiles of a half) and the two halves of a
//         row's normalisation sum meet through LDS (pair_sum); the K x B table (40 000 entries at configs[4]: no LDS holds it) is folded by several folder
//         workgroups, a slice of clusters each, and the block's penalty rows are read per level from memory (write-through stores, drained counter).
// WPS: waves per SIMD the register budget is cut for (update workgroup = 256*WPS threads).  USIG: one sigma for all clusters
// (the reference's default, R/ui.R:219-221): ce / cl become scalars, 2-3 register arrays of NCT floats disappear.
template <int NCT, int MODE, int WPS = 2, bool USIG = false, bool BF = (HMX_TILE_BF != 0)>
__global__ __launch_bounds__(256 * WPS) void k_tile(Dev D, int j) {
  constexpr bool LEAN = WPS > 3;       // (WPS = 3: the two-waves-per-SIMD code at a 170-register budget -- Lloyd's 768-thread workgroups, round 6)
  constexpr bool CHAIN = (MODE == 4 || MODE == 5 || MODE == 6);     // MODE 5: the chain of a round whose R rows nobody reads (Dev::r_store == 0), see below
  constexpr bool NOSTORE = (MODE == 5);
  constexpr bool PAIR = (MODE == 6);
  // ONE LDS object (a second __shared__ object de-pipelines hipcc's waits):
  //   [ centroid image: NQ*NS*64 float4 | MODE 0: pen[B][K] + qlev[Q][C] (if they fit) | MODE 2: int64 sums[K][d] + counts[K] ]
  extern __shared__ __attribute__((aligned(16))) f32x4 lds4[];
  const int KS = D.K, C = D.C, zs = D.zs;          // KS: row stride of R and of the K x B tables
  // MODE 6: this wave's half of the clusters -- kb its first cluster, K their number (every index below is relative to kb)
  // (the pair = waves 2p and 2p + 1 of the workgroup, on DIFFERENT SIMDs: the two halves of a tile run side by side, and the two waves a SIMD hosts belong
  //  to different pairs -- independent streams whose MFMA and VALU phases overlap; with both waves of a pair on one SIMD they ran in lockstep)
  const int kh = PAIR ? __builtin_amdgcn_readfirstlane((int)((threadIdx.x >> 6) & 1)) : 0;
  const int kb = (PAIR && kh) ? D.KH : 0;
  const int K = PAIR ? (kh ? D.K - D.KH : D.KH) : D.K;
  const int nY4 = BF ? NCT * D.NS2 * 3 * 64 : D.NQ * D.NS * 64;     // 16-byte entries of the centroid image (f32 steps | three bf16 parts); MODE 6: of one half's
  const int nYall = PAIR ? 2 * nY4 : nY4;
  const u32x4* const ldsB = reinterpret_cast<const u32x4*>(lds4) + (PAIR ? kh * nY4 : 0);
  // MODE 0 with D.fused_fold: [ image | O' int64 [B][K] | pen | qlev ] -- the fold + penalty of this block step is
  // recomputed by EVERY workgroup in its own LDS (k_foldpen's launch and its boundary disappear); workgroup 0 also
  // publishes O' and zeroes the replica set of the NEXT launch (three sets rotate, so nobody reads what is zeroed).
  const int nBK = D.B * KS;
  long long* ldsO = reinterpret_cast<long long*>(lds4 + nY4);
  float* ldsPen = ((MODE == 0 && D.fused_fold) || CHAIN) ? reinterpret_cast<float*>(ldsO + nBK) : reinterpret_cast<float*>(lds4 + nY4);
  int* ldsQlev = PAIR ? reinterpret_cast<int*>(lds4 + nYall) : reinterpret_cast<int*>(ldsPen + ((nBK + 3) & ~3));      // (MODE 6: [ both images | qlev | exchange slots ])
  // MODE 6: the pair's exchange slots, [4 pairs][2 parities][2 halves][16 rows] x { sequence number << 32 | float bits }
  unsigned long long* const ldsX = reinterpret_cast<unsigned long long*>(ldsQlev + ((D.Q * C + 3) & ~3));
  long long* ltab = reinterpret_cast<long long*>(lds4 + nY4);
  constexpr bool UPD = (MODE == 0 || CHAIN);   // block update modes (gathered cells, penalty, O contributions)
  int p0 = 0, ntiles;
  if constexpr (MODE == 0) { p0 = D.boff[j]; ntiles = (D.boff[j + 1] - p0) >> 4; }  // padded: combination-pure tiles
  else if constexpr (CHAIN) { p0 = D.boff[0]; ntiles = (D.boff[1] - p0) >> 4; }
  else if (MODE == 1 && D.head_gather) ntiles = D.boff[D.nb] >> 4;     // the head runs over the NEXT round's padded order (see flush_run)
  else ntiles = D.ntitems;
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  // wave index as a SCALAR: tile numbers and all loop control become SALU work (no exec-mask branches in the tile loop)
  // (MODE 4: the last workgroup is the folder, the others are the workers)
  const int nfold = PAIR ? D.chain_folders : (CHAIN ? 1 : 0);      // folder workgroups at the end of the grid
  // (MODE 6: a tile stream = a wave PAIR -- waves 2p and 2p + 1 of a workgroup --, four streams per workgroup)
  const int nw = PAIR ? ((int)gridDim.x - nfold) * 4 : (((gridDim.x - nfold) * blockDim.x) >> 6);
  // (streams numbered pair-major: the streams that take the extra tile of a block -- the lowest numbers, chain_range -- are the FIRST pair of as many
  //  workgroups as possible, one per workgroup, instead of all four streams of the first workgroups: 7 instead of 8 half-tile epilogues on the busiest SIMDs)
  int wave_ = PAIR ? (int)(threadIdx.x >> 7) * ((int)gridDim.x - nfold) + (int)blockIdx.x : (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if constexpr (CHAIN && !PAIR) {
    // tiles are dealt t = wave + i * nw, so the waves with the low indices get the extra tile of a block: number the first
    // wave of every SIMD (all workgroups) before the second ones, and each SIMD hosts one heavy and one light wave -- the
    // same tile count on every SIMD instead of 4 tiles on half the CUs and 2 on the others
    const int wpg = (int)blockDim.x >> 6, wib = (int)threadIdx.x >> 6, half = wpg >> 1, nwg = (int)gridDim.x - 1;
    // (second waves numbered workgroup-minor: the few SIMDs that must take a fourth tile are spread one per workgroup instead of
    //  filling whole CUs -- a CU's store / atomic queues are shared by its SIMDs)
    if (half >= 1) wave_ = (wib < half) ? (int)blockIdx.x * half + wib : nwg * half + (wib - half) * nwg + (int)blockIdx.x;
  }
  const int wave = __builtin_amdgcn_readfirstlane(wave_);
  auto stamp = [&](int slot) {  // diagnostics build only (-DHMX_TRACE, tools/trace_update.py): per-wave phase stamps
#ifdef HMX_TRACE
    if constexpr (MODE == 0) {
      if (D.trace && lane == 0) D.trace[(size_t)wave * 16 + slot] = (slot == 0 || slot == 7) ? wall_clock64() : __builtin_readcyclecounter();
    }
#endif
  };
  stamp(0); stamp(1);
  // MODE 0 (short launches, grid capped at the resident capacity): tiles are dealt round-robin, tile = wave + i*nw, so
  // every wave gets 1-2 tiles and no CU runs a second round of workgroups.  Static modes: contiguous ranges.
  // (dealing tiles workgroup-major instead -- equal tiles per CU -- measured 25% SLOWER: the 8 consecutive tiles of a
  //  workgroup share lorder/lcombo cache lines and the lighter half of the CUs finishing early helps the tail)
  const int per = (ntiles + nw - 1) / nw;
  // MODE 0 with many tiles per wave (D.upd_contig): contiguous ranges -- consecutive tiles share their (combination, next block)
  // key, so the wave flushes its O contributions once per RUN of tiles instead of once per tile (the flush atomics were 15 % of
  // a 10M-cell block step once every tile filed its sums twice, see flush_run)
  // MODE 4 (two-accumulator chain): contiguous BALANCED ranges, re-derived for every block -- T = base nw + rem tiles: the rem
  // lowest-numbered waves own base + 1 consecutive tiles, the others base.  A wave's tiles of a block are neighbours in the padded
  // order: they mostly share their (combination, next block) key, i.e. one contribution flush and one penalty fetch per wave and
  // block instead of one per tile, and their pair loads share cache lines.
  constexpr bool CHAIN_CONTIG = (CHAIN) && !LEAN;
  auto chain_range = [&](const int T, int& s0, int& e0) {
    const int base = T / nw, rem = T - base * nw;
    s0 = wave * base + min(wave, rem);
    e0 = s0 + base + (wave < rem ? 1 : 0);
  };
  const bool strided = (CHAIN && !CHAIN_CONTIG) || (MODE == 0 && !D.upd_contig);
  int ts = strided ? wave : wave * per;
  int te = strided ? ntiles : min(ntiles, ts + per);     // (MODE 4 re-derives it for every block)
  if constexpr (CHAIN_CONTIG) chain_range(ntiles, ts, te);
  if (CHAIN && (int)blockIdx.x >= (int)gridDim.x - nfold) te = ts;   // the folders own no tiles
  const int tstep = strided ? nw : 1;
  // MODE 0: the first tile's cell ids and the first 16 bytes of their embedding rows are requested BEFORE the
  // LDS staging below, so the two dependent HBM round trips overlap with it
  // Software pipeline over tiles (when the rows fit in registers, D.NT4 <= 4): cell ids two tiles ahead, embedding rows
  // one tile ahead.  MODE 0 requests the first tile's ids and rows BEFORE the LDS staging below.
  const bool pre = !LEAN && D.NT4 <= 4 && NCT <= 8;    // (K > 128: the extra row registers would spill)
  // the three forms of a tile's distance GEMM (rows in registers | rows streamed), fp32 MFMA or split bf16 (BF; hmx_setup offers BF
  // only where the register form exists for the same shapes: NS2 <= 2 whenever NT4 <= 4)
  const int rowmask = BF ? rows_mask_bf(g, zs) : 0;
  auto ld_rows = [&](const float* __restrict__ zr, RowRegs& r) __attribute__((always_inline)) {
    if constexpr (BF) load_rows_bf(zr, g, zs, r); else load_rows(zr, g, D.NT4, D.tail, r);
  };
  auto dots_regs = [&](const RowRegs& r, const bool valid, f32x4 (&acc)[NCT]) __attribute__((always_inline)) {
    if constexpr (BF) tile_dots_bf_regs<NCT>(ldsB, r, valid, rowmask, lane, D.NS2, acc);
    else tile_dots_regs<NCT>(lds4, r, valid, lane, D.NS, D.NT4, D.tail, acc);
  };
  auto dots_stream = [&](const float* __restrict__ zr, const bool valid, f32x4 (&acc)[NCT]) __attribute__((always_inline)) {
    if constexpr (BF) tile_dots_bf<NCT>(ldsB, zr, valid, rowmask, g, lane, D.NS2, zs, acc);
    else tile_dots<NCT>(lds4, zr, valid, g, lane, D.NS, D.NT4, D.tail, acc);
  };
  // (cell id, combination) of this lane's A-operand row, ONE vector load per tile: a separate uniform load of the tile's
  // combination ends in a readfirstlane right behind the load, i.e. a vmcnt(0) -- a drain of the 28 outstanding R stores
  // of the previous tile plus a full memory latency -- in every iteration.
  int2 cellN = make_int2(-1, -1), cellNN = make_int2(-1, -1);
  RowRegs rowsN;
  auto tile_cell = [&](int tile) -> int2 {     // (-1, .): padding slot / beyond the end
    if (tile >= te) return make_int2(-1, -1);
    if constexpr (UPD) return D.lpair[p0 + 16 * tile + c];
    else if (MODE == 1 && D.head_gather) return D.lpair[16 * tile + c];
    else {
      // keep this a per-lane (vector) load: with the uniform tile index hipcc would emit load + readfirstlane, i.e. a
      // vmcnt(0) -- a full memory latency per tile that also drains the prefetched rows
      const Item* tp = D.titems + tile;
      asm volatile("" : "+v"(tp));
      const Item it = *tp;
      return make_int2((c < it.cnt) ? it.start + c : -1, it.q);
    }
  };
  {
    // Staging.  Every global load of this prologue is ISSUED before the first one is consumed (the launch is a link of
    // the block-step chain, its prologue a serial section): first the fold inputs -- replica tables written by the
    // previous launch's atomics, i.e. L2 misses -- then the centroid image, then they are consumed in the same order.
    constexpr int FE = 2;                     // fold entries per thread and chunk (B*K <= 2 * blockDim in one chunk)
    const bool fold = (MODE == 0) && D.fused_fold;
    const int bd = blockDim.x, tid = threadIdx.x;
    long long fv[FE][10];
    float fth[FE], fpr[FE];
    const long long* sold = fold ? D.Sold_fx + (size_t)j * nBK : nullptr;
    auto fold_issue = [&](int base) {
#pragma unroll
      for (int e = 0; e < FE; e++) {
        const int ic = min(base + tid + e * bd, nBK - 1);
#pragma unroll
        for (int r = 0; r < 8; r++) fv[e][r] = D.fold_prev[(size_t)min(r, D.nrep - 1) * nBK + ic];
        fv[e][8] = D.O_fx[ic]; fv[e][9] = sold[ic];
        const int b = ic / K;
        fth[e] = D.theta[b]; fpr[e] = D.Pr_b[b];
      }
    };
    auto fold_consume = [&](int base) {
#pragma unroll
      for (int e = 0; e < FE; e++) {
        const int i = base + tid + e * bd;
        if (i < nBK) {
          long long o = fv[e][8] - fv[e][9];
#pragma unroll
          for (int r = 0; r < 8; r++) if (r < D.nrep) o += fv[e][r];
          ldsO[i] = o;
          if (blockIdx.x == 0) {
            D.O_alt[i] = o;
            for (int r = 0; r < D.nrep; r++) D.fold_zero[(size_t)r * nBK + i] = 0;
          }
        }
      }
    };
    auto pen_entry = [&](int i, float th, float pr) {   // same arithmetic as k_foldpen (sharded path): tables must agree bitwise
      const int b = i / K, k = i - b * K;
      long long rs = 0;
      for (int b0 = 0; b0 < D.B0; b0++) rs += ldsO[b0 * K + k];
      const float of = (float)((double)ldsO[i] * FX_INV);
      const float ef = (float)(((double)rs * FX_INV) * (double)pr);
      ldsPen[i] = pen_pow((2.0f * ef) + 1.0f, of + ef + 1.0f, th);
    };
    if (fold) fold_issue(0);
    const int nQC = D.Q * C;
    int qlv0 = 0;
    if (fold) qlv0 = D.qlev[min(tid, nQC - 1)];
    if (ts < te) { cellN = tile_cell(ts); cellNN = tile_cell(ts + tstep); }   // first tiles' (cell, combination) pairs
    const f32x4* src = PAIR ? reinterpret_cast<const f32x4*>(D.Yimg3p) : BF ? reinterpret_cast<const f32x4*>(D.Yimg3) : reinterpret_cast<const f32x4*>(D.Yimg);
    {   // first chunk straight-line (a loop header here would make hipcc drain the loads above before the first image load)
      f32x4 t[4];
#pragma unroll
      for (int k = 0; k < 4; k++) t[k] = src[min(tid + k * bd, nYall - 1)];
#pragma unroll
      for (int k = 0; k < 4; k++) if (tid + k * bd < nYall) lds4[tid + k * bd] = t[k];
    }
    stamp(12);
    if (ts < te && pre) ld_rows(D.Zc + (size_t)(cellN.x >= 0 ? cellN.x : 0) * zs, rowsN);
    stamp(13);
    for (int base = 4 * bd; base < nYall; base += 4 * bd) {
      f32x4 t[4];
#pragma unroll
      for (int k = 0; k < 4; k++) t[k] = src[min(base + tid + k * bd, nYall - 1)];
#pragma unroll
      for (int k = 0; k < 4; k++) if (base + tid + k * bd < nYall) lds4[base + tid + k * bd] = t[k];
    }
    if constexpr (MODE == 0) {
      if (D.fused_fold) {
        fold_consume(0);
        for (int base = FE * bd; base < nBK; base += FE * bd) { fold_issue(base); fold_consume(base); }
        if (tid < nQC) ldsQlev[tid] = qlv0;
        for (int i = tid + bd; i < nQC; i += bd) ldsQlev[i] = D.qlev[i];
        stamp(14);
        __syncthreads();
        stamp(15);
        if (nBK <= FE * bd) {
#pragma unroll
          for (int e = 0; e < FE; e++) if (tid + e * bd < nBK) pen_entry(tid + e * bd, fth[e], fpr[e]);
        } else {
          for (int i = tid; i < nBK; i += bd) pen_entry(i, D.theta[i / K], D.Pr_b[i / K]);
        }
      } else if (D.pen_lds) {
        for (int i = threadIdx.x; i < D.B * K; i += blockDim.x) ldsPen[i] = D.pen[i];
        for (int i = threadIdx.x; i < D.Q * C; i += blockDim.x) ldsQlev[i] = D.qlev[i];
      }
    }
    if constexpr (CHAIN) for (int i = threadIdx.x; i < D.Q * C; i += blockDim.x) ldsQlev[i] = D.qlev[i];
    if constexpr (PAIR) for (int i = threadIdx.x; i < 4 * 2 * 2 * 16; i += blockDim.x) ldsX[i] = 0ull;      // (sequence numbers start at 1)
    if constexpr (MODE == 2) for (int i = threadIdx.x; i < K * D.d + K; i += blockDim.x) ltab[i] = 0;
    __syncthreads();
  }
  stamp(2);
  const float* penT = ((MODE == 0 && (D.pen_lds || D.fused_fold)) || CHAIN) ? ldsPen : D.pen;
  const int* qlevT = ((MODE == 0 && (D.pen_lds || D.fused_fold)) || CHAIN) ? ldsQlev : D.qlev;
  long long* snew = D.Snew_fx + (size_t)(wave & (D.nrep - 1)) * D.B * KS + kb;  // this wave's table replica (MODE 6: its half of the columns)
  // per-lane cluster constants: exp(-dist/sigma) = exp2(dist * ce), ce = -log2(e)/sigma;  sigma r ln r = cl r log2 r,
  // cl = sigma ln 2;  lpen = log2(penalty of the current combination), clp = cl * lpen (general sigma only).
  constexpr int NSIG = USIG ? 1 : NCT;
  float ce[NSIG], cl[NSIG], clp[NSIG], lpen[NCT];
  unsigned long long oacc[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) {
    const bool kv = kcol(NCT, ct, c) < K;
    const size_t ks = (size_t)min(kcol(NCT, ct, c), K - 1);
    if (ct < NSIG) {
      if constexpr (MODE == 2) { ce[ct] = ld_or(D.ynorm, ks, kv, 0.0f); cl[ct] = 0.0f; }
      else if constexpr (USIG) { ce[ct] = D.ce[0]; cl[ct] = D.cl[0]; }
      else { ce[ct] = ld_or(D.ce, ks, kv, 0.0f); cl[ct] = ld_or(D.cl, ks, kv, 0.0f); }
      clp[ct] = 0.0f;
    }
    lpen[ct] = 0.0f; oacc[ct] = 0ull;
  }
  // MODE 3: per-lane running minima of the packed (key bits, global cell) race values and the per-anchor hash keys
  unsigned long long best[MODE == 3 ? NCT : 1], sk[MODE == 3 ? NCT : 1];
  if constexpr (MODE == 3) {
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) {
      best[ct] = ~0ull;
      sk[ct] = splitmix64(D.seed_key ^ ((uint64_t)(1 + kcol(NCT, ct, c)) * 0xD1342543DE82EF95ull));
    }
  }
  auto CE = [&](int ct) -> float { return ce[USIG ? 0 : ct]; };
  auto CL = [&](int ct) -> float { return cl[USIG ? 0 : ct]; };
  double od = 0.0, oe = 0.0;
  int curq = -1;
  // ---- per-tile stages ------------------------------------------------------------------------------------------
  // the tile's combination: slot 0 of a tile is always a real cell (static tiles: every lane holds it)
  auto tile_q = [&](const int2 cq) -> int { return __builtin_amdgcn_readfirstlane(cq.y); };
  const RowRegs* erows = nullptr;   // MODE 2: the A-operand registers of the tile whose epilogue runs (single-accumulator loop)
  // MODE 0/1 epilogue, split so that the fused loop below can interleave it with the next tile's MFMAs:
  // epi_begin: run change -> flush the O contributions of the finished combination, fetch the new penalty row
  // A tile's combination word (lpair.y) when the shuffle keyed the tiles by it (D.nxt): bits 0..18 the covariate combination,
  // bits 19..24 the block its cells belong to in the NEXT round, bits 25..30 their block in THIS round.  The R rows a block update
  // writes are at the same time the cells' old contribution to their next block (D.Sold_next), and the R rows the head writes --
  // run over this round's order -- are their old contribution to this round's blocks (D.Sold_head): the pass over R that used to
  // collect them (k_oldsum) disappears.
  const int QMASK = D.qmask;      // 0x7FFFF when shuffles may be keyed (then Q < 2^19), else all bits (Q up to 2^24)
  auto flush_run = [&]() __attribute__((always_inline)) {
    long long* t2 = nullptr;
    if (UPD && D.Sold_next) t2 = D.Sold_next + (size_t)((curq >> 19) & 63) * D.B * KS + kb;
    if (MODE == 1 && D.head_gather && D.Sold_head) t2 = D.Sold_head + (size_t)((curq >> 25) & 63) * D.B * KS;
#ifdef HMX_TRACE
    if (D.upd_debug & 16) t2 = nullptr;                   // timing experiments (WRONG RESULTS): no carry atomics | no contribution atomics at all
    if (D.upd_debug & 8) {
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) oacc[ct] = 0ull;
      return;
    }
#endif
    flush_tile_fx<NCT>(snew, t2, qlevT, curq & QMASK, C, K, KS, c, g, oacc);
  };
  // MODE 6: the block's penalty rows come from memory (the folders' write-through stores, visible once their counter was seen).  Right behind the flag a
  // wave fetches the rows of ALL its tiles of the block at once -- lane = cluster, coalesced device-scope loads, every load in flight together: one round
  // trip per block -- and leaves log2(sum over the covariates) per (tile, cluster) in its own LDS cache (pen_cache_fill); a tile's epilogue reads its row
  // from there.  Tiles beyond the cache (more than four per stream and block) fetch their rows themselves, level by level.
  constexpr int KC = 16 * NCT, PCT = 4;
  float* const lpenT = reinterpret_cast<float*>(ldsX + 4 * 2 * 2 * 16) + (size_t)(threadIdx.x >> 6) * (PCT * KC);
  int tord = 0, ncache = 0;       // ordinal of the next tile of this block; tiles whose rows are cached
  auto epi_begin = [&](const int q0) __attribute__((always_inline)) {
    if constexpr (PAIR) {
      if (q0 != curq) { if (curq >= 0) flush_run(); curq = q0; }
      constexpr int NFULL = NCT >> 2, RT = NCT & 3;
      if (tord < ncache) {
        const float* pr = lpenT + tord * KC;
#pragma unroll
        for (int q = 0; q < NFULL; q++) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(pr + 64 * q + 4 * c);
#pragma unroll
          for (int jj = 0; jj < 4; jj++) lpen[4 * q + jj] = v[jj];
        }
#pragma unroll
        for (int jj = 0; jj < RT; jj++) lpen[4 * NFULL + jj] = pr[64 * NFULL + RT * c + jj];
      } else {
        float penv[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) penv[ct] = 0.0f;
#pragma unroll 1
        for (int cc = 0; cc < C; cc++) {
          const float* pr = D.pen + (size_t)__builtin_amdgcn_readfirstlane(qlevT[(q0 & QMASK) * C + cc]) * KS + kb;
          float v[NCT];
#pragma unroll
          for (int ct = 0; ct < NCT; ct++) v[ct] = __hip_atomic_load(pr + min(kcol(NCT, ct, c), K - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
          for (int ct = 0; ct < NCT; ct++) penv[ct] += (kcol(NCT, ct, c) < K) ? v[ct] : 0.0f;
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) lpen[ct] = __builtin_amdgcn_logf(fmaxf(penv[ct], FLT_MIN));
      }
      tord++;
      return;
    }
    if (q0 != curq) {
      if (curq >= 0) flush_run();
      curq = q0;
      if constexpr (UPD) {
        float penv[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) penv[ct] = 0.0f;
        for (int cc = 0; cc < C; cc++) {  // penalty of a cell = SUM over its covariates (:322 is a matrix product)
          const int b = qlevT[(q0 & QMASK) * C + cc];
          const float* __restrict__ pr = penT + (size_t)b * K;
          if (D.rvec) {
            // a lane's clusters are consecutive (kcol): one 16-byte read per quad of cluster tiles, ALL reads of the level in
            // flight before the first is used (one latency per level instead of one per cluster tile)
            constexpr int NFULL = NCT >> 2, RT = NCT & 3;
            f32x4 vq[NFULL > 0 ? NFULL : 1];
            float vt[RT > 0 ? RT : 1];
#pragma unroll
            for (int q = 0; q < NFULL; q++) vq[q] = *reinterpret_cast<const f32x4*>(pr + min(64 * q + 4 * c, K - 4));
#pragma unroll
            for (int jj = 0; jj < RT; jj++) vt[jj] = pr[min(64 * NFULL + RT * c + jj, K - 1)];
#pragma unroll
            for (int q = 0; q < NFULL; q++) {
              const bool ok = 4 * q < first_partial_ct(NCT) || 64 * q + 4 * c < K;
#pragma unroll
              for (int jj = 0; jj < 4; jj++) penv[4 * q + jj] += ok ? vq[q][jj] : 0.0f;
            }
#pragma unroll
            for (int jj = 0; jj < RT; jj++) penv[4 * NFULL + jj] += (64 * NFULL + RT * c + jj < K) ? vt[jj] : 0.0f;
          } else {
#pragma unroll
            for (int ct = 0; ct < NCT; ct++) penv[ct] += ld_or(penT, (size_t)b * K + min(kcol(NCT, ct, c), K - 1), kcol(NCT, ct, c) < K, 0.0f);
          }
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) { lpen[ct] = __builtin_amdgcn_logf(fmaxf(penv[ct], FLT_MIN)); if constexpr (!USIG) clp[ct] = cl[ct] * lpen[ct]; }
      }
    }
  };
  // put_row: one R row (register `reg` of every cluster tile) -> memory.  A lane's columns are consecutive clusters (kcol): one
  // 16-byte store per quad of cluster tiles and one 12/8/4-byte store for the rest -- 2 store instructions per row at K = 100
  // instead of 7 (the epilogue is store-ISSUE-bound, DESIGN 4).  Rows are 16-byte aligned when K % 4 == 0 (D.rvec).
  auto put_row = [&](float* __restrict__ row, const f32x4 (&acc)[NCT], const int reg) __attribute__((always_inline)) {
    constexpr int NFULL = NCT >> 2, RT = NCT & 3;
    if (D.rvec) {
#pragma unroll
      for (int q = 0; q < NFULL; q++) {
        const int k0 = 64 * q + 4 * c;
        if (4 * q < first_partial_ct(NCT) || k0 < K) {      // (K % 4 == 0: a lane's four clusters are all inside K or all outside)
          f32x4 v; v[0] = acc[4 * q][reg]; v[1] = acc[4 * q + 1][reg]; v[2] = acc[4 * q + 2][reg]; v[3] = acc[4 * q + 3][reg];
          *reinterpret_cast<f32x4*>(row + k0) = v;
        }
      }
      if constexpr (RT > 0) {
        const int k0 = 64 * NFULL + RT * c;
        if (k0 + RT <= K) {
          if constexpr (RT == 3) { F3 v; v.x = acc[4 * NFULL][reg]; v.y = acc[4 * NFULL + 1][reg]; v.z = acc[4 * NFULL + 2][reg]; *reinterpret_cast<F3*>(row + k0) = v; }
          else if constexpr (RT == 2) { F2 v; v.x = acc[4 * NFULL][reg]; v.y = acc[4 * NFULL + 1][reg]; *reinterpret_cast<F2*>(row + k0) = v; }
          else row[k0] = acc[4 * NFULL][reg];
        } else {
#pragma unroll
          for (int jj = 0; jj < RT; jj++) if (k0 + jj < K) row[k0 + jj] = acc[4 * NFULL + jj][reg];
        }
      }
    } else {
#pragma unroll
      for (int ct = 0; ct < NCT; ct++)
        if (ct < first_partial_ct(NCT) || kcol(NCT, ct, c) < K) row[kcol(NCT, ct, c)] = acc[ct][reg];
    }
  };
  // MODE 6: a row's normalisation sum runs over BOTH halves of the clusters.  Each wave of the pair leaves its four row sums of the batch in LDS
  // as { sequence number, bits } words (one 8-byte write: self-validating, no ordering needed) and adds what its partner left; the slots alternate
  // with the sequence number (a wave can be at most one exchange ahead of its partner: it needs the partner's word to finish its own).  Both waves
  // own the same tiles, i.e. make the same sequence of calls; a + b == b + a: both get the same bits.
  unsigned xseq = 0;
  auto pair_sum = [&](auto& se) __attribute__((always_inline)) {
    constexpr int RBn = sizeof(se) / sizeof(float);
    static_assert(RBn <= 4, "a batch holds at most the four rows of a lane");
    xseq++;
    const int pslot = (((int)(threadIdx.x >> 7) * 2 + (int)(xseq & 1u)) * 2);
    volatile unsigned long long* mine = ldsX + (size_t)(pslot + kh) * 16 + 4 * g;
    const volatile unsigned long long* other = ldsX + (size_t)(pslot + (kh ^ 1)) * 16 + 4 * g;
    float v = se[0];
#pragma unroll
    for (int i = 1; i < RBn; i++) v = (c == i) ? se[i] : v;
    if (c < RBn) mine[c] = ((unsigned long long)xseq << 32) | (unsigned long long)__float_as_uint(v);
    // every lane fetches ONE of the partner's words (lane c: row c & 3 of its group) and the rows are dealt by DPP row broadcasts: two registers
    // instead of eight at the point where the register pressure of the epilogue peaks
    unsigned long long o;
    int spins = 0;
    for (;;) {
      o = other[c & 3];
      if (__all((unsigned)(o >> 32) == xseq || (c & 3) >= RBn)) break;
      __builtin_amdgcn_s_sleep(1);
      if (++spins > (1 << 22)) { if (lane == 0) atomicExch(&D.chain_ctl[1], 7); break; }
    }
    const int ob = (int)(unsigned)o;
    if constexpr (RBn > 0) se[0] += __int_as_float(__builtin_amdgcn_update_dpp(0, ob, 0x150, 0xF, 0xF, true));      // row_newbcast:0
    if constexpr (RBn > 1) se[1] += __int_as_float(__builtin_amdgcn_update_dpp(0, ob, 0x151, 0xF, 0xF, true));
    if constexpr (RBn > 2) se[2] += __int_as_float(__builtin_amdgcn_update_dpp(0, ob, 0x152, 0xF, 0xF, true));
    if constexpr (RBn > 3) se[3] += __int_as_float(__builtin_amdgcn_update_dpp(0, ob, 0x153, 0xF, 0xF, true));
  };
  // epi_rows: the four accumulator registers (rows 4g..4g+3 of the tile; their cell ids live in lanes 4g+reg of cellA)
  // TOGETHER, stage by stage: a gfx950 wave issues a dependent VALU instruction only every ~26 cycles (measured,
  // tools/ubench/issue.hip) and few waves share a SIMD here, so the code must carry its own instruction-level
  // parallelism -- up to 28 independent values per stage instead of one row after the other.
  //   t_k   = x_k ce_k + log2 pen_k,  e_k = exp2(t_k)      x_k = 2 - 2 z.y_k                   (:141-150, :318-322)
  //   r_k   = e_k / sum_k e_k                   (ONE L1 normalisation: the reference's first one cancels, :323-326)
  //   sum_k r_k x_k              = inv * sum e_k x_k                                       (objective_kmeans_dist, :160)
  //   sum_k sigma_k r_k ln r_k   = inv * sum cl_k e_k (t_k + log2 inv)                     (entropy, :161; log2 r_k = t_k + log2 inv)
  //        uniform sigma:  = inv cl (ce sum e_k x_k + sum e_k lpen_k + log2(inv) sum e_k)
  //        general sigma:  = inv (sum e_k clp_k - sum e_k x_k + log2(inv) sum e_k cl_k)     (cl_k ce_k = -1)
  //   -- no logarithm per value, one per row
  // DEFER (std::true_type, MODE 4's last tile of a block): the normalised values replace `acc` instead of being stored, so that the
  // O contributions can be flushed BEFORE the tile's 28 stores are issued (store_rows) -- the arrival then waits for the
  // atomics only, not for the block's R rows to reach HBM (vector memory operations retire in issue order on gfx9).
  auto epi_rows = [&](const int cellA, f32x4 (&acc)[NCT], auto defer_tag) __attribute__((always_inline)) {
    constexpr bool DEFER = decltype(defer_tag)::value;
    constexpr int RB = (NCT <= 7 && !LEAN) ? 4 : 2;   // rows per batch: all four while the registers last
#pragma unroll
    for (int r0 = 0; r0 < 4; r0 += RB) {
      float se[RB], sx[RB], sp[RB], sc[RB];   // sums of e, e x, e lpen (or e clp), e (lane local) (or e cl)
      float* Rrow[RB];
      bool cv[RB];
#pragma unroll
      for (int i = 0; i < RB; i++) {
        const int cell = __shfl(cellA, 4 * g + r0 + i, 64);
        cv[i] = cell >= 0;
        Rrow[i] = D.R + (size_t)(cv[i] ? cell : D.n) * KS + kb;       // invalid rows: the dummy row behind R (zeros)
        se[i] = 0.0f; sx[i] = 0.0f; sp[i] = 0.0f; sc[i] = 0.0f;
      }
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) {
#pragma unroll
        for (int i = 0; i < RB; i++) {
          const float x = fmaf(acc[ct][r0 + i], -2.0f, 2.0f);
          float e = __builtin_amdgcn_exp2f(UPD ? fmaf(x, CE(ct), lpen[ct]) : x * CE(ct));
          if (ct >= first_partial_ct(NCT)) e = (kcol(NCT, ct, c) < K) ? e : 0.0f;
          acc[ct][r0 + i] = e;
          se[i] += e;
          sx[i] = fmaf(e, x, sx[i]);
          if constexpr (UPD) sp[i] = fmaf(e, USIG ? lpen[ct] : clp[USIG ? 0 : ct], sp[i]);
          if constexpr (!USIG) sc[i] = fmaf(e, CL(ct), sc[i]);
        }
      }
      if constexpr (USIG) {
#pragma unroll
        for (int i = 0; i < RB; i++) sc[i] = se[i];   // this lane's own sum, before the row reduction
      }
      rowsum16xN<RB>(se);
      if constexpr (PAIR) pair_sum(se);      // + the other half of the clusters (the pair's partner wave)
      float inv[RB], pd = 0.0f, pe = 0.0f;
#pragma unroll
      for (int i = 0; i < RB; i++) {
        float i2 = __builtin_amdgcn_rcpf(se[i]);
        i2 = i2 * fmaf(-se[i], i2, 2.0f);               // one Newton step: <= 1 ulp
        i2 = (se[i] == 0.0f) ? 1.0f : i2;
        const float linv = __builtin_amdgcn_logf(i2);
        i2 = cv[i] ? i2 : 0.0f;                          // padding rows contribute exactly nothing
        inv[i] = i2;
        pd = fmaf(i2, sx[i], pd);
        if constexpr (USIG) pe = fmaf(i2 * CL(0), fmaf(CE(0), sx[i], fmaf(linv, sc[i], sp[i])), pe);
        else pe = fmaf(i2, fmaf(linv, sc[i], sp[i] - sx[i]), pe);
      }
      od += (double)pd; oe += (double)pe;
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) {
        unsigned s32 = 0u;                 // RB <= 4 values of at most 2^29 each: no carry out of 32 bits
#pragma unroll
        for (int i = 0; i < RB; i++) {
          const float rn = acc[ct][r0 + i] * inv[i];
          acc[ct][r0 + i] = rn;            // the normalised value replaces the distance (stored below, or later by store_rows)
          s32 += fx32_of(rn);
        }
        oacc[ct] += (unsigned long long)s32;
      }
      if constexpr (!DEFER) {
#ifdef HMX_TRACE
        if (!(D.upd_debug & 4))   // timing experiment: no R stores
#endif
        if (!NOSTORE && D.r_store) {    // (a pass whose R rows nobody will read leaves them in the registers: see Dev::r_store)
#pragma unroll
          for (int i = 0; i < RB; i++) put_row(Rrow[i], acc, r0 + i);
        }
      }
    }
  };
  // the deferred stores of epi_rows<DEFER>: `acc` holds the normalised rows
  auto store_rows = [&](const int cellA, const f32x4 (&acc)[NCT]) __attribute__((always_inline)) {
#ifdef HMX_TRACE
    if (D.upd_debug & 4) return;
#endif
    if (NOSTORE || !D.r_store) return;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int cell = __shfl(cellA, 4 * g + i, 64);
      put_row(D.R + (size_t)(cell >= 0 ? cell : D.n) * KS + kb, acc, i);
    }
  };
  // epilogue of a tile whose distances are in `acc`
  auto epilogue = [&](const int cellA, const int q0, f32x4 (&acc)[NCT]) __attribute__((always_inline)) {
    if constexpr (MODE == 2) {
      // nearest centre of every cell of the tile: argmin_k ||y_k||^2 - 2 x.y_k ; ties -> smallest k.  All four rows
      // together (ILP), the 16-lane reductions by DPP: first the minimum score, then the smallest k that attains it.
      float bs[4]; int bk[4];
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        bs[reg] = INFINITY; bk[reg] = 0x7fffffff;
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) {
          const float sc = (ct < first_partial_ct(NCT) || kcol(NCT, ct, c) < K) ? fmaf(acc[ct][reg], -2.0f, ce[ct]) : INFINITY;
          const bool lt = sc < bs[reg];               // strict: the smaller k (ct ascending) wins a tie
          bs[reg] = lt ? sc : bs[reg];
          bk[reg] = lt ? kcol(NCT, ct, c) : bk[reg];
        }
      }
      float m[4];
#pragma unroll
      for (int reg = 0; reg < 4; reg++) m[reg] = bs[reg];
#pragma unroll
      for (int st = 0; st < 4; st++) {
        float t[4];
#pragma unroll
        for (int reg = 0; reg < 4; reg++) t[reg] = (st == 0) ? dpp_f(m[reg], 0) : (st == 1) ? dpp_f(m[reg], 1) : (st == 2) ? dpp_f(m[reg], 2) : dpp_f(m[reg], 3);
#pragma unroll
        for (int reg = 0; reg < 4; reg++) m[reg] = fminf(m[reg], t[reg]);
      }
      int kb[4];
#pragma unroll
      for (int reg = 0; reg < 4; reg++) kb[reg] = (bs[reg] == m[reg]) ? bk[reg] : 0x7fffffff;
#pragma unroll
      for (int st = 0; st < 4; st++) {
        int t[4];
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
          const float kf = __int_as_float(kb[reg]);
          t[reg] = __float_as_int((st == 0) ? dpp_f(kf, 0) : (st == 1) ? dpp_f(kf, 1) : (st == 2) ? dpp_f(kf, 2) : dpp_f(kf, 3));
        }
#pragma unroll
        for (int reg = 0; reg < 4; reg++) kb[reg] = min(kb[reg], t[reg]);
      }
      // the 16 lanes of a row group add the row's PCs (2^30 fixed point) to the LDS table of its centre: ALL loads of the
      // tile are issued before the first is used (they hit L1/L2 -- the rows were just read as MFMA operands)
      const int dd = D.d;          // locals: after the first LDS atomic hipcc would re-read D's fields from a spilled copy
      const float* const Zcp = D.Zc;
      if (erows) {
        // the rows are still in the A-operand registers (lane = cell l & 15, k-slot l >> 4): no second read of the tile.  The
        // centre of THIS lane's cell sits in the row group (l & 15) >> 2, register (l & 15) & 3.
        int t4[4];
#pragma unroll
        for (int reg = 0; reg < 4; reg++) t4[reg] = __shfl(kb[reg], 16 * (c >> 2), 64);
        const int kc = ((c & 3) == 0) ? t4[0] : ((c & 3) == 1) ? t4[1] : ((c & 3) == 2) ? t4[2] : t4[3];
        if (cellA >= 0) {
          long long* row = ltab + (size_t)kc * dd;
          if constexpr (BF) {      // split-bf16 row layout: v[2 s + h][e] = PC 32 s + 8 g + 4 h + e
#pragma unroll
            for (int t = 0; t < 4; t++) {
#pragma unroll
              for (int e = 0; e < 4; e++) {
                const int jj = 32 * (t >> 1) + 8 * g + 4 * (t & 1) + e;
                if (t < 2 * D.NS2 && jj < dd) atomicAdd((unsigned long long*)&row[jj], (unsigned long long)(long long)__float2int_rn(erows->v[t][e] * 1073741824.0f));
              }
            }
            if (g == 0) atomicAdd((unsigned long long*)&ltab[K * dd + kc], 1ull);
            return;
          }
#pragma unroll
          for (int t = 0; t < 4; t++) {
            if (t < D.NT4) {
#pragma unroll
              for (int e = 0; e < 4; e++) {
                const int jj = 16 * t + 4 * g + e;
                if (jj < dd) atomicAdd((unsigned long long*)&row[jj], (unsigned long long)(long long)__float2int_rn(erows->v[t][e] * 1073741824.0f));
              }
            }
          }
#pragma unroll
          for (int u = 0; u < 3; u++) {
            const int jj = 16 * D.NT4 + 4 * u + g;
            if (u < D.tail && jj < dd) atomicAdd((unsigned long long*)&row[jj], (unsigned long long)(long long)__float2int_rn(erows->t[u] * 1073741824.0f));
          }
          if (g == 0) atomicAdd((unsigned long long*)&ltab[K * dd + kc], 1ull);
        }
        return;
      }
      int cellr[4];
#pragma unroll
      for (int reg = 0; reg < 4; reg++) cellr[reg] = __shfl(cellA, 4 * g + reg, 64);
      for (int j0 = 0; j0 < dd; j0 += 64) {
        float z[4][4];
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
          const float* zr = Zcp + (size_t)max(cellr[reg], 0) * zs;
#pragma unroll
          for (int u = 0; u < 4; u++) z[reg][u] = zr[min(j0 + 16 * u + c, dd - 1)];
        }
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int jj = j0 + 16 * u + c;
            if (cellr[reg] >= 0 && jj < dd) {
              // |z| <= 1 (normalised rows): the 2^30 fixed-point value fits int32 -> rndne + cvt + sign extension
              const unsigned long long v = (unsigned long long)(long long)__float2int_rn(z[reg][u] * 1073741824.0f);
              atomicAdd((unsigned long long*)&ltab[kb[reg] * dd + jj], v);
            }
          }
        }
      }
#pragma unroll
      for (int reg = 0; reg < 4; reg++)
        if (c == 0 && cellr[reg] >= 0) atomicAdd((unsigned long long*)&ltab[K * dd + kb[reg]], 1ull);
    } else if constexpr (MODE == 3) {
      // exponential race of every anchor (src/utils.cpp:24-34): u from splitmix64(anchor key + global cell), key = -log(u) / |dist|
      int gc[4]; bool ok[4];
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int cell = __shfl(cellA, 4 * g + reg, 64);
        ok[reg] = cell >= 0;
        gc[reg] = D.perm[max(cell, 0)];
      }
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const uint64_t gg = D.seed_goff + (uint64_t)gc[reg];
        bool skip = !ok[reg];
        for (int x = 0; x < D.seed_nexcl; x++) skip |= ((uint64_t)D.seed_excl[x] == gg);   // re-probe passes only
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) {
          const float dis = fabsf(2.0f * (1.0f - acc[ct][reg]));
          const uint64_t h = splitmix64(sk[ct] + gg);
          const float u = ((float)(h >> 40) + 0.5f) * (1.0f / 16777216.0f);
          const float key = -logf(u) / dis;  // >= 0 (or +inf / nan when dis == 0)
          unsigned kb = __float_as_uint(key);
          if (!(key >= 0.0f)) kb = 0x7f800000u;
          kb &= 0x7fffffffu;   // -0.0 (u == 1: -log(u) = -0) must order as zero, not as the largest unsigned pattern  // nan -> +inf: never the minimum
          const unsigned long long pk = ((unsigned long long)kb << 32) | (unsigned long long)(uint32_t)gg;
          const bool take = !skip && (ct < first_partial_ct(NCT) || kcol(NCT, ct, c) < K) && pk < best[ct];
          best[ct] = take ? pk : best[ct];
        }
      }
    } else {
      epi_begin(q0);
      epi_rows(cellA, acc, std::false_type{});
    }
  };
  constexpr bool DUAL = !LEAN && NCT <= 7;  // two accumulator sets fit the 256-VGPR budget (2 waves/SIMD) only up to K = 112
  auto next_rows = [&](const int2 nxt, const int2 cur) {  // row address of the NEXT tile's lane (any valid row if padding)
    return D.Zc + (size_t)(nxt.x >= 0 ? nxt.x : (cur.x >= 0 ? cur.x : 0)) * zs;
  };
  if constexpr (CHAIN) {
    // ======================= persistent block chain of one round =======================
    // Cross-workgroup traffic (L2s of different XCDs are not coherent, so nothing here relies on plain loads of data another
    // workgroup wrote during this launch):
    //   Snew replicas   workers: device-scope atomic adds;  folder: atomic exchange with 0 (read + reset in one RMW)
    //   ctl[2 + j]      arrivals of block j (atomic add, after the wave's vmcnt(0) drained its contribution atomics)
    //   pen_g[i]        8-byte granules { tag << 32 | penalty bits } written through with ONE sc1 store each and read
    //                   with sc1 loads until the tag is this block's (self-validating: no ordering assumed)
    //   ctl[0]          block flag (tag), stored after the granules drained; one lane per workgroup polls it
    // Every spin is bounded: on a timeout ctl[1] is raised and the launch runs out with garbage instead of hanging the GPU.
    int* const ctl = D.chain_ctl;
    unsigned long long* const peng = D.pen_g;
    const unsigned tag0 = D.chain_tag;
    const int nbk = D.nb, nworkWG = (int)gridDim.x - nfold, bd = blockDim.x, tid = threadIdx.x;
    constexpr int SPIN_LIMIT = 1 << 20;     // ~1 s of polling; once ANY spin has timed out (ctl[1] != 0) the others give up at once
    auto dead = [&](int spins) -> bool { return (spins & 255) == 255 && __hip_atomic_load(&ctl[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0; };
    if constexpr (PAIR) {
      if ((int)blockIdx.x >= nworkWG) {
        // ---------------- MODE 6: one of the folders.  It owns the clusters [k0, k0 + kw) of every level: their O entries and cluster masses stay in its LDS
        // for the whole round; per block step it takes the workers' new contributions out of the table (exchange with zero), removes the next block's old
        // ones, recomputes its slice of the penalty table and writes it through to memory; the stores drained, it counts itself done (ctl[2]).
        const int f = (int)blockIdx.x - nworkWG, kw = D.chain_kw, kq = kw >> 2, k0 = f * kw;
        const int nE = D.B * kw, nIt = D.B * kq;
        long long* const fO = reinterpret_cast<long long*>(lds4);      // [B][kw]   (the staged image is not needed here)
        long long* const fRS = fO + nE;                                // [kw] cluster masses: sum over the first covariate's levels
        for (int e = tid; e < nE; e += bd) { const int b = e / kw, kk = e - b * kw; fO[e] = (k0 + kk < KS) ? D.O_fx[(size_t)b * KS + k0 + kk] : 0; }
        __syncthreads();
        for (int kk = tid; kk < kw; kk += bd) { long long rs = 0; for (int b0 = 0; b0 < D.B0; b0++) rs += fO[b0 * kw + kk]; fRS[kk] = rs; }
        __syncthreads();
        unsigned long long tw = 0, tf = 0, tp = 0, t_prev = wall_clock64();
        for (int jj = 0; jj <= nbk; jj++) {
          long long so0[4] = {0, 0, 0, 0};      // the old contributions of this thread's first item: requested before the wait
          if (jj < nbk && tid < nIt) {
            const int b = tid / kq, k4 = (tid - b * kq) * 4;
#pragma unroll
            for (int u = 0; u < 4; u++) so0[u] = D.Sold_fx[(size_t)jj * nBK + min((size_t)b * KS + k0 + k4 + u, (size_t)nBK - 1)];
          }
          if (jj > 0) {
            if (tid == 0) {
              int spins = 0;
              const int* arr = &ctl[8 + 8 * (jj - 1)];
              auto arrived = [&]() { int t = 0; for (int x = 0; x < 8; x++) t += __hip_atomic_load(&arr[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return t; };
              while (arrived() < nworkWG) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > SPIN_LIMIT) { atomicExch(&ctl[1], 1); break; }
                if (dead(spins)) break;
              }
            }
            __syncthreads();
          }
          { const unsigned long long t = wall_clock64(); tw += t - t_prev; t_prev = t; }
          if (D.p2p_world > 1) {
            // Sharded run: what this rank's workers filed for block jj - 1, minus its cells' old contributions to block jj, goes straight into every
            // peer's inbox (k_tile MODE 4's exchange: two self-validating granules per entry, the plane alternating with the exchange number) -- all
            // of this folder's entries first, then the peers' words are awaited and added: integer sums, the same O on every rank.
            const int G = D.p2p_world, me = D.p2p_rank;
            const unsigned tagx = tag0 + (unsigned)jj;
            const size_t par = (size_t)((D.chain_xseq + (unsigned)jj) & 1u) * 8;
            long long* const fD = fRS + kw;                              // [B][kw] this rank's deltas
            for (int it = tid; it < nIt; it += bd) {
              const int b = it / kq, k4 = (it - b * kq) * 4;
              if (k0 + k4 < KS) {
                const size_t i0 = (size_t)b * KS + k0 + k4;
                unsigned long long a[4] = {0ull, 0ull, 0ull, 0ull};
                long long so[4] = {0, 0, 0, 0};
                if (jj > 0) {
#pragma unroll
                  for (int u = 0; u < 4; u++) a[u] = atomicExch((unsigned long long*)&D.Snew_fx[i0 + u], 0ull);
                }
                if (jj < nbk) {
#pragma unroll
                  for (int u = 0; u < 4; u++) so[u] = (it == tid) ? so0[u] : D.Sold_fx[(size_t)jj * nBK + i0 + u];
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                  const long long dl = (long long)a[u] - so[u];
                  fD[b * kw + k4 + u] = dl;
                  p2p_send(D, par, (int)(i0 + u), tagx, dl);
                }
              }
            }
            for (int it = tid; it < nIt; it += bd) {
              const int b = it / kq, k4 = (it - b * kq) * 4;
              if (k0 + k4 < KS) {
                const size_t i0 = (size_t)b * KS + k0 + k4;
#pragma unroll
                for (int u = 0; u < 4; u++) {
                  const int e = b * kw + k4 + u;
                  long long o = fO[e] + fD[e];
#pragma unroll
                  for (int gq = 0; gq < 8; gq++) if (gq < G && gq != me) {
                    const unsigned long long* src = D.p2p_inbox_self() + ((par + gq) * P2P_CAP + i0 + u) * 2;
                    unsigned long long lo = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    unsigned long long hi = __hip_atomic_load(src + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    int spins = 0;
                    while ((unsigned)(lo >> 32) != tagx || (unsigned)(hi >> 32) != tagx) {
                      __builtin_amdgcn_s_sleep(1);
                      if (++spins > SPIN_LIMIT) { atomicExch(&ctl[1], 5); break; }
                      if (dead(spins)) break;
                      lo = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                      hi = __hip_atomic_load(src + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                    o += (long long)((hi << 32) | (lo & 0xffffffffull));
                  }
                  if (b < D.B0 && o != fO[e]) atomicAdd((unsigned long long*)&fRS[k4 + u], (unsigned long long)(o - fO[e]));
                  fO[e] = o;
                  if (jj == nbk) D.O_fx[i0 + u] = o;
                }
              }
            }
          } else
          for (int it = tid; it < nIt; it += bd) {
            const int b = it / kq, k4 = (it - b * kq) * 4;
            if (k0 + k4 < KS) {      // (KS % 4 == 0: the four clusters of an item are all inside or all outside)
              const size_t i0 = (size_t)b * KS + k0 + k4;
              unsigned long long a[4] = {0ull, 0ull, 0ull, 0ull};
              long long so[4] = {0, 0, 0, 0};
              if (jj > 0) {
#pragma unroll
                for (int u = 0; u < 4; u++) a[u] = atomicExch((unsigned long long*)&D.Snew_fx[i0 + u], 0ull);      // (one replica: 40 000 addresses spread the workers' atomics by themselves)
              }
              if (jj < nbk) {
#pragma unroll
                for (int u = 0; u < 4; u++) so[u] = (it == tid) ? so0[u] : D.Sold_fx[(size_t)jj * nBK + i0 + u];
              }
#pragma unroll
              for (int u = 0; u < 4; u++) {
                const int e = b * kw + k4 + u;
                const long long o = fO[e] + (long long)a[u] - so[u];
                if (b < D.B0 && o != fO[e]) atomicAdd((unsigned long long*)&fRS[k4 + u], (unsigned long long)(o - fO[e]));
                fO[e] = o;
                if (jj == nbk) D.O_fx[i0 + u] = o;      // the round's final O
              }
            }
          }
          if (jj == nbk) break;
          __syncthreads();
          { const unsigned long long t = wall_clock64(); tf += t - t_prev; t_prev = t; }
          for (int it = tid; it < nIt; it += bd) {      // same arithmetic as k_foldpen / k_penalty: identical tables
            const int b = it / kq, k4 = (it - b * kq) * 4;
            if (k0 + k4 < KS) {
              float pv[4];
#pragma unroll
              for (int u = 0; u < 4; u++) {
                const float of = (float)((double)fO[b * kw + k4 + u] * FX_INV);
                const float ef = (float)(((double)fRS[k4 + u] * FX_INV) * (double)D.Pr_b[b]);
                pv[u] = pen_pow((2.0f * ef) + 1.0f, of + ef + 1.0f, D.theta[b]);
              }
              unsigned long long* dst = reinterpret_cast<unsigned long long*>(D.pen + (size_t)b * KS + k0 + k4);
              __hip_atomic_store(dst, ((unsigned long long)__float_as_uint(pv[1]) << 32) | (unsigned long long)__float_as_uint(pv[0]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              __hip_atomic_store(dst + 1, ((unsigned long long)__float_as_uint(pv[3]) << 32) | (unsigned long long)__float_as_uint(pv[2]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
          }
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's rows have been written through
          __syncthreads();
          if (tid == 0) atomicAdd(&ctl[2], 1);                  // ... every wave's: this folder is done with block jj
          { const unsigned long long t = wall_clock64(); tp += t - t_prev; t_prev = t; }
        }
        if (f == 0 && tid == 0 && D.chain_dbg) { atomicAdd(&D.chain_dbg[0], tw); atomicAdd(&D.chain_dbg[1], tf); atomicAdd(&D.chain_dbg[2], tp); atomicAdd(&D.chain_dbg[3], 1ull); }
        return;
      }
    }
    if (!PAIR && (int)blockIdx.x == nworkWG) {
      // ---------------- the folder: O' = O + new(block j-1) - old(block j), E, penalty table of block j (:312-322,:329-330)
      for (int i = tid; i < nBK; i += bd) ldsO[i] = D.O_fx[i];
      __syncthreads();
      // cluster masses rs[k] = sum over the first covariate's levels of O[.,k] (E = rs Pr_b^T), kept up to date entry by entry in
      // the fold instead of re-summed B0 times per entry in the publish step.  (The folder never reads the centroid image: its
      // LDS region holds the masses.)
      long long* const ldsRS = reinterpret_cast<long long*>(lds4);
      for (int k = tid; k < K; k += bd) {
        long long rs = 0;
        for (int b0 = 0; b0 < D.B0; b0++) rs += ldsO[b0 * K + k];
        ldsRS[k] = rs;
      }
      __syncthreads();
      const int nRS = D.B0 * K;
      constexpr int FE = 4;
      unsigned long long tw = 0, tf = 0, tp = 0, t_prev = wall_clock64();   // diagnostics: wait / fold / publish time of the folder
      for (int jj = 0; jj <= nbk; jj++) {
        long long sv[FE];
#pragma unroll
        for (int e = 0; e < FE; e++) sv[e] = (jj < nbk) ? D.Sold_fx[(size_t)jj * nBK + min(tid + e * bd, nBK - 1)] : 0;   // before the wait
        if (jj > 0) {
          if (tid == 0) {
            int spins = 0;
            // arrivals are sharded over 8 counters (workgroup b -> counter b & 7: one per XCD under the observed placement);
            // 255 increments of ONE word serialise at ~12 ns each
            const int* arr = &ctl[8 + 8 * (jj - 1)];
            auto arrived = [&]() { int t = 0; for (int x = 0; x < 8; x++) t += __hip_atomic_load(&arr[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return t; };
            while (arrived() < nworkWG) {
              __builtin_amdgcn_s_sleep(1);
              if (++spins > SPIN_LIMIT) { atomicExch(&ctl[1], 1); break; }
              if (dead(spins)) break;
            }
          }
          __syncthreads();
        }
        { const unsigned long long t = wall_clock64(); tw += t - t_prev; t_prev = t; }
        if (D.p2p_world > 1) {
          // Sharded run: the new contributions of block jj-1 are summed over the GPUs INSIDE the launch.  One-shot exchange over
          // xGMI: every folder writes its local sums straight into every peer's inbox (two self-validating 8-byte granules
          // {tag, half of the int64} per entry, system-scope write-through stores), then sums what the peers wrote into its own.
          // Integer sums: every rank folds exactly the same O.  Two parities suffice: a rank can run at most one exchange ahead
          // of a peer (it needs that peer's contribution of step jj to finish step jj).
          const int G = D.p2p_world, me = D.p2p_rank;
          const unsigned tagx = tag0 + (unsigned)jj;
          // (round 4) EVERY step exchanges, jj = 0 included, and what travels is  new(jj - 1) - old_local(jj): the old contributions are filed
          // rank-locally by the previous round's tile kernels and are summed over the ranks right here -- the per-round all-reduce of the
          // nb x K x B table (24 host-launched collectives per run) is gone.  The plane alternates with the exchange NUMBER, carried across
          // rounds (nb + 1 exchanges per round: with jj & 1 two consecutive exchanges of neighbouring rounds would share a plane).
          const size_t par = (size_t)((D.chain_xseq + (unsigned)jj) & 1u) * 8;
          for (int base = 0; base < nBK; base += FE * bd) {
            long long dl[FE];
#pragma unroll
            for (int e = 0; e < FE; e++) {
              const int i = base + tid + e * bd;
              dl[e] = 0;
              if (i < nBK) {
                long long so = 0;
                if (jj < nbk) so = D.Sold_fx[(size_t)jj * nBK + i];
                if (jj > 0) {
                  unsigned long long a[8];
#pragma unroll
                  for (int r = 0; r < 8; r++) a[r] = (r < D.nrep) ? atomicExch((unsigned long long*)&D.Snew_fx[(size_t)r * nBK + i], 0ull) : 0ull;
#pragma unroll
                  for (int r = 0; r < 8; r++) dl[e] += (long long)a[r];
                }
                dl[e] -= so;
                p2p_send(D, par, i, tagx, dl[e]);
              }
            }
#pragma unroll
            for (int e = 0; e < FE; e++) {
              const int i = base + tid + e * bd;
              if (i < nBK) {
                long long o = ldsO[i] + dl[e];
                {
                  unsigned long long lo[8], hi[8];
#pragma unroll
                  for (int gq = 0; gq < 8; gq++) if (gq < G && gq != me) {
                    const unsigned long long* src = D.p2p_inbox_self() + ((par + gq) * P2P_CAP + i) * 2;
                    lo[gq] = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    hi[gq] = __hip_atomic_load(src + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                  }
#pragma unroll
                  for (int gq = 0; gq < 8; gq++) if (gq < G && gq != me) {
                    const unsigned long long* src = D.p2p_inbox_self() + ((par + gq) * P2P_CAP + i) * 2;
                    int spins = 0;
                    while ((unsigned)(lo[gq] >> 32) != tagx || (unsigned)(hi[gq] >> 32) != tagx) {
                      __builtin_amdgcn_s_sleep(1);
                      if (++spins > SPIN_LIMIT) { atomicExch(&ctl[1], 5); break; }
                      if (dead(spins)) break;
                      lo[gq] = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                      hi[gq] = __hip_atomic_load(src + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                    o += (long long)((hi[gq] << 32) | (lo[gq] & 0xffffffffull));
                  }
                }
                if (i < nRS && o != ldsO[i]) atomicAdd((unsigned long long*)&ldsRS[i % K], (unsigned long long)(o - ldsO[i]));
                ldsO[i] = o;
                if (jj == nbk) D.O_fx[i] = o;
              }
            }
          }
        }
        auto fold_entry = [&](int i, long long soldv) {
          long long o = ldsO[i];
          // every memory operation of the entry in flight before the first is consumed: the new contributions (exchange = read + reset)
          unsigned long long a[8];
#pragma unroll
          for (int r = 0; r < 8; r++) a[r] = (jj > 0 && r < D.nrep) ? atomicExch((unsigned long long*)&D.Snew_fx[(size_t)r * nBK + i], 0ull) : 0ull;
#pragma unroll
          for (int r = 0; r < 8; r++) o += (long long)a[r];
          if (jj < nbk) o -= soldv;
          if (i < nRS && o != ldsO[i]) atomicAdd((unsigned long long*)&ldsRS[i % K], (unsigned long long)(o - ldsO[i]));
          ldsO[i] = o;
          if (jj == nbk) D.O_fx[i] = o;      // the round's final O (read by the kernels that follow this launch)
        };
        if (D.p2p_world <= 1) {
#pragma unroll
          for (int e = 0; e < FE; e++) { const int i = tid + e * bd; if (i < nBK) fold_entry(i, sv[e]); }
          for (int i = tid + FE * bd; i < nBK; i += bd) fold_entry(i, jj < nbk ? D.Sold_fx[(size_t)jj * nBK + i] : 0);
        }
        if (jj == nbk) break;
        __syncthreads();
        { const unsigned long long t = wall_clock64(); tf += t - t_prev; t_prev = t; }
        const unsigned long long tagbits = (unsigned long long)(tag0 + (unsigned)jj) << 32;
        for (int i = tid; i < nBK; i += bd) {      // same arithmetic as k_foldpen / the fused prologue: identical tables
          const int b = i / K, k = i - b * K;
          const long long rs = ldsRS[k];
          const float of = (float)((double)ldsO[i] * FX_INV);
          const float ef = (float)(((double)rs * FX_INV) * (double)D.Pr_b[b]);
          const float pv = pen_pow((2.0f * ef) + 1.0f, of + ef + 1.0f, D.theta[b]);
          __hip_atomic_store(&peng[i], tagbits | (unsigned long long)__float_as_uint(pv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // the flag needs no ordering against the granules (they validate themselves by tag): raise it at once
        if (tid == 0) __hip_atomic_store(&ctl[0], (int)(tag0 + (unsigned)jj), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        { const unsigned long long t = wall_clock64(); tp += t - t_prev; t_prev = t; }
      }
      if (tid == 0 && D.chain_dbg) { atomicAdd(&D.chain_dbg[0], tw); atomicAdd(&D.chain_dbg[1], tf); atomicAdd(&D.chain_dbg[2], tp); atomicAdd(&D.chain_dbg[3], 1ull); }
      if (D.chain_tail) {
        // ---- the round's tail, by the folder (compute_objective, src/harmony.cpp:158-170): the workers' per-wave objective sums, the
        // cross-entropy term from the O / E tables this workgroup holds in LDS anyway, the snapshot straight into the pinned host slot;
        // then the tables this round consumed are cleared and the control words reset.  (k_round_tail does the same after the
        // launch-per-step paths; here it would be one more launch + ~60 us of gap behind every round.)
        if (tid == 0) {
          int spins = 0;
          const int* arr = &ctl[16 + 8 * nbk];
          auto arrived = [&]() { int t = 0; for (int x = 0; x < 8; x++) t += __hip_atomic_load(&arr[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return t; };
          while (arrived() < nworkWG) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > SPIN_LIMIT) { atomicExch(&ctl[1], 6); break; }
            if (dead(spins)) break;
          }
        }
        __syncthreads();
        double* const red = reinterpret_cast<double*>(lds4) + ((K + 1) & ~1);      // [waves][3], behind the cluster masses (the centroid image's space: the folder never stages it)
        const int nwv = nworkWG * (bd >> 6);
        double pa = 0.0, pb = 0.0;
        for (int w2 = tid; w2 < nwv; w2 += bd) {       // fixed order per thread, fixed order of the reduction below: deterministic
          pa += __hip_atomic_load(&D.objpart[2 * w2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          pb += __hip_atomic_load(&D.objpart[2 * w2 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(&D.objpart[2 * w2], 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(&D.objpart[2 * w2 + 1], 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        double cr = 0.0;
        for (int k = tid; k < K; k += bd) {              // (same arithmetic as k_objective_tables)
          const double rsd = (double)ldsRS[k] * FX_INV;
          double ck = 0.0;
          for (int bb = 0; bb < D.B; bb++) {
            const double od = (double)ldsO[bb * K + k] * FX_INV;
            const float o = (float)od, e = (float)(rsd * (double)D.Pr_b[bb]);
            const float m = D.theta[bb] * logf((o + e + 1.0f) / ((2.0f * e) + 1.0f));
            ck += od * (double)m;
          }
          cr += ck * (double)D.sigma[k];
        }
        pa = wsumd(pa); pb = wsumd(pb); cr = wsumd(cr);
        __syncthreads();                                  // (every wave is done reading the masses next to `red`)
        if (lane == 0) { red[3 * (tid >> 6)] = pa; red[3 * (tid >> 6) + 1] = pb; red[3 * (tid >> 6) + 2] = cr; }
        __syncthreads();
        if (tid == 0) {
          double sa = 0.0, sb = 0.0, sc = 0.0;
          for (int w2 = 0; w2 < (bd >> 6); w2++) { sa += red[3 * w2]; sb += red[3 * w2 + 1]; sc += red[3 * w2 + 2]; }
          if (D.p2p_world > 1) {
            // sharded: the two per-cell sums of every rank meet in the inboxes as well (one more exchange of the round, entries behind the
            // K x B table) and are added in RANK ORDER -- identical objective values on every rank, no host-launched collective per round
            // (the cross-entropy term comes from the global O / E tables: the same on every rank already)
            const int G = D.p2p_world, me = D.p2p_rank;
            const unsigned tagt = tag0 + (unsigned)nbk + 1u;
            const size_t part = (size_t)((D.chain_xseq + (unsigned)nbk + 1u) & 1u) * 8;
            p2p_send(D, part, nBK, tagt, __double_as_longlong(sa));
            p2p_send(D, part, nBK + 1, tagt, __double_as_longlong(sb));
            double va[8], vb[8];
#pragma unroll
            for (int gq = 0; gq < 8; gq++) {
              va[gq] = sa; vb[gq] = sb;
              if (gq < G && gq != me) {
                for (int which = 0; which < 2; which++) {
                  const unsigned long long* src = D.p2p_inbox_self() + ((part + gq) * P2P_CAP + nBK + which) * 2;
                  unsigned long long lo = 0, hi = 0;
                  int spins = 0;
                  for (;;) {
                    lo = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    hi = __hip_atomic_load(src + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    if ((unsigned)(lo >> 32) == tagt && (unsigned)(hi >> 32) == tagt) break;
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > SPIN_LIMIT) { atomicExch(&ctl[1], 5); break; }
                    if (dead(spins)) break;
                  }
                  const double x = __longlong_as_double((long long)((hi << 32) | (lo & 0xffffffffull)));
                  if (which == 0) va[gq] = x; else vb[gq] = x;
                }
              }
            }
            sa = 0.0; sb = 0.0;
            for (int gq = 0; gq < G; gq++) { sa += va[gq]; sb += vb[gq]; }
          }
          const double err = (double)__hip_atomic_load(&ctl[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + ((D.solve_err && *D.solve_err) ? 16.0 : 0.0);
          D.obj[0] = sa; D.obj[1] = sb; D.obj[2] = sa; D.obj[3] = sb; D.obj[4] = sc; D.obj[5] = err;
          if (D.tail_host_slot) {     // pinned host memory, mapped into the device: visible to the host once the event behind this launch completed
            __hip_atomic_store(&D.tail_host_slot[0], sa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&D.tail_host_slot[1], sb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&D.tail_host_slot[2], sc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&D.tail_host_slot[3], err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          }
        }
        for (unsigned long long i = tid; i < D.tail_n0; i += bd) D.tail_z0[i] = 0;
        for (unsigned long long i = tid; i < D.tail_n1; i += bd) D.tail_z1[i] = 0;
        __syncthreads();
        for (int i = tid; i < 8 * nbk + 24; i += bd) ctl[i] = 0;
      }
      return;
    }
    // ---------------- the workers
    {
    static_assert(!LEAN, "the chain runs two waves per SIMD (the 3- and 4-wave variants lost rounds 2 and 3 and were removed in round 5)");
    f32x4 accC[NCT], accS[NCT];
    int2 cellC = make_int2(-1, -1), cellS = make_int2(-1, -1);
    bool have = ts < te, have2 = false;
    // MODE 5 (no R stores: the accumulators are dead once a tile's contributions are summed): the rows of the wave's SECOND tile of the next
    // block are requested into a second register buffer in front of the contribution flush -- their latency passes during the flush, the
    // barrier and the arrival instead of between the two tiles' MFMAs behind it (the workers' phase in the folder's shadow: 5.0 us, the
    // folder needs 3-4).  With the stores the normalised rows of both tiles occupy the accumulators until behind the arrival: no room
    // (a second buffer there: 28 spilled VGPRs, DESIGN 4.1).
    RowRegs rowsN2; bool rows2_ok = false;
    // BOTH accumulator sets are filled ahead of the flag: the MFMAs of this wave's first tile of the current block (rows were
    // requested earlier) and, if it owns a second one, of that too -- after the flag only epilogues remain for up to two tiles
    auto first_tile_a = [&]() __attribute__((always_inline)) {
      cellC = cellN;
      const RowRegs rowsA = rowsN;
      cellN = cellNN;
      cellNN = tile_cell(ts + 2 * tstep);
      if constexpr (NOSTORE) { if (rows2_ok) rowsN = rowsN2; else ld_rows(next_rows(cellN, cellC), rowsN); }
      else ld_rows(next_rows(cellN, cellC), rowsN);
      dots_regs(rowsA, cellC.x >= 0, accC);
      // (the general-sigma variant has no registers to spare: 95 spills.  The wave-pair chain hoists ONE tile: with the second accumulator set live across
      //  the flag as well it needs 87 spilled registers instead of 13 and a block step at K = 200 takes 44.8 instead of 42.6 us, profiles/r6_pair_chain_tuning.txt)
      have2 = !PAIR && USIG && ts + tstep < te;
    };
    auto first_tile_b = [&]() __attribute__((always_inline)) {
      if (have2) {
        cellS = cellN;
        const RowRegs rowsB = rowsN;
        cellN = cellNN;
        cellNN = tile_cell(ts + 3 * tstep);
        ld_rows(next_rows(cellN, cellS), rowsN);
        dots_regs(rowsB, cellS.x >= 0, accS);
      }
    };
    // both hoisted tiles against one read of the centroid image, when the second tile's rows are in registers already (MODE 5: rowsN2)
    auto first_tiles = [&]() __attribute__((always_inline)) {
      if constexpr (NOSTORE && BF) {
        if (rows2_ok && USIG && ts + tstep < te) {
          cellC = cellN; cellS = cellNN;
          const RowRegs rowsA = rowsN, rowsB = rowsN2;
          cellN = tile_cell(ts + 2 * tstep); cellNN = tile_cell(ts + 3 * tstep);
          tile_dots_bf_regs2<NCT>(ldsB, rowsA, cellC.x >= 0, rowsB, cellS.x >= 0, rowmask, lane, D.NS2, accC, accS);
          ld_rows(next_rows(cellN, cellS), rowsN);
          have2 = true;
          return;
        }
      }
      first_tile_a(); first_tile_b();
    };
    if (have) first_tiles();
    // Geometry of the block AFTER the current one and the (cell, combination) pairs of this wave's first two tiles in it.  Requested
    // in the slack behind an arrival, a whole block ahead of their use: at the top of the epilogue phase the two dependent round trips
    // (scalar load of the block offsets, then the pairs) were 1.6 us of every block step's critical path.
    int p0n = 0, ten = 0, tsn = ts; bool haveN = false;
    int2 cN1 = make_int2(-1, -1), cNN1 = make_int2(-1, -1);
    auto fetch_next = [&](const int jb) __attribute__((always_inline)) {
      p0n = 0; ten = 0; haveN = false; cN1 = make_int2(-1, -1); cNN1 = make_int2(-1, -1);
      if (jb < nbk) {
        p0n = D.boff[jb];
        ten = (D.boff[jb + 1] - p0n) >> 4;
        if constexpr (CHAIN_CONTIG) chain_range(ten, tsn, ten);      // (ten: from here on the end of THIS wave's range)
        haveN = tsn < ten;
        if (haveN) { cN1 = D.lpair[p0n + 16 * tsn + c]; if (tsn + tstep < ten) cNN1 = D.lpair[p0n + 16 * (tsn + tstep) + c]; }
      }
    };
    fetch_next(1);
    unsigned long long wq = 0, wg = 0, ww = 0, wd = 0, wm = 0, w1 = 0, w2 = 0, w3 = 0, w_prev = wall_clock64();   // diagnostics (workgroup 0, wave 0)
    unsigned long long wv_busy = 0, wv_tiles = 0;    // per wave: table in LDS -> own work done (before the barrier), tiles owned
    auto lap = [&](unsigned long long& acc) { const unsigned long long t = wall_clock64(); acc += t - w_prev; w_prev = t; };
    for (int jj = 0; jj < nbk; jj++) {
      const unsigned tag = tag0 + (unsigned)jj;
      // MODE 6: the (cell, combination) pair of the wave's FOURTH tile of this block, requested ahead of the flag (the first three are in registers: the penalty
      // cache below then covers four tiles -- a stream's fourth tile fetched its rows level by level, three round trips on the busiest streams)
      int2 cell3 = make_int2(-1, -1);
      if constexpr (PAIR) { if (have && !have2) cell3 = tile_cell(ts + 3 * tstep); }
      if (tid == 0) {                       // one lane per workgroup polls the block flag (MODE 6: the count of folders done with this block)
        int spins = 0;
        if constexpr (PAIR) {
          while (__hip_atomic_load(&ctl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < nfold * (jj + 1)) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > SPIN_LIMIT) { atomicExch(&ctl[1], 2); break; }
            if (dead(spins)) break;
          }
        } else
        while ((int)((unsigned)__hip_atomic_load(&ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - tag) < 0) {
          __builtin_amdgcn_s_sleep(1);
          if (++spins > SPIN_LIMIT) { atomicExch(&ctl[1], 2); break; }
          if (dead(spins)) break;
        }
      }
      __syncthreads();
      lap(wq);
      if constexpr (PAIR) {
        // pen_cache_fill: the penalty rows of this wave's (up to four) tiles of the block -> log2(sum over the covariates) in its LDS cache
        tord = 0;
        ncache = (have && C <= 4) ? min(te - ts, PCT) : 0;      // (the tiles whose (cell, combination) pairs are in registers by now)
        const int qv[PCT] = {cellC.y, have2 ? cellS.y : cellN.y, have2 ? cellN.y : cellNN.y, have2 ? cellNN.y : cell3.y};
        float pv[PCT][4][2];
#pragma unroll
        for (int t = 0; t < PCT; t++) {
          const int q = max(__builtin_amdgcn_readfirstlane(qv[t]), 0) & QMASK;      // (no such tile: combination 0, never read)
#pragma unroll
          for (int cc = 0; cc < 4; cc++) {
            // (the level is wave-uniform: a scalar row base + the lane's 32-bit offset -- no 64-bit address arithmetic per load)
            const float* pr = D.pen + (size_t)__builtin_amdgcn_readfirstlane(ldsQlev[q * C + min(cc, C - 1)]) * KS + kb;
#pragma unroll
            for (int h = 0; h < 2; h++) pv[t][cc][h] = __hip_atomic_load(pr + min(lane + 64 * h, K - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
#pragma unroll
        for (int t = 0; t < PCT; t++) {
#pragma unroll
          for (int h = 0; h < 2; h++) {
            float sv = 0.0f;
#pragma unroll
            for (int cc = 0; cc < 4; cc++) sv += (cc < C) ? pv[t][cc][h] : 0.0f;      // (level order: the order of the launch-per-step kernels' sums)
            if (lane + 64 * h < KC) lpenT[t * KC + lane + 64 * h] = __builtin_amdgcn_logf(fmaxf(sv, FLT_MIN));
          }
        }
      } else
      for (int i = tid; i < nBK; i += bd) {   // the block's penalty table -> LDS (granules validate themselves)
        unsigned long long gv = __hip_atomic_load(&peng[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int spins = 0;
        while ((unsigned)(gv >> 32) != tag && ++spins < SPIN_LIMIT && !dead(spins)) { __builtin_amdgcn_s_sleep(1); gv = __hip_atomic_load(&peng[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        if ((unsigned)(gv >> 32) != tag) atomicExch(&ctl[1], 3);
        ldsPen[i] = __uint_as_float((unsigned)(gv & 0xffffffffu));
      }
      __syncthreads();
      lap(wg);
      const unsigned long long t_tab = w_prev;
      curq = -1;                            // the table changed: the penalty row of the first tile must be re-read
      // (od / oe: this wave's objective partial sums run through ALL blocks of the round in registers, one wave reduction and one
      //  slot store at the end of the launch instead of two 6-step 64-bit reductions per block on the critical path)
      // (geometry of the next block and the pairs of this wave's first two tiles in it: fetch_next, requested one block ahead)
      const bool more = jj + 1 < nbk;
      // The R rows of a wave's LAST TWO tiles of the block leave BEHIND the arrival.  Nobody reads a block's R rows before the launch
      // ends, but their stores -- 20 MB per block step from all workgroups at once, an HBM write burst the issuing waves sit behind --
      // were 3.2 of the 6.7 us a two-tile wave needed between "table in LDS" and its arrival (tools/chain_probe.py).  The normalised
      // rows stay in the two accumulator sets (epi_rows<DEFER>) through the contribution atomics, the barrier and the arrival, and are
      // stored in the folder's shadow, interleaved with the next block's MFMAs (which overwrite the same registers).
      bool two = false;                     // both hoisted tiles are the wave's last ones of this block: both epilogues deferred
      if (have) {
        int tile0 = ts + tstep;
        if (have2) two = ts + 2 * tstep >= te;
        // (waves that enter the tile loop: every load has landed before it, see the two-accumulator loop below; the others must not wait
        //  here -- the oldest operations in flight are the R stores they issued behind the previous arrival)
        if (!two) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
        if (have2) {
          if (!two) {                         // more than two tiles: the first one's epilogue now, the second becomes the pending tile
            epilogue(cellC.x, tile_q(cellC), accC);
#pragma unroll
            for (int ct = 0; ct < NCT; ct++) accC[ct] = accS[ct];
            cellC = cellS;
            tile0 = ts + 2 * tstep;
          }
        }
        if (!two) {
          for (int tile = tile0; tile < te; tile += tstep) {
            const int2 cellT = cellN;
            const RowRegs rowsA = rowsN;
            cellN = cellNN;
            cellNN = tile_cell(tile + 2 * tstep);
            ld_rows(next_rows(cellN, cellT), rowsN);
            f32x4 accT[NCT];
            dots_regs(rowsA, cellT.x >= 0, accT);   // MFMA pipe: tile i+1
            epilogue(cellC.x, tile_q(cellC), accC);                                           // VALU pipe: tile i
#pragma unroll
            for (int ct = 0; ct < NCT; ct++) accC[ct] = accT[ct];
            cellC = cellT;
          }
        }
        // next block's first rows requested first (older than everything below), then the epilogue(s) with DEFERRED stores and the
        // contribution atomics
        lap(w1);
        if (haveN) ld_rows(D.Zc + (size_t)(cN1.x >= 0 ? cN1.x : 0) * zs, rowsN);
        epi_begin(tile_q(cellC));
        epi_rows(cellC.x, accC, std::true_type{});
        if (two) {
          epi_begin(tile_q(cellS));
          epi_rows(cellS.x, accS, std::true_type{});
        }
        lap(w2);
        if constexpr (NOSTORE) {
          rows2_ok = haveN && tsn + tstep < ten;          // (uniform: the wave owns a second tile in the next block)
          if (rows2_ok) ld_rows(next_rows(cNN1, cN1), rowsN2);
        }
        if (curq >= 0) flush_run();
        lap(w3);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the wave's atomics have been performed (no stores queued behind them)
      } else {
        rows2_ok = false;
        if (haveN) ld_rows(D.Zc + (size_t)(cN1.x >= 0 ? cN1.x : 0) * zs, rowsN);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      lap(ww);
      wv_busy += w_prev - t_tab; wv_tiles += have ? (unsigned long long)((te - ts + tstep - 1) / tstep) : 0ull;
      // a BARE s_barrier (not __syncthreads(): nothing another wave of this workgroup reads is published here -- the barrier only
      // says "every wave's contribution atomics have been performed", each wave waited for its own above).
      __builtin_amdgcn_s_barrier();
      if (tid == 0) atomicAdd(&ctl[8 + 8 * jj + ((int)blockIdx.x & 7)], 1);          // arrival of this workgroup
      const bool st1 = have, st2 = have && two;
      const int sc1 = cellC.x, sc2 = cellS.x;
      if (more) { p0 = p0n; ts = tsn; te = ten; cellN = cN1; cellNN = cNN1; }
      lap(wd);
      have = haveN;
      // off the critical path, in the folder's shadow: rows of the finished tiles out, MFMAs of the next block's tiles in
      if constexpr (NOSTORE) { if (have) first_tiles(); else have2 = false; }
      else {
        if (st1) store_rows(sc1, accC);
        if (have) first_tile_a();
        if (st2) store_rows(sc2, accS);
        if (have) first_tile_b(); else have2 = false;
      }
      fetch_next(jj + 2);
      lap(wm);
    }
    od = wsumd(od); oe = wsumd(oe);
    if (D.chain_tail) {                     // the folder closes the round: the wave's sums go out write-through, then the workgroup arrives once more
      if (lane == 0) {
        double* slot = D.objpart + (size_t)wave * 2;
        __hip_atomic_store(&slot[0], od, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&slot[1], oe, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (tid == 0) atomicAdd(&ctl[16 + 8 * nbk + ((int)blockIdx.x & 7)], 1);
    } else if (lane == 0) {                 // slot row 0 (the other rows stay zero: k_round_tail sums and clears all of them)
      double* slot = D.objpart + (size_t)(PAIR ? (int)(blockIdx.x * 8 + (threadIdx.x >> 6)) : wave) * 2;      // (MODE 6: both waves of a pair carry partial sums)
      slot[0] += od; slot[1] += oe;
    }
    if (blockIdx.x == 0 && tid == 0 && D.chain_dbg) {
      atomicAdd(&D.chain_dbg[4], wq); atomicAdd(&D.chain_dbg[5], wg); atomicAdd(&D.chain_dbg[6], ww); atomicAdd(&D.chain_dbg[7], wd); atomicAdd(&D.chain_dbg[8], wm);
      atomicAdd(&D.chain_dbg[9], w1); atomicAdd(&D.chain_dbg[10], w2); atomicAdd(&D.chain_dbg[11], w3);
    }
    if ((blockIdx.x == 0 || blockIdx.x == 100) && lane == 0 && D.chain_dbg) {
      const int o = (blockIdx.x == 0 ? 16 : 32) + (tid >> 6);
      atomicAdd(&D.chain_dbg[o], wv_busy); atomicAdd(&D.chain_dbg[o + 8], wv_tiles);
    }
    if (blockIdx.x == 0 && (tid == 256 || tid == 320) && D.chain_dbg) {      // the same phase clocks for a SIMD's YOUNGER wave: wave 4 (two tiles), wave 5 (one)
      unsigned long long* const o = D.chain_dbg + (tid == 256 ? 48 : 56);
      atomicAdd(&o[0], wq); atomicAdd(&o[1], wg); atomicAdd(&o[2], ww); atomicAdd(&o[3], wd); atomicAdd(&o[4], wm); atomicAdd(&o[5], w1); atomicAdd(&o[6], w2); atomicAdd(&o[7], w3);
    }
    return;
    }
  }
  if (pre && (!DUAL || MODE == 2)) {   // (Lloyd: one accumulator set, its epilogue wants the tile's rows still in registers)
    for (int tile = ts; tile < te; tile += tstep) {
      const int2 cellA = cellN;
      const RowRegs rowsA = rowsN;
      cellN = cellNN;
      cellNN = tile_cell(tile + 2 * tstep);
      ld_rows(next_rows(cellN, cellA), rowsN);
      f32x4 acc[NCT];
      dots_regs(rowsA, cellA.x >= 0, acc);
      if constexpr (MODE == 2) erows = &rowsA;
      epilogue(cellA.x, tile_q(cellA), acc);
    }
  } else if (pre) {
    // two accumulator sets: the MFMAs of tile i+1 are issued before the (VALU / transcendental / store) epilogue of tile i
    // Head of cluster_cpp (MODE 1, D.head_norm): Z_corr <- normalise(Z_corr) (src/harmony.cpp:220) happens HERE, on the A-operand
    // registers of the tile -- the four lanes that hold a cell's row (k-slots 0..3) add up their squares, scale, and write the
    // normalised pieces back where they came from: no separate pass over Z_corr (it was 67 us of 256 per head at 1M cells).
    auto norm_rows = [&](RowRegs& r, const int cell) __attribute__((always_inline)) {
      if constexpr (BF) {     // split-bf16 row layout: the groups beyond the row were loaded clamped -- zero them, then as below
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
        float ss = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; t++) {
          r.v[t] = (rowmask >> t) & 1 ? r.v[t] : zero4;
          ss += r.v[t][0] * r.v[t][0] + r.v[t][1] * r.v[t][1] + r.v[t][2] * r.v[t][2] + r.v[t][3] * r.v[t][3];
        }
        ss += __shfl_xor(ss, 16, 64);
        ss += __shfl_xor(ss, 32, 64);
        float nrm = sqrtf(ss);
        nrm = (nrm == 0.0f) ? 1.0f : nrm;
        const float inv = 1.0f / nrm;
        float* zrow = D.Zc + (size_t)(cell >= 0 ? cell : 0) * zs;
#pragma unroll
        for (int t = 0; t < 4; t++) {
          r.v[t] = r.v[t] * inv;
          if (cell >= 0 && ((rowmask >> t) & 1)) *reinterpret_cast<f32x4*>(zrow + 32 * (t >> 1) + 8 * g + 4 * (t & 1)) = r.v[t];
        }
        return;
      }
      float ss = 0.0f;
#pragma unroll
      for (int t = 0; t < 4; t++) if (t < D.NT4) ss += r.v[t][0] * r.v[t][0] + r.v[t][1] * r.v[t][1] + r.v[t][2] * r.v[t][2] + r.v[t][3] * r.v[t][3];
#pragma unroll
      for (int u = 0; u < 3; u++) if (u < D.tail) ss += r.t[u] * r.t[u];
      ss += __shfl_xor(ss, 16, 64);
      ss += __shfl_xor(ss, 32, 64);
      float nrm = sqrtf(ss);
      nrm = (nrm == 0.0f) ? 1.0f : nrm;            // arma::normalise leaves a zero column alone
      const float inv = 1.0f / nrm;
      float* zrow = D.Zc + (size_t)(cell >= 0 ? cell : 0) * zs;
#pragma unroll
      for (int t = 0; t < 4; t++) if (t < D.NT4) {
        r.v[t] = r.v[t] * inv;
        if (cell >= 0) *reinterpret_cast<f32x4*>(zrow + 16 * t + 4 * g) = r.v[t];
      }
#pragma unroll
      for (int u = 0; u < 3; u++) if (u < D.tail) {
        r.t[u] *= inv;
        if (cell >= 0) zrow[16 * D.NT4 + 4 * u + g] = r.t[u];
      }
    };
    if (ts < te) {
      f32x4 accC[NCT];
      int2 cellC = cellN;
      {
        RowRegs rowsA = rowsN;
        cellN = cellNN;
        cellNN = tile_cell(ts + 2 * tstep);
        ld_rows(next_rows(cellN, cellC), rowsN);
        if constexpr (MODE == 1) { if (D.head_norm) norm_rows(rowsA, cellC.x); }
        dots_regs(rowsA, cellC.x >= 0, accC);
      }
      stamp(3);
      // every load of the prologue has landed before the loop is entered: hipcc merges the wait state of the two loop
      // entries conservatively, and row loads still pending on THIS edge would turn the loop-top waits into vmcnt(0..2),
      // which on the back edge means draining the 28 R stores of the tile just finished
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
      for (int tile = ts + tstep; tile < te; tile += tstep) {
        stamp(8);
        const int2 cellT = cellN;
        RowRegs rowsA = rowsN;
        cellN = cellNN;
        cellNN = tile_cell(tile + 2 * tstep);
        ld_rows(next_rows(cellN, cellT), rowsN);
        if constexpr (MODE == 1) { if (D.head_norm) norm_rows(rowsA, cellT.x); }
        stamp(9);
        f32x4 accT[NCT];
#ifdef HMX_TRACE
        const int dbg = D.upd_debug;   // 1 = no epilogue work, 2 = no MFMAs (WRONG RESULTS; timing experiments only)
        if (dbg & 2) {
#pragma unroll
          for (int ct = 0; ct < NCT; ct++) accT[ct] = rowsA.v[0];
        } else dots_regs(rowsA, cellT.x >= 0, accT);
        stamp(10);
        if (!(dbg & 1)) epilogue(cellC.x, tile_q(cellC), accC);
        else {
#pragma unroll
          for (int ct = 0; ct < NCT; ct++) od += (double)(accC[ct][0] + accC[ct][1] + accC[ct][2] + accC[ct][3]);
        }
        stamp(11);
#else
        dots_regs(rowsA, cellT.x >= 0, accT);   // MFMA pipe: tile i+1
        epilogue(cellC.x, tile_q(cellC), accC);                                           // VALU pipe: tile i
#endif
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) accC[ct] = accT[ct];
        cellC = cellT;
      }
      stamp(4);
      epilogue(cellC.x, tile_q(cellC), accC);
      stamp(5);
    }
  } else {
    for (int tile = ts; tile < te; tile += tstep) {
      const int2 cellA = cellN;
      cellN = cellNN;
      cellNN = tile_cell(tile + 2 * tstep);
      f32x4 acc[NCT];
      dots_stream(D.Zc + (size_t)(cellA.x >= 0 ? cellA.x : 0) * zs, cellA.x >= 0, acc);
      epilogue(cellA.x, tile_q(cellA), acc);
    }
  }
  if constexpr (MODE == 2) {
    __syncthreads();
    for (int i = threadIdx.x; i < K * D.d; i += blockDim.x)
      if (ltab[i]) atomicAdd((unsigned long long*)&D.lsum[i], (unsigned long long)ltab[i]);
    for (int i = threadIdx.x; i < K; i += blockDim.x)
      if (ltab[K * D.d + i]) atomicAdd(&D.lcnt[i], (unsigned long long)ltab[K * D.d + i]);
  } else if constexpr (MODE == 3) {
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) {   // the four row groups hold candidates for the same anchors
      unsigned long long v = best[ct];
      unsigned long long o = shfl_xor_u64(v, 16); v = o < v ? o : v;
      o = shfl_xor_u64(v, 32); v = o < v ? o : v;
      if (g == 0 && kcol(NCT, ct, c) < K && v != ~0ull) atomicMin(&D.seedmin[kcol(NCT, ct, c)], v);
    }
  } else {
    if (ts >= te) return;
    if (curq >= 0) flush_run();
    od = wsumd(od); oe = wsumd(oe);
    if (lane == 0 && !(MODE == 1 && D.head_noobj)) {      // (head_noobj: cluster_cpp's head, whose sums the first round's close overwrites unread)
      const int slotrow = (MODE == 0) ? (j % D.objslots) : 0;
      double* slot = D.objpart + ((size_t)slotrow * D.nwmax + wave) * 2;
      if (MODE == 0 && D.nb <= D.objslots) { slot[0] = od; slot[1] = oe; }  // written once per round: plain store
      else { slot[0] += od; slot[1] += oe; }
    }
    stamp(6);
    stamp(7);
  }
}




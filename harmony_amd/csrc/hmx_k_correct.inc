// hmx_k_correct.inc -- part of hmx_kernels.hip (included inside namespace hmx): objective tables and terms, the MoE ridge correction (statistics, device-side
// solve, apply), the VALU seeding / Lloyd fallbacks, centroid images.  Not built into the split-bf16 unit.
#if !HMX_TILE_BF
// cross-entropy term of the objective from the K x B tables alone (src/harmony.cpp:162):
//   sum_k sigma_k sum_b theta_b log((O+E+1)/(2E+1)) * O[k,b]     (O[k,b] = sum_{i in b} R_ki)
// single workgroup; obj[2..4] = {dist, entropy, cross} snapshot, obj[0..1] reset.
__global__ __launch_bounds__(TPB) void k_objective_tables(Dev D) {
  __shared__ double red[TPB];
  const int K = D.K, B = D.B;
  double cross = 0.0;
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    long long rs = 0;
    for (int b = 0; b < B; b++) {
      if (b < D.B0) rs += D.O_fx[(size_t)b * K + k];
    }
    const double rsd = (double)rs * FX_INV;
    double ck = 0.0;
    for (int b = 0; b < B; b++) {
      const double od = (double)D.O_fx[(size_t)b * K + k] * FX_INV;
      const float o = (float)od, e = (float)(rsd * (double)D.Pr_b[b]);
      const float m = D.theta[b] * logf((o + e + 1.0f) / ((2.0f * e) + 1.0f));
      ck += od * (double)m;
    }
    cross += ck * (double)D.sigma[k];
  }
  red[threadIdx.x] = cross;
  __syncthreads();
  for (int off = TPB / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    D.obj[2] = D.obj[0]; D.obj[3] = D.obj[1]; D.obj[4] = red[0];
    D.obj[5] = (D.chain_ctl ? (double)D.chain_ctl[1] : 0.0) + ((D.solve_err && *D.solve_err) ? 16.0 : 0.0);      // the chain's error word (+ 16: singular ridge system) rides along with the objective snapshot
  }
  // (this single-workgroup kernel closes every round: it also resets the chain's control block for the next one -- one memset
  //  launch less per round; the shuffle kernels cannot do it, they may run on the side stream while a chain is in flight)
  __syncthreads();
  if (D.chain_ctl) for (int i = threadIdx.x; i < 8 * D.nb + 24; i += blockDim.x) D.chain_ctl[i] = 0;
}

// obj_arith: the objective's three K x N term matrices (src/harmony.cpp:160-162, see hmx_seq.hip k_obj_terms) with the distances from the
// matrix cores: static 16-cell tiles like the head, the R row and the term rows as 16-byte accesses (a lane's clusters are consecutive,
// kcol).  Round 3's cluster-lane VALU version took 1.44 ms per evaluation at 1M cells, a quarter of the reference-arithmetic run.
// T[0] = R % dist, T[1] = (R % log R) % sigma, T[2] = (R % sigma) % (M Phi); rows at the cells' ORIGINAL positions, k fastest.
// Round 5: (1) tiles run over the ORIGINAL cell order (16 consecutive original cells per tile, rows gathered through invperm): a tile's 16 rows
// of each term array are 16 K contiguous floats -- whole 128-byte lines at K = 100; the cells of a tile no longer share a combination, so the
// M rows are fetched per row.  (2) A software pipeline like k_tile's: cell ids two tiles ahead, and ALL loads of tile i + 1 (embedding rows in
// registers, R rows, M rows) are issued before the stores of tile i -- vector memory operations retire in issue order on gfx9, so a load queued
// behind a tile's 84 stores waits for them to drain; the round-4 kernel did that four times per tile (1.02 ms per evaluation at 1M cells, 21
// evaluations per run).  (3) log R through v_log_f32 (1 ulp; the term enters a sum of K N values): 3 instructions instead of logf's ~30.
// (4) all3 = 0 (the default since round 5): only T[0] = R % dist is materialised -- the entropy and cross-entropy terms are recomputed from R by
// the pass itself (k_seq_objr_pass, hmx_seq.hip: the same roundings), a third of the writes here and a third less to read in every pass.
template <int NCT, bool all3, bool DIST = false>      // DIST: T[0] = dist_mat itself (the cache of a cluster_cpp call's rounds: Y and Z_corr do not change between them)
__global__ __launch_bounds__(256, (NCT <= 8 ? 2 : 1)) void k_obj_terms_mfma(Dev D, const float* __restrict__ M, float* __restrict__ T, long long stride) {      // (two waves per SIMD: with 268 registers there was one, and nothing hid the tile's memory latencies)
  extern __shared__ __attribute__((aligned(16))) f32x4 ldsI[];
  constexpr int NFULL = NCT >> 2, RT = NCT & 3;
  const int K = D.K, C = D.C, zs = D.zs, n = D.n;
  const int nY4 = D.NQ * D.NS * 64;
  { const f32x4* src = reinterpret_cast<const f32x4*>(D.Yimg);
    for (int i = threadIdx.x; i < nY4; i += blockDim.x) ldsI[i] = src[i]; }
  __syncthreads();
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nw = (int)((gridDim.x * blockDim.x) >> 6);
  const float lmin = __builtin_amdgcn_logf(FLT_MIN) * 0.69314718055994530942f;
  const int ntiles = (n + 15) >> 4;
  const int per = (ntiles + nw - 1) / nw;           // contiguous tile ranges per wave: consecutive tiles write consecutive lines
  const int t_lo = min(wave * per, ntiles), t_hi = min(t_lo + per, ntiles);
  if (t_lo >= t_hi) return;
  const float* __restrict__ Rp = D.R;
  const float* __restrict__ Zp = D.Zc;
  const int* __restrict__ qlevp = D.qlev;
  struct Ids { int cell, q; };
  auto ids_of = [&](const int tile) -> Ids {         // this lane's A-operand cell of `tile` (clamped: any valid cell beyond the end)
    Ids I; I.cell = D.invperm[min(16 * min(tile, ntiles - 1) + c, n - 1)]; I.q = D.combo[I.cell]; return I;
  };
  // per tile and lane: the R and M values of rows 4g .. 4g + 3 at this lane's clusters -- the layout of the accumulators
  struct Vals { f32x4 r[NCT], m[NCT]; };
  auto vals_of = [&](const Ids& I, Vals& V) __attribute__((always_inline)) {
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int cell = __shfl(I.cell, 4 * g + reg, 64), q = __shfl(I.q, 4 * g + reg, 64);
      const float* __restrict__ rrow = Rp + (size_t)cell * K;
      int lev[4];
#pragma unroll
      for (int cc = 0; cc < 4; cc++) lev[cc] = qlevp[q * C + min(cc, C - 1)];
#pragma unroll
      for (int qd = 0; qd < NFULL; qd++) {
        const int k0 = min(64 * qd + 4 * c, K - 4);
        const f32x4 r4 = *reinterpret_cast<const f32x4*>(rrow + k0);
        f32x4 m4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int cc = 0; cc < 4; cc++) {
          if (all3 && cc < C) {
            const f32x4 mm = *reinterpret_cast<const f32x4*>(M + (size_t)lev[cc] * K + k0);
#pragma unroll
            for (int i = 0; i < 4; i++) m4[i] = __fadd_rn(m4[i], mm[i]);
          }
        }
        for (int cc = 4; cc < C && all3; cc++) {
          const f32x4 mm = *reinterpret_cast<const f32x4*>(M + (size_t)qlevp[q * C + cc] * K + k0);
#pragma unroll
          for (int i = 0; i < 4; i++) m4[i] = __fadd_rn(m4[i], mm[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) { V.r[4 * qd + i][reg] = r4[i]; V.m[4 * qd + i][reg] = m4[i]; }
      }
#pragma unroll
      for (int jj = 0; jj < RT; jj++) {
        const int k = min(64 * NFULL + RT * c + jj, K - 1);
        float m = 0.0f;
        for (int cc = 0; cc < C && all3; cc++) m = __fadd_rn(m, M[(size_t)qlevp[q * C + cc] * K + k]);
        V.r[4 * NFULL + jj][reg] = rrow[k]; V.m[4 * NFULL + jj][reg] = m;
      }
    }
  };
  float sg[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) sg[ct] = D.sigma[min(kcol(NCT, ct, c), K - 1)];
  Ids idN = ids_of(t_lo), idNN = ids_of(t_lo + 1);
  RowRegs rowsN;
  Vals VN;
  load_rows(Zp + (size_t)idN.cell * zs, g, D.NT4, D.tail, rowsN);
  vals_of(idN, VN);
  for (int tile = t_lo; tile < t_hi; tile++) {
    const int o0 = 16 * tile;
    const bool av = o0 + c < n;
    const RowRegs rowsA = rowsN;
    const Vals V = VN;
    f32x4 acc[NCT];
    tile_dots_regs<NCT>(ldsI, rowsA, av, lane, D.NS, D.NT4, D.tail, acc);
    // everything tile + 1 needs, requested BEFORE this tile's stores
    idN = idNN; idNN = ids_of(tile + 2);
    load_rows(Zp + (size_t)idN.cell * zs, g, D.NT4, D.tail, rowsN);
    vals_of(idN, VN);
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int cl = 4 * g + reg;
      const bool cv = o0 + cl < n;
      float* __restrict__ t0p = T + (size_t)(o0 + (cv ? cl : 0)) * K;
      float* __restrict__ t1p = t0p + (size_t)stride;
      float* __restrict__ t2p = t1p + (size_t)stride;
      float a0[NCT], a1[NCT], a2[NCT];
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) {
        const float r = V.r[ct][reg];
        const float dist = __fmul_rn(2.0f, __fsub_rn(1.0f, acc[ct][reg]));
        a0[ct] = DIST ? dist : __fmul_rn(r, dist);
        if constexpr (all3) {
          const float lg = (r > 0.0f) ? __fmul_rn(__builtin_amdgcn_logf(r), 0.69314718055994530942f) : lmin;      // arma::trunc_log
          a1[ct] = __fmul_rn(__fmul_rn(r, lg), sg[ct]);
          a2[ct] = __fmul_rn(__fmul_rn(r, sg[ct]), V.m[ct][reg]);
        } else { a1[ct] = 0.0f; a2[ct] = 0.0f; }
      }
      if (cv) {
#pragma unroll
        for (int qd = 0; qd < NFULL; qd++) {
          const int k0 = 64 * qd + 4 * c;
          if (4 * qd < first_partial_ct(NCT) || k0 < K) {
            const f32x4 v0 = {a0[4 * qd], a0[4 * qd + 1], a0[4 * qd + 2], a0[4 * qd + 3]}, v1 = {a1[4 * qd], a1[4 * qd + 1], a1[4 * qd + 2], a1[4 * qd + 3]},
                        v2 = {a2[4 * qd], a2[4 * qd + 1], a2[4 * qd + 2], a2[4 * qd + 3]};
            // (streaming stores: the arrays are read back by the passes only after the whole evaluation has been written -- 1.2 GB, nothing to keep in L2)
            __builtin_nontemporal_store(v0, reinterpret_cast<f32x4*>(t0p + k0));
            if constexpr (all3) { __builtin_nontemporal_store(v1, reinterpret_cast<f32x4*>(t1p + k0)); __builtin_nontemporal_store(v2, reinterpret_cast<f32x4*>(t2p + k0)); }
          }
        }
#pragma unroll
        for (int jj = 0; jj < RT; jj++) {
          const int k = 64 * NFULL + RT * c + jj;
          if (k < K) { t0p[k] = a0[4 * NFULL + jj]; if constexpr (all3) { t1p[k] = a1[4 * NFULL + jj]; t2p[k] = a2[4 * NFULL + jj]; } }
        }
      }
    }
  }
}

// --------------------------------------------------------------------------------------
// MoE ridge correction (src/harmony.cpp:345-638)
//   k_moe_stats : per combination q and cluster k:  nq = sum_i R_ki,  Sq = sum_i R_ki z_i
//                 (the sufficient statistics of Phi* diag(R_k) Phi*^T and Phi* diag(R_k) Z^T)
//   host        : K small ridge solves in fp64 -> correction table Wq[q][k][:]
//   k_moe_apply : Z_corr_i = Z_orig_i - sum_k R_ki Wq[q(i)][k][:]
// --------------------------------------------------------------------------------------
// grid.y = cluster chunks of 128, grid.z = PC chunks of DP (DP = 4..32 in steps of 4, chosen so that the
// chunks cover d with little padding: d=50 -> 2 chunks of 28)
template <int DP>
__global__ __launch_bounds__(TPB) void k_moe_stats(Dev D) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
  const int d = D.d, K = D.K;
  const int k0 = blockIdx.y * 128 + lane, k1 = k0 + 64;
  const int zoff = blockIdx.z * DP;
  const int dch = min(DP, d - zoff);
  for (int it = wave; it < D.nitems; it += nw) {
    const Item item = D.items[it];
    float a0[DP], a1[DP];
#pragma unroll
    for (int j = 0; j < DP; j++) { a0[j] = 0.0f; a1[j] = 0.0f; }
    double n0 = 0.0, n1 = 0.0;
    size_t cell = (size_t)item.start;
    const int ls = min(lane, dch - 1), k0s = min(k0, K - 1), k1s = min(k1, K - 1);
    float zn = ld_or(D.Zo, cell * D.zs + zoff + ls, lane < dch, 0.0f);
    float r0n = ld_or(D.R, cell * K + k0s, k0 < K, 0.0f);
    float r1n = ld_or(D.R, cell * K + k1s, k1 < K, 0.0f);
    for (int p = 0; p < item.cnt; p++) {
      const float zr = zn, r0 = r0n, r1 = r1n;
      if (p + 1 < item.cnt) {  // software prefetch of the next cell's rows
        cell = (size_t)(item.start + p + 1);
        zn = ld_or(D.Zo, cell * D.zs + zoff + ls, lane < dch, 0.0f);
        r0n = ld_or(D.R, cell * K + k0s, k0 < K, 0.0f);
        r1n = ld_or(D.R, cell * K + k1s, k1 < K, 0.0f);
      }
      n0 += (double)r0; n1 += (double)r1;
#pragma unroll
      for (int j = 0; j < DP; j++) {
        const float zj = rlane(zr, j);
        a0[j] = fmaf(r0, zj, a0[j]);
        a1[j] = fmaf(r1, zj, a1[j]);
      }
    }
    double* S = D.Sq + (size_t)item.q * d * K;
#pragma unroll
    for (int j = 0; j < DP; j++) {
      if (j < dch) {
        if (k0 < K) atomicAdd(&S[(size_t)k0 * d + zoff + j], (double)a0[j]);
        if (k1 < K) atomicAdd(&S[(size_t)k1 * d + zoff + j], (double)a1[j]);
      }
    }
    if (blockIdx.z == 0) {
      if (k0 < K) atomicAdd(&D.nq[(size_t)item.q * K + k0], n0);
      if (k1 < K) atomicAdd(&D.nq[(size_t)item.q * K + k1], n1);
    }
  }
}

// one workgroup per apply item (<= APPLY_CELLS cells of one combination); Wq[q] staged in LDS
// as [K][DS] (DS = 64*DPL); lane = PC.
template <int KPL, int DPL>
__global__ __launch_bounds__(TPB) void k_moe_apply(Dev D) {
  extern __shared__ __attribute__((aligned(16))) float ldsW[];
  constexpr int CB = 4;
  constexpr int DS = 64 * DPL;
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const int d = D.d, K = D.K;
  for (int it = blockIdx.x; it < D.naitems; it += gridDim.x) {
    const Item item = D.aitems[it];
    __syncthreads();
    const float* W = D.Wq + (size_t)item.q * K * d;
    for (int i = threadIdx.x; i < K * DS; i += blockDim.x) {
      const int k = i / DS, jj = i - k * DS;
      ldsW[i] = ld_or(W, (size_t)k * d + min(jj, d - 1), jj < d, 0.0f);
    }
    __syncthreads();
    const int per = (item.cnt + 3) / 4;
    const int s = item.start + wib * per, e = min(item.start + item.cnt, s + per);
    for (int p = s; p < e; p += CB) {
      const int nc = min(CB, e - p);
      float rr[CB][KPL], corr[CB][DPL];
#pragma unroll
      for (int c = 0; c < CB; c++) {
#pragma unroll
        for (int q = 0; q < KPL; q++) {
          const int k = lane + 64 * q;
          rr[c][q] = ld_or(D.R, (size_t)min(p + c, e - 1) * K + min(k, K - 1), c < nc && k < K, 0.0f);
        }
#pragma unroll
        for (int t = 0; t < DPL; t++) corr[c][t] = 0.0f;
      }
#pragma unroll
      for (int q = 0; q < KPL; q++) {
        const int kend = min(64, K - 64 * q);
        for (int kk = 0; kk < kend; ++kk) {
          float w[DPL];
#pragma unroll
          for (int t = 0; t < DPL; t++) w[t] = ldsW[(64 * q + kk) * DS + 64 * t + lane];
#pragma unroll
          for (int c = 0; c < CB; c++) {
            const float rk = rlane(rr[c][q], kk);
#pragma unroll
            for (int t = 0; t < DPL; t++) corr[c][t] = fmaf(rk, w[t], corr[c][t]);
          }
        }
      }
#pragma unroll
      for (int c = 0; c < CB; c++) {
        if (c < nc) {
          const size_t cell = (size_t)(p + c);
#pragma unroll
          for (int t = 0; t < DPL; t++) {
            const int jj = 64 * t + lane;
            if (jj < d) D.Zc[cell * D.zs + jj] = D.Zo[cell * D.zs + jj] - corr[c][t];
          }
        }
      }
    }
  }
}

// index of centroid entry (PC j, cluster k) in the MFMA B-operand image (inverse of the host builder in upload_Y)
__device__ __forceinline__ size_t yimg_index(const Dev& D, int j, int k) {
  int s_, p_;
  if (j < 16 * D.NT4) { const int t = j >> 4, r = j & 15; p_ = r >> 2; s_ = 4 * t + (r & 3); }
  else { const int r = j - 16 * D.NT4; s_ = 4 * D.NT4 + (r >> 2); p_ = r & 3; }
  int qd, i, c;
  kcol_inv(D.NCT, k, qd, i, c);
  return ((((size_t)qd * D.NS + s_) * 4 + p_) * 16 + c) * 4 + i;
}
// k_moe_solve: the K ridge systems of moe_correct_ridge_cpp ON THE DEVICE (src/harmony.cpp:358-611), fp64, one workgroup
// per cluster -- no D2H of the statistics, no host solve, no H2D of the correction table: the whole correction is a
// chain of kernels with no host synchronisation.  Per cluster k:
//   kept levels (O[k,b] / N_b > cutoff and >= 2 such levels in the covariate, :368-402), lambda_k (fixed or alpha * E, :434-439),
//   cov = Phi* diag(R_k) Phi*^T + Lambda and rhs = Phi* diag(R_k) Z^T assembled from the per-combination statistics
//   (subset path = masks, :440-547), blocked Cholesky -- Phi* diag(R_k) Phi*^T + Lambda is symmetric positive definite whenever the
//   reference's arma::inv succeeds; a non-positive pivot raises flag bit 2 (HMX_ERR_SOLVE at the next objective read or getter; the
//   host solve path, HMX_MOE_SOLVE=host, retries with LU) --, W = cov^-1 rhs, Y[:,k] = W[0,:], W[0,:] = 0 (:610-611), correction table Wq[q][k][:] = sum of the kept
//   levels' rows of combination q (+ its MFMA image), Y <- normalise (:633).
// flags[k]: bit 0 subset path, bit 1 skipped (no covariate with two kept levels), bit 2 singular system.
// SYSLDS: cov and rhs live in LDS behind the rest (A.lds_sys_off) instead of the global scratch: the ~20 workgroup barriers of a solve then separate LDS accesses,
// not global round trips.  Same operations in the same order either way.
// (two kernels over one body, k_moe_solve: global scratch, k_moe_solve_lds: SYSLDS)
template <bool SYSLDS>
__device__ __forceinline__ void moe_solve_body(const Dev& D, const SolveArgs& A) {
  extern __shared__ int sm_[];
  const int K = D.K, B = D.B, C = D.C, d = D.d, Q = D.Q, M = B + 1;
  const int k = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  int* row_of = sm_;                 // [B]
  int* keepl = sm_ + B;              // [B] kept levels in order
  int* okb = sm_ + 2 * B;            // [B]
  int* misc = sm_ + 3 * B;           // [0] m, [1] active, [2] full, [3] fail, [4..4+C) cov_levels
  int* prow = sm_ + 3 * B + 4 + C;   // [B + 1] design row (reference order: intercept, kept levels ascending) -> row of the system as it is solved
  const int PAN_OFF = (4 * B + 6 + C) & ~1;      // ints in front of the fp64 panel space
  __shared__ int sch_nd;             // levels of the covariate whose (diagonal) block is eliminated first, 0: none
  double* cov; double* rhs;
  if constexpr (SYSLDS) { cov = reinterpret_cast<double*>(reinterpret_cast<char*>(sm_) + A.lds_sys_off); rhs = cov + (size_t)M * M; }
  else { cov = A.cov + (size_t)k * M * M; rhs = A.rhs + (size_t)k * d * M; }
  for (int b = tid; b < B; b += nt) {
    const float o = A.Of ? A.Of[(size_t)b * K + k] : (float)((double)D.O_fx[(size_t)b * K + k] * FX_INV);
    okb[b] = (o / D.sizes[b]) > A.cutoff ? 1 : 0;
  }
  __syncthreads();
  if (tid == 0) {
    for (int c = 0; c < C; c++) misc[4 + c] = 0;
    for (int b = 0, cv = 0; b < B; b++) { if (!(b < A.cov_bounds[cv])) cv++; if (okb[b]) misc[4 + cv]++; }
    int nk = 0;
    for (int b = 0, cv = 0; b < B; b++) {
      if (cv < C && !(b < A.cov_bounds[cv])) cv++;
      if (okb[b] && misc[4 + cv] > 1) { keepl[nk] = b; row_of[b] = nk + 1; nk++; } else row_of[b] = -1;
    }
    int act = 0; for (int c = 0; c < C; c++) if (misc[4 + c] > 1) act++;
    misc[0] = nk + 1; misc[1] = act; misc[2] = (nk == B) ? 1 : 0; misc[3] = 0;
    // Every covariate's own block of Phi* diag(R_k) Phi*^T + Lambda is DIAGONAL (a cell has one level per covariate).  The rows of
    // the covariate with the most kept levels go LAST and are eliminated in closed form (Schur complement): the dense Cholesky
    // shrinks from m to m - nd rows -- 201 -> 73 at configs[4]'s 8 > 64 > 128 levels, 1 + B -> 1 for a single covariate.
    int cstar = -1, nd = 0;
    for (int c = 0; c < C; c++) if (misc[4 + c] > 1 && misc[4 + c] > nd) { nd = misc[4 + c]; cstar = c; }
    if (nd < 8 || A.solve_f32) { nd = 0; cstar = -1; }
    sch_nd = nd;
    prow[0] = 0;
    int nx = 1, nl = nk + 1 - nd;
    for (int a = 1; a <= nk; a++) {
      const int b = keepl[a - 1];
      int cv = 0; while (cv < C - 1 && !(b < A.cov_bounds[cv])) cv++;
      prow[a] = (cv == cstar) ? nl++ : nx++;
    }
  }
  __syncthreads();
  const int m = misc[0];
  const bool full = misc[2] != 0, skipped = !full && misc[1] == 0;
  // correction rows of this cluster start from zero (also the result for a skipped cluster, :449-452)
  for (int i = tid; i < Q * d; i += nt) { const int q = i / d, j = i - q * d; D.Wq[((size_t)q * K + k) * d + j] = 0.0f; }
  // Combination -> design rows table in LDS (the panel space, free until the Cholesky): with it every entry of the system is summed by ONE
  // thread over the combinations in ascending order -- the same order as the combination-by-combination loop below (bit-identical
  // results), without its Q workgroup barriers and read-modify-write round trips (0.26 ms of a 1.2 ms solve at configs[4]).
  const int nd_ = sch_nd, ms_ = m - nd_;
  const bool qtab = !skipped && ((size_t)2 * Q * (C + 1) + M + 1) * sizeof(int) <= A.lds_body_bytes;
  unsigned long long* const dmask = (A.lds_mask_off && qtab && nd_ > 0) ? reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(sm_) + A.lds_mask_off) : nullptr;
  const int mw = (nd_ + 63) >> 6;         // mask words per row: bit (r - ms) of dmask[a] <=> B[r][a] != 0 (level r meets row a in some combination)
  if (qtab) {
    int* const qr = sm_ + PAN_OFF;          // [Q][C + 1]: qr[q][0] = 0 (intercept) if any level of q is kept, else -1; qr[q][1 + c] = row of covariate c's level or -1
    if (dmask) for (int i = tid; i < ms_ * mw; i += nt) dmask[i] = 0ull;
    __syncthreads();
    for (int q = tid; q < Q; q += nt) {
      int any = -1, rD = -1;
      for (int c = 0; c < C; c++) {
        const int ro = row_of[D.qlev[q * C + c]];
        const int r = ro >= 0 ? prow[ro] : -1;
        qr[q * (C + 1) + 1 + c] = r;
        if (r >= 0) any = 0;
        if (r >= ms_) rD = r;
      }
      qr[q * (C + 1)] = any;
      if (dmask && rD >= 0) {
        atomicOr(&dmask[0 * mw + ((rD - ms_) >> 6)], 1ull << ((rD - ms_) & 63));
        for (int c = 0; c < C; c++) { const int r = qr[q * (C + 1) + 1 + c]; if (r >= 0 && r < ms_) atomicOr(&dmask[(size_t)r * mw + ((rD - ms_) >> 6)], 1ull << ((rD - ms_) & 63)); }
      }
    }
    __syncthreads();
    auto in_q = [&](const int* r, const int a) { bool in = (a == 0); for (int c = 0; c < C; c++) in |= (r[1 + c] == a); return in; };
    // per design row: the combinations that contain it, ascending (row 0: every combination with a kept level)
    int* const qoff = qr + Q * (C + 1);     // [m + 1]
    int* const qlst = qoff + M + 1;         // [<= Q (C + 1)]
    for (int a = tid; a < m; a += nt) {
      int cnt = 0;
      for (int q = 0; q < Q; q++) { const int* r = qr + q * (C + 1); if (r[0] == 0 && in_q(r, a)) cnt++; }
      qoff[a + 1] = cnt;
    }
    __syncthreads();
    if (tid == 0) { qoff[0] = 0; for (int a = 0; a < m; a++) qoff[a + 1] += qoff[a]; }
    __syncthreads();
    for (int a = tid; a < m; a += nt) {
      int o = qoff[a];
      for (int q = 0; q < Q; q++) { const int* r = qr + q * (C + 1); if (r[0] == 0 && in_q(r, a)) qlst[o++] = q; }
    }
    __syncthreads();
    if (!A.ref_tot) {
    for (int i = tid; i < m * d; i += nt) {
      const int j = i / m, a = i - j * m;
      double sacc = 0.0;
      for (int x = qoff[a]; x < qoff[a + 1]; x++) sacc += D.Sq[((size_t)qlst[x] * K + k) * d + j];
      rhs[i] = sacc;
    }
    for (int i = tid; i < m * m; i += nt) {
      const int cb = i / m, ra = i - cb * m;
      if (ra < cb) continue;                              // lower triangle, mirrored below
      double sacc = 0.0;
      if (!(cb >= ms_ && ra != cb)) {                    // (the eliminated covariate's own block is diagonal)
        // (the lists of the rows ra > 0 are short -- a level's combinations --; every one of them contains row 0)
        for (int x = qoff[ra]; x < qoff[ra + 1]; x++) { const int q = qlst[x]; if (cb == 0 || cb == ra || in_q(qr + q * (C + 1), cb)) sacc += D.nq[(size_t)q * K + k]; }
      }
      cov[(size_t)cb * m + ra] = sacc;
      cov[(size_t)ra * m + cb] = sacc;
    }
    }   // (!A.ref_tot)
    __syncthreads();
  }
  if (!skipped) {
    if (A.ref_tot) {
      // ridge_arith with several covariates: every entry of the system IS one of the reference's sequential fp32 accumulators
      // (hmx_seq.hip): Phi_Rk * Phi_moe_t entry (a, a2) = the sum of R_k over the kept cells that carry both design rows, in original order
      // (src/harmony.cpp:561-568; the intercept row is in every cell, a level row in its level's cells, two levels of different covariates
      // in their pair's cells, two levels of one covariate never meet); the right-hand sides = the same chains over fl(z_j R_k) (:592-608).
      auto chain_of = [&](const int a) { return a == 0 ? 0 : 1 + keepl[a - 1]; };
      for (int i = tid; i < m * d; i += nt) {
        const int j = i / m, a = i - j * m;
        rhs[(size_t)j * m + prow[a]] = (double)A.ref_tot[((size_t)chain_of(a) * K + k) * 64 + j];
      }
      for (int i = tid; i < m * m; i += nt) {
        const int a2 = i / m, a = i - a2 * m;
        float v;
        if (a == 0 || a2 == 0 || a == a2) v = A.ref_tot[((size_t)chain_of(a == 0 ? a2 : a) * K + k) * 64 + 63];
        else {
          const int b = keepl[a - 1], b2 = keepl[a2 - 1];
          int cv = 0, cv2 = 0;
          while (cv < C - 1 && !(b < A.cov_bounds[cv])) cv++;
          while (cv2 < C - 1 && !(b2 < A.cov_bounds[cv2])) cv2++;
          const int pi = (cv == cv2) ? -1 : A.pair_idx[(size_t)min(b, b2) * B + max(b, b2)];
          v = pi >= 0 ? A.pair_tot[(size_t)pi * K + k] : 0.0f;
        }
        cov[(size_t)prow[a2] * m + prow[a]] = (double)v;
      }
      __syncthreads();
    }
    if (!qtab && !A.ref_tot) {
    for (int i = tid; i < m * m; i += nt) cov[i] = 0.0;
    for (int i = tid; i < m * d; i += nt) rhs[i] = 0.0;
    __syncthreads();
    for (int q = 0; q < Q; q++) {   // sequential over combinations (fixed order), parallel inside
      int rows[17]; int nr = 1; rows[0] = 0;
      for (int c = 0; c < C; c++) { const int ro = row_of[D.qlev[q * C + c]]; if (ro >= 0) rows[nr++] = prow[ro]; }
      if (nr > 1) {   // (none of its levels kept: the combination's cells do not enter, :400,456-460)
        const double n = D.nq[(size_t)q * K + k];
        for (int i = tid; i < nr * nr; i += nt) { const int a = i / nr, b2 = i - a * nr; cov[(size_t)rows[b2] * m + rows[a]] += n; }
        const double* sq = D.Sq + ((size_t)q * K + k) * d;
        for (int i = tid; i < nr * d; i += nt) { const int j = i / nr, a = i - j * nr; rhs[(size_t)j * m + rows[a]] += sq[j]; }
      }
      __syncthreads();
    }
    }   // (!qtab)
    if (A.use_s0 && !A.ref_tot) {   // ridge_arith = 1, one covariate: the intercept row's own sequential fp32 totals (k_seq_ridge_store)
      if (tid == 0) cov[0] = D.n0[k];
      for (int j = tid; j < d; j += nt) rhs[(size_t)j * m] = D.S0[(size_t)k * d + j];
    }
    // lambda on the diagonal (intercept 0): estimation lambda = alpha * E[k,b]
    long long rs = 0;
    for (int b0 = 0; b0 < D.B0; b0++) rs += D.O_fx[(size_t)b0 * K + k];
    const double rsd = (double)rs * FX_INV;
    for (int a = 1 + tid; a < m; a += nt) {
      const int b = keepl[a - 1];
      const float lam = A.lambda ? A.lambda[b + 1] : (A.Ef ? A.Ef[(size_t)b * K + k] : (float)(rsd * (double)D.Pr_b[b])) * A.alpha;
      const int pa = prow[a];
      if (A.solve_f32 || A.use_s0) cov[(size_t)pa * m + pa] = (double)__fadd_rn((float)cov[(size_t)pa * m + pa], lam);     // an fp32 matrix in the reference
      else cov[(size_t)pa * m + pa] += (double)lam;
    }
    __syncthreads();
    if (A.solve_f32 && C == 1) {
      // The reference's own inverse for one covariate (src/harmony.cpp:575-586): Phi_cov is an arrowhead matrix, inverted in closed
      // form in fp32, and W = inv_cov * (the right-hand sides) accumulates in fp32, column of inv_cov after column (:599-608).
      float* const ac = reinterpret_cast<float*>(sm_ + PAN_OFF);     // [m] each (the Cholesky's panel space; solve_f32: no elimination, prow is the identity)
      float* const bb = ac + m; float* const acb = bb + m; float* const uu = acb + m;
      for (int a = tid; a < m; a += nt) {
        ac[a] = (a == 0) ? 1.0f : -(float)cov[(size_t)a * m];
        bb[a] = (a == 0) ? 0.0f : 1.0f / (float)cov[(size_t)a * m + a];
      }
      __syncthreads();
      if (tid == 0) {
        // accu(square(ac) % b) as Armadillo's linear accumulate walks it: two accumulators over the even / odd elements, added at the end
        // (arma::accu on an expression, src/harmony.cpp:581; the oracle restates the same order)
        float u1 = 0.0f, u2 = 0.0f;
        int a = 0;
        for (; a + 1 < m; a += 2) {
          u1 = __fadd_rn(u1, __fmul_rn(__fmul_rn(ac[a], ac[a]), bb[a]));
          u2 = __fadd_rn(u2, __fmul_rn(__fmul_rn(ac[a + 1], ac[a + 1]), bb[a + 1]));
        }
        if (a < m) u1 = __fadd_rn(u1, __fmul_rn(__fmul_rn(ac[a], ac[a]), bb[a]));
        const float u = __fadd_rn(u1, u2);
        uu[0] = 1.0f / __fsub_rn((float)cov[0], u);
        if (!(__fsub_rn((float)cov[0], u) != 0.0f)) misc[3] = 1;
      }
      for (int a = tid; a < m; a += nt) acb[a] = (a == 0) ? 1.0f : __fmul_rn(ac[a], bb[a]);
      __syncthreads();
      const float iu = uu[0];
      // W[r2][j] = sum_c2 inv[r2][c2] rhs[c2][j], c2 ascending; the result replaces rhs only after every entry has been computed
      float* const Wtmp = A.Wall + (size_t)k * d * M;
      for (int i = tid; i < m * d; i += nt) {
        const int j = i / m, r2 = i - j * m;
        float sacc = 0.0f;
        for (int c2 = 0; c2 < m; c2++) {
          float iv = __fmul_rn(iu, __fmul_rn(acb[r2], acb[c2]));
          if (c2 == r2) iv = __fadd_rn(iv, bb[r2]);
          sacc = __fadd_rn(sacc, __fmul_rn(iv, (float)rhs[(size_t)j * m + c2]));
        }
        Wtmp[i] = sacc;
      }
      __syncthreads();
      for (int i = tid; i < m * d; i += nt) rhs[i] = (double)Wtmp[i];
      __syncthreads();
    } else if (A.solve_f32 && C > 1) {
      // Several covariates: the reference calls arma::inv (src/harmony.cpp:573), i.e. LAPACK's LU of the fp32 matrix.  LAPACK's blocked
      // rounding order cannot be pinned without the reference's BLAS; what is reproduced bit for bit is the oracle's restatement: unblocked
      // fp32 LU with partial pivoting (first largest pivot) applied to the identity, back substitution column by column, then
      // W = inv_cov * rhs with sequential fp32 accumulation.  One workgroup per cluster; the m x m fp32 matrix and its inverse live in the
      // cluster's fp64 scratch (2 m^2 floats = m^2 doubles).
      float* const ac = reinterpret_cast<float*>(sm_ + PAN_OFF);      // [m] multipliers of the current column (the panel space)
      __shared__ unsigned long long pivkey;
      // the fp64 scratch holds the assembled fp32 values: repack them as floats (through registers: the two layouts overlap)
      {
        const int per = (m * m + nt - 1) / nt;
        float* const Af = reinterpret_cast<float*>(cov);
        for (int base = 0; base < per; base += 16) {
          float v[16];
#pragma unroll
          for (int u = 0; u < 16; u++) { const int i = (base + u) * nt + tid; v[u] = (base + u < per && i < m * m) ? (float)cov[i] : 0.0f; }
          __syncthreads();
#pragma unroll
          for (int u = 0; u < 16; u++) { const int i = (base + u) * nt + tid; if (base + u < per && i < m * m) Af[i] = v[u]; }
          __syncthreads();
        }
      }
      float* const Af = reinterpret_cast<float*>(cov);
      float* const If = Af + (size_t)m * m;
      for (int i = tid; i < m * m; i += nt) If[i] = (i / m == i % m) ? 1.0f : 0.0f;
      __syncthreads();
      for (int cc = 0; cc < m && !misc[3]; cc++) {
        if (tid == 0) pivkey = 0ull;
        __syncthreads();
        unsigned long long best = 0ull;
        for (int r = cc + tid; r < m; r += nt) {
          const unsigned long long key = ((unsigned long long)(__float_as_uint(fabsf(Af[(size_t)cc * m + r]))) << 32) | (unsigned)(0x7fffffff - r);   // largest |a|, then the smallest row
          best = key > best ? key : best;
        }
        if (best) atomicMax(&pivkey, best);
        __syncthreads();
        const unsigned long long pk = pivkey;
        if ((pk >> 32) == 0ull) { if (tid == 0) misc[3] = 1; __syncthreads(); break; }
        const int pr = 0x7fffffff - (int)(pk & 0xffffffffull);
        if (pr != cc) {
          for (int j = tid; j < 2 * m; j += nt) {
            float* M2 = j < m ? Af + (size_t)j * m : If + (size_t)(j - m) * m;
            const float t = M2[cc]; M2[cc] = M2[pr]; M2[pr] = t;
          }
        }
        __syncthreads();
        const float inv = 1.0f / Af[(size_t)cc * m + cc];
        for (int r = cc + 1 + tid; r < m; r += nt) { const float f = __fmul_rn(Af[(size_t)cc * m + r], inv); ac[r] = f; }
        __syncthreads();
        for (int r = cc + 1 + tid; r < m; r += nt) if (ac[r] != 0.0f) Af[(size_t)cc * m + r] = ac[r];
        const int h = m - cc - 1;              // rows below the pivot
        // A[j][r] -= f_r A[j][cc] (j > cc), I[j][r] -= f_r I[j][cc] (all j): element-wise, one rounding for the product, one for the difference
        for (int i = tid; i < (h + m) * h; i += nt) {
          const int jj = i / h, r = cc + 1 + (i - jj * h);
          float* col = jj < h ? Af + (size_t)(cc + 1 + jj) * m : If + (size_t)(jj - h) * m;
          const float f = ac[r];
          if (f != 0.0f) col[r] = __fsub_rn(col[r], __fmul_rn(f, col[cc]));
        }
        __syncthreads();
      }
      if (!misc[3]) {
        // back substitution of every column of the identity: s -= A[c][r] * x[c], c ascending, then / A[r][r]
        for (int j = tid; j < m; j += nt) {
          float* x = If + (size_t)j * m;
          for (int r = m - 1; r >= 0; r--) {
            float sacc = x[r];
            for (int c2 = r + 1; c2 < m; c2++) sacc = __fsub_rn(sacc, __fmul_rn(Af[(size_t)c2 * m + r], x[c2]));
            x[r] = sacc / Af[(size_t)r * m + r];
          }
        }
        __syncthreads();
        float* const Wtmp = A.Wall + (size_t)k * d * M;
        for (int i = tid; i < m * d; i += nt) {
          const int j = i / m, r2 = i - j * m;
          float sacc = 0.0f;
          for (int c2 = 0; c2 < m; c2++) sacc = __fadd_rn(sacc, __fmul_rn(If[(size_t)c2 * m + r2], (float)rhs[(size_t)j * m + c2]));
          Wtmp[i] = sacc;
        }
        __syncthreads();
        for (int i = tid; i < m * d; i += nt) rhs[i] = (double)Wtmp[i];
      }
      __syncthreads();
    } else {
    // ---- blocked right-looking Cholesky (lower, column-major, in place in the L2-resident scratch).  Panels of NBW columns
    // are factored in LDS; the trailing matrix then receives ONE rank-NBW update per panel (16 fused multiply-adds per global
    // read-modify-write) instead of one rank-1 update per column -- at m = 201 (configs[4]: 200 levels) 13 passes over the
    // trailing matrix and ~40 workgroup barriers instead of 201 passes and 600 barriers (8.3 ms -> well under 1 ms per correction).
    constexpr int NBW = 16;
    double* const P = reinterpret_cast<double*>(sm_ + PAN_OFF);     // [rows of the panel][NBW], LDS
    const int nd = sch_nd, ms = m - nd;      // rows [ms, m): the diagonal block D; [0, ms): everything else
    if (nd > 0) {
      // S = A - B^T D^-1 B, rhs_A -= B^T D^-1 rhs_D   (cov = [[A, B^T], [B, D]], B = rows >= ms of the first ms columns)
      for (int r = ms + tid; r < m; r += nt) { const double dv = cov[(size_t)r * m + r]; if (!(dv > 0.0)) misc[3] = 1; cov[(size_t)r * m + r] = 1.0 / dv; }
      __syncthreads();
      // (with the coupling masks only the levels that really meet a row are visited -- the skipped terms are exact zeros, the sums
      //  keep their order: B is sparse, at configs[4]'s nested covariates a level of the eliminated one meets 3 of the 73 other rows)
      for (int i = tid; i < ms * ms; i += nt) {
        const int cb = i / ms, ra = i - cb * ms;
        if (ra < cb) continue;                      // the Cholesky reads the lower triangle only
        const double* ca = cov + (size_t)ra * m; const double* cc = cov + (size_t)cb * m;
        double sacc = 0.0;
        if (dmask) {
          for (int w2 = 0; w2 < mw; w2++) {
            unsigned long long bits = dmask[(size_t)ra * mw + w2] & dmask[(size_t)cb * mw + w2];
            while (bits) { const int r = ms + 64 * w2 + __builtin_ctzll(bits); bits &= bits - 1; sacc += ca[r] * cov[(size_t)r * m + r] * cc[r]; }
          }
        } else {
          for (int r = ms; r < m; r++) sacc += ca[r] * cov[(size_t)r * m + r] * cc[r];
        }
        cov[(size_t)cb * m + ra] -= sacc;
      }
      for (int i = tid; i < ms * d; i += nt) {
        const int j = i / ms, ra = i - j * ms;
        const double* ca = cov + (size_t)ra * m;
        double sacc = 0.0;
        if (dmask) {
          for (int w2 = 0; w2 < mw; w2++) {
            unsigned long long bits = dmask[(size_t)ra * mw + w2];
            while (bits) { const int r = ms + 64 * w2 + __builtin_ctzll(bits); bits &= bits - 1; sacc += ca[r] * cov[(size_t)r * m + r] * rhs[(size_t)j * m + r]; }
          }
        } else {
          for (int r = ms; r < m; r++) sacc += ca[r] * cov[(size_t)r * m + r] * rhs[(size_t)j * m + r];
        }
        rhs[(size_t)j * m + ra] -= sacc;
      }
      __syncthreads();
    }
    for (int c0 = 0; c0 < ms && !misc[3]; c0 += NBW) {
      const int nbw = min(NBW, ms - c0), h = ms - c0;
      for (int i = tid; i < h * nbw; i += nt) { const int kk = i / h, r = i - kk * h; P[r * NBW + kk] = cov[(size_t)(c0 + kk) * m + c0 + r]; }
      __syncthreads();
      for (int kk = 0; kk < nbw; kk++) {
        if (tid == 0) { const double sdiag = P[kk * NBW + kk]; if (!(sdiag > 0.0)) misc[3] = 1; else P[kk * NBW + kk] = sqrt(sdiag); }
        __syncthreads();
        if (misc[3]) break;
        const double linv = 1.0 / P[kk * NBW + kk];
        for (int r = kk + 1 + tid; r < h; r += nt) P[r * NBW + kk] *= linv;
        __syncthreads();
        const int rest = nbw - kk - 1;
        for (int i = tid; i < rest * h; i += nt) {
          const int k2 = kk + 1 + i / h, r = i % h;
          if (r >= k2) P[r * NBW + k2] -= P[r * NBW + kk] * P[k2 * NBW + kk];
        }
        __syncthreads();
      }
      if (misc[3]) break;
      for (int i = tid; i < h * nbw; i += nt) { const int kk = i / h, r = i - kk * h; if (r >= kk) cov[(size_t)(c0 + kk) * m + c0 + r] = P[r * NBW + kk]; }
      // trailing update: 32 consecutive rows per column and thread row (coalesced), the column's panel row cached in registers
      const int tx = tid & 31, ty = tid >> 5, TY = nt >> 5;
      for (int c2 = c0 + nbw + ty; c2 < ms; c2 += TY) {
        double pc[NBW];
#pragma unroll
        for (int kk = 0; kk < NBW; kk++) pc[kk] = (kk < nbw) ? P[(c2 - c0) * NBW + kk] : 0.0;
        double* colp = cov + (size_t)c2 * m;
        for (int r = c2 + tx; r < ms; r += 32) {
          const double* pr = P + (r - c0) * NBW;
          double sacc = 0.0;
#pragma unroll
          for (int kk = 0; kk < NBW; kk++) sacc += pr[kk] * pc[kk];
          colp[r] -= sacc;
        }
      }
      __syncthreads();
    }
    if (!misc[3]) {
      // ---- forward / back substitution for the d right-hand sides, 16 lanes per right-hand side, b in LDS when it fits
      const bool blds = (size_t)d * m * sizeof(double) <= A.lds_b_bytes;
      double* const bl = blds ? P : rhs;     // (the panel space is free now)
      if (blds) { for (int i = tid; i < d * m; i += nt) bl[i] = rhs[i]; }
      __syncthreads();
      const int ln = tid & 15;
      for (int j = tid >> 4; j < d; j += nt >> 4) {
        double* b = bl + (size_t)j * m;
        // L y = b, column by column: y_r = b_r / L_rr, then b_k -= L_kr y_r (k > r): L's column r is contiguous in k
        for (int r = 0; r < ms; r++) {
          const double* Lc = cov + (size_t)r * m;
          const double y = b[r] / Lc[r];
          if (ln == 0) b[r] = y;
          for (int kk = r + 1 + ln; kk < ms; kk += 16) b[kk] -= Lc[kk] * y;
        }
        // L^T x = y, row by row from the bottom: x_r = (y_r - sum_{k>r} L_kr x_k) / L_rr
        for (int r = ms - 1; r >= 0; r--) {
          const double* Lc = cov + (size_t)r * m;
          double t = 0.0;
          for (int kk = r + 1 + ln; kk < ms; kk += 16) t += Lc[kk] * b[kk];
          t += __shfl_xor(t, 8, 64); t += __shfl_xor(t, 4, 64); t += __shfl_xor(t, 2, 64); t += __shfl_xor(t, 1, 64);
          const double x = (b[r] - t) / Lc[r];
          if (ln == 0) b[r] = x;
        }
      }
      __syncthreads();
      if (blds) { for (int i = tid; i < d * m; i += nt) rhs[i] = bl[i]; }
      if (nd > 0) {      // x_D = D^-1 (rhs_D - B x_A): B's entries (rows >= ms of the first ms columns) were never touched
        __syncthreads();
        for (int i = tid; i < nd * d; i += nt) {
          const int j = i / nd, r = ms + (i - j * nd);
          double sacc = rhs[(size_t)j * m + r];
          if (dmask) { for (int a = 0; a < ms; a++) if ((dmask[(size_t)a * mw + ((r - ms) >> 6)] >> ((r - ms) & 63)) & 1ull) sacc -= cov[(size_t)a * m + r] * rhs[(size_t)j * m + a]; }
          else for (int a = 0; a < ms; a++) sacc -= cov[(size_t)a * m + r] * rhs[(size_t)j * m + a];
          rhs[(size_t)j * m + r] = sacc * cov[(size_t)r * m + r];
        }
      }
    }
    }   // (fp64 Cholesky branch)
    __syncthreads();
  }
  if (tid == 0) {
    A.flags[k] = (full ? 0 : 1) | (skipped ? 2 : 0) | (misc[3] ? 4 : 0);
    if (misc[3] && A.err) atomicOr(A.err, 1);
    A.mrows[k] = skipped ? 0 : m;
  }
  const bool solved = !skipped && !misc[3];
  float* Wk = A.Wall + (size_t)k * d * M;
  __shared__ float ynew[128];
  for (int j = tid; j < d; j += nt) {
    float y = D.Ycur[(size_t)k * d + j];                      // a skipped cluster keeps its centroid
    if (solved) { y = (float)rhs[(size_t)j * m]; rhs[(size_t)j * m] = 0.0; }   // :610-611
    ynew[j] = y;
  }
  __syncthreads();
  if (solved) {
    for (int i = tid; i < m * d; i += nt) { const int j = i / m, a = i - j * m; Wk[i] = (float)rhs[(size_t)j * m + prow[a]]; }     // reference row order
    __syncthreads();
    for (int i = tid; i < Q * d; i += nt) {
      const int q = i / d, j = i - q * d;
      float w = 0.0f;
      for (int c = 0; c < C; c++) { const int ro = row_of[D.qlev[q * C + c]]; if (ro >= 0) w += Wk[(size_t)j * m + ro]; }
      D.Wq[((size_t)q * K + k) * d + j] = w;
    }
  }
  if (D.moe_mfma) {   // MFMA B-operand image of the correction table (clusters = reduction dim), wimg_index(D, q, k, j) with the cluster's step and slot hoisted
    int s_, p_;
    if (k < 16 * D.wNT4) { const int t = k >> 4, r = k & 15; p_ = r >> 2; s_ = 4 * t + (r & 3); }
    else { const int r = k - 16 * D.wNT4; s_ = 4 * D.wNT4 + (r >> 2); p_ = r & 3; }
    __syncthreads();
    for (int i = tid; i < Q * d; i += nt) {
      const int q = i / d, j = i - q * d;
      const int qd = j >> 6, ii = (j & 63) >> 4, cc = j & 15;
      D.Wimg[((((size_t)q * D.wNQ + qd) * D.wNS + s_) * 4 + p_) * 64 + cc * 4 + ii] = D.Wq[((size_t)q * K + k) * d + j];
    }
  }
  // Y[:,k] <- normalise (:633): sequential fp32 sum of squares, as the host-side normalise does
  __shared__ float nrm_;
  if (tid == 0) { float sacc = 0.0f; for (int j = 0; j < d; j++) sacc += ynew[j] * ynew[j]; float nn = sqrtf(sacc); if (nn == 0.0f) nn = 1.0f; nrm_ = nn; }
  __syncthreads();
  for (int j = tid; j < d; j += nt) {
    const float y = ynew[j] / nrm_;
    D.Ycur[(size_t)k * d + j] = y;
    D.Yt[(size_t)j * K + k] = y;
    D.Yimg[yimg_index(D, j, k)] = y;
    bfimg_store_all(D, j, k, y);
  }
}
__global__ __launch_bounds__(1024) void k_moe_solve(Dev D, SolveArgs A) { moe_solve_body<false>(D, A); }
__global__ __launch_bounds__(1024) void k_moe_solve_lds(Dev D, SolveArgs A) { moe_solve_body<true>(D, A); }

// ---- MFMA variants of the two MoE passes (static 16-cell tiles, rows of a tile are contiguous in HBM) ----
// k_moe_stats_q: Sq[q] (K x d) += R_tile^T (K x 16) * Zo_tile (16 x d): the 16 cells are the MFMA reduction dim.  A workgroup streams a contiguous range of tiles; its
// wave w owns PC tile w (blockDim = 64 * PC tiles, the ones column at index d included), so a wave carries only NCT fp32 MFMA accumulators, folded into fp64 shadows every
// 4 tiles = 64 cells, and the K x (d + 1) result of a combination run is written ONCE per workgroup, not once per wave.  Against the first MFMA form (dword operand gathers,
// fp64 atomics into Sq; retired, docs/history.md) it has (a) 16-byte operand loads and (b) a bit-reproducible reduction.
//  (a) Which cluster an MFMA row stands for is free: inside a quad of cluster tiles (64 clusters) row m of tile i stands for
//      cluster 64 qd + nt m + i (nt = tiles of the quad: 4, or what is left in the last quad), so the nt A operands a lane
//      needs for one cell are CONSECUTIVE floats of its R row -- one dwordx4 (x3 / x2 / x1) load instead of nt dword gathers:
//      9 load instructions per tile and lane at K = 100 instead of 32.  Only the flush has to know the mapping.
//  (b) no floating-point atomics: every workgroup writes the K x (d+1) partial of each combination run it meets to its own slot
//      (slot order = workgroup order = cell order); k_moe_stats_reduce adds a combination's slots in ascending order -> Sq, nq
//      (and with them Z_corr) are identical from run to run.
// SHL (round 6): the fp64 shadow sums live in LDS ([wave][NCT * 4][64 lanes]: a lane's own slots, conflict-free) instead of 56 registers, and the operands of
// tile t + 1 are requested before tile t's MFMAs -- round 3 measured that software pipeline SLOWER because its 290 registers left one wave per SIMD; without the
// shadow registers it fits two.  Same operations in the same order: bit-identical statistics.
template <int NCT, bool SHL = false>
__global__ __launch_bounds__(320) void k_moe_stats_q(Dev D, int tiles_per_wg) {
  extern __shared__ double shl_[];
  constexpr int NQD = (NCT + 3) / 4, NTL = NCT - 4 * (NQD - 1);     // quads; tiles in the last quad
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int pt = threadIdx.x >> 6;
  // (two halves of the clusters, gridDim.y == 2: this workgroup's clusters are [kb, kb + K) of the KS a row holds; slots and tiles as for one half)
  const int KS = D.K, d = D.d, zs = D.zs;
  const int kb = (gridDim.y > 1 && blockIdx.y) ? D.st_KH : 0;
  const int K = gridDim.y > 1 ? (blockIdx.y ? D.K - D.st_KH : D.st_KH) : D.K;
  const int ts = (int)blockIdx.x * tiles_per_wg, te = min(D.ntitems, ts + tiles_per_wg);
  if (ts >= te) return;
  const int jj = 16 * pt + c;           // this lane's PC
  const bool jv = jj < d;
  const bool bcol1 = jj == d;           // column d of the B operand is all ones: its output column is sum_i R_ki (the launcher
                                        // adds a wave when d is a multiple of 16)
  f32x4 acc[NCT];
  double sh[SHL ? 1 : NCT][4];
  double* const shw = shl_ + (size_t)pt * (NCT * 4 * 64) + lane;      // SHL: this lane's slots, entry (ct, reg) at (4 ct + reg) * 64
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) {
    acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int reg = 0; reg < 4; reg++) { if constexpr (SHL) shw[(4 * ct + reg) * 64] = 0.0; else sh[ct][reg] = 0.0; }
  }
  auto kmap = [&](int ct, int m) -> int { const int qd = ct >> 2, nt = (qd == NQD - 1) ? NTL : 4; return 64 * qd + nt * m + (ct & 3); };
  auto fold = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) {
#pragma unroll
      for (int reg = 0; reg < 4; reg++) { if constexpr (SHL) shw[(4 * ct + reg) * 64] += (double)acc[ct][reg]; else sh[ct][reg] += (double)acc[ct][reg]; }
      acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  int slot = D.st_slot0[blockIdx.x];
  auto flush = [&]() {
    double* S = D.st_part + (size_t)slot * ((size_t)KS * d + KS);
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) {
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int k = kmap(ct, 4 * g + reg);
        double v;
        if constexpr (SHL) { v = shw[(4 * ct + reg) * 64]; shw[(4 * ct + reg) * 64] = 0.0; } else { v = sh[ct][reg]; sh[ct][reg] = 0.0; }
        if (jv && k < K) S[(size_t)(kb + k) * d + jj] = v;
        if (bcol1 && k < K) S[(size_t)KS * d + kb + k] = v;       // the ones column: sum_i R_ki
      }
    }
    slot++;
  };
  auto item_at = [&](int tile) -> Item {       // per-lane load (a uniform one costs a vmcnt(0) per tile, see k_tile)
    const Item* tp = D.titems + min(tile, te - 1);
    asm volatile("" : "+v"(tp));
    return *tp;
  };
  // this lane's first cluster in every quad (clamped so that the whole load stays inside the row) and which of them exist
  int koff[NQD];
#pragma unroll
  for (int qd = 0; qd < NQD; qd++) {
    const int nt = (qd == NQD - 1) ? NTL : 4;
    // (a lane whose first cluster exists loads at its exact offset: the tail of a partially valid load runs into the next row --
    //  R has a dummy row behind the last cell -- and is masked by kval; only fully invalid lanes are clamped)
    koff[qd] = (64 * qd + nt * c < K) ? 64 * qd + nt * c : K - nt;
  }
  // (a software pipeline over tiles -- operands of tile t+1 requested before tile t's MFMAs -- was measured SLOWER in round 3, 413 vs 388 us: 290 VGPRs left
  //  one wave per SIMD.  SHL: with the shadow sums in LDS it fits two, and the tile's operand latency passes behind the previous tile's MFMAs.)
  struct Ops { float a[4][NCT], b[4]; };
  auto load_ops = [&](const Item& it, Ops& o) __attribute__((always_inline)) {
    const size_t c0 = (size_t)it.start;
#pragma unroll
    for (int st = 0; st < 4; ++st) {           // all of the tile's operand loads first
      const int cell = 4 * st + g;
      const size_t row = c0 + (cell < it.cnt ? cell : 0);
      const float* rr = D.R + row * KS + kb;
#pragma unroll
      for (int qd = 0; qd < NQD; qd++) {
        if (qd < NQD - 1 || NTL == 4) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(rr + koff[qd]);
#pragma unroll
          for (int i = 0; i < 4; i++) if (4 * qd + i < NCT) o.a[st][4 * qd + i] = v[i];
        } else if (NTL == 3) {
          struct __attribute__((packed, aligned(4))) F3 { float x, y, z; };
          const F3 v = *reinterpret_cast<const F3*>(rr + koff[qd]);
          o.a[st][4 * qd] = v.x; o.a[st][4 * qd + 1] = v.y; o.a[st][4 * qd + 2] = v.z;
        } else if (NTL == 2) {
          const float2 v = *reinterpret_cast<const float2*>(rr + koff[qd]);
          o.a[st][4 * qd] = v.x; o.a[st][4 * qd + 1] = v.y;
        } else o.a[st][4 * qd] = rr[koff[qd]];
      }
      o.b[st] = D.Zo[row * zs + min(jj, zs - 1)];
    }
  };
  Item itC = item_at(ts), itN = item_at(ts + 1);      // (descriptors two tiles ahead: the operand loads of tile t + 1 must not wait for its descriptor)
  int curq = __builtin_amdgcn_readfirstlane(itC.q);
  Ops opN;
  if constexpr (SHL) load_ops(itC, opN);
  for (int tile = ts; tile < te; ++tile) {
    const Item it = itC;
    const int tq = __builtin_amdgcn_readfirstlane(it.q);
    if (tq != curq) { fold(); flush(); curq = tq; }
    Ops op;
    if constexpr (SHL) { op = opN; load_ops(itN, opN); }      // (behind the last tile: item_at clamps to it -- loaded again, never used)
    else load_ops(it, op);
    itC = itN; itN = item_at(tile + 2);
    auto& a = op.a; auto& b = op.b;
    if (it.cnt == 16) {
      // full tile (all but the last tile of a combination): NO masking at all.  Rows of the result that stand for clusters >= K
      // and columns that stand for PCs >= d hold finite garbage (clamped loads) and are never flushed.  sum_i R_ki comes out of
      // the same MFMAs: the PC tile that has room for it feeds a column of ones (bcol1).
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const float bb = bcol1 ? 1.0f : b[st];
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[st][ct], bb, acc[ct], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const bool cv = 4 * st + g < it.cnt;
        const float bb = cv ? (bcol1 ? 1.0f : b[st]) : 0.0f;
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(cv ? a[st][ct] : 0.0f, bb, acc[ct], 0, 0, 0);
      }
    }
    if (((tile - ts) & 3) == 3) fold();
  }
  fold(); flush();
}
// Sq[q], nq[q] = sum of the combination's partial slots in ascending slot (= cell) order: fixed order, no atomics
__global__ __launch_bounds__(256) void k_moe_stats_reduce(Dev D) {
  const int q = blockIdx.x;
  const size_t per = (size_t)D.K * D.d + D.K;
  const int s0 = D.st_qptr[q], s1 = D.st_qptr[q + 1];
  const size_t e = (size_t)blockIdx.y * blockDim.x + threadIdx.x;    // one entry per thread, eight slots in flight
  if (e >= per) return;
  double v = 0.0;
  int sidx = s0;
  for (; sidx + 8 <= s1; sidx += 8) {
    double t[8];
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = D.st_part[(size_t)D.st_qslots[sidx + i] * per + e];
#pragma unroll
    for (int i = 0; i < 8; i++) v += t[i];                            // ascending slot order: the sum is reproducible
  }
  for (; sidx < s1; sidx++) v += D.st_part[(size_t)D.st_qslots[sidx] * per + e];
  if (e < (size_t)D.K * D.d) D.Sq[(size_t)q * D.K * D.d + e] = v;
  else D.nq[(size_t)q * D.K + (e - (size_t)D.K * D.d)] = v;
}

// k_moe_apply_mfma: Z_corr tile (16 x d) = Z_orig tile - R tile (16 x K) * Wq[q] (K x d); clusters are the MFMA reduction
// dim, so this is tile_dots with (rows = R rows, "centroid image" = Wimg[q] staged in LDS).  One workgroup per apply item.
// (round 6) The R row of a tile's lane -- its A operands of ALL reduction steps, up to 8 float4 groups + 3 single steps: K <= 140 -- and its Z_orig values are
// requested one tile AHEAD and held in registers (k_tile's scheme): tile_dots streamed the row one group ahead, i.e. a wave sat through seven dependent
// memory latencies per tile.  Same MFMAs in the same order: bit-identical Z_corr.
struct RRow { f32x4 v[8]; float t[3]; };
__device__ __forceinline__ void load_rrow(const float* __restrict__ rrow, int g, int NT4, int tail, RRow& r) {
  const int tmax = NT4 > 0 ? NT4 - 1 : 0, umax = tail > 0 ? tail - 1 : 0;
  if (NT4 > 0) {
#pragma unroll
    for (int t = 0; t < 8; t++) r.v[t] = *reinterpret_cast<const f32x4*>(rrow + 16 * min(t, tmax) + 4 * g);
  }
  if (tail > 0) {
#pragma unroll
    for (int u = 0; u < 3; u++) r.t[u] = rrow[16 * NT4 + 4 * min(u, umax) + g];
  }
}
template <int NCT>
__device__ __forceinline__ void tile_dots_rrow(const f32x4* __restrict__ ldsY4, const RRow& r, bool valid, int lane, int NS, int NT4, int tail, f32x4 (&acc)[NCT]) {
  constexpr int NQ = (NCT + 3) / 4;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) acc[ct] = zero4;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
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
template <int NPT>
__global__ __launch_bounds__(256) void k_moe_apply_mfma(Dev D) {
  extern __shared__ __attribute__((aligned(16))) f32x4 ldsW4[];
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4, wib = threadIdx.x >> 6;
  const int K = D.K, d = D.d, zs = D.zs;
  const int nW4 = D.wNQ * D.wNS * 64;
  const bool regs = D.wNT4 <= 8;           // (K <= 140; otherwise the streamed form)
  for (int itx = blockIdx.x; itx < D.naitems; itx += gridDim.x) {
    const Item item = D.aitems[itx];
    __syncthreads();
    const f32x4* src = reinterpret_cast<const f32x4*>(D.Wimg) + (size_t)item.q * nW4;
    for (int i = threadIdx.x; i < nW4; i += blockDim.x) ldsW4[i] = src[i];
    const int ntl = (item.cnt + 15) >> 4;
    // the R row of a tile's lane (its A operands), one tile ahead; the tile's Z_orig values are requested in front of its own MFMA chain (their latency
    // hides behind the 100 MFMAs; held a tile ahead as well they cost 32 more registers: 192, two waves per SIMD -- 206 us per pass instead of 231)
    auto fetch = [&](const int tl, RRow& rr) __attribute__((always_inline)) {
      const int cell0 = item.start + 16 * tl;
      const int nvalid = min(16, item.start + item.cnt - cell0);
      if (regs) load_rrow(D.R + (size_t)(cell0 + (c < nvalid ? c : 0)) * K, g, D.wNT4, D.wtail, rr);
    };
    RRow rrN;
    if (wib < ntl) fetch(wib, rrN);      // (requested before the barrier: the first tile's latency passes during the staging of the correction image)
    __syncthreads();
    for (int tl = wib; tl < ntl; tl += 4) {
      const int cell0 = item.start + 16 * tl;
      const int nvalid = min(16, item.start + item.cnt - cell0);
      const bool av = c < nvalid;
      const RRow rr = rrN;
      float zo[4][NPT];
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int cl = 4 * g + reg;
        const size_t row = (size_t)(cell0 + (cl < nvalid ? cl : 0)) * zs;
#pragma unroll
        for (int pt = 0; pt < NPT; pt++) zo[reg][pt] = D.Zo[row + min(16 * pt + c, zs - 1)];
      }
      if (tl + 4 < ntl) fetch(tl + 4, rrN);
      f32x4 acc[NPT];
      if (regs) tile_dots_rrow<NPT>(ldsW4, rr, av, lane, D.wNS, D.wNT4, D.wtail, acc);
      else tile_dots<NPT>(ldsW4, D.R + (size_t)(cell0 + (av ? c : 0)) * K, av, g, lane, D.wNS, D.wNT4, D.wtail, acc);
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int cl = 4 * g + reg;
        const bool cv = cl < nvalid;
        const size_t row = (size_t)(cell0 + (cv ? cl : 0)) * zs;
#pragma unroll
        for (int pt = 0; pt < NPT; pt++) {
          const int jj = 16 * pt + c;
          if (cv && jj < d) D.Zc[row + jj] = zo[reg][pt] - acc[pt][reg];
        }
      }
    }
  }
}

// --------------------------------------------------------------------------------------
// kmeans_centers (src/utils.cpp:10-64): the seeding race and Lloyd run on the tile kernel (k_tile MODE 3 / 2, hmx_k_tile.inc);
//   k_seed_race_u: the race on uniforms from the host;  k_lloyd: one Lloyd iteration where the K x d sum table does not fit
//   the tile kernel's LDS.
// --------------------------------------------------------------------------------------
// R-compatible seeding race (hmx_set_int "rng" = 1): the uniforms come from the HOST's stream (MT19937 seeded like set.seed, or
// the host's unif_rand), u[a][local original cell] for the anchors a0 .. a0+na-1; per anchor the race of src/utils.cpp:24-34
// over this shard's cells: key = -log(u) / |2(1 - y_a.x)|, index_min (ties -> the smaller global cell index).
__global__ __launch_bounds__(256) void k_seed_race_u(Dev D, const float* __restrict__ u, int a0, int na, int a_lo, int a_hi,
                                                     uint64_t goff, const unsigned* __restrict__ excl, int nexcl) {
  extern __shared__ float ys_[];   // [na][d] anchor rows
  const int d = D.d, zs = D.zs, n = D.n;
  for (int i = threadIdx.x; i < na * d; i += blockDim.x) ys_[i] = D.Ycur[(size_t)a0 * d + i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const size_t gt = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (int a = a_lo; a < a_hi; a++) {
    unsigned long long best = ~0ull;
    const float* y = ys_ + a * d;
    for (size_t p = gt; p < (size_t)n; p += stride) {
      const float* z = D.Zc + p * zs;
      float dot = 0.0f;
      for (int j = 0; j < d; j++) dot = fmaf(y[j], z[j], dot);
      const int loc = D.perm[p];
      const uint64_t gg = goff + (uint64_t)loc;
      bool skip = false;
      for (int x = 0; x < nexcl; x++) skip |= ((uint64_t)excl[x] == gg);
      const float dis = fabsf(2.0f * (1.0f - dot));
      const float key = -logf(u[(size_t)a * n + loc]) / dis;
      unsigned kb = __float_as_uint(key);
      if (!(key >= 0.0f)) kb = 0x7f800000u;
          kb &= 0x7fffffffu;   // -0.0 (u == 1: -log(u) = -0) must order as zero, not as the largest unsigned pattern
      const unsigned long long pk = ((unsigned long long)kb << 32) | (unsigned long long)(uint32_t)gg;
      if (!skip && pk < best) best = pk;
    }
    best = wmin64(best);
    if (lane == 0 && best != ~0ull) atomicMin(&D.seedmin[a0 + a], best);
  }
}

// rows[k][:] = Z_corr row of global cell gcells[k] if it lives on this shard, else 0 (summed across ranks)
__global__ void k_gather_rows(Dev D, const long long* __restrict__ gcells, uint64_t goff, double* __restrict__ rows) {
  const int k = blockIdx.x;
  const long long g = gcells[k];
  const long long loc = g - (long long)goff;
  const bool mine = (loc >= 0 && loc < (long long)D.n);
  for (int j = threadIdx.x; j < D.d; j += blockDim.x)
    rows[(size_t)k * D.d + j] = mine ? (double)D.Zc[(size_t)D.invperm[loc] * D.zs + j] : 0.0;
}

template <int KPL, int DPL>
__global__ __launch_bounds__(TPB) void k_lloyd(Dev D) {
  // LDS: centroids d*KP floats.  The K x d sums go straight to memory: this kernel runs only where the tile kernel's centroid image (zs*KP*4
  // bytes) and the sum table exceed 160 KB together (hmx_api_kmeans.inc), so the table does not fit beside d*KP*4 bytes of centroids either.
  extern __shared__ __attribute__((aligned(16))) float ldsY[];
  stage_Y(ldsY, D.Yt, D.d, D.K, D.KP);
  constexpr int CB = 4;
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
  const int d = D.d, K = D.K;
  float yn[KPL];
#pragma unroll
  for (int q = 0; q < KPL; q++) yn[q] = ld_or(D.ynorm, (size_t)min(lane + 64 * q, K - 1), lane + 64 * q < K, 0.0f);
  for (int it = wave; it < D.nitems; it += nw) {
    const Item item = D.items[it];
    for (int p = 0; p < item.cnt; p += CB) {
      const int nc = min(CB, item.cnt - p);
      float z[CB][DPL];
#pragma unroll
      for (int c = 0; c < CB; c++) {
        if (c < nc) load_row<DPL>(D.Zc, (size_t)(item.start + p + c), D.zs, d, lane, z[c]);
        else {
#pragma unroll
          for (int t = 0; t < DPL; t++) z[c][t] = 0.0f;
        }
      }
      float acc[CB][KPL];
      group_dots<KPL, DPL, CB>(ldsY, d, D.KP, lane, z, acc);
#pragma unroll
      for (int c = 0; c < CB; c++) {
        if (c < nc) {
          unsigned long long best = ~0ull;
#pragma unroll
          for (int q = 0; q < KPL; q++) {
            const int k = lane + 64 * q;
            if (k < K) {
              const float sc = yn[q] - 2.0f * acc[c][q];  // ||x-y||^2 - ||x||^2
              unsigned ub = __float_as_uint(sc);
              ub = (ub & 0x80000000u) ? ~ub : (ub | 0x80000000u);  // order-preserving map
              const unsigned long long pk = ((unsigned long long)ub << 32) | (unsigned)k;
              best = pk < best ? pk : best;
            }
          }
          best = wmin64(best);
          const int kb = (int)(best & 0xffffffffu);
#pragma unroll
          // unit-vector components as 2^30 fixed point: exact, order-independent 64-bit sums
          for (int t = 0; t < DPL; t++) {
            const int jj = 64 * t + lane;
            if (jj < d) atomicAdd((unsigned long long*)&D.lsum[(size_t)kb * d + jj], (unsigned long long)__float2ll_rn(z[c][t] * 1073741824.0f));
          }
          if (lane == 0) atomicAdd(&D.lcnt[kb], 1ull);
        }
      }
    }
  }
}

// Lloyd centre update on the device (src/utils.cpp:56-61): mean of the members (2^30 fixed-point sums / counts), an
// empty cluster keeps its centre; refreshes Ycur [K][d], Yt [d][K], the MFMA image and ||y||^2.  One workgroup per cluster.
__global__ __launch_bounds__(64) void k_lloyd_finish(Dev D) {
  const int k = blockIdx.x, lane = threadIdx.x, d = D.d, K = D.K;
  const unsigned long long cnt = D.lcnt[k];
  float s2 = 0.0f;
  for (int j = lane; j < d; j += 64) {
    float y = D.Ycur[(size_t)k * d + j];
    if (cnt > 0) y = (float)(((double)D.lsum[(size_t)k * d + j] * (1.0 / 1073741824.0)) / (double)cnt);
    D.lsum[(size_t)k * d + j] = 0;              // (consumed: the next Lloyd iteration needs no memset launch)
    D.Ycur[(size_t)k * d + j] = y;
    D.Yt[(size_t)j * K + k] = y;
    D.Yimg[yimg_index(D, j, k)] = y;
    bfimg_store_all(D, j, k, y);
    s2 += y * y;
  }
  // ||y_k||^2 as the host computes it: sequential fp32 sum over j (d <= 128: lane-serial is fine for K blocks)
  __shared__ float ys[128];
  for (int j = lane; j < d; j += 64) ys[j] = D.Ycur[(size_t)k * d + j];
  __syncthreads();
  if (lane == 0) { float s = 0.0f; for (int j = 0; j < d; j++) s += ys[j] * ys[j]; D.ynorm[k] = s; D.lcnt[k] = 0ull; }      // (every lane read the count before the barrier)
  (void)s2;
}

// Ycur [K][d] (or, rows != nullptr, the fp64 rows gathered from the seed cells) -> Ycur, Yt [d][K], the fp32 MFMA image, the split-bf16 image and
// ||y_k||^2 -- on the device: the centroids never travel to the host and back between the stages of kmeans_centers / init_cluster_cpp
// (round 3: four synchronous uploads per stage).  normalise: Y[:,k] <- Y[:,k] / ||Y[:,k]|| first (arma::normalise(Y, 2, 0),
// src/harmony.cpp:136: sequential fp32 sum of squares, a zero column is left alone).  One workgroup per cluster.
__global__ __launch_bounds__(64) void k_y_images(Dev D, const double* __restrict__ rows, int normalise) {
  const int k = blockIdx.x, lane = threadIdx.x, d = D.d, K = D.K;
  __shared__ float ys[128];
  __shared__ float nrm_;
  for (int j = lane; j < d; j += 64) ys[j] = rows ? (float)rows[(size_t)k * d + j] : D.Ycur[(size_t)k * d + j];
  __syncthreads();
  if (lane == 0) {
    float s = 0.0f;
    for (int j = 0; j < d; j++) s = __fadd_rn(s, __fmul_rn(ys[j], ys[j]));
    float nn = sqrtf(s);
    if (nn == 0.0f) nn = 1.0f;
    nrm_ = normalise ? nn : 1.0f;
  }
  __syncthreads();
  for (int j = lane; j < d; j += 64) {
    const float y = normalise ? ys[j] / nrm_ : ys[j];
    ys[j] = y;
    D.Ycur[(size_t)k * d + j] = y;
    D.Yt[(size_t)j * K + k] = y;
    D.Yimg[yimg_index(D, j, k)] = y;
    bfimg_store_all(D, j, k, y);
  }
  __syncthreads();
  if (lane == 0) { float s = 0.0f; for (int j = 0; j < d; j++) s = __fadd_rn(s, __fmul_rn(ys[j], ys[j])); D.ynorm[k] = s; }
}
void l_y_images(const Launch& L, const Dev& D, const double* rows, int normalise) {
  hipLaunchKernelGGL(k_y_images, dim3(D.K), dim3(64), 0, L.stream, D, rows, normalise);
}
#endif  // !HMX_TILE_BF

// hmx_k_stream.inc -- part of hmx_kernels.hip (included inside namespace hmx): ingest / egress, the objective of the current state, the rounds' shuffle
// (counting sort and the sort-free form), the old-contribution passes, fold / penalty kernels.  Not built into the split-bf16 unit.
#if !HMX_TILE_BF   // (the split-bf16 translation unit builds k_tile and its launchers only)
// --------------------------------------------------------------------------------------
// src: [n][d] doubles or floats in local original order (host slab staged in HBM, or the caller's device buffer)
// -> dst: [n][zs] floats in internal order
template <class T>
__global__ void k_convert_in(const T* __restrict__ src, float* __restrict__ dst, const int* __restrict__ invperm,
                             int n, int d, int zs) {
  const size_t total = (size_t)n * d;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t cell = i / d; const int j = (int)(i - cell * d);
    dst[(size_t)invperm[cell] * zs + j] = (float)src[i];
  }
}
// egress of a slab of cells in ORIGINAL order: dst[i][0..w) = src[invperm[i]][0..w) (rows gathered, output written
// contiguously -> the slab can be copied to the host while the next one is converted).  T = double (the R seam) or float.
template <class T>
__global__ void k_convert_out(const float* __restrict__ src, T* __restrict__ dst, const int* __restrict__ invperm,
                              int n, int w, int ws) {
  const size_t total = (size_t)n * w;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t cell = i / w; const int j = (int)(i - cell * w);
    dst[i] = (T)src[(size_t)invperm[cell] * ws + j];
  }
}
__global__ void k_copy(const float* __restrict__ src, float* __restrict__ dst, size_t count) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = src[i];
}
// up to four buffers of 8-byte words cleared by ONE launch (round 6: the head of a clustering call issued three memsets in a row, a kernel slot each)
__global__ void k_zero4(unsigned long long* a, size_t na, unsigned long long* b, size_t nb, unsigned long long* c, size_t nc, unsigned long long* d, size_t nd) {
  const size_t step = (size_t)gridDim.x * blockDim.x, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = t; i < na; i += step) a[i] = 0ull;
  for (size_t i = t; i < nb; i += step) b[i] = 0ull;
  for (size_t i = t; i < nc; i += step) c[i] = 0ull;
  for (size_t i = t; i < nd; i += step) d[i] = 0ull;
}
// arma::normalise(Z, 2, 0) (src/harmony.cpp:42,220): one wave per cell
__global__ __launch_bounds__(TPB) void k_normalize(float* __restrict__ Z, int n, int d, int zs) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
  for (int cell = wave; cell < n; cell += nw) {
    float* z = Z + (size_t)cell * zs;
    const float a = ld_or(z, (size_t)min(lane, d - 1), lane < d, 0.0f), b = ld_or(z, (size_t)min(64 + lane, d - 1), 64 + lane < d, 0.0f);
    float nrm = sqrtf(wsum(a * a + b * b));
    if (nrm == 0.0f) nrm = 1.0f;
    if (lane < d) z[lane] = a / nrm;
    if (64 + lane < d) z[64 + lane] = b / nrm;
  }
}

// --------------------------------------------------------------------------------------
// Objective partials of the current state (harmony::compute_objective, src/harmony.cpp:158-170):
// dist = 2(1 - Y^T Z) (:141) against the R rows as they stand.  One wave per static work item (a run
// of cells with one combination).
// --------------------------------------------------------------------------------------
template <int KPL, int DPL>
__global__ __launch_bounds__(TPB) void k_head(Dev D) {
  extern __shared__ __attribute__((aligned(16))) float ldsY[];
  stage_Y(ldsY, D.Yt, D.d, D.K, D.KP);
  constexpr int CB = 4;
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
  const int d = D.d, K = D.K;
  float sig[KPL];
#pragma unroll
  for (int q = 0; q < KPL; q++) sig[q] = ld_or(D.sigma, (size_t)min(lane + 64 * q, K - 1), lane + 64 * q < K, 1.0f);
  double od = 0.0, oe = 0.0;
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
          const size_t cell = (size_t)(item.start + p + c);
          float r[KPL], dist[KPL];
#pragma unroll
          for (int q = 0; q < KPL; q++) {
            const int k = lane + 64 * q;
            dist[q] = 2.0f * (1.0f - acc[c][q]);
            r[q] = ld_or(D.R, cell * K + min(k, K - 1), k < K, 0.0f);
          }
#pragma unroll
          for (int q = 0; q < KPL; q++) {
            if (lane + 64 * q < K) {
              od += (double)(r[q] * dist[q]);
              oe += (double)((r[q] * trunc_logf_dev(r[q])) * sig[q]);
            }
          }
        }
      }
    }
  }
  od = wsumd(od); oe = wsumd(oe);
  if (lane == 0) { D.objpart[2 * wave] += od; D.objpart[2 * wave + 1] += oe; }  // private slot (slot row 0): no atomics
}

// --------------------------------------------------------------------------------------
// per-round block membership + stable counting sort by block
// --------------------------------------------------------------------------------------
// Stable counting sort of the cells by block, with every (block, combination) bin padded to a multiple of
// 16 positions (dummy entries = -1) so that a 16-cell MFMA tile never straddles two combinations.
// Sort chunks are static runs of <= SORT_CHUNK cells of ONE combination (D.schunks, built at setup), so the
// per-chunk histogram counts[blk][chunk] also yields the per-(block, combination) bin sizes.
// one wave per sort chunk.  FUSED: the block id is computed here from the Feistel bijection (no separate block-id kernel: saves a
// launch and a write + read of blk); the histogram is one ds_add_u32 per 64 cells instead of a ballot loop over the
// distinct block values.
// D.nxt (own shuffle only): the sort key of a cell is (block of this round, block of the NEXT round) -- nV = nb * nb keys --, so that
// every 16-cell tile also has ONE next block and the tile kernels can file the tile's new R sums as that block's old contribution
// (flush_tile_fx): 16 padding slots per (block, combination, next block) instead of per (block, combination).
struct BlockIdArgs { FeistelKeys fk, fk2; uint64_t Nglob, goff, cpb; float inv_cpb; };
struct BlockIdBatch { BlockIdArgs a[4]; };      // one entry per round of a batched sort (blockIdx.y)
// block of a position: min(pos / cells_per_block, n_blocks - 1) (src/harmony.cpp:296-300) without the 64-bit division (~100 instructions
// per cell, twice per cell and round): a float estimate, corrected exactly by two integer comparisons
__device__ __forceinline__ int block_of(uint64_t pos, const BlockIdArgs& A, int nb) {
  long long b = (long long)((float)pos * A.inv_cpb);
  if (b > nb) b = nb;                                        // (keeps the products below in range)
  if ((uint64_t)b * A.cpb > pos) b--;
  else if ((uint64_t)(b + 1) * A.cpb <= pos) b++;
  return (int)(b < (long long)(nb - 1) ? b : (long long)(nb - 1));
}
template <bool FUSED>
__global__ __launch_bounds__(WAVE) void k_sort_hist(Dev D, BlockIdBatch AB, SortBatch S) {
  extern __shared__ int cnt[];
  const BlockIdArgs& A = AB.a[blockIdx.y]; const SortPtrs& P = S.p[blockIdx.y];      // (blockIdx.y: the round of a batched sort)
  const int lane = threadIdx.x, chunk = blockIdx.x, nb = D.nb, nV = D.nxt ? nb * nb : nb;
  for (int v = lane; v < nV; v += WAVE) cnt[v] = 0;
  __syncthreads();
  const Item ch = D.schunks[chunk];
  const int s = ch.start, e = ch.start + ch.cnt;
  constexpr int NSTEP = SORT_CHUNK / WAVE;
  int pm[NSTEP];      // the chunk's cell ids, all loads in flight together (one exposed latency per chunk instead of one per step)
#pragma unroll
  for (int u = 0; u < NSTEP; u++) pm[u] = FUSED ? D.perm[min(s + u * WAVE + lane, e - 1)] : 0;
#pragma unroll
  for (int u = 0; u < NSTEP; u++) {
    const int base = s + u * WAVE;
    if (base >= e) break;
    const int i = base + lane;
    int b = -1;
    if (i < e) {
      if constexpr (FUSED) {
        const uint64_t pos = feistel_apply(A.fk, A.Nglob, A.goff + (uint64_t)pm[u]);
        b = block_of(pos, A, nb);
        P.blk[i] = b;
        if (D.nxt) {
          const uint64_t pos2 = feistel_apply(A.fk2, A.Nglob, A.goff + (uint64_t)pm[u]);
          b = b * nb + block_of(pos2, A, nb);
          P.blkv[i] = b;
        }
      } else b = P.blk[i];
      atomicAdd(&cnt[b], 1);
    }
  }
  __syncthreads();
  for (int v = lane; v < nV; v += WAVE) P.counts[(size_t)v * D.nchunks + chunk] = cnt[v];
}
// one wave per (block, combination) bin: exclusive prefix of the bin's chunk counts -> offs (offset inside the bin),
// padded bin size -> binoff[bin].  The chunks of a combination are contiguous, so the loads are coalesced.
__global__ __launch_bounds__(WAVE) void k_sort_binscan(Dev D, SortBatch S) {
  const SortPtrs& P = S.p[blockIdx.y];
  const int lane = threadIdx.x, bin = blockIdx.x, Q = D.Q, nch = D.nchunks, nV = D.nxt ? D.nb * D.nb : D.nb;
  const int v = bin / Q, q = bin - v * Q;
  const int lo = D.qchunk[q], hi = D.qchunk[q + 1];
  const int* __restrict__ cin = P.counts + (size_t)v * nch;
  int* __restrict__ cout = P.offs + v;      // offs[chunk][key]: the scatter kernel reads a chunk's nV offsets as one contiguous run
  int run = 0;
  for (int base = lo; base < hi; base += WAVE) {
    const int i = base + lane;
    const int c = ld_or(cin, (size_t)min(i, hi - 1), i < hi, 0);
    int incl = c;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { const int o = __shfl_up(incl, m, 64); if (lane >= m) incl += o; }
    if (i < hi) cout[(size_t)i * nV] = run + incl - c;
    run += __shfl(incl, 63, 64);
  }
  if (lane == 0) { P.binoff[bin] = (run + 15) & ~15; P.bincnt[bin] = run; }
}
// single workgroup: exclusive scan of the padded bin sizes (block-major) -> binoff; boff[v] = padded start of block v
__global__ __launch_bounds__(1024) void k_sort_binoff(Dev D, SortBatch S) {
  const SortPtrs& P = S.p[blockIdx.x];
  __shared__ int part[1024];
  const int t = threadIdx.x, nb = D.nb, Q = D.Q, vpb = D.nxt ? nb : 1, nbins = nb * vpb * Q;   // vpb: sort keys per block
  int* bins = P.binoff;
  const int per = (nbins + 1023) / 1024;
  const int s = t * per, e = min(nbins, s + per);
  int sum = 0;
  for (int i = s; i < e; i++) sum += bins[i];
  part[t] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = (t >= off) ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - sum;
  for (int i = s; i < e; i++) { const int c = bins[i]; bins[i] = run; run += c; }
  if (t == 1023) bins[nbins] = part[1023];
  __syncthreads();
  for (int v = t; v <= nb; v += 1024) P.boff[v] = bins[v < nb ? v * vpb * Q : nbins];
}
// Placement of a chunk's cells into their (key, combination) bins, 64 cells per step; the chunk's first slot in every bin comes from
// k_sort_binscan / k_sort_binoff, the rank inside the chunk from an LDS atomic (see below).
__global__ __launch_bounds__(WAVE) void k_sort_scatter(Dev D, SortBatch S) {
  extern __shared__ int base_[];
  const SortPtrs& P = S.p[blockIdx.y];
  const int lane = threadIdx.x, chunk = blockIdx.x, nb = D.nb, nV = D.nxt ? nb * nb : nb;
  const Item ch = D.schunks[chunk];
  const int* __restrict__ key = D.nxt ? P.blkv : P.blk;
  const int s = ch.start, e = ch.start + ch.cnt;
  constexpr int NSTEP = SORT_CHUNK / WAVE;
  for (int v0 = 0; v0 < nV; v0 += 8 * WAVE) {     // (eight independent pairs of loads in flight per pass)
    int t0[8], t1[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int v = min(v0 + u * WAVE + lane, nV - 1);
      t0[u] = P.binoff[v * D.Q + ch.q]; t1[u] = P.offs[(size_t)chunk * nV + v];
    }
#pragma unroll
    for (int u = 0; u < 8; u++) if (v0 + u * WAVE + lane < nV) base_[v0 + u * WAVE + lane] = t0[u] + t1[u];
  }
  __syncthreads();
  int kk[NSTEP];      // the chunk's keys, all loads in flight together
#pragma unroll
  for (int u = 0; u < NSTEP; u++) kk[u] = ld_or(key, (size_t)min(s + u * WAVE + lane, e - 1), s + u * WAVE + lane < e, 0x00FFFFFF);   // (past the end: sorts behind every key)
#pragma unroll
  for (int u = 0; u < NSTEP; u++) {
    const int base = s + u * WAVE;
    if (base >= e) break;
    // rank of a cell among the chunk's cells of the same key = the value its LDS atomic returns: the 64 lanes of one ds_add_rtn are
    // served one after the other, the chunk's steps run in order on this one wave -- every cell gets a distinct slot of its bin, and
    // which slot is irrelevant (a bin only has to be PURE: same block, combination and next block).  (The first version ranked the
    // cells with a 21-stage bitonic sort of (key, lane) per step to keep the sort stable: 44 us per round, all of it on the critical
    // path between two chain launches.)
    const int ks = kk[u];
    if (base + lane < e) {
      const int dst = atomicAdd(&base_[ks], 1), cell = base + lane;
      if (D.need_lorder) { P.lorder[dst] = cell; P.lcombo[dst] = ch.q; }
      P.lpair[dst] = make_int2(cell, D.nxt ? (ch.q | ((ks % nb) << 19) | ((ks / nb) << 25)) : ch.q);     // (combination, next block, block): see flush_run in k_tile
    }
  }
  // the padding slots (< 16 per bin) of this combination's bins: "no cell" -- written here, so that no memset of the whole order
  // precedes every shuffle
  // (the keys are dealt over the combination's chunks: a couple of bins per wave)
  const int ci = chunk - D.qchunk[ch.q], ncq = D.qchunk[ch.q + 1] - D.qchunk[ch.q];
  for (int v = ci + ncq * lane; v < nV; v += ncq * WAVE) {
    const int bin = v * D.Q + ch.q, st = P.binoff[bin], cnt = P.bincnt[bin], pad = (cnt + 15) & ~15;
    for (int k = cnt; k < pad; k++) { if (D.need_lorder) P.lorder[st + k] = -1; P.lpair[st + k] = make_int2(-1, -1); }
  }
}

// --------------------------------------------------------------------------------------
// The same padded order WITHOUT sorting the cells by block (round 4).  The round's shuffle is a bijection of positions with a closed-form
// inverse, so the cells of block b are simply the inverse images of the positions [b * cpb, (b + 1) * cpb): the cells arrive grouped by
// block for free, and only the (next block, combination) bins INSIDE a block are left to count.  Four wide launches serve up to four rounds
// (blockIdx.y = round of the batch; k_shuf_blocks -- block id per cell, D.blk -- runs only for a round whose old contributions were not
// carried and must be summed from R); the unit of work is a PART of a block (SHUF_PART consecutive positions, one 1024-thread workgroup):
//   k_shuf_count   per (round, part): cell = inverse image of the position (-1: another rank's), its next block = block of its image under the
//                  NEXT round's bijection, its rank inside (part, bin) from a returning LDS atomic -> posr[round][position] = (cell, rank |
//                  combination | next block); the part's offset inside every bin from a returning atomic on the bin's size
//   k_shuf_scan    per round, one workgroup: bins padded to 16 -> first slot of every bin, padded block offsets
//   k_shuf_place   per (round, part): lpair[first slot of the bin + part offset + rank] = (cell, keys); part 0 of a block writes the padding
// Against the counting sort above (four dependent launches of ONE-WAVE workgroups over an (nb^2 keys) x (N / 512 chunks) count matrix: 150 us
// per four rounds at 1M cells) the count matrix is (nb * Q bins) x (N / SHUF_PART parts).  The counting sort stays for host-provided
// orders and sharded runs.
// --------------------------------------------------------------------------------------
constexpr int SHUF_PART = 4096;
__host__ __device__ __forceinline__ uint64_t feistel_invert(const FeistelKeys& fk, uint64_t N, uint64_t pos) {
  uint64_t x = pos;
  do {
    uint32_t L = (uint32_t)(x >> fk.half), Rr = (uint32_t)(x & fk.mask);
#pragma unroll
    for (int r = 5; r >= 0; r--) {
      const uint32_t t = Rr ^ (fmix32(L * 0x9E3779B1u + fk.k[r]) & fk.mask);
      Rr = L; L = t;
    }
    x = ((uint64_t)L << fk.half) | Rr;
  } while (x >= N);
  return x;
}
struct ShufBatch {
  FeistelKeys fk[5];
  int2* posr[4];                // [position] (internal cell | -1, rank inside its (part, bin))
  int2* lpair[4]; int* lorder[4]; int* lcombo[4]; int* boff[4];
  int* partcnt[4];              // [block][part][bin] the part's offset inside the bin
  int* binbase[4]; int* bincnt[4]; int* binacc[4];     // [block][bin] first slot / cells / cells, accumulated by the parts (zero between batches)
  uint64_t Nglob, goff, cpb; float inv_cpb; int nr, P;
};
__global__ __launch_bounds__(256) void k_shuf_blocks(Dev D, BlockIdArgs A) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D.n) return;
  D.blk[i] = block_of(feistel_apply(A.fk, A.Nglob, A.goff + (uint64_t)D.perm[i]), A, D.nb);
}
// positions [s, e) of (block b, part p)
__device__ __forceinline__ void shuf_range(const ShufBatch& S, int nb, int b, int p, uint64_t& s, uint64_t& e) {
  const uint64_t p0 = min((uint64_t)b * S.cpb, S.Nglob), p1 = (b == nb - 1) ? S.Nglob : min((uint64_t)(b + 1) * S.cpb, S.Nglob);
  s = min(p0 + (uint64_t)p * SHUF_PART, p1); e = min(s + SHUF_PART, p1);
}
// One pass of the six-round network over x: forward with keys k[0..5], or -- swap the halves, keys in reverse order, swap back -- its inverse.
__device__ __forceinline__ uint64_t feistel_pass(const FeistelKeys& kf, const FeistelKeys& ki, const bool inv, const uint64_t x) {
  const int half = kf.half; const uint32_t mask = kf.mask;          // (same domain: the two key sets differ in the keys only)
  uint32_t hi = (uint32_t)(x >> half), lo = (uint32_t)(x & mask);
  uint32_t L = inv ? lo : hi, Rr = inv ? hi : lo;
#pragma unroll
  for (int r = 0; r < 6; r++) {
    const uint32_t kr = inv ? ki.k[5 - r] : kf.k[r];
    const uint32_t t = L ^ (fmix32(Rr * 0x9E3779B1u + kr) & mask);
    L = Rr; Rr = t;
  }
  hi = inv ? Rr : L; lo = inv ? L : Rr;
  return ((uint64_t)hi << half) | lo;
}
constexpr int SHUF_THREADS = 256, SHUF_U = SHUF_PART / SHUF_THREADS;
// The bijection walks cycles: an image outside [0, N) is mapped again (up to 3/4 of all images when N is just above a power of four).  With
// one position per lane and pass, a wave repeats a pass until its UNLUCKIEST lane is inside -- 13 passes instead of 3.3 at 1.25M cells.  Here
// every lane works through its 16 positions as a little state machine (position -> cell: inverse passes; cell -> next block: forward
// passes of the next round's keys) and starts its next position the moment one is done: a wave then runs for the lane with the largest SUM of
// passes, which is close to the mean.  Results go to LDS; cell lookup, bin count and rank follow in a second, unrolled phase.
__global__ __launch_bounds__(SHUF_THREADS) void k_shuf_count(Dev D, ShufBatch S) {
  extern __shared__ int sm_[];
  const int r = blockIdx.y, b = blockIdx.x / S.P, p = blockIdx.x - b * S.P, tid = threadIdx.x, nb = D.nb, Q = D.Q;
  const int nbin = (D.nxt ? nb : 1) * Q;
  int* const cnt = sm_; int* const qf = sm_ + nbin;
  unsigned* const gbuf = reinterpret_cast<unsigned*>(qf + (Q + 1)); unsigned char* const nbuf = reinterpret_cast<unsigned char*>(gbuf + SHUF_PART);
  for (int v = tid; v < nbin; v += SHUF_THREADS) cnt[v] = 0;
  for (int v = tid; v <= Q; v += SHUF_THREADS) qf[v] = D.qstart[v];
  uint64_t s, e; shuf_range(S, nb, b, p, s, e);
  int2* __restrict__ const pr = S.posr[r];
  const bool nxt = D.nxt != 0;
  BlockIdArgs A; A.cpb = S.cpb; A.inv_cpb = S.inv_cpb;
  const FeistelKeys ki = S.fk[r], kf = S.fk[r + 1];
  const int nitem = (s + tid < e) ? min(SHUF_U, (int)((e - s - tid + SHUF_THREADS - 1) / SHUF_THREADS)) : 0;
  {
    int u = 0; bool inv = true; unsigned gcur = 0;
    uint64_t x = s + tid;
    while (u < nitem) {
      const uint64_t y = feistel_pass(kf, ki, inv, x);
      if (y >= S.Nglob) { x = y; continue; }
      if (inv) {
        const bool local = y >= S.goff && y < S.goff + (uint64_t)D.n;
        if (local && nxt) { gcur = (unsigned)(y - S.goff); inv = false; x = y; continue; }
        gbuf[u * SHUF_THREADS + tid] = local ? (unsigned)(y - S.goff) : 0xFFFFFFFFu; nbuf[u * SHUF_THREADS + tid] = 0;
      } else {
        gbuf[u * SHUF_THREADS + tid] = gcur; nbuf[u * SHUF_THREADS + tid] = (unsigned char)block_of(y, A, nb);
        inv = true;
      }
      u++; x = s + (uint64_t)u * SHUF_THREADS + tid;
    }
  }
  __syncthreads();                                  // (cnt / qf initialised; a lane reads back only what it wrote itself)
  int ci[SHUF_U];
#pragma unroll
  for (int u = 0; u < SHUF_U; u++) {
    const unsigned g = u < nitem ? gbuf[u * SHUF_THREADS + tid] : 0xFFFFFFFFu;
    ci[u] = ld_or(D.invperm, (size_t)(g != 0xFFFFFFFFu ? g : 0u), g != 0xFFFFFFFFu, -1);
  }
#pragma unroll
  for (int u = 0; u < SHUF_U; u++) if (u < nitem) {
    int rank = 0;
    if (ci[u] >= 0) {
      const int nbk = nbuf[u * SHUF_THREADS + tid];
      int lo = 0, hi = Q;                         // qf[q] <= cell < qf[q + 1]
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (qf[mid] <= ci[u]) lo = mid; else hi = mid; }
      rank = atomicAdd(&cnt[nbk * Q + lo], 1) | (lo << 12) | (nbk << 23);     // (a part has 4096 positions: the rank fits 12 bits; combination (11) and next block (6) ride along)
    }
    pr[s + (uint64_t)u * SHUF_THREADS + tid] = make_int2(ci[u], rank);
  }
  __syncthreads();
  // the part's offset inside every bin of its block: whatever a returning atomic on the bin's size hands out (a bin has to be pure, the
  // order of the parts inside it is free); k_shuf_scan reads the sizes and leaves them zero for the next batch into this order set
  for (int v = tid; v < nbin; v += SHUF_THREADS) {
    const int c = cnt[v];
    S.partcnt[r][((size_t)b * S.P + p) * nbin + v] = c ? atomicAdd(&S.binacc[r][b * nbin + v], c) : 0;
  }
}
__global__ __launch_bounds__(1024) void k_shuf_scan(Dev D, ShufBatch S) {
  __shared__ int red[16];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nb = D.nb, P = S.P;
  const int nbin = (D.nxt ? nb : 1) * D.Q, nbt = nb * nbin;
  const int per = (nbt + 1023) >> 10;
  int own = 0;
  for (int k = 0; k < per; k++) {
    const int t = min(tid * per + k, nbt - 1);
    const int c = S.binacc[r][t];
    if (tid * per + k < nbt) { S.binacc[r][t] = 0; S.bincnt[r][t] = c; own += (c + 15) & ~15; }
  }
  int incl = own;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off, 64); if (lane >= off) incl += t; }
  if (lane == 63) red[w] = incl;
  __syncthreads();
  int wbase = 0, total = 0;
  for (int x = 0; x < 16; x++) { const int t = red[x]; if (x < w) wbase += t; total += t; }
  int run = wbase + incl - own;
  for (int k = 0; k < per; k++) {
    const int t = tid * per + k;
    if (t < nbt) {
      S.binbase[r][t] = run;
      if (t % nbin == 0) S.boff[r][t / nbin] = run;
      run += (S.bincnt[r][t] + 15) & ~15;
    }
  }
  if (tid == 0) S.boff[r][nb] = total;
}
__global__ __launch_bounds__(1024) void k_shuf_place(Dev D, ShufBatch S) {
  extern __shared__ int sm_[];
  const int r = blockIdx.y, b = blockIdx.x / S.P, p = blockIdx.x - b * S.P, tid = threadIdx.x, nb = D.nb, Q = D.Q;
  const int nbin = (D.nxt ? nb : 1) * Q;
  int* const base = sm_;
  for (int v = tid; v < nbin; v += 1024) base[v] = S.binbase[r][b * nbin + v] + S.partcnt[r][((size_t)b * S.P + p) * nbin + v];
  __syncthreads();
  uint64_t s, e; shuf_range(S, nb, b, p, s, e);
  const int2* __restrict__ const pr = S.posr[r];
  const bool nxt = D.nxt != 0;
  int2* __restrict__ const lp = S.lpair[r];
  int* __restrict__ const lo_ = S.lorder[r]; int* __restrict__ const lc_ = S.lcombo[r];
  constexpr int U = SHUF_PART / 1024;
  int2 cr[U];
#pragma unroll
  for (int u = 0; u < U; u++) { const uint64_t pos = s + (uint64_t)u * 1024 + tid; cr[u] = pos < e ? pr[pos] : make_int2(-1, 0); }
#pragma unroll
  for (int u = 0; u < U; u++) if (cr[u].x >= 0) {
    const int q = (cr[u].y >> 12) & 0x7FF, nbk = cr[u].y >> 23, dst = base[nbk * Q + q] + (cr[u].y & 0xFFF);
    if (D.need_lorder) { lo_[dst] = cr[u].x; lc_[dst] = q; }
    lp[dst] = make_int2(cr[u].x, nxt ? (q | (nbk << 19) | (b << 25)) : q);        // (combination, next block, block): see flush_run in k_tile
  }
  if (p == 0)                                    // the padding slots of the block's bins: "no cell"
    for (int v = tid; v < nbin; v += 1024) {
      const int c = S.bincnt[r][b * nbin + v], st = S.binbase[r][b * nbin + v], pad = (c + 15) & ~15;
      for (int k = c; k < pad; k++) { if (D.need_lorder) lo_[st + k] = -1; lp[st + k] = make_int2(-1, -1); }
    }
}
// oe_arith: the round's shuffled order itself, posord[position] = internal cell id (arma::shuffle's update_order, src/harmony.cpp:272-273,
// for the documented generator: cell g sits at position feistel(seed, round, g))
__global__ void k_ref_posord(Dev D, FeistelKeys fk, uint64_t Nglob, int* __restrict__ posord, int* __restrict__ poslev) {
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < D.n; g += gridDim.x * blockDim.x) {
    const int cell = D.invperm[g];
    const size_t pos = (size_t)feistel_apply(fk, Nglob, (uint64_t)g);
    posord[pos] = cell;
    if (poslev) {       // the position's level codes, [c][n]: the sequential-sum kernels then need no combo / qlev lookups
      const int q = D.combo[cell];
      for (int c = 0; c < D.C && c < 4; c++) poslev[(size_t)c * D.n + pos] = D.qlev[q * D.C + c];
    }
  }
}

// --------------------------------------------------------------------------------------
// update_R (src/harmony.cpp:269-342): the streaming passes around the block update (k_tile MODE 0, hmx_k_tile.inc)
//   k_oldsum*  one pass: old contribution of EVERY block of this round (:312-313 for all blocks)
//   k_fold / k_penalty, k_foldpen   O <- O + new(prev block) - old(this block); penalty table (:322)
//   k_obj_reduce / k_obj_final      the objective partials of the wave slots -> obj[0..1]
// --------------------------------------------------------------------------------------
template <int KPL>
__global__ __launch_bounds__(TPB) void k_oldsum(Dev D) {
  constexpr int CB = 4;
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
  const int K = D.K;
  const int total = D.boff[D.nb];  // padded length of this round's order
  const int per = (total + nw - 1) / nw;
  const int s = wave * per, e = min(total, s + per);
  if (s >= e) return;
  unsigned long long oacc[KPL];
#pragma unroll
  for (int q = 0; q < KPL; q++) oacc[q] = 0ull;
  int curq = -1, curb = -1;
  for (int p = s; p < e; p += CB) {
    const int nc = min(CB, e - p);
    int cell[CB]; float r[CB][KPL];
#pragma unroll
    for (int c = 0; c < CB; c++) {
      cell[c] = ld_or(D.lorder, (size_t)min(p + c, e - 1), c < nc, -1);  // -1: padding slot
#pragma unroll
      for (int q = 0; q < KPL; q++) {
        const int k = lane + 64 * q;
        r[c][q] = ld_or(D.R, (size_t)max(cell[c], 0) * K + min(k, K - 1), cell[c] >= 0 && k < K, 0.0f);
      }
    }
#pragma unroll
    for (int c = 0; c < CB; c++) {
      if (cell[c] >= 0) {
        const int b = D.blk[cell[c]], q0 = D.lcombo[p + c];
        if (b != curb || q0 != curq) {
          if (curq >= 0) flush_fx<KPL>(D.Sold_fx + (size_t)curb * D.B * K, D.qlev, curq, D.C, K, lane, oacc);
          curb = b; curq = q0;
        }
#pragma unroll
        for (int q = 0; q < KPL; q++) oacc[q] += fx_of(r[c][q]);
      }
    }
  }
  if (curq >= 0) flush_fx<KPL>(D.Sold_fx + (size_t)curb * D.B * K, D.qlev, curq, D.C, K, lane, oacc);
}

// k_oldsum_stream: the same sums, but R is read in INTERNAL cell order -- a pure sequential stream of the K-float rows
// instead of a gather through this round's sorted order.  The target table of a cell depends on its block id, so the
// accumulators live in LDS ([nb][K] 64-bit fixed point, ds_add_u64; the 64 lanes of a wave hit 64 different clusters of
// one block: conflict free) and are flushed with global atomics when the combination changes and at the end of the
// workgroup's contiguous range of sort chunks (<= SORT_CHUNK cells of one combination each).  Integer sums: exact,
// order independent, identical to k_oldsum's.
template <int KPL>
__global__ __launch_bounds__(256) void k_oldsum_stream(Dev D) {
  extern __shared__ unsigned long long otab[];   // [nb][K]
  const int K = D.K, nT = D.nb * K;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int cpw = (D.nchunks + gridDim.x - 1) / gridDim.x;
  const int c0 = blockIdx.x * cpw, c1 = min(D.nchunks, c0 + cpw);
  if (c0 >= c1) return;
  for (int i = threadIdx.x; i < nT; i += blockDim.x) otab[i] = 0ull;
  __syncthreads();
  auto flush = [&](int q) {   // + zero
    for (int i = threadIdx.x; i < nT; i += blockDim.x) {
      const unsigned long long v = otab[i];
      if (v) {
        const int blk = i / K, k = i - blk * K;
        for (int cc = 0; cc < D.C; cc++)
          atomicAdd((unsigned long long*)&D.Sold_fx[((size_t)blk * D.B + D.qlev[q * D.C + cc]) * K + k], v);
        otab[i] = 0ull;
      }
    }
  };
  int curq = D.schunks[c0].q;
  for (int ch = c0; ch < c1; ch++) {
    const Item it = D.schunks[ch];
    if (it.q != curq) { __syncthreads(); flush(curq); __syncthreads(); curq = it.q; }
    const int per = (it.cnt + 3) >> 2;                          // the chunk's cells: one contiguous quarter per wave
    const int s = it.start + w * per, e = min(it.start + it.cnt, s + per);
    for (int base = s; base < e; base += 64) {
      const int n = min(64, e - base);
      const int bv = D.blk[min(base + lane, e - 1)];           // block ids of the next 64 cells, one per lane
      for (int u = 0; u < n; u += 8) {                          // eight rows (3.2 KB at K = 100) in flight per wave
        float r[8][KPL];
#pragma unroll
        for (int c = 0; c < 8; c++) {
          const size_t row = (size_t)min(base + u + c, e - 1) * K;
#pragma unroll
          for (int q = 0; q < KPL; q++) r[c][q] = D.R[row + min(lane + 64 * q, K - 1)];
        }
#pragma unroll
        for (int c = 0; c < 8; c++) {
          if (u + c < n) {
            const int b = __builtin_amdgcn_readlane(bv, u + c);
#pragma unroll
            for (int q = 0; q < KPL; q++)
              if (lane + 64 * q < K) atomicAdd(&otab[b * K + lane + 64 * q], fx_of(r[c][q]));
          }
        }
      }
    }
  }
  __syncthreads();
  flush(curq);
}

// k_oldsum_stream4: as k_oldsum_stream for K % 4 == 0 -- the rows of a sort chunk are ONE contiguous run of floats, read
// with 16-byte loads (four in flight per lane); a lane's four floats belong to one cell, whose block id selects the LDS row.
// 1024-thread workgroups over ~4 chunks each: full occupancy with a quarter of the flush atomics (measured: the 4M global
// atomics of one-chunk workgroups cost 32 of 128 us).
__global__ __launch_bounds__(1024) void k_oldsum_stream4(Dev D) {
  extern __shared__ unsigned long long otab[];   // [nb][K]
  const int K = D.K, nT = D.nb * K;
  const int cpw = (D.nchunks + gridDim.x - 1) / gridDim.x;
  const int c0 = blockIdx.x * cpw, c1 = min(D.nchunks, c0 + cpw);
  if (c0 >= c1) return;
  for (int i = threadIdx.x; i < nT; i += blockDim.x) otab[i] = 0ull;
  __syncthreads();
  // LDS layout of a block's row: entry (k % 4) * K/4 + k / 4 holds cluster k -- a lane owns four CONSECUTIVE clusters of a cell, and
  // with the natural layout its four ds_add_u64 would sit 32 bytes from its neighbours' (8 lanes per bank pair: rocprof counted
  // 77 % of the LDS cycles of this kernel as bank conflicts); transposed, the lanes of one atomic instruction hit consecutive slots
  const int K4 = K >> 2;
  auto flush = [&](int q) {   // + zero
    for (int i = threadIdx.x; i < nT; i += blockDim.x) {
      const unsigned long long v = otab[i];
      if (v) {
        const int blk = i / K, kp = i - blk * K, k = (kp % K4) * 4 + kp / K4;
        for (int cc = 0; cc < D.C; cc++)
          atomicAdd((unsigned long long*)&D.Sold_fx[((size_t)blk * D.B + D.qlev[q * D.C + cc]) * K + k], v);
        otab[i] = 0ull;
      }
    }
  };
  const unsigned magic = (unsigned)((0x100000000ull + (unsigned)K - 1) / (unsigned)K);   // floor(n / K) = umulhi(n, magic), n < 2^32 / K
  int curq = D.schunks[c0].q;
  for (int ch = c0; ch < c1; ch++) {
    const Item it = D.schunks[ch];
    if (it.q != curq) { __syncthreads(); flush(curq); __syncthreads(); curq = it.q; }
    const f32x4* src = reinterpret_cast<const f32x4*>(D.R + (size_t)it.start * K);
    const int n4 = it.cnt * (K >> 2);                            // float4 groups of this chunk
    for (int base = 0; base < n4; base += 4 * (int)blockDim.x) {
      f32x4 v[4]; int bl[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int f = min(base + u * (int)blockDim.x + (int)threadIdx.x, n4 - 1);
        v[u] = src[f];
        bl[u] = D.blk[it.start + (int)__umulhi((unsigned)(4 * f), magic)];
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int f = base + u * (int)blockDim.x + (int)threadIdx.x;
        if (f < n4) {
          const int cell = (int)__umulhi((unsigned)(4 * f), magic);
          unsigned long long* row = otab + bl[u] * K + ((4 * f - cell * K) >> 2);
#pragma unroll
          for (int e = 0; e < 4; e++) {
#ifdef HMX_OS_NOATOM   // timing experiment (tools/oldsum_cmp.sh): no LDS atomics
            if (fx_of(v[u][e]) == 0x123456789ull) row[e * K4] = 1;
#else
            atomicAdd(&row[e * K4], fx_of(v[u][e]));
#endif
          }
        }
      }
    }
  }
  __syncthreads();
  flush(curq);
}

// fold the finished block into O and build the penalty table of block j (j < 0: fold only).
// Phase 1 (k_fold): O_fx[b][k] += Snew - Sold[j]; Snew = 0.   Phase 2 (k_penalty): pen[b][k].
// One thread per table entry; two launches because phase 2 reads a column sum of phase 1.
// mode 0: O += sum_rep Snew[rep] - Sold[j] (single GPU).  mode 1: Snew[0] = sum_rep Snew[rep] only (the
// sharded path all-reduces Snew[0] next).  mode 2: O += Snew[0] - Sold[j] (after that all-reduce).  mode 3: O = sum_rep Snew[rep] -- the head's
// fold: O is written, never read, so nobody has to clear it first.
__global__ void k_fold(Dev D, int j, int mode) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = D.B * D.K;
  if (i >= n) return;
  long long sn = D.Snew_fx[i];
  if (mode != 2) for (int r = 1; r < D.nrep; r++) { sn += D.Snew_fx[(size_t)r * n + i]; D.Snew_fx[(size_t)r * n + i] = 0; }
  if (mode == 1) { D.Snew_fx[i] = sn; return; }
  long long o = (mode == 3 ? 0 : D.O_fx[i]) + sn;
  if (j >= 0) o -= D.Sold_fx[(size_t)j * n + i];
  D.O_fx[i] = o;
  D.Snew_fx[i] = 0;
}
// objective partial slots -> obj[0..1]
__global__ __launch_bounds__(1024) void k_obj_reduce(Dev D) {
  __shared__ double ra[1024], rb[1024];
  double a = 0.0, b = 0.0;
  double* row = D.objpart + (size_t)blockIdx.x * D.nwmax * 2;
  for (int i = threadIdx.x; i < D.nwmax; i += 1024) { a += row[2 * i]; b += row[2 * i + 1]; row[2 * i] = 0.0; row[2 * i + 1] = 0.0; }
  ra[threadIdx.x] = a; rb[threadIdx.x] = b;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if (threadIdx.x < off) { ra[threadIdx.x] += ra[threadIdx.x + off]; rb[threadIdx.x] += rb[threadIdx.x + off]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { D.objrow[2 * blockIdx.x] = ra[0]; D.objrow[2 * blockIdx.x + 1] = rb[0]; }
}
// fixed-order sum of the slot rows -> obj[0..1]
__global__ void k_obj_final(Dev D) {
  double a = 0.0, b = 0.0;
  for (int s = 0; s < D.objslots; s++) { a += D.objrow[2 * s]; b += D.objrow[2 * s + 1]; }
  D.obj[0] = a; D.obj[1] = b;
}
// One GPU: the three kernels that close a clustering round (slot rows -> obj[0..1] -> cross-entropy term, snapshot, chain control
// reset) as ONE launch: every workgroup reduces its slot row, the last one to finish (ticket) does the rest.  Same fixed-order sums.
__global__ __launch_bounds__(1024) void k_round_tail(Dev D, double* __restrict__ host_slot, long long* __restrict__ z0, size_t n0,
                                                      long long* __restrict__ z1, size_t n1) {
  __shared__ double ra[1024], rb[1024];
  __shared__ int last;
  const int tid = threadIdx.x;
  {  // the old-contribution table this round consumed and the replica sets start the next rounds from zero: cleared here instead
     // of by memset launches
    for (size_t i = (size_t)blockIdx.x * 1024 + tid; i < n0; i += (size_t)gridDim.x * 1024) z0[i] = 0;
    for (size_t i = (size_t)blockIdx.x * 1024 + tid; i < n1; i += (size_t)gridDim.x * 1024) z1[i] = 0;
  }
  double a = 0.0, b = 0.0;
  double* row = D.objpart + (size_t)blockIdx.x * D.nwmax * 2;
  for (int i = tid; i < D.nwmax; i += 1024) { a += row[2 * i]; b += row[2 * i + 1]; row[2 * i] = 0.0; row[2 * i + 1] = 0.0; }
  ra[tid] = a; rb[tid] = b;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if (tid < off) { ra[tid] += ra[tid + off]; rb[tid] += rb[tid + off]; }
    __syncthreads();
  }
  if (tid == 0) {
    // No fences: an agent-scope release here would write back everything the round left dirty in this XCD's L2 (tens of MB of R
    // rows).  The two sums go out as write-through device-scope stores, the ticket follows once they are acknowledged, and the
    // last workgroup reads them with device-scope loads (the scheme of the block chain, DESIGN 4.1).
    __hip_atomic_store(&D.objrow[2 * blockIdx.x], ra[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&D.objrow[2 * blockIdx.x + 1], rb[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = (atomicAdd(D.tail_ticket, 1) == (int)gridDim.x - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!last) return;
  const int K = D.K, B = D.B;
  double cross = 0.0;
  // many levels (B >= 64; configs[4]: 200 x 200 entries, each a division and a logarithm): G threads per cluster take every G-th level and their partial sums are
  // added in ascending order -- one thread per cluster needed 75 of this launch's 88 us (rocprofv3, round 6), 2.1 ms of a 52 ms run.  (The level sums then
  // associate differently from k_objective_tables': ~1e-16 of the term.)
  const int G = (B >= 64 && K <= 512) ? min(8, 1024 / K) : 1;
  if (G > 1) {
    const int k = tid % K, j = tid / K;
    double part = 0.0;
    if (j < G) {
      long long rs = 0;
      for (int b0 = 0; b0 < D.B0; b0++) rs += D.O_fx[(size_t)b0 * K + k];
      const double rsd = (double)rs * FX_INV;
      for (int bb = j; bb < B; bb += G) {
        const double od = (double)D.O_fx[(size_t)bb * K + k] * FX_INV;
        const float o = (float)od, e = (float)(rsd * (double)D.Pr_b[bb]);
        const float m = D.theta[bb] * logf((o + e + 1.0f) / ((2.0f * e) + 1.0f));
        part += od * (double)m;
      }
    }
    __syncthreads();
    rb[tid] = part;
    __syncthreads();
    if (tid < K) {
      double ck = 0.0;
      for (int jj = 0; jj < G; jj++) ck += rb[jj * K + tid];
      cross = ck * (double)D.sigma[tid];
    }
  } else
  for (int k = tid; k < K; k += 1024) {      // (same arithmetic as k_objective_tables)
    long long rs = 0;
    for (int b0 = 0; b0 < D.B0; b0++) rs += D.O_fx[(size_t)b0 * K + k];
    const double rsd = (double)rs * FX_INV;
    double ck = 0.0;
    for (int bb = 0; bb < B; bb++) {
      const double od = (double)D.O_fx[(size_t)bb * K + k] * FX_INV;
      const float o = (float)od, e = (float)(rsd * (double)D.Pr_b[bb]);
      const float m = D.theta[bb] * logf((o + e + 1.0f) / ((2.0f * e) + 1.0f));
      ck += od * (double)m;
    }
    cross += ck * (double)D.sigma[k];
  }
  __syncthreads();
  ra[tid] = cross;
  __syncthreads();
  // (K <= 256: every thread holds at most one cluster, the entries from 256 on are zero -- the same pairwise tree as
  //  k_objective_tables' 256-entry one, preceded by two levels that add zeros: identical bits)
  for (int off = 512; off > 0; off >>= 1) {
    if (tid < off) ra[tid] += ra[tid + off];
    __syncthreads();
  }
  // the slot rows' sums: fetched by 2 x objslots threads at once (objslots <= 64), added in slot order by one -- the 40 device-scope
  // loads used to be ONE thread's dependent chain, ~20 us of every round
  if (tid < 2 * D.objslots) rb[tid] = __hip_atomic_load(&D.objrow[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (tid == 0) {
    double sa = 0.0, sb = 0.0;
    for (int sl = 0; sl < D.objslots; sl++) { sa += rb[2 * sl]; sb += rb[2 * sl + 1]; }
    D.obj[0] = sa; D.obj[1] = sb;
    D.obj[2] = sa; D.obj[3] = sb; D.obj[4] = ra[0];
    // error word of the snapshot: the chain's code (< 16) + 16 if a ridge system of the correction before this round was singular
    const double err = (D.chain_ctl ? (double)D.chain_ctl[1] : 0.0) + ((D.solve_err && *D.solve_err) ? 16.0 : 0.0);
    D.obj[5] = err;
    if (host_slot) {     // pinned host memory, mapped into the device: visible to the host once the event behind this launch completed
      __hip_atomic_store(&host_slot[0], sa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&host_slot[1], sb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&host_slot[2], ra[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(&host_slot[3], err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    *D.tail_ticket = 0;
  }
  __syncthreads();
  if (D.chain_ctl) for (int i = tid; i < 8 * D.nb + 24; i += 1024) D.chain_ctl[i] = 0;
}
// Single-launch variant (one GPU): fold + penalty with ping-pong tables, so no thread reads what another writes;
// one workgroup per 16 clusters, the new O column block goes through LDS for the covariate-0 row sums.
//   Oin/Sin: O and the replicas filled by the previous block update;  Oout: new O;  Szero: the replica set the NEXT
//   update accumulates into (zeroed here).  j < 0: fold only.
__global__ __launch_bounds__(256) void k_foldpen(Dev D, int j, const long long* __restrict__ Oin, long long* __restrict__ Oout,
                                                 const long long* __restrict__ Sin, long long* __restrict__ Szero) {
  extern __shared__ long long shO[];  // [B][16] new O of this workgroup's 16 clusters
  const int K = D.K, B = D.B, n = B * K;
  const int kk = threadIdx.x & 15, k = blockIdx.x * 16 + kk;
  const long long* sold = (j >= 0) ? D.Sold_fx + (size_t)j * n : nullptr;
  for (int b = threadIdx.x >> 4; b < B; b += 16) {
    long long o = 0;
    if (k < K) {
      const size_t i = (size_t)b * K + k;
      o = Oin[i];
      for (int r = 0; r < D.nrep; r++) { o += Sin[(size_t)r * n + i]; Szero[(size_t)r * n + i] = 0; }
      if (sold) o -= sold[i];
      Oout[i] = o;
    }
    shO[b * 16 + kk] = o;
  }
  if (j < 0) return;
  __syncthreads();
  long long rs = 0;  // rowsum(R) of the cells currently "in" = sum over the levels of covariate 0 of the NEW O
  for (int b0 = 0; b0 < D.B0; b0++) rs += shO[b0 * 16 + kk];
  const double rsd = (double)rs * FX_INV;
  if (k < K)
    for (int b = threadIdx.x >> 4; b < B; b += 16) {
      const float of = (float)((double)shO[b * 16 + kk] * FX_INV);
      const float ef = (float)(rsd * (double)D.Pr_b[b]);
      D.pen[(size_t)b * K + k] = pen_pow((2.0f * ef) + 1.0f, of + ef + 1.0f, D.theta[b]);
    }
}
__global__ void k_penalty(Dev D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D.B * D.K) return;
  const int K = D.K, b = i / K, k = i - b * K;
  // rowsum(R) over the cells currently "in" = sum over the levels of covariate 0
  // (every cell has exactly one level per covariate)
  long long rs = 0;
  for (int b0 = 0; b0 < D.B0; b0++) rs += D.O_fx[(size_t)b0 * K + k];
  const float o = (float)((double)D.O_fx[i] * FX_INV);
  const float e = (float)(((double)rs * FX_INV) * (double)D.Pr_b[b]);
  D.pen[i] = pen_pow((2.0f * e) + 1.0f, o + e + 1.0f, D.theta[b]);
}

#endif  // !HMX_TILE_BF

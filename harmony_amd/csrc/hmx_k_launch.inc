// hmx_k_launch.inc -- part of hmx_kernels.hip AND of hmx_tile_bf.hip (included inside namespace hmx): the launchers (l_*), the peer-inbox self-test and all-reduces.
// --------------------------------------------------------------------------------------
// launchers
// --------------------------------------------------------------------------------------
#if HMX_TILE_BF
#define HMX_LNAME(x) x##_bf
#else
#define HMX_LNAME(x) x
size_t lds_bytes_y(const Dev& D) { return (size_t)D.d * D.KP * sizeof(float); }
#endif
// bytes of the centroid image the tile kernels of THIS translation unit stage in LDS, and of the split-bf16 one
static inline size_t bf_image_bytes(const Dev& D) { return (size_t)D.NCT * D.NS2 * 3 * 1024; }
static inline size_t tile_image_bytes(const Dev& D) { return HMX_TILE_BF ? bf_image_bytes(D) : (size_t)D.NQ * D.NS * 64 * sizeof(f32x4); }
constexpr size_t LDS_PER_CU = 160 * 1024;
// the split-bf16 build of a launch is taken when the workgroups that are to share a CU still fit its LDS with the larger image
static inline bool bf_fits(const Dev& D, size_t rest, long long blocks) {
  const long long per_cu = (blocks + 255) / 256;
  return D.dot_bf && D.Yimg3 && (bf_image_bytes(D) + rest) * (size_t)(per_cu < 1 ? 1 : per_cu) <= LDS_PER_CU;
}

#if !HMX_TILE_BF
#define HMX_DISPATCH_KD(KERNEL, GRID, LDS, ...)                                                \
  do {                                                                                         \
    const int kpl_ = D.KP / 64, dpl_ = D.d > 64 ? 2 : 1;                                       \
    if (dpl_ == 1) {                                                                           \
      switch (kpl_) {                                                                          \
        case 1: hipLaunchKernelGGL((KERNEL<1, 1>), GRID, dim3(TPB), LDS, L.stream, __VA_ARGS__); break; \
        case 2: hipLaunchKernelGGL((KERNEL<2, 1>), GRID, dim3(TPB), LDS, L.stream, __VA_ARGS__); break; \
        case 3: hipLaunchKernelGGL((KERNEL<3, 1>), GRID, dim3(TPB), LDS, L.stream, __VA_ARGS__); break; \
        default: hipLaunchKernelGGL((KERNEL<4, 1>), GRID, dim3(TPB), LDS, L.stream, __VA_ARGS__); break; \
      }                                                                                        \
    } else {                                                                                   \
      switch (kpl_) {                                                                          \
        case 1: hipLaunchKernelGGL((KERNEL<1, 2>), GRID, dim3(TPB), LDS, L.stream, __VA_ARGS__); break; \
        case 2: hipLaunchKernelGGL((KERNEL<2, 2>), GRID, dim3(TPB), LDS, L.stream, __VA_ARGS__); break; \
        case 3: hipLaunchKernelGGL((KERNEL<3, 2>), GRID, dim3(TPB), LDS, L.stream, __VA_ARGS__); break; \
        default: hipLaunchKernelGGL((KERNEL<4, 2>), GRID, dim3(TPB), LDS, L.stream, __VA_ARGS__); break; \
      }                                                                                        \
    }                                                                                          \
  } while (0)

static int stream_grid(const Launch& L, long long work_waves) {
  long long blocks = (work_waves + 3) / 4;
  if (blocks < 1) blocks = 1;
  if (blocks > L.grid) blocks = L.grid;
  return (int)blocks;
}

void l_convert_in(const Launch& L, const void* src, int f32, float* dst, const int* invperm, int n, int d, int zs) {
  if (f32) hipLaunchKernelGGL(k_convert_in<float>, dim3(2048), dim3(256), 0, L.stream, (const float*)src, dst, invperm, n, d, zs);
  else hipLaunchKernelGGL(k_convert_in<double>, dim3(2048), dim3(256), 0, L.stream, (const double*)src, dst, invperm, n, d, zs);
}
void l_convert_out(const Launch& L, const float* src, void* dst, int f32, const int* invperm, int n, int w, int ws) {
  if (f32) hipLaunchKernelGGL(k_convert_out<float>, dim3(2048), dim3(256), 0, L.stream, src, (float*)dst, invperm, n, w, ws);
  else hipLaunchKernelGGL(k_convert_out<double>, dim3(2048), dim3(256), 0, L.stream, src, (double*)dst, invperm, n, w, ws);
}
void l_zero4(const Launch& L, void* a, size_t na, void* b, size_t nb, void* c, size_t nc, void* d, size_t nd) {
  const size_t n = std::max(std::max(na, nb), std::max(nc, nd));
  if (!n) return;
  hipLaunchKernelGGL(k_zero4, dim3((unsigned)std::min<size_t>((n + 255) / 256, 1024)), dim3(256), 0, L.stream, (unsigned long long*)a, na, (unsigned long long*)b, nb,
                     (unsigned long long*)c, nc, (unsigned long long*)d, nd);
}
void l_copy(const Launch& L, const float* src, float* dst, size_t count) {
  hipLaunchKernelGGL(k_copy, dim3(2048), dim3(256), 0, L.stream, src, dst, count);
}
void l_normalize(const Launch& L, float* Z, int n, int d, int zs) {
  const int nq = zs / 4;
  if (nq <= 16) hipLaunchKernelGGL(k_normalize4<1>, dim3(stream_grid(L, (n + 15) / 16)), dim3(TPB), 0, L.stream, Z, Z, n, nq);
  else if (nq <= 32) hipLaunchKernelGGL(k_normalize4<2>, dim3(stream_grid(L, (n + 15) / 16)), dim3(TPB), 0, L.stream, Z, Z, n, nq);
  else hipLaunchKernelGGL(k_normalize, dim3(stream_grid(L, n)), dim3(TPB), 0, L.stream, Z, n, d, zs);
}
// dst = normalise(src) in one pass (restart: Z_corr = normalise(Z_orig), src/harmony.cpp:42)
void l_normalize_from(const Launch& L, const float* src, float* dst, int n, int d, int zs) {
  const int nq = zs / 4;
  if (nq <= 16) hipLaunchKernelGGL(k_normalize4<1>, dim3(stream_grid(L, (n + 15) / 16)), dim3(TPB), 0, L.stream, src, dst, n, nq);
  else if (nq <= 32) hipLaunchKernelGGL(k_normalize4<2>, dim3(stream_grid(L, (n + 15) / 16)), dim3(TPB), 0, L.stream, src, dst, n, nq);
  else { l_copy(L, src, dst, (size_t)n * zs); hipLaunchKernelGGL(k_normalize, dim3(stream_grid(L, n)), dim3(TPB), 0, L.stream, dst, n, d, zs); }
}
#endif  // !HMX_TILE_BF
// MFMA tile passes over the static 16-cell tiles: mode 1 = head, mode 2 = Lloyd, mode 3 = seeding race
void HMX_LNAME(l_tile_static)(const Launch& L, const Dev& D, int mode) {
  const int wpb = tile_threads(D.NCT) / 64;
  long long blocks = (((long long)D.ntitems + D.upd_tpw - 1) / D.upd_tpw + wpb - 1) / wpb;
  if (blocks > D.nwmax / wpb) blocks = D.nwmax / wpb;
  if (D.static_maxblocks > 0 && blocks > D.static_maxblocks) blocks = D.static_maxblocks;      // (seeding with three workgroups per CU -- 166 registers would allow it -- measured: no gain, 1.53 / 1.55 ms of k-means initialisation)
  const size_t rest = mode == 2 ? ((size_t)D.K * D.d + D.K) * sizeof(long long) : 0;
  if (mode == 2 && blocks > 512) blocks = 512;
  if (blocks < 1) blocks = 1;
  int thr = tile_threads(D.NCT);
#if !HMX_TILE_BF
  if (bf_fits(D, rest, blocks) || (mode == 2 && bf_fits(D, rest, 256))) { l_tile_static_bf(L, D, mode); return; }
#else
  // Lloyd with the larger image: two 256-thread workgroups per CU no longer fit next to their K x d sum tables -> one of 512 threads
  if (mode == 2 && !bf_fits(D, rest, blocks)) { thr = 512; blocks = (blocks + 1) / 2; if (blocks > 256) blocks = 256; }
#endif
  const size_t lds = tile_image_bytes(D) + rest;
  const dim3 grid((unsigned)blocks);
#if HMX_TILE_BF
  // Lloyd, one workgroup per CU (image + K x d sum table: 84 KB): THREE waves per SIMD -- the kernel needs 150 registers, and the MFMA chain, the
  // arg-min and the LDS sums of a tile run one after the other on one accumulator set: a third wave fills the gaps (round 6: 0.13 ms of 1.69 per
  // k-means initialisation at 1M cells against two waves per SIMD)
  if (mode == 2 && thr == 512 && D.NCT >= 5 && D.NCT <= 7) {
    switch (D.NCT) {
      case 5: hipLaunchKernelGGL((k_tile<5, 2, 3>), grid, dim3(768), lds, L.stream, D, 0); break;
      case 6: hipLaunchKernelGGL((k_tile<6, 2, 3>), grid, dim3(768), lds, L.stream, D, 0); break;
      default: hipLaunchKernelGGL((k_tile<7, 2, 3>), grid, dim3(768), lds, L.stream, D, 0); break;
    }
    return;
  }
#endif
  // head / Lloyd.  Head variants: general sigma | uniform sigma (D.usig) | uniform sigma at 4 waves per SIMD (K <= 64)
#define HMX_TS(N) case N: if (mode == 3) hipLaunchKernelGGL((k_tile<N, 3>), grid, dim3(thr), lds, L.stream, D, 0); \
                          else if (mode == 2) hipLaunchKernelGGL((k_tile<N, 2>), grid, dim3(thr), lds, L.stream, D, 0); \
                          else if (D.usig) hipLaunchKernelGGL((k_tile<N, 1, 2, true>), grid, dim3(thr), lds, L.stream, D, 0); \
                          else hipLaunchKernelGGL((k_tile<N, 1>), grid, dim3(thr), lds, L.stream, D, 0); break;
#define HMX_TSL(N) case N: hipLaunchKernelGGL((k_tile<N, 1, 4, true>), grid, dim3(thr), lds, L.stream, D, 0); break;
  if (mode == 1 && D.upd_wps == 4) {
    switch (D.NCT) {
      HMX_TSL(1) HMX_TSL(2) HMX_TSL(3) HMX_TSL(4)
      default: break;
    }
    return;
  }
  switch (D.NCT) {
    HMX_TS(1) HMX_TS(2) HMX_TS(3) HMX_TS(4) HMX_TS(5) HMX_TS(6) HMX_TS(7) HMX_TS(8)
    HMX_TS(10) HMX_TS(12) HMX_TS(13) HMX_TS(14) HMX_TS(16)
    default: break;
  }
#undef HMX_TS
#undef HMX_TSL
}
#if !HMX_TILE_BF
void l_head(const Launch& L, const Dev& D) {
  HMX_DISPATCH_KD(k_head, dim3(stream_grid(L, D.nitems)), lds_bytes_y(D), D);
}
// fused = true: D.blk is produced by the histogram kernel from (seed, round); false: the host uploaded D.blk (injected shuffle)
static SortPtrs sort_ptrs_of(const Dev& D) { return SortPtrs{D.blk, D.blkv, D.counts, D.offs, D.binoff, D.bincnt, D.boff, D.lorder, D.lcombo, D.lpair}; }
static BlockIdArgs block_id_args(uint64_t seed, uint64_t round, uint64_t Nglob, uint64_t goff, uint64_t cells_per_block) {
  BlockIdArgs A;
  A.fk = make_keys(seed, round, Nglob); A.fk2 = make_keys(seed, round + 1, Nglob); A.Nglob = Nglob; A.goff = goff; A.cpb = cells_per_block;
  A.inv_cpb = 1.0f / (float)cells_per_block;
  return A;
}
// the histogram half (block ids from the Feistel bijection + per-chunk counts): depends on nothing but (seed, round)
void l_sort_hist(const Launch& L, const Dev& D, bool fused, uint64_t seed, uint64_t round, uint64_t Nglob, uint64_t goff, uint64_t cells_per_block) {
  const int nV = D.nxt ? D.nb * D.nb : D.nb;
  const size_t lds = (size_t)nV * sizeof(int);
  BlockIdBatch AB{}; AB.a[0] = block_id_args(seed, round, Nglob, goff, cells_per_block);
  SortBatch S{}; S.p[0] = sort_ptrs_of(D);
  if (fused) hipLaunchKernelGGL(k_sort_hist<true>, dim3(D.nchunks), dim3(WAVE), lds, L.stream, D, AB, S);
  else hipLaunchKernelGGL(k_sort_hist<false>, dim3(D.nchunks), dim3(WAVE), lds, L.stream, D, AB, S);
}
// the dependent half: bin offsets from the counts, then the placement (padding slots = -1: written by k_sort_scatter, bin by bin)
void l_sort_tail(const Launch& L, const Dev& D) {
  const int nV = D.nxt ? D.nb * D.nb : D.nb;
  const size_t lds = (size_t)nV * sizeof(int);
  SortBatch S{}; S.p[0] = sort_ptrs_of(D);
  hipLaunchKernelGGL(k_sort_binscan, dim3(nV * D.Q), dim3(WAVE), 0, L.stream, D, S);
  hipLaunchKernelGGL(k_sort_binoff, dim3(1), dim3(1024), 0, L.stream, D, S);
  hipLaunchKernelGGL(k_sort_scatter, dim3(D.nchunks), dim3(WAVE), lds, L.stream, D, S);
}
void l_sort_blocks(const Launch& L, const Dev& D, bool fused, uint64_t seed, uint64_t round, uint64_t Nglob, uint64_t goff,
                   uint64_t cells_per_block) {
  l_sort_hist(L, D, fused, seed, round, Nglob, goff, cells_per_block);
  l_sort_tail(L, D);
}
// The shuffles of `nr` consecutive rounds (first: `round`) in ONE set of four launches, blockIdx.y = the round: the four kernels of a
// sort are latency-bound chains of small dependent steps, so four rounds cost little more than one -- and inside a cluster_cpp call
// no sort is left between two block chains (round 3: 4 x ~70 us of sort tail, event hand-over and dispatch per call).
void l_sort_batch(const Launch& L, const Dev& D, const SortBatch& S, int nr, uint64_t seed, uint64_t round, uint64_t Nglob, uint64_t goff,
                  uint64_t cells_per_block) {
  const int nV = D.nxt ? D.nb * D.nb : D.nb;
  const size_t lds = (size_t)nV * sizeof(int);
  BlockIdBatch AB{};
  for (int r = 0; r < nr; r++) AB.a[r] = block_id_args(seed, round + (uint64_t)r, Nglob, goff, cells_per_block);
  hipLaunchKernelGGL(k_sort_hist<true>, dim3(D.nchunks, nr), dim3(WAVE), lds, L.stream, D, AB, S);
  hipLaunchKernelGGL(k_sort_binscan, dim3(nV * D.Q, nr), dim3(WAVE), 0, L.stream, D, S);
  hipLaunchKernelGGL(k_sort_binoff, dim3(nr), dim3(1024), 0, L.stream, D, S);
  hipLaunchKernelGGL(k_sort_scatter, dim3(D.nchunks, nr), dim3(WAVE), lds, L.stream, D, S);
}
// the padded orders of rounds round..round + nr - 1 from the inverse of the shuffle (k_shuf_*)
int shuffle_parts(uint64_t Nglob, int nb, uint64_t cells_per_block) {
  const uint64_t last = Nglob > (uint64_t)(nb - 1) * cells_per_block ? Nglob - (uint64_t)(nb - 1) * cells_per_block : 0;
  return (int)((std::max<uint64_t>(std::max(cells_per_block, last), 1) + SHUF_PART - 1) / SHUF_PART);
}
void l_shuffle_inv(const Launch& L, const Dev& D, const ShufSets& T, int nr, uint64_t seed, uint64_t round, uint64_t Nglob, uint64_t goff,
                   uint64_t cells_per_block) {
  ShufBatch S{};
  for (int r = 0; r < nr + 1; r++) S.fk[r] = make_keys(seed, round + (uint64_t)r, Nglob);
  for (int r = 0; r < nr; r++) {
    S.posr[r] = T.posr[r]; S.lpair[r] = T.lpair[r]; S.lorder[r] = T.lorder[r]; S.lcombo[r] = T.lcombo[r]; S.boff[r] = T.boff[r];
    S.partcnt[r] = T.partcnt[r]; S.binbase[r] = T.binbase[r]; S.bincnt[r] = T.bincnt[r]; S.binacc[r] = T.binacc[r];
  }
  S.Nglob = Nglob; S.goff = goff; S.cpb = cells_per_block; S.inv_cpb = 1.0f / (float)cells_per_block; S.nr = nr;
  S.P = shuffle_parts(Nglob, D.nb, cells_per_block);
  const int nbin = (D.nxt ? D.nb : 1) * D.Q;
  hipLaunchKernelGGL(k_shuf_count, dim3((unsigned)(S.P * D.nb), nr), dim3(SHUF_THREADS), ((size_t)nbin + D.Q + 1 + SHUF_PART) * sizeof(int) + SHUF_PART, L.stream, D, S);
  hipLaunchKernelGGL(k_shuf_scan, dim3(nr), dim3(1024), 0, L.stream, D, S);
  hipLaunchKernelGGL(k_shuf_place, dim3((unsigned)(S.P * D.nb), nr), dim3(1024), (size_t)nbin * sizeof(int), L.stream, D, S);
}
// D.blk of one round (the sort-free shuffle does not need it; the passes that sum a round's old contributions from R do)
void l_shuffle_blocks(const Launch& L, const Dev& D, uint64_t seed, uint64_t round, uint64_t Nglob, uint64_t goff, uint64_t cells_per_block) {
  hipLaunchKernelGGL(k_shuf_blocks, dim3((unsigned)((D.n + 255) / 256)), dim3(256), 0, L.stream, D, block_id_args(seed, round, Nglob, goff, cells_per_block));
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
void l_ref_posord(const Launch& L, const Dev& D, uint64_t seed, uint64_t round, uint64_t Nglob, int* posord, int* poslev) {
  hipLaunchKernelGGL(k_ref_posord, dim3(1024), dim3(256), 0, L.stream, D, make_keys(seed, round, Nglob), Nglob, posord, poslev);
}
void l_oldsum(const Launch& L, const Dev& D) {
  const size_t tab = (size_t)D.nb * D.K * sizeof(unsigned long long);
  if (D.oldsum_stream && tab <= 64 * 1024) {   // sequential pass over R with LDS accumulators
    const int wgs = tab <= 20 * 1024 ? 2048 : 512;   // 8 workgroups (32 waves) per CU while the LDS tables allow it
    const dim3 sg((unsigned)std::min(wgs, D.nchunks));
    if (D.K % 4 == 0 && D.oldsum_stream == 1) {
      const dim3 g4((unsigned)std::min(tab <= 20 * 1024 ? 512 : 256, D.nchunks));
      hipLaunchKernelGGL(k_oldsum_stream4, g4, dim3(1024), tab, L.stream, D);
      return;
    }
    switch (D.KP / 64) {
      case 1: hipLaunchKernelGGL(k_oldsum_stream<1>, sg, dim3(256), tab, L.stream, D); break;
      case 2: hipLaunchKernelGGL(k_oldsum_stream<2>, sg, dim3(256), tab, L.stream, D); break;
      case 3: hipLaunchKernelGGL(k_oldsum_stream<3>, sg, dim3(256), tab, L.stream, D); break;
      default: hipLaunchKernelGGL(k_oldsum_stream<4>, sg, dim3(256), tab, L.stream, D); break;
    }
    return;
  }
  const dim3 grid(stream_grid(L, (D.n + 63) / 64));
  switch (D.KP / 64) {
    case 1: hipLaunchKernelGGL(k_oldsum<1>, grid, dim3(TPB), 0, L.stream, D); break;
    case 2: hipLaunchKernelGGL(k_oldsum<2>, grid, dim3(TPB), 0, L.stream, D); break;
    case 3: hipLaunchKernelGGL(k_oldsum<3>, grid, dim3(TPB), 0, L.stream, D); break;
    default: hipLaunchKernelGGL(k_oldsum<4>, grid, dim3(TPB), 0, L.stream, D); break;
  }
}
void l_fold(const Launch& L, const Dev& D, int j, int mode) {
  const int n = D.B * D.K;
  hipLaunchKernelGGL(k_fold, dim3((n + 255) / 256), dim3(256), 0, L.stream, D, j, mode);
}
void l_foldpen(const Launch& L, const Dev& D, int j, const long long* Oin, long long* Oout, const long long* Sin,
               long long* Szero) {
  hipLaunchKernelGGL(k_foldpen, dim3((D.K + 15) / 16), dim3(256), (size_t)D.B * 16 * sizeof(long long), L.stream, D, j, Oin,
                     Oout, Sin, Szero);
}
void l_penalty(const Launch& L, const Dev& D) {
  const int n = D.B * D.K;
  hipLaunchKernelGGL(k_penalty, dim3((n + 255) / 256), dim3(256), 0, L.stream, D);
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
void l_round_tail(const Launch& L, const Dev& D, double* host_slot, long long* z0, size_t n0, long long* z1, size_t n1) {
  hipLaunchKernelGGL(k_round_tail, dim3(D.objslots), dim3(1024), 0, L.stream, D, host_slot, z0, n0, z1, n1);
}
void l_obj_reduce(const Launch& L, const Dev& D) {
  hipLaunchKernelGGL(k_obj_reduce, dim3(D.objslots), dim3(1024), 0, L.stream, D);
  hipLaunchKernelGGL(k_obj_final, dim3(1), dim3(1), 0, L.stream, D);
}
#endif  // !HMX_TILE_BF
// launch with the start / stop events of profile mode attached to the dispatch (no barrier packets around the launch), or plainly
#define HMX_LAUNCH_EV(KERNEL, GRID, BLOCK, LDS, ...)                                                                      \
  do {                                                                                                                     \
    if (L.ev0) hipExtLaunchKernelGGL(KERNEL, GRID, BLOCK, (std::uint32_t)(LDS), L.stream, L.ev0, L.ev1, 0, __VA_ARGS__);   \
    else hipLaunchKernelGGL(KERNEL, GRID, BLOCK, LDS, L.stream, __VA_ARGS__);                                              \
  } while (0)
void HMX_LNAME(l_update)(const Launch& L, const Dev& D, int j) {
  const long long tiles = ((long long)D.n / (D.nb > 0 ? D.nb : 1) + 15) / 16 + (long long)D.Q + 1;
  const int wpb = D.upd_threads / 64;
  long long blocks = ((tiles + D.upd_tpw - 1) / D.upd_tpw + wpb - 1) / wpb;
  if (blocks > D.upd_maxblocks) blocks = D.upd_maxblocks;   // resident capacity (workgroups per CU x CUs)
  if (blocks > D.nwmax / wpb) blocks = D.nwmax / wpb;
  if (blocks < 1) blocks = 1;
  const dim3 grid((unsigned)blocks);
  const size_t rest = (D.fused_fold ? (size_t)D.B * D.K * 8 : 0) +
                      ((D.pen_lds || D.fused_fold) ? ((size_t)((D.B * D.K + 3) & ~3) + (size_t)D.Q * D.C) * 4 : 0);
#if !HMX_TILE_BF
  if (bf_fits(D, rest, blocks)) { l_update_bf(L, D, j); return; }
#endif
  const size_t lds = tile_image_bytes(D) + rest;
#define HMX_UPDL(N) case N: HMX_LAUNCH_EV((k_tile<N, 0, 4, true>), grid, dim3(1024), lds, D, j); break;
  if (D.upd_wps == 4) {   // hmx_setup: upd_threads == 1024, uniform sigma, K <= 64
    switch (D.NCT) {
      HMX_UPDL(1) HMX_UPDL(2) HMX_UPDL(3) HMX_UPDL(4)
      default: break;
    }
    return;
  }
#undef HMX_UPDL
#define HMX_UPD(N) case N: if (D.usig) HMX_LAUNCH_EV((k_tile<N, 0, 2, true>), grid, dim3(D.upd_threads), lds, D, j); \
                           else HMX_LAUNCH_EV((k_tile<N, 0>), grid, dim3(D.upd_threads), lds, D, j); break;
  switch (D.NCT) {
    HMX_UPD(1) HMX_UPD(2) HMX_UPD(3) HMX_UPD(4) HMX_UPD(5) HMX_UPD(6) HMX_UPD(7) HMX_UPD(8)
    HMX_UPD(10) HMX_UPD(12) HMX_UPD(13) HMX_UPD(14) HMX_UPD(16)
    default: break;
  }
#undef HMX_UPD
}
void HMX_LNAME(l_chain)(const Launch& L, const Dev& D, int workgroups) {
  const size_t rest = (size_t)D.B * D.K * 8 + ((size_t)((D.B * D.K + 3) & ~3) + (size_t)D.Q * D.C) * 4;
#if !HMX_TILE_BF
  if (D.chain_pair) { l_chain_bf(L, D, workgroups); return; }      // (the wave-pair chain exists in the split-bf16 build only)
  if (bf_image_bytes(D) + rest + 64 <= 150 * 1024 && bf_fits(D, rest, 1)) { l_chain_bf(L, D, workgroups); return; }
#else
  if (D.chain_pair) {
    // MODE 6: workers [ both halves' images | qlev | exchange slots ], folders [ O slice | cluster masses ]
    const int nctp = (D.KH + 15) / 16;
    const size_t lds_w = (size_t)2 * nctp * D.NS2 * 3 * 1024 + (size_t)((D.Q * D.C + 3) & ~3) * 4 + 4 * 2 * 2 * 16 * 8 + (size_t)8 * 4 * 16 * nctp * 4;      // + [8 waves][4 tiles][16 nctp] log2 penalties
    const size_t lds_f = ((size_t)2 * D.B * D.chain_kw + D.chain_kw) * 8;
    const size_t ldsp = std::max(lds_w, lds_f);
    const dim3 gridp((unsigned)workgroups);
    switch (nctp) {      // (cluster tiles of a half: K = 116 .. 128 -> 4, .. 160 -> 5, .. 192 -> 6, .. 224 -> 7)
      case 4: HMX_LAUNCH_EV((k_tile<4, 6, 2, true>), gridp, dim3(512), ldsp, D, 0); break;
      case 5: HMX_LAUNCH_EV((k_tile<5, 6, 2, true>), gridp, dim3(512), ldsp, D, 0); break;
      case 6: HMX_LAUNCH_EV((k_tile<6, 6, 2, true>), gridp, dim3(512), ldsp, D, 0); break;
      default: HMX_LAUNCH_EV((k_tile<7, 6, 2, true>), gridp, dim3(512), ldsp, D, 0); break;
    }
    return;
  }
#endif
  const size_t lds = tile_image_bytes(D) + rest;
  const dim3 grid((unsigned)workgroups);
  // (two waves per SIMD, two accumulator sets; MODE 5 = the variant without R stores, split-bf16 build only)
#if HMX_TILE_BF
#define HMX_CH(N) case N: if (D.usig && !D.r_store) HMX_LAUNCH_EV((k_tile<N, 5, 2, true>), grid, dim3(512), lds, D, 0); \
                          else if (D.usig) HMX_LAUNCH_EV((k_tile<N, 4, 2, true>), grid, dim3(512), lds, D, 0); \
                          else HMX_LAUNCH_EV((k_tile<N, 4>), grid, dim3(512), lds, D, 0); break;
#else
#define HMX_CH(N) case N: if (D.usig) HMX_LAUNCH_EV((k_tile<N, 4, 2, true>), grid, dim3(512), lds, D, 0); \
                          else HMX_LAUNCH_EV((k_tile<N, 4>), grid, dim3(512), lds, D, 0); break;
#endif
  switch (D.NCT) {
    HMX_CH(1) HMX_CH(2) HMX_CH(3) HMX_CH(4) HMX_CH(5) HMX_CH(6) HMX_CH(7)
    default: break;
  }
#undef HMX_CH
}
#if !HMX_TILE_BF
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
void l_p2p_selftest(const Launch& L, const Dev& D, unsigned tag, int* result) {
  hipLaunchKernelGGL(k_p2p_selftest, dim3(1), dim3(512), 0, L.stream, D, tag, result);
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
void l_p2p_allreduce(const Launch& L, const Dev& D, void* buf, int n, int dtype, unsigned seq, int* err) {
  hipLaunchKernelGGL(k_p2p_allreduce, dim3(1), dim3(1024), 0, L.stream, D, (unsigned long long*)buf, n, dtype, seq, err);
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
void l_p2p_allreduce_big(const Launch& L, const Dev& D, void* buf, int n, int dtype, unsigned seq, int* err) {
  int blocks = (n + 4095) / 4096; if (blocks > 128) blocks = 128; if (blocks < 1) blocks = 1;        // (all resident at once: the sweeps wait on peers, never on each other)
  hipLaunchKernelGGL(k_p2p_allreduce_big, dim3(blocks), dim3(1024), 0, L.stream, D, (unsigned long long*)buf, n, dtype, seq, err);
}
void l_objective_tables(const Launch& L, const Dev& D) {
  hipLaunchKernelGGL(k_objective_tables, dim3(1), dim3(TPB), 0, L.stream, D);
}
// false: shape outside this kernel's envelope (the caller falls back to the cluster-lane version)
bool l_obj_terms_mfma(const Launch& L, const Dev& D, const float* M, float* T, long long stride, int all3) {
  const size_t lds = (size_t)D.NQ * D.NS * 64 * sizeof(f32x4);
  if (D.K % 4 != 0 || lds > 64 * 1024 || !D.Yimg || D.obj_stale || D.NT4 > 4) return false;      // (rows of <= 64 + 3 PCs in registers)
  int blocks = ((D.n + 15) / 16 + 3) / 4; if (blocks > 1024) blocks = 1024; if (blocks < 1) blocks = 1;
  // all3 == 2 (round 6): T = dist_mat itself, for the rounds of one cluster_cpp call (the three-array form is a template parameter nobody instantiates any more)
#define HMX_OT(N) case N: if (all3 == 2) hipLaunchKernelGGL((k_obj_terms_mfma<N, false, true>), dim3(blocks), dim3(256), lds, L.stream, D, M, T, stride); \
                          else hipLaunchKernelGGL((k_obj_terms_mfma<N, false>), dim3(blocks), dim3(256), lds, L.stream, D, M, T, stride); break;
  switch (D.NCT) {
    HMX_OT(1) HMX_OT(2) HMX_OT(3) HMX_OT(4) HMX_OT(5) HMX_OT(6) HMX_OT(7) HMX_OT(8) HMX_OT(10) HMX_OT(12) HMX_OT(13) HMX_OT(14) HMX_OT(16)
    default: return false;
  }
#undef HMX_OT
  return true;
}
void l_moe_stats(const Launch& L, const Dev& D) {
  const int zch = (D.d + 31) / 32;
  int dp = (D.d + zch - 1) / zch;
  dp = (dp + 3) / 4 * 4;
  const dim3 grid(stream_grid(L, D.nitems), (D.K + 127) / 128, (D.d + dp - 1) / dp);
  switch (dp) {
    case 4: hipLaunchKernelGGL(k_moe_stats<4>, grid, dim3(TPB), 0, L.stream, D); break;
    case 8: hipLaunchKernelGGL(k_moe_stats<8>, grid, dim3(TPB), 0, L.stream, D); break;
    case 12: hipLaunchKernelGGL(k_moe_stats<12>, grid, dim3(TPB), 0, L.stream, D); break;
    case 16: hipLaunchKernelGGL(k_moe_stats<16>, grid, dim3(TPB), 0, L.stream, D); break;
    case 20: hipLaunchKernelGGL(k_moe_stats<20>, grid, dim3(TPB), 0, L.stream, D); break;
    case 24: hipLaunchKernelGGL(k_moe_stats<24>, grid, dim3(TPB), 0, L.stream, D); break;
    case 28: hipLaunchKernelGGL(k_moe_stats<28>, grid, dim3(TPB), 0, L.stream, D); break;
    default: hipLaunchKernelGGL(k_moe_stats<32>, grid, dim3(TPB), 0, L.stream, D); break;
  }
}
void l_moe_apply(const Launch& L, const Dev& D) {
  const int dpl = D.d > 64 ? 2 : 1;
  const size_t lds = (size_t)D.K * 64 * dpl * sizeof(float);
  int g = D.naitems < 4 * L.grid ? D.naitems : 4 * L.grid;
  if (g < 1) g = 1;
  const dim3 grid(g);
  HMX_DISPATCH_KD(k_moe_apply, grid, lds, D);
}
void l_moe_solve(const Launch& L, const Dev& D, const SolveArgs& A0) {
  SolveArgs A = A0;
  const size_t M = (size_t)D.B + 1;
  const size_t ints = (((size_t)4 * D.B + 6 + D.C) & ~(size_t)1) * sizeof(int);
  const size_t panel = M * 16 * sizeof(double), ball = M * D.d * sizeof(double);
  size_t body = panel;
  if (ints + ball <= 150 * 1024) body = std::max(panel, ball);     // the d right-hand sides live in LDS during the substitution
  if (ints + body > 158 * 1024) body = 0;                           // (B + 1 > ~1200 levels: outside the device-solve envelope, see hmx_setup)
  A.lds_b_bytes = (body >= ball) ? ball : 0;
  A.lds_body_bytes = body;
  // coupling masks of the Schur complement: one bit per (row, eliminated level) -- only while they are small
  const size_t maskb = M * ((M + 63) / 64) * sizeof(unsigned long long);
  const size_t moff = (ints + body + 7) & ~(size_t)7;
  A.lds_mask_off = (D.C > 1 && body > 0 && moff + maskb <= 159 * 1024) ? moff : 0;
  const int threads = M > 48 ? 1024 : 256;
  hipLaunchKernelGGL(k_moe_solve, dim3(D.K), dim3(threads), A.lds_mask_off ? moff + maskb : ints + body, L.stream, D, A);
}
void l_moe_stats_mfma(const Launch& L, const Dev& D) {
  const int npt = (D.d + 15) / 16;
  if (D.st_dma) {   // 16-byte operand loads + deterministic slot reduction (K <= 128)
    const dim3 grid((unsigned)D.st_nwg, (unsigned)D.st_halves), block(64 * ((D.d + 16) / 16));   // PC tiles incl. the ones column at index d; y: the halves of the clusters (K > 128)
    const int nct_q = D.st_halves == 2 ? (D.st_KH + 15) / 16 : D.NCT;
    // (round 6) fp64 shadow sums in LDS + operands one tile ahead where two workgroups still fit a CU next to them (else the round-3 form)
    const size_t shl = (size_t)(block.x / 64) * nct_q * 4 * 64 * sizeof(double);
    const bool use_shl = 2 * shl <= 150 * 1024;
#define HMX_MSQ(N) case N: if (use_shl) hipLaunchKernelGGL((k_moe_stats_q<N, true>), grid, block, shl, L.stream, D, D.st_cpw); \
                           else hipLaunchKernelGGL((k_moe_stats_q<N>), grid, block, 0, L.stream, D, D.st_cpw); break;
    switch (nct_q) { HMX_MSQ(1) HMX_MSQ(2) HMX_MSQ(3) HMX_MSQ(4) HMX_MSQ(5) HMX_MSQ(6) HMX_MSQ(7) HMX_MSQ(8) default: break; }
#undef HMX_MSQ
    const size_t per = (size_t)D.K * D.d + D.K;
    hipLaunchKernelGGL(k_moe_stats_reduce, dim3((unsigned)D.Q, (unsigned)((per + 255) / 256)), dim3(256), 0, L.stream, D);
    return;
  }
  int tpw = (D.ntitems + 2 * 256 - 1) / (2 * 256);   // ~2 workgroups per CU
  if (tpw < 16) tpw = 16;
  const bool split = D.NCT > 8;                       // K > 128: two workgroups (cluster-tile halves) per tile range
  const dim3 grid(((D.ntitems + tpw - 1) / tpw) * (split ? 2 : 1)), block(64 * npt);
#define HMX_MS(N) case N: hipLaunchKernelGGL((k_moe_stats_mfma<N, 1>), grid, block, 0, L.stream, D, tpw, npt); break;
#define HMX_MS2(N) case N: hipLaunchKernelGGL((k_moe_stats_mfma<N, 2>), grid, block, 0, L.stream, D, tpw, npt); break;
  switch (D.NCT) {
    HMX_MS(1) HMX_MS(2) HMX_MS(3) HMX_MS(4) HMX_MS(5) HMX_MS(6) HMX_MS(7) HMX_MS(8)
    HMX_MS2(10) HMX_MS2(12) HMX_MS2(13) HMX_MS2(14) HMX_MS2(16)
    default: break;
  }
#undef HMX_MS
#undef HMX_MS2
}
void l_moe_apply_mfma(const Launch& L, const Dev& D) {
  int g = D.naitems < 4 * L.grid ? D.naitems : 4 * L.grid;
  if (g < 1) g = 1;
  const dim3 grid(g);
  const size_t lds = (size_t)D.wNQ * D.wNS * 64 * sizeof(f32x4);
  switch ((D.d + 15) / 16) {
    case 1: hipLaunchKernelGGL(k_moe_apply_mfma<1>, grid, dim3(256), lds, L.stream, D); break;
    case 2: hipLaunchKernelGGL(k_moe_apply_mfma<2>, grid, dim3(256), lds, L.stream, D); break;
    case 3: hipLaunchKernelGGL(k_moe_apply_mfma<3>, grid, dim3(256), lds, L.stream, D); break;
    default: hipLaunchKernelGGL(k_moe_apply_mfma<4>, grid, dim3(256), lds, L.stream, D); break;
  }
}
void l_seed_race_u(const Launch& L, const Dev& D, const float* u, int a0, int na, int only, uint64_t goff, const unsigned* excl,
                   int nexcl) {
  int blocks = (D.n + 255) / 256; if (blocks > 1024) blocks = 1024; if (blocks < 1) blocks = 1;
  const int lo = excl ? only : 0, hi = excl ? only + 1 : na;
  hipLaunchKernelGGL(k_seed_race_u, dim3(blocks), dim3(256), (size_t)na * D.d * sizeof(float), L.stream, D, u, a0, na, lo, hi, goff,
                     excl, nexcl);
}
void l_gather_rows(const Launch& L, const Dev& D, const long long* gcells, uint64_t goff, double* rows) {
  hipLaunchKernelGGL(k_gather_rows, dim3(D.K), dim3(64), 0, L.stream, D, gcells, goff, rows);
}
void l_lloyd_finish(const Launch& L, const Dev& D) {
  hipLaunchKernelGGL(k_lloyd_finish, dim3(D.K), dim3(64), 0, L.stream, D);
}
void l_lloyd(const Launch& L, const Dev& D) {
  HMX_DISPATCH_KD(k_lloyd, dim3(stream_grid(L, D.nitems)), lds_bytes_y(D), D);
}

#endif  // !HMX_TILE_BF

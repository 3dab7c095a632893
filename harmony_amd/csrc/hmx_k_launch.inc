// hmx_k_launch.inc -- part of hmx_kernels.hip AND of hmx_tile_bf.hip (included inside namespace hmx): the launchers (l_*).  No kernel lives here, and no launch of k_tile
// is decided here: hmx_plan.h plans it (plan_tile_launch), dispatch_k_tile maps the plan to this unit's instantiation.  The split-bf16 unit builds dispatch_k_tile_bf only.
// every launch of this section is tallied for the handle it is made for (Launch::count, hmx_get "diag:launches")
#define HMX_KLAUNCH(...) do { if (L.count) ++*L.count; hipLaunchKernelGGL(__VA_ARGS__); } while (0)
#define HMX_KLAUNCH_EXT(...) do { if (L.count) ++*L.count; hipExtLaunchKernelGGL(__VA_ARGS__); } while (0)
// launch with the start / stop events of profile mode attached to the dispatch (no barrier packets around the launch), or plainly
#define HMX_LAUNCH_EV(KERNEL, GRID, BLOCK, LDS, ...)                                                                      \
  do {                                                                                                                     \
    if (L.ev0) HMX_KLAUNCH_EXT(KERNEL, GRID, BLOCK, (std::uint32_t)(LDS), L.stream, L.ev0, L.ev1, 0, __VA_ARGS__);         \
    else HMX_KLAUNCH(KERNEL, GRID, BLOCK, LDS, L.stream, __VA_ARGS__);                                              \
  } while (0)
// Every k_tile instantiation of this translation unit, once: X(NCT, MODE, WPS, USIG).  Cluster tiles {1..8, 10, 12, 13, 14, 16} (plan_shape's list); the
// lean 4-waves-per-SIMD variants up to 4 tiles (K <= 64), the chains up to 7 (K <= 112).  Split-bf16 build only: Lloyd at three waves per SIMD (768
// threads), the chain without R stores (MODE 5), the wave-pair chain (MODE 6).
#define HMX_NCT_1_4(X, M, W, U) X(1, M, W, U) X(2, M, W, U) X(3, M, W, U) X(4, M, W, U)
#define HMX_NCT_5_7(X, M, W, U) X(5, M, W, U) X(6, M, W, U) X(7, M, W, U)
#define HMX_NCT_1_7(X, M, W, U) HMX_NCT_1_4(X, M, W, U) HMX_NCT_5_7(X, M, W, U)
#define HMX_NCT_ALL(X, M, W, U) HMX_NCT_1_7(X, M, W, U) X(8, M, W, U) X(10, M, W, U) X(12, M, W, U) X(13, M, W, U) X(14, M, W, U) X(16, M, W, U)
#define HMX_TILE_TUPLES_BOTH(X)                                                                                                                              \
  HMX_NCT_ALL(X, 0, 2, false) HMX_NCT_ALL(X, 0, 2, true) HMX_NCT_1_4(X, 0, 4, true) HMX_NCT_ALL(X, 1, 2, false) HMX_NCT_ALL(X, 1, 2, true) HMX_NCT_1_4(X, 1, 4, true) \
  HMX_NCT_ALL(X, 2, 2, false) HMX_NCT_ALL(X, 3, 2, false) HMX_NCT_1_7(X, 4, 2, false) HMX_NCT_1_7(X, 4, 2, true)
#if HMX_TILE_BF
#define HMX_LNAME(x) x##_bf
#define HMX_TILE_TUPLES(X) HMX_TILE_TUPLES_BOTH(X) HMX_NCT_5_7(X, 2, 3, false) HMX_NCT_1_7(X, 5, 2, true) X(4, 6, 2, true) HMX_NCT_5_7(X, 6, 2, true)
#else
#define HMX_LNAME(x) x
#define HMX_TILE_TUPLES(X) HMX_TILE_TUPLES_BOTH(X)
#endif
// the planned launch (hmx_plan.h: plan_tile_launch) on this translation unit's build of k_tile; false: no such instantiation, nothing launched
bool HMX_LNAME(dispatch_k_tile)(const Launch& L, const Dev& D, const TileLaunch& t, int j) {
  const dim3 grid((unsigned)t.blocks), block((unsigned)t.threads);
#define HMX_TILE_CASE(N, M, W, U) case N * 1000 + M * 100 + W * 10 + U: HMX_LAUNCH_EV((k_tile<N, M, W, U>), grid, block, t.lds, D, j); return true;
  switch (t.nct * 1000 + t.mode * 100 + t.wps * 10 + (t.usig ? 1 : 0)) {
    HMX_TILE_TUPLES(HMX_TILE_CASE)
    default: return false;
  }
#undef HMX_TILE_CASE
}

#if !HMX_TILE_BF
#define HMX_DISPATCH_KD(KERNEL, GRID, LDS, ...)                                                \
  do {                                                                                         \
    const int kpl_ = D.KP / 64, dpl_ = D.d > 64 ? 2 : 1;                                       \
    if (dpl_ == 1) {                                                                           \
      switch (kpl_) {                                                                          \
        case 1: HMX_KLAUNCH((KERNEL<1, 1>), GRID, dim3(TPB), LDS, L.stream, __VA_ARGS__); break; \
        case 2: HMX_KLAUNCH((KERNEL<2, 1>), GRID, dim3(TPB), LDS, L.stream, __VA_ARGS__); break; \
        case 3: HMX_KLAUNCH((KERNEL<3, 1>), GRID, dim3(TPB), LDS, L.stream, __VA_ARGS__); break; \
        default: HMX_KLAUNCH((KERNEL<4, 1>), GRID, dim3(TPB), LDS, L.stream, __VA_ARGS__); break; \
      }                                                                                        \
    } else {                                                                                   \
      switch (kpl_) {                                                                          \
        case 1: HMX_KLAUNCH((KERNEL<1, 2>), GRID, dim3(TPB), LDS, L.stream, __VA_ARGS__); break; \
        case 2: HMX_KLAUNCH((KERNEL<2, 2>), GRID, dim3(TPB), LDS, L.stream, __VA_ARGS__); break; \
        case 3: HMX_KLAUNCH((KERNEL<3, 2>), GRID, dim3(TPB), LDS, L.stream, __VA_ARGS__); break; \
        default: HMX_KLAUNCH((KERNEL<4, 2>), GRID, dim3(TPB), LDS, L.stream, __VA_ARGS__); break; \
      }                                                                                        \
    }                                                                                          \
  } while (0)

static size_t lds_bytes_y(const Dev& D) { return (size_t)D.d * D.KP * sizeof(float); }
static int stream_grid(const Launch& L, long long work_waves) {
  long long blocks = (work_waves + 3) / 4;
  if (blocks < 1) blocks = 1;
  if (blocks > L.grid) blocks = L.grid;
  return (int)blocks;
}

void l_convert_in(const Launch& L, const void* src, int f32, float* dst, const int* invperm, int n, int d, int zs) {
  if (f32) HMX_KLAUNCH(k_convert_in<float>, dim3(2048), dim3(256), 0, L.stream, (const float*)src, dst, invperm, n, d, zs);
  else HMX_KLAUNCH(k_convert_in<double>, dim3(2048), dim3(256), 0, L.stream, (const double*)src, dst, invperm, n, d, zs);
}
void l_convert_out(const Launch& L, const float* src, void* dst, int f32, const int* invperm, int n, int w, int ws) {
  if (f32) HMX_KLAUNCH(k_convert_out<float>, dim3(2048), dim3(256), 0, L.stream, src, (float*)dst, invperm, n, w, ws);
  else HMX_KLAUNCH(k_convert_out<double>, dim3(2048), dim3(256), 0, L.stream, src, (double*)dst, invperm, n, w, ws);
}
void l_zero4(const Launch& L, void* a, size_t na, void* b, size_t nb, void* c, size_t nc, void* d, size_t nd) {
  const size_t n = std::max(std::max(na, nb), std::max(nc, nd));
  if (!n) return;
  HMX_KLAUNCH(k_zero4, dim3((unsigned)std::min<size_t>((n + 255) / 256, 1024)), dim3(256), 0, L.stream, (unsigned long long*)a, na, (unsigned long long*)b, nb,
                     (unsigned long long*)c, nc, (unsigned long long*)d, nd);
}
void l_copy(const Launch& L, const float* src, float* dst, size_t count) {
  HMX_KLAUNCH(k_copy, dim3(2048), dim3(256), 0, L.stream, src, dst, count);
}
void l_normalize(const Launch& L, float* Z, int n, int d, int zs) {
  const int nq = zs / 4;
  if (nq <= 16) HMX_KLAUNCH(k_normalize4<1>, dim3(stream_grid(L, (n + 15) / 16)), dim3(TPB), 0, L.stream, Z, Z, n, nq);
  else if (nq <= 32) HMX_KLAUNCH(k_normalize4<2>, dim3(stream_grid(L, (n + 15) / 16)), dim3(TPB), 0, L.stream, Z, Z, n, nq);
  else HMX_KLAUNCH(k_normalize, dim3(stream_grid(L, n)), dim3(TPB), 0, L.stream, Z, n, d, zs);
}
// dst = normalise(src) in one pass (restart: Z_corr = normalise(Z_orig), src/harmony.cpp:42)
void l_normalize_from(const Launch& L, const float* src, float* dst, int n, int d, int zs) {
  const int nq = zs / 4;
  if (nq <= 16) HMX_KLAUNCH(k_normalize4<1>, dim3(stream_grid(L, (n + 15) / 16)), dim3(TPB), 0, L.stream, src, dst, n, nq);
  else if (nq <= 32) HMX_KLAUNCH(k_normalize4<2>, dim3(stream_grid(L, (n + 15) / 16)), dim3(TPB), 0, L.stream, src, dst, n, nq);
  else { l_copy(L, src, dst, (size_t)n * zs); HMX_KLAUNCH(k_normalize, dim3(stream_grid(L, n)), dim3(TPB), 0, L.stream, dst, n, d, zs); }
}
static TileGeom tile_geom(const Dev& D) {
  TileGeom g;
  g.n = D.n; g.nb = D.nb; g.K = D.K; g.d = D.d; g.B = D.B; g.C = D.C; g.Q = D.Q; g.NCT = D.NCT; g.NQ = D.NQ; g.NS = D.NS; g.NS2 = D.NS2; g.KH = D.KH; g.ntitems = D.ntitems; g.nwmax = D.nwmax;
  g.upd_tpw = D.upd_tpw; g.upd_threads = D.upd_threads; g.upd_maxblocks = D.upd_maxblocks; g.upd_wps = D.upd_wps; g.static_maxblocks = D.static_maxblocks; g.usig = D.usig; g.dot_bf = D.dot_bf;
  g.img3 = D.Yimg3 != nullptr; g.fused_fold = D.fused_fold; g.pen_lds = D.pen_lds; g.chain_pair = D.chain_pair; g.chain_kw = D.chain_kw; g.r_store = D.r_store;
  return g;
}
// The three tile launchers: the plan decides (build, instantiation, grid, LDS), the planned build's translation unit dispatches.  Returned: what was
// launched; valid = false: nothing was (LDS over a CU's, no such instantiation) -- the caller reports it.
static TileLaunch launch_k_tile(const Launch& L, const Dev& D, TileKind kind, int workgroups, int j) {
  TileLaunch t = plan_tile_launch(tile_geom(D), kind, workgroups);
  if (t.valid) t.valid = t.bf ? dispatch_k_tile_bf(L, D, t, j) : dispatch_k_tile(L, D, t, j);
  return t;
}
// MFMA tile passes over the static 16-cell tiles: head, Lloyd, seeding race
TileLaunch l_tile_static(const Launch& L, const Dev& D, TileKind kind) { return launch_k_tile(L, D, kind, 0, 0); }
TileLaunch l_update(const Launch& L, const Dev& D, int j) { return launch_k_tile(L, D, TileKind::Update, 0, j); }
TileLaunch l_chain(const Launch& L, const Dev& D, int workgroups) { return launch_k_tile(L, D, TileKind::Chain, workgroups, 0); }
void l_head(const Launch& L, const Dev& D) {
  HMX_DISPATCH_KD(k_head, dim3(stream_grid(L, D.nitems)), lds_bytes_y(D), D);
}
static SortPtrs sort_ptrs_of(const Dev& D) { return SortPtrs{D.blk, D.blkv, D.counts, D.offs, D.binoff, D.bincnt, D.boff, D.lorder, D.lcombo, D.lpair}; }
static BlockIdArgs block_id_args(uint64_t seed, uint64_t round, uint64_t Nglob, uint64_t goff, uint64_t cells_per_block) {
  BlockIdArgs A;
  A.fk = make_keys(seed, round, Nglob); A.fk2 = make_keys(seed, round + 1, Nglob); A.Nglob = Nglob; A.goff = goff; A.cpb = cells_per_block;
  A.inv_cpb = 1.0f / (float)cells_per_block;
  return A;
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
  HMX_KLAUNCH(k_sort_hist<true>, dim3(D.nchunks, nr), dim3(WAVE), lds, L.stream, D, AB, S);
  HMX_KLAUNCH(k_sort_binscan, dim3(nV * D.Q, nr), dim3(WAVE), 0, L.stream, D, S);
  HMX_KLAUNCH(k_sort_binoff, dim3(nr), dim3(1024), 0, L.stream, D, S);
  HMX_KLAUNCH(k_sort_scatter, dim3(D.nchunks, nr), dim3(WAVE), lds, L.stream, D, S);
}
// the padded order of one round whose D.blk the host uploaded (injected shuffle): per-chunk counts, bin offsets from the counts, then the
// placement (padding slots = -1: written by k_sort_scatter, bin by bin)
void l_sort_blocks(const Launch& L, const Dev& D) {
  const int nV = D.nxt ? D.nb * D.nb : D.nb;
  const size_t lds = (size_t)nV * sizeof(int);
  SortBatch S{}; S.p[0] = sort_ptrs_of(D);
  HMX_KLAUNCH(k_sort_hist<false>, dim3(D.nchunks), dim3(WAVE), lds, L.stream, D, BlockIdBatch{}, S);
  HMX_KLAUNCH(k_sort_binscan, dim3(nV * D.Q), dim3(WAVE), 0, L.stream, D, S);
  HMX_KLAUNCH(k_sort_binoff, dim3(1), dim3(1024), 0, L.stream, D, S);
  HMX_KLAUNCH(k_sort_scatter, dim3(D.nchunks), dim3(WAVE), lds, L.stream, D, S);
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
  HMX_KLAUNCH(k_shuf_count, dim3((unsigned)(S.P * D.nb), nr), dim3(SHUF_THREADS), ((size_t)nbin + D.Q + 1 + SHUF_PART) * sizeof(int) + SHUF_PART, L.stream, D, S);
  HMX_KLAUNCH(k_shuf_scan, dim3(nr), dim3(1024), 0, L.stream, D, S);
  HMX_KLAUNCH(k_shuf_place, dim3((unsigned)(S.P * D.nb), nr), dim3(1024), (size_t)nbin * sizeof(int), L.stream, D, S);
}
// D.blk of one round (the sort-free shuffle does not need it; the passes that sum a round's old contributions from R do)
void l_shuffle_blocks(const Launch& L, const Dev& D, uint64_t seed, uint64_t round, uint64_t Nglob, uint64_t goff, uint64_t cells_per_block) {
  HMX_KLAUNCH(k_shuf_blocks, dim3((unsigned)((D.n + 255) / 256)), dim3(256), 0, L.stream, D, block_id_args(seed, round, Nglob, goff, cells_per_block));
}
void l_ref_posord(const Launch& L, const Dev& D, uint64_t seed, uint64_t round, uint64_t Nglob, int* posord, int* poslev) {
  HMX_KLAUNCH(k_ref_posord, dim3(1024), dim3(256), 0, L.stream, D, make_keys(seed, round, Nglob), Nglob, posord, poslev);
}
void l_oldsum(const Launch& L, const Dev& D) {
  const size_t tab = (size_t)D.nb * D.K * sizeof(unsigned long long);
  if (D.oldsum_stream && tab <= 64 * 1024) {   // sequential pass over R with LDS accumulators
    const int wgs = tab <= 20 * 1024 ? 2048 : 512;   // 8 workgroups (32 waves) per CU while the LDS tables allow it
    const dim3 sg((unsigned)std::min(wgs, D.nchunks));
    if (D.K % 4 == 0 && D.oldsum_stream == 1) {
      const dim3 g4((unsigned)std::min(tab <= 20 * 1024 ? 512 : 256, D.nchunks));
      HMX_KLAUNCH(k_oldsum_stream4, g4, dim3(1024), tab, L.stream, D);
      return;
    }
    switch (D.KP / 64) {
      case 1: HMX_KLAUNCH(k_oldsum_stream<1>, sg, dim3(256), tab, L.stream, D); break;
      case 2: HMX_KLAUNCH(k_oldsum_stream<2>, sg, dim3(256), tab, L.stream, D); break;
      case 3: HMX_KLAUNCH(k_oldsum_stream<3>, sg, dim3(256), tab, L.stream, D); break;
      default: HMX_KLAUNCH(k_oldsum_stream<4>, sg, dim3(256), tab, L.stream, D); break;
    }
    return;
  }
  const dim3 grid(stream_grid(L, (D.n + 63) / 64));
  switch (D.KP / 64) {
    case 1: HMX_KLAUNCH(k_oldsum<1>, grid, dim3(TPB), 0, L.stream, D); break;
    case 2: HMX_KLAUNCH(k_oldsum<2>, grid, dim3(TPB), 0, L.stream, D); break;
    case 3: HMX_KLAUNCH(k_oldsum<3>, grid, dim3(TPB), 0, L.stream, D); break;
    default: HMX_KLAUNCH(k_oldsum<4>, grid, dim3(TPB), 0, L.stream, D); break;
  }
}
void l_fold(const Launch& L, const Dev& D, int j, int mode) {
  const int n = D.B * D.K;
  HMX_KLAUNCH(k_fold, dim3((n + 255) / 256), dim3(256), 0, L.stream, D, j, mode);
}
void l_foldpen(const Launch& L, const Dev& D, int j, const long long* Oin, long long* Oout, const long long* Sin,
               long long* Szero) {
  HMX_KLAUNCH(k_foldpen, dim3((D.K + 15) / 16), dim3(256), (size_t)D.B * 16 * sizeof(long long), L.stream, D, j, Oin,
                     Oout, Sin, Szero);
}
void l_penalty(const Launch& L, const Dev& D) {
  const int n = D.B * D.K;
  HMX_KLAUNCH(k_penalty, dim3((n + 255) / 256), dim3(256), 0, L.stream, D);
}
void l_round_tail(const Launch& L, const Dev& D, double* host_slot, long long* z0, size_t n0, long long* z1, size_t n1) {
  HMX_KLAUNCH(k_round_tail, dim3(D.objslots), dim3(1024), 0, L.stream, D, host_slot, z0, n0, z1, n1);
}
void l_obj_reduce(const Launch& L, const Dev& D) {
  HMX_KLAUNCH(k_obj_reduce, dim3(D.objslots), dim3(1024), 0, L.stream, D);
  HMX_KLAUNCH(k_obj_final, dim3(1), dim3(1), 0, L.stream, D);
}
void l_p2p_selftest(const Launch& L, const Dev& D, unsigned tag, int* result) {
  HMX_KLAUNCH(k_p2p_selftest, dim3(1), dim3(512), 0, L.stream, D, tag, result);
}
void l_p2p_allreduce(const Launch& L, const Dev& D, void* buf, int n, int dtype, unsigned seq, int* err) {
  HMX_KLAUNCH(k_p2p_allreduce, dim3(1), dim3(1024), 0, L.stream, D, (unsigned long long*)buf, n, dtype, seq, err);
}
void l_p2p_allreduce_big(const Launch& L, const Dev& D, void* buf, int n, int dtype, unsigned seq, int* err) {
  int blocks = (n + 4095) / 4096; if (blocks > 128) blocks = 128; if (blocks < 1) blocks = 1;        // (all resident at once: the sweeps wait on peers, never on each other)
  HMX_KLAUNCH(k_p2p_allreduce_big, dim3(blocks), dim3(1024), 0, L.stream, D, (unsigned long long*)buf, n, dtype, seq, err);
}
void l_objective_tables(const Launch& L, const Dev& D) {
  HMX_KLAUNCH(k_objective_tables, dim3(1), dim3(TPB), 0, L.stream, D);
}
// false: shape outside this kernel's envelope (the caller falls back to the cluster-lane version)
bool l_obj_terms_mfma(const Launch& L, const Dev& D, const float* M, float* T, long long stride, int all3) {
  const size_t lds = (size_t)D.NQ * D.NS * 64 * sizeof(f32x4);
  if (D.K % 4 != 0 || lds > 64 * 1024 || !D.Yimg || D.obj_stale || D.NT4 > 4) return false;      // (rows of <= 64 + 3 PCs in registers)
  int blocks = ((D.n + 15) / 16 + 3) / 4; if (blocks > 1024) blocks = 1024; if (blocks < 1) blocks = 1;
  // all3 == 2 (round 6): T = dist_mat itself, for the rounds of one cluster_cpp call (the three-array form is a template parameter nobody instantiates any more)
#define HMX_OT(N) case N: if (all3 == 2) HMX_KLAUNCH((k_obj_terms_mfma<N, false, true>), dim3(blocks), dim3(256), lds, L.stream, D, M, T, stride); \
                          else HMX_KLAUNCH((k_obj_terms_mfma<N, false>), dim3(blocks), dim3(256), lds, L.stream, D, M, T, stride); break;
  switch (D.NCT) {
    HMX_OT(1) HMX_OT(2) HMX_OT(3) HMX_OT(4) HMX_OT(5) HMX_OT(6) HMX_OT(7) HMX_OT(8) HMX_OT(10) HMX_OT(12) HMX_OT(13) HMX_OT(14) HMX_OT(16)
    default: return false;
  }
#undef HMX_OT
  return true;
}
// ---- the ridge correction's launches: hmx_plan.h plans them (plan_ridge_launch), the launchers map the plan to an instantiation.  Every instantiation of a family, once:
#define HMX_RIDGE_STATS_TUPLES(X) X(4) X(8) X(12) X(16) X(20) X(24) X(28) X(32)                                                       /* k_moe_stats<DP> */
#define HMX_RIDGE_STATS_Q_TUPLES(X) X(1, false) X(2, false) X(3, false) X(4, false) X(5, false) X(6, false) X(7, false) X(8, false)   /* k_moe_stats_q<NCT, SHL> */ \
                                  X(1, true) X(2, true) X(3, true) X(4, true) X(5, true) X(6, true) X(7, true) X(8, true)
#define HMX_RIDGE_APPLY_TUPLES(X) X(1, 1) X(2, 1) X(3, 1) X(4, 1) X(1, 2) X(2, 2) X(3, 2) X(4, 2)                                       /* k_moe_apply<KPL, DPL> */
#define HMX_RIDGE_APPLY_MFMA_TUPLES(X) X(1) X(2) X(3) X(4)                                                                             /* k_moe_apply_mfma<NPT> */
RidgeGeom ridge_geom(const Dev& D, const Launch& L) {
  RidgeGeom g;
  g.K = D.K; g.KP = D.KP; g.d = D.d; g.B = D.B; g.C = D.C; g.Q = D.Q; g.NCT = D.NCT; g.moe_mfma = D.moe_mfma; g.st_dma = D.st_dma; g.st_halves = D.st_halves; g.st_KH = D.st_KH;
  g.st_nwg = D.st_nwg; g.wNQ = D.wNQ; g.wNS = D.wNS; g.nitems = D.nitems; g.naitems = D.naitems; g.grid = L.grid; g.solve_lds = D.solve_lds;
  return g;
}
// The three launchers: plan, dispatch, return the launch as it ran; valid = false: nothing was launched (LDS over the limit, no such instantiation) -- the caller reports it.
#define HMX_RIDGE_LAUNCH(KERNEL, ...) HMX_KLAUNCH(KERNEL, dim3((unsigned)t.gx, (unsigned)t.gy, (unsigned)t.gz), dim3((unsigned)t.threads), t.lds, L.stream, __VA_ARGS__)
RidgeLaunch l_moe_stats(const Launch& L, const Dev& D) {
  RidgeLaunch t = plan_ridge_launch(ridge_geom(D, L), RidgeKind::Stats);
  if (!t.valid) return t;
#define HMX_MS_CASE(DP) case DP: HMX_RIDGE_LAUNCH(k_moe_stats<DP>, D); return t;
#define HMX_MSQ_CASE(N, SHL) case 2 * N + (SHL ? 1 : 0): HMX_RIDGE_LAUNCH((k_moe_stats_q<N, SHL>), D, D.st_cpw); break;
  if (!t.mfma) switch (t.p0) { HMX_RIDGE_STATS_TUPLES(HMX_MS_CASE) default: t.valid = false; return t; }
  switch (2 * t.p0 + t.p1) { HMX_RIDGE_STATS_Q_TUPLES(HMX_MSQ_CASE) default: t.valid = false; return t; }
#undef HMX_MS_CASE
#undef HMX_MSQ_CASE
  HMX_KLAUNCH(k_moe_stats_reduce, dim3((unsigned)t.rgx, (unsigned)t.rgy), dim3(256), 0, L.stream, D);      // the slots of every combination, in ascending order
  return t;
}
// A: filled by the host, its three lds_* values from this plan (plan_ridge_launch of ridge_geom, RidgeKind::Solve)
RidgeLaunch l_moe_solve(const Launch& L, const Dev& D, const SolveArgs& A) {
  RidgeLaunch t = plan_ridge_launch(ridge_geom(D, L), RidgeKind::Solve);
  if (!t.valid) return t;
  const dim3 grid((unsigned)t.gx), block((unsigned)t.threads);      // (lds_total: the form's LDS + the systems behind it)
  if (t.lds_sys_off) HMX_KLAUNCH(k_moe_solve_lds, grid, block, t.lds_total, L.stream, D, A);
  else HMX_KLAUNCH(k_moe_solve, grid, block, t.lds_total, L.stream, D, A);
  return t;
}
RidgeLaunch l_moe_apply(const Launch& L, const Dev& D) {
  RidgeLaunch t = plan_ridge_launch(ridge_geom(D, L), RidgeKind::Apply);
  if (!t.valid) return t;
#define HMX_MA_CASE(KPL, DPL) case 2 * KPL + DPL: HMX_RIDGE_LAUNCH((k_moe_apply<KPL, DPL>), D); return t;
#define HMX_MAM_CASE(NPT) case NPT: HMX_RIDGE_LAUNCH(k_moe_apply_mfma<NPT>, D); return t;
  if (!t.mfma) switch (2 * t.p0 + t.p1) { HMX_RIDGE_APPLY_TUPLES(HMX_MA_CASE) default: break; }
  else switch (t.p0) { HMX_RIDGE_APPLY_MFMA_TUPLES(HMX_MAM_CASE) default: break; }
#undef HMX_MA_CASE
#undef HMX_MAM_CASE
  t.valid = false;
  return t;
}
void l_seed_race_u(const Launch& L, const Dev& D, const float* u, int a0, int na, int only, uint64_t goff, const unsigned* excl,
                   int nexcl) {
  int blocks = (D.n + 255) / 256; if (blocks > 1024) blocks = 1024; if (blocks < 1) blocks = 1;
  const int lo = excl ? only : 0, hi = excl ? only + 1 : na;
  HMX_KLAUNCH(k_seed_race_u, dim3(blocks), dim3(256), (size_t)na * D.d * sizeof(float), L.stream, D, u, a0, na, lo, hi, goff,
                     excl, nexcl);
}
void l_gather_rows(const Launch& L, const Dev& D, const long long* gcells, uint64_t goff, double* rows) {
  HMX_KLAUNCH(k_gather_rows, dim3(D.K), dim3(64), 0, L.stream, D, gcells, goff, rows);
}
void l_lloyd_finish(const Launch& L, const Dev& D) {
  HMX_KLAUNCH(k_lloyd_finish, dim3(D.K), dim3(64), 0, L.stream, D);
}
void l_lloyd(const Launch& L, const Dev& D) {
  HMX_DISPATCH_KD(k_lloyd, dim3(stream_grid(L, D.nitems)), lds_bytes_y(D), D);
}

#endif  // !HMX_TILE_BF

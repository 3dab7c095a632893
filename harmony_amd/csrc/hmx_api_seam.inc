// hmx_api_seam.inc -- part of hmx_api.cpp (included there, ONE translation unit): typed copies and the device buffers of one call (CallBufs); the handle (hmx_ctx); head pass, objective series and the other helpers the clustering sections share
// ---- copies between host and HBM, typed: the byte count follows from the pointers, whose elements must agree in size and kind; a count of 0
// queues nothing (an empty vector's data() may be null) ----------------------------------------------------------------------------------------
template <class D, class S> constexpr bool same_layout() { return sizeof(D) == sizeof(S) && std::is_floating_point<D>::value == std::is_floating_point<S>::value; }
template <class D, class S> hipError_t upload(D* dev, const S* host, size_t count, hipStream_t st) {
  static_assert(same_layout<D, S>(), "host and device elements differ");
  return count ? hipMemcpyAsync(dev, host, count * sizeof(D), hipMemcpyHostToDevice, st) : hipSuccess;
}
template <class H, class D> hipError_t download(H* host, const D* dev, size_t count, hipStream_t st) {
  static_assert(same_layout<H, D>(), "host and device elements differ");
  return count ? hipMemcpyAsync(host, dev, count * sizeof(D), hipMemcpyDeviceToHost, st) : hipSuccess;
}
template <class T> hipError_t zero_fill(T* dev, size_t count, hipStream_t st) { return count ? hipMemsetAsync(dev, 0, count * sizeof(T), st) : hipSuccess; }

struct CallBufs {        // device buffers of one call: freed when it returns, on every path
  std::vector<void*> v;
  ~CallBufs() { for (void* p : v) (void)hipFree(p); }
  template <class T> hipError_t get(T** p, size_t count) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
    if (e == hipSuccess) v.push_back(q);
    *p = (T*)q;
    return e;
  }
  template <class T, class S> hipError_t put(T** p, const S* host, size_t count, hipStream_t st) {      // get, then upload
    const hipError_t e = get(p, count);
    return e != hipSuccess ? e : upload(*p, host, count, st);
  }
};

}  // namespace

struct hmx_ctx {
  // ---- sharding -------------------------------------------------------------------
  int rank = 0, world = 1;
  int64_t goff = 0, N_global = 0;
  hmx_allreduce_fn ar = nullptr; void* ar_user = nullptr;
  ncclComm_t comm = nullptr;   // built-in all-reduce: RCCL over xGMI (hmx_comm_init)
  int64_t comm_calls = 0, comm_bytes = 0;
  bool comm_force = false;     // test hook: issue the collectives even when world == 1
  // peer-to-peer block chain (hmx_p2p_*): inboxes shared through HIP IPC; on only after the connection self-test passed everywhere
  unsigned long long* p2p_self = nullptr; unsigned long long* p2p_peer[8] = {}; int p2p_rank = 0, p2p_world = 0; bool p2p_on = false;
  unsigned p2p_tests = 0; int* p2p_result = nullptr; double p2p_exchange_us = 0.0; std::string p2p_note = "not connected";
  unsigned p2p_ar_seq = 0, p2p_xseq = 0; int64_t p2p_ar_calls = 0, p2p_ar_big_windows = 0;     // generic inbox all-reduces issued (same on every rank) / chain exchanges issued
  int (*poll)(void*) = nullptr; void* poll_user = nullptr;
  // ---- problem --------------------------------------------------------------------
  int64_t N = 0;  // local cells
  int d = 0, K = 0, B = 0, C = 0, Q = 0;
  std::vector<int> B_vec, cov_bounds;
  std::vector<float> sigma, theta, lambda, Pr_b, sizes;
  bool lambda_estimation = false;
  float alpha = 0.2f, block_size = 0.05f, eps_k = 1e-3f, eps_h = 1e-2f, cutoff = 1e-5f;
  int max_iter_kmeans = 4, window_size = 3, verbose = 0;
  uint64_t seed = 0, round_counter = 0;
  int nb = 20; uint64_t cells_per_block = 1;
  // ---- host-side state --------------------------------------------------------------
  std::vector<float> Y;  // d x K column-major (reference layout)
  std::vector<float> W; int W_rows = 0;
  std::vector<float> obj_kmeans, obj_dist, obj_entropy, obj_cross, obj_harmony;
  std::vector<int> kmeans_rounds;
  std::vector<int> qlev, perm;
  std::vector<long long> seed_cells;
  std::deque<std::vector<int64_t>> injected;
  int64_t subset_clusters = 0, skipped_clusters = 0;
  // objective snapshots are read back asynchronously: one pinned 3-double slot per clustering round, resolved into the
  // four series when a value is needed (convergence checks, getters) -- no host sync per round
  double* h_obj = nullptr; int obj_cap = 0, obj_pending = 0; hipEvent_t obj_event = nullptr; bool obj_harmony_pending = false;
  // obj_unrecorded: a round has written its slot from inside its closing launch and obj_event has not been recorded behind it yet -- recorded once at the
  // end of hmx_cluster, or by flush_objectives when a value is needed earlier (an event record is a barrier packet between two dependent launches)
  bool obj_unrecorded = false;
  long long n_launches = 0, n_event_records = 0, n_gate_records = 0;      // since setup: kernel launches of the launchers (Launch::count) / events the library recorded / those of them that were the chain gate's ("diag:launches", "diag:event_records", "diag:gate_records")
  // randomness: 0 = documented counter-based generator, 1 = R-compatible (MT19937 seeded like set.seed, arma draw order)
  int rng_mode = 0; hmx::RRng rrng; bool rrng_seeded = false;
  // device-side ridge solve (default; HMX_MOE_SOLVE=host selects the synchronous host path): scratch and result buffers
  bool solve_on_device = true, y_on_device = false, solve_pending = false;
  double* sv_cov = nullptr; double* sv_rhs = nullptr; float* sv_Wall = nullptr; int* sv_mrows = nullptr; int* sv_flags = nullptr;
  float* sv_lambda = nullptr; int* sv_cov_bounds = nullptr;
  // Reference arithmetic (DESIGN 2.2): which accumulator groups follow the reference's fp32 operation order instead of the exact /
  // fp64 default -- the same four groups as the oracle's arithmetic mask.  ridge_arith: the ridge statistics (sequential fp32 sums
  // over the cells, src/harmony.cpp:567,599-608); oe_arith: the O / E tables (fp32, block sums in the round's shuffled order,
  // -= / += drift, :149-150,312-313,329-330); obj_arith: my_accu's K*N-term sequential fp32 sums (src/utils.cpp:67-75);
  // solve_arith: the closed-form fp32 arrowhead inverse (:575-586).  "ref_arith" sets all four.
  int ridge_arith = 0, oe_arith = 0, obj_arith = 0, solve_arith = 0;
  // "stale_dist" = 1: a stand-alone compute_objective between a correction and the next cluster_cpp evaluates the k-means term on the
  // distances of the LAST head (the reference's stored dist_mat, src/harmony.cpp:160, which moe_correct_ridge_cpp does not refresh):
  // the correction keeps a snapshot of the normalised Z_corr and of Y it is about to overwrite
  int stale_dist = 0; float* Zc_head = nullptr; float* Yt_head = nullptr; bool head_is_stale = false;
  // restarted sequential sums (hmx_seq.hip): plans (segments + chains on the device), shared workspace, cell lists
  struct SeqPlan { SeqSeg* d_segs = nullptr; SeqChain* d_chains = nullptr; size_t cap_segs = 0, cap_chains = 0; int nsegs = 0, nchains = 0;
                   std::vector<int> seg0;   /* [nchains + 1] first segment of every chain */ int seg_cells = 0; std::vector<int> cells;   /* [nchains] cells of every chain */ };
  SeqPlan plan_head, plan_ridge, plan_round, plan_pair;
  // ridge_arith with several covariates: Phi_Rk * Phi_moe_t has one entry per PAIR of levels that meet in a cell (src/harmony.cpp:561-568):
  // a sequential sum of R_k over the cells that carry both levels, in original order.  pairlist = those cells pair by pair, pair_idx[b][b2]
  // (b < b2) = the pair's chain or -1; rg_tot / rp_tot = the chain totals the device solve assembles its systems from.
  int* pairlist = nullptr; int* pair_idx = nullptr; int npairs = 0;
  float* rg_tot = nullptr; float* rp_tot = nullptr; float* rp_start = nullptr; bool rp_warm = false;
  float* sq_start = nullptr; float* sq_end = nullptr; size_t sq_cap = 0;
  float* sq_total = nullptr; size_t sq_total_cap = 0;
  unsigned* sq_mismatch = nullptr; int seq_passes = 2, seq_warm_passes = 2; int64_t seq_runs = 0;      // (round 5: 2 passes cold AND warm, see seq_tol / seq_iterate)
  bool seq_scan_final = false;      // set by seq_iterate around the scan behind the last pass of a non-adaptive sum (the O / E scans then only reduce)
  bool seq_stats = false;     // the last scan of NON-adaptive groups also counts the starts that still moved ("seq:mismatch" / "seq:residual" then cover every group)
  // long chains (>= seq_adaptive_cells cells) are iterated until the starts stop moving (chain-relative residual <= 2^-22) or seq_max_passes
  unsigned* sq_conv = nullptr; int seq_max_passes = 24; int64_t seq_adaptive_cells = 200000, seq_extra_passes = 0; double seq_resid_max = 0.0; uint64_t seq_mismatch_sum = 0;
  // seq_strict: EVERY group of restarted sums (short chains too) is iterated until no segment start moves any more -- the fixed point, at which
  // the concatenated segment loops are the reference's one-after-the-other loop bit for bit (tests/test_gpu_seq.py) -- instead of stopping at the
  // default pass count / the 2^-22 residual.  seq_group_passes / seq_group_runs: passes and runs per group (0 O/E, 1 objective, 2 ridge, 3 level pairs)
  // seq_tol: adaptive groups (long chains) stop when the largest move of a start in the last scan, relative to the largest start of its lane
  // group, is below it.  What is left after such a pass is the move times the iteration's contraction factor (the relative size of the
  // rounding bias itself, 1e-2 .. 1e-4; 0.25 where the accumulators saturate at 10M cells), i.e. far below the move.
  // Round 5 (tools/strict_probe.py at BASELINE configs[2], profiles/r5_strict_probe_1M_*.json): 2 passes + tol 1e-5, the round-3 default (3 passes +
  // tol 2^-22), 6 passes and the bit-for-bit fixed point (seq_strict, 1.2 s per run) all end 1.9-2.1e-6 from the oracle's faithful run and
  // 1.6-2.0e-6 from EACH OTHER -- the faithful trajectory itself moves by that much under any ulp-level change (the oracle's own liberties:
  // profiles/r5_oracle_liberties.json) -- so the cheap setting is the default; seq_passes / seq_tol_ppb / seq_strict select the others.
  double seq_tol = 1e-5;
  bool seq_strict = false; uint64_t seq_last_mismatch = 0, seq_unsettled = 0; double seq_oe_cell_passes = 0.0;      // (cells x passes the O / E sums have walked: the bench's roofline of that phase)
  int64_t seq_group_passes[4] = {0, 0, 0, 0}, seq_group_runs[4] = {0, 0, 0, 0};
  int* headlist = nullptr;                 // [(1 + C) n] cells in original order | cells by (level of covariate c, original order)
  int* headq = nullptr;                    // the same entries' combinations (ridge_arith: static, saves a dependent load per batch of the ridge pass)
  std::vector<int> lev_off, lev_cnt;       // [B] a level's range inside its covariate's part of headlist
  int* headlev = nullptr; int* roundlev = nullptr;     // [min(C, 4)][n] level codes of the positions of headlist's first part / of roundlist
  int* roundlist = nullptr;                // [(1 + C) n] this round's cells in shuffled order | by (block, level of covariate c), shuffled order
  std::vector<int> invperm_h, combo_h;     // host copies (internal order)
  float* Of = nullptr; float* Ef = nullptr; float* Mtab = nullptr;    // [B][K] fp32 O / E (oe_arith), theta log((O+E+1)/(2E+1))
  float* objT = nullptr; size_t objT_cap = 0;                         // the objective's three K x N term matrices (obj_arith)
  // round 6: dist_mat of the cluster_cpp call in progress, K x N in the term arrays' order -- Y and Z_corr do not change between the rounds of a call, so the
  // distances of its first objective evaluation serve the others (the first chain's terms R % dist are formed inside the fused launch); valid only while
  // hmx_cluster's round loop runs (in_cluster_rounds), never for a stand-alone compute_objective or the stale-distance snapshot
  float* objD = nullptr; size_t objD_cap = 0; bool objD_valid = false, in_cluster_rounds = false;
  // one evaluation of the objective's one-launch sums (objf_begin / objf_settle): where it runs and on which data
  struct ObjfRun { Launch L; Dev D; int mat = 0; long long nt = 0; const float* T = nullptr; float* tot = nullptr; double* objv = nullptr; int np = 0, done = 0; bool adaptive = false; };
  unsigned char* inset = nullptr;                                      // [Q][K] cells of combination q enter cluster k's regression
  // the objective's and the ridge statistics' segment starts live in their own buffers and survive from one evaluation to the next
  // (same chains, slowly changing terms): every evaluation after the first starts warm and needs one pass less
  float* obj_start = nullptr; size_t obj_start_cap = 0; bool obj_warm = false;
  double* obj_partial = nullptr; size_t obj_partial_cap = 0;      // per array and 256-segment workgroup of k_seq_arr_pass: the sum of its deltas (k_seq_scan1's bases)
  // round 6: the objective's chains in one launch (k_seq_obj_fused): granule slots of the in-launch exchange (zeroed once), statistics words, launch epoch
  unsigned long long* objf_slots = nullptr; size_t objf_slots_cap = 0; unsigned* objf_stats = nullptr; unsigned objf_epoch = 0; int obj_fused = 1; int obj_dist_cache = 1; int objf_segs = 0; bool objf_continued = false;
  float* rg_start = nullptr; size_t rg_start_cap = 0; bool rg_warm = false;
  int ridge_kl = 1, rg_start_kl = -1; float* rg_totkl = nullptr; size_t rg_totkl_cap = 0;      // round 6: the ridge pass with lane = cluster (k_seq_ridge_pass_kl) and its chain totals [chain][d + 1][K]
  std::map<std::string, double> timers;
  // ---- device -------------------------------------------------------------------------
  int device = -1;
  Dev D{}; Launch L{};
  bool own_stream = false, ran_setup = false, ran_init = false;
  std::vector<void*> allocs;
  // profiling of the dominant kernel
  int profile = 0;             // 0 off | 1 the dominant kernel's launches carry a start / stop event pair | 2 and every phase is bracketed by events (PhaseScope)
  bool fused_ok = false;       // k_tile prologue fold usable (LDS budget) and not disabled
  // Old-contribution tables: two buffers.  ledger.cur is what this round's block steps subtract; the other one collects, inside this
  // round's tile kernels, the old contributions of the NEXT round's blocks (carry_ok: the shuffle keys every tile by its cells'
  // next block) -- then the next round needs no pass over R (k_oldsum).  What the tables, the order sets and the replica sets hold: the ledger (hmx_round.h).
  long long* sold_buf[2] = {nullptr, nullptr}; RoundLedger ledger;
  bool carry_ok = false, last_round_hint = false, round_may_be_last = true;
  int fold_impl = 0;           // Switches::fold_impl, read at setup
  RoundPlan last_round; bool round_seen = false;      // the plan of the last round of update_R (hmx_get "round:last")
  // R rows that nobody reads are not stored (Dev::r_store = 0: the head inside cluster_cpp, rounds that cannot be a call's last).  R_valid says
  // whether D.R holds the rows of the LAST head / round: cleared when a pass starts, set when a storing pass has been queued completely.  A call
  // that fails half way leaves it false, and the getters / the correction refuse to consume stale rows.  r_store_always: HMX_R_STORE=1, read at setup.
  bool R_valid = false, r_store_always = false;
  int64_t rounds_without_R = 0;
  TileLaunch last_tile[5]; bool tile_seen[5] = {};      // the last k_tile launch of every TileKind, as it ran (hmx_get "launch:<kind>")
  RidgeLaunch last_ridge[3]; bool ridge_seen[3] = {};   // the last launch of every RidgeKind, as it ran (hmx_get "launch:stats" | "launch:solve" | "launch:apply")
  int64_t carried_rounds = 0;
  bool chain_ok = false; int chain_wgs = 0; uint64_t chain_rounds = 0;   // persistent block chain (one launch per round)
  int tun_tpw = -1, tun_wps = -1;  // tunables set through hmx_set_int before setup
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool; size_t ev_used = 0;
  // GPU phase timers (profile mode): event pairs tagged with a phase name, named after the reference's Timer phases
  // (src/harmony.cpp:302-335,557-615) where a phase has a counterpart; resolved lazily into gpu_timers
  struct PhaseEv { hipEvent_t a, b; int name; };
  std::vector<PhaseEv> ph_pool; size_t ph_used = 0; std::vector<std::string> ph_names; std::map<std::string, double> gpu_timers;
  double prof_update_ms = 0; int64_t prof_update_launches = 0, prof_update_cells = 0, prof_update_steps = 0;
  bool chain_check = false;    // a persistent-chain launch has run since the error word was last read
  // The round's shuffle (counting sort by block) touches no algorithmic state, and with the counter-based generator it depends
  // on (seed, round) only: the shuffles of FOUR consecutive rounds run in one set of launches on the main stream (l_sort_batch / l_shuffle_inv),
  // into four full order sets (round & 3) -- rounds keep their numbers across cluster_cpp calls, so a batch serves whichever calls its rounds
  // fall into; between two block chains of a batch there is no sort kernel and no event at all.  The batches are aligned groups (round >> 2).
  // A host-provided order is sorted on its own into its round's set.  (Sorting ahead on a side stream was measured and lost twice: DESIGN 4.5.)
  struct SortSet { int* blk; int* lorder; int2* lpair; int* lcombo; int* boff; int* binoff; int* counts; int* offs; int* blkv; int* bincnt; };
  SortSet sets[4] = {};
  // the sort-free form of the batched shuffle (k_shuf_*): position -> (cell, rank) per order set, the blocks of the round behind a batch,
  // the (block, bin, part) count matrix
  bool shuf_inv = false; int2* posr[4] = {}; int* shuf_partcnt[4] = {}; int* shuf_binacc[4] = {}; int64_t injected_round = -1;   // (injected_round: the round whose order the host provided -- its D.blk came with it)
  // ---- query mapping (hmx_map_query): a handle that mapped a query serves Z_corr / Z_orig / R and nothing else
  bool query_done = false;
  // ---- count projection (hmx_project_counts): the lab field "project_slab_bytes" (0: the default cap) and the slabs the last host-resident call ran
  int64_t project_slab_bytes = 0, project_slabs = 0;
  // ---- the host matrix seam (hmx_api_xfer.inc): the lab field "xfer_slab_bytes", a cap on the bytes of a staging slab (0: the path's default)
  int64_t xfer_slab_bytes = 0;
  // ---- rank sums (hmx_rank_sums): the lab field "ranksum_list_bytes" (0: the default budget of a gene block) and the gene blocks the last call ran
  int64_t ranksum_list_bytes = 0, ranksum_blocks = 0;
  // ---- connected components (hmx_graph_components): the hook-and-jump rounds of the last call ("graph:cc_rounds")
  int64_t graph_cc_rounds = 0;
  // ---- the SNN graph (hmx_snn_from_knn / hmx_snn_graph): the pruning threshold and the long rows of the last call ("snn:s_min", "snn:long_rows")
  int64_t snn_s_min = 0, snn_long_rows = 0;
  // ---- Louvain clustering (hmx_louvain): the counters of the last call ("louvain:levels" ...) and the lab field "louvain_short_cap", a cap
  // below the short path's own on the entries of a row it takes (-1: the default)
  int64_t louvain_levels = 0, louvain_best_level = 0, louvain_sweeps = 0, louvain_clusters = 0, louvain_long_rows = 0, louvain_short_cap = -1;
  // ---- Leiden clustering (hmx_leiden): the counters of the last call ("leiden:levels" ...); the short path's cap is Louvain's lab field
  int64_t leiden_levels = 0, leiden_sweeps = 0, leiden_refine_sweeps = 0, leiden_clusters = 0, leiden_converged = 0, leiden_long_rows = 0;
  // ---- the UMAP layout (hmx_umap_layout): the counters of the last call ("umap:fired" ...) and the lab field "umap_short_cap", the entries of
  // a row the one-wave path takes in place of its own cap (-1: the default)
  int64_t umap_fired = 0, umap_epochs = 0, umap_long_rows = 0, umap_short_cap = -1;
  // ---- query cells in a fitted layout (hmx_umap_transform): the counters of the last call ("umap_transform:fired", "umap_transform:epochs")
  int64_t umap_transform_fired = 0, umap_transform_epochs = 0;
  // ---- the reference's PCA (hmx_pca_prepare / apply / release, hmx_api_pca.inc): the prepared lists (a PcaState) and their entry count
  std::shared_ptr<void> pca; int64_t pca_entries = 0;
  QueryDev qd{};            // the query's device tables (rows in D.Zo / D.Zc, internal order in D.perm / D.invperm)
  std::string err, warn, warn_ret;
};

namespace {

int fail(hmx_ctx* c, int code, const std::string& msg) { c->err = msg; return code; }

#define HIPCHK(expr)                                                                            \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return fail(ctx, HMX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));      \
  } while (0)

template <class T> int dalloc(hmx_ctx* ctx, T** p, size_t count) {
  void* q = nullptr;
  if (count == 0) count = 1;
  HIPCHK(hipMalloc(&q, count * sizeof(T)));
  ctx->allocs.push_back(q);
  *p = (T*)q;
  return 0;
}
void free_all(hmx_ctx* ctx) {
  for (void* p : ctx->allocs) (void)hipFree(p);
  ctx->allocs.clear();
  for (auto& e : ctx->ev_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  ctx->ev_pool.clear(); ctx->ev_used = 0;
  for (auto& e : ctx->ph_pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  ctx->ph_pool.clear(); ctx->ph_used = 0;
  ctx->ledger.reset();
  {   // reference-arithmetic buffers (grown on demand, not in `allocs`)
    void* ps[] = {ctx->sq_start, ctx->sq_end, ctx->sq_total, ctx->sq_mismatch, ctx->headlist, ctx->roundlist, ctx->Of, ctx->Ef, ctx->Mtab, ctx->objT, ctx->objD,
                  ctx->inset, ctx->headq, ctx->obj_start, ctx->obj_partial, ctx->objf_slots, ctx->objf_stats, ctx->rg_totkl, ctx->rg_start, ctx->headlev, ctx->roundlev, ctx->pairlist, ctx->pair_idx, ctx->rg_tot, ctx->rp_tot, ctx->rp_start, ctx->plan_pair.d_segs, ctx->plan_pair.d_chains, ctx->plan_head.d_segs, ctx->plan_head.d_chains, ctx->plan_ridge.d_segs, ctx->plan_ridge.d_chains,
                  ctx->plan_round.d_segs, ctx->plan_round.d_chains};
    for (void* q : ps) if (q) (void)hipFree(q);
    ctx->sq_start = ctx->sq_end = ctx->sq_total = nullptr; ctx->sq_mismatch = nullptr; ctx->sq_conv = nullptr; ctx->headlist = ctx->roundlist = nullptr; ctx->headq = nullptr;
    ctx->Of = ctx->Ef = ctx->Mtab = ctx->objT = nullptr; ctx->inset = nullptr; ctx->sq_cap = ctx->sq_total_cap = ctx->objT_cap = 0;
    ctx->objD = nullptr; ctx->objD_cap = 0; ctx->objD_valid = false; ctx->in_cluster_rounds = false;
    ctx->obj_start = ctx->rg_start = nullptr; ctx->obj_start_cap = ctx->rg_start_cap = 0; ctx->obj_warm = ctx->rg_warm = false;
    ctx->obj_partial = nullptr; ctx->obj_partial_cap = 0; ctx->objf_slots = nullptr; ctx->objf_slots_cap = 0; ctx->objf_stats = nullptr; ctx->objf_segs = 0; ctx->rg_totkl = nullptr; ctx->rg_totkl_cap = 0; ctx->rg_start_kl = -1;
    ctx->plan_head = hmx_ctx::SeqPlan(); ctx->plan_ridge = hmx_ctx::SeqPlan(); ctx->plan_round = hmx_ctx::SeqPlan(); ctx->plan_pair = hmx_ctx::SeqPlan();
    ctx->headlev = ctx->roundlev = nullptr; ctx->pairlist = ctx->pair_idx = nullptr; ctx->rg_tot = ctx->rp_tot = ctx->rp_start = nullptr; ctx->npairs = 0; ctx->rp_warm = false;
  }
  if (ctx->h_obj) { (void)hipHostFree(ctx->h_obj); ctx->h_obj = nullptr; ctx->obj_cap = 0; }
  if (ctx->obj_event) { (void)hipEventDestroy(ctx->obj_event); ctx->obj_event = nullptr; }
  ctx->obj_pending = 0; ctx->obj_harmony_pending = false; ctx->obj_unrecorded = false;
}
template <class T> int h2d(hmx_ctx* ctx, T* dst, const T* src, size_t count) {
  if (count) HIPCHK(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, ctx->L.stream));
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  return 0;
}
template <class T> int d2h(hmx_ctx* ctx, T* dst, const T* src, size_t count) {
  if (count) HIPCHK(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, ctx->L.stream));
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  return 0;
}
int allreduce(hmx_ctx* ctx, void* buf, int64_t count, int dtype) {
  if (ctx->world <= 1 && !ctx->comm_force) return 0;
  // small buffers go through the peers' inboxes when they are connected and tested (k_p2p_allreduce: one launch, one trip over xGMI, no ring):
  // everything but the big ridge statistics of many-level designs.  HMX_P2P_AR=0: always the communicator / hook.
  if (ctx->p2p_on && ctx->p2p_world == ctx->world && !ctx->comm_force && ctx->ran_setup && ctx->D.chain_ctl) {
    static const bool off = [] { const char* e = getenv("HMX_P2P_AR"); return e && atoi(e) == 0; }();
    static const bool big_off = [] { const char* e = getenv("HMX_P2P_AR_BIG"); return e && atoi(e) == 0; }();      // (0: buffers above P2P_CAP entries go to the communicator / hook as in round 4)
    if (!off && (count <= (int64_t)P2P_CAP || !big_off)) {
      Dev T = ctx->D; T.p2p_world = ctx->p2p_world; T.p2p_rank = ctx->p2p_rank;
      for (int g = 0; g < 8; g++) T.p2p_inbox[g] = ctx->p2p_peer[g];
      if (count <= (int64_t)P2P_CAP) {
        l_p2p_allreduce(ctx->L, T, buf, (int)count, dtype, ctx->p2p_ar_seq++, ctx->D.chain_ctl + 1);
        ctx->p2p_ar_calls++;
      } else {
        // big buffers (ridge statistics of many-level designs): reduce-scatter + all-gather through the inboxes, a window at a time
        const int64_t win = (int64_t)(P2P_CAP / 2) * ctx->p2p_world;
        for (int64_t off0 = 0; off0 < count; off0 += win) {
          l_p2p_allreduce_big(ctx->L, T, (char*)buf + 8 * off0, (int)std::min(win, count - off0), dtype, ctx->p2p_ar_seq++, ctx->D.chain_ctl + 1);
          ctx->p2p_ar_calls++; ctx->p2p_ar_big_windows++;
        }
      }
      if (hipGetLastError() != hipSuccess) return fail(ctx, HMX_ERR_COMM, "inbox all-reduce launch failed");
      return 0;
    }
  }
  ctx->comm_calls++; ctx->comm_bytes += count * 8;
  if (ctx->ar) {
    int st = ctx->ar(ctx->ar_user, buf, count, dtype, (void*)ctx->L.stream);
    if (st) return fail(ctx, HMX_ERR_COMM, "all-reduce callback failed");
    return 0;
  }
  // (a handle that has inboxes but neither a communicator nor a hook -- hmx_p2p_connect by hand -- gets here with what the inboxes do not take:
  //  the collectives of hmx_setup, buffers above P2P_CAP entries, everything under HMX_P2P_AR=0.  That is an error, not an RCCL call on a null communicator.)
  if (!ctx->comm) return fail(ctx, HMX_ERR_COMM, ctx->p2p_on ? "this collective does not go through the peer inboxes (before setup / HMX_P2P_AR=0): the handle also needs hmx_comm_init or an all-reduce hook"
                                                            : "sharded handle without hmx_comm_init or an all-reduce hook");
  RcclApi* api = rccl_api(nullptr);
  if (!api || !api->AllReduce) return fail(ctx, HMX_ERR_COMM, "librccl is not loadable");
  ncclResult_t r = api->AllReduce(buf, buf, (size_t)count, dtype == 1 ? ncclFloat64 : ncclInt64,
                                  dtype == 2 ? ncclMin : ncclSum, ctx->comm, ctx->L.stream);
  if (r != ncclSuccess) return fail(ctx, HMX_ERR_COMM, std::string("ncclAllReduce: ") + (api->GetErrorString ? api->GetErrorString(r) : "error"));
  return 0;
}
#define CHK(expr) do { int s_ = (expr); if (s_) return s_; } while (0)
#define KCHK() HIPCHK(hipGetLastError())
// a k_tile launch as its launcher returned it: kept for hmx_get("launch:<kind>"); one that could not be made is a limit of the shape
int tile_ran(hmx_ctx* ctx, TileKind kind, const TileLaunch& t) {
  ctx->last_tile[(int)kind] = t; ctx->tile_seen[(int)kind] = true;
  return t.valid ? 0 : fail(ctx, HMX_ERR_LIMIT, std::string("no k_tile launch for kind ") + TILE_KIND_NAME[(int)kind] + ": NCT " + std::to_string(t.nct) + ", mode " + std::to_string(t.mode) +
                                                    ", " + std::to_string(t.lds) + " bytes of LDS (" + (t.lds > LDS_PER_CU ? "over a compute unit's" : "no such instantiation") + ")");
}

// profile mode only: bracket a group of launches with an event pair tagged `name`
struct PhaseScope {
  hmx_ctx* c; int idx = -1;
  PhaseScope(hmx_ctx* ctx, const char* name) : c(ctx) {
    if (c->profile < 2) return;      // (an event record is a barrier packet of its own: ~2-5 us each between dependent kernels -- 200 of them per run were 0.4-1 ms of a 15 ms run)
    int id = -1;
    for (size_t i = 0; i < c->ph_names.size(); i++) if (c->ph_names[i] == name) { id = (int)i; break; }
    if (id < 0) { id = (int)c->ph_names.size(); c->ph_names.push_back(name); }
    if (c->ph_used == c->ph_pool.size()) {
      hmx_ctx::PhaseEv e; e.name = id;
      if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
      c->ph_pool.push_back(e);
    }
    idx = (int)c->ph_used++;
    c->ph_pool[idx].name = id;
    (void)hipEventRecord(c->ph_pool[idx].a, c->L.stream); c->n_event_records++;
  }
  ~PhaseScope() { if (idx >= 0) { (void)hipEventRecord(c->ph_pool[idx].b, c->L.stream); c->n_event_records++; } }
};
// profile mode: the dominant kernel's launches carry their own start / stop events (hipExtLaunchKernelGGL: the timestamps of the dispatch
// packet itself, no barrier packets around it)
int launch_with_events(hmx_ctx* ctx, Launch& L) {
  L = ctx->L;
  if (!ctx->profile) return 0;
  if (ctx->ev_used == ctx->ev_pool.size()) { hipEvent_t a, b; HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b)); ctx->ev_pool.emplace_back(a, b); }
  L.ev0 = ctx->ev_pool[ctx->ev_used].first; L.ev1 = ctx->ev_pool[ctx->ev_used].second;
  ctx->ev_used++;
  return 0;
}
void resolve_phases(hmx_ctx* c) {
  if (!c->ph_used) return;
  (void)hipStreamSynchronize(c->L.stream);
  for (size_t i = 0; i < c->ph_used; i++) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ph_pool[i].a, c->ph_pool[i].b) == hipSuccess) c->gpu_timers[c->ph_names[c->ph_pool[i].name]] += ms;
  }
  c->ph_used = 0;
}

void normalise_cols(std::vector<float>& Y, int d, int K) {  // arma::normalise(Y, 2, 0)
  for (int k = 0; k < K; k++) {
    float s = 0.f;
    for (int j = 0; j < d; j++) s += Y[(size_t)k * d + j] * Y[(size_t)k * d + j];
    float nrm = std::sqrt(s); if (nrm == 0.f) nrm = 1.f;
    for (int j = 0; j < d; j++) Y[(size_t)k * d + j] /= nrm;
  }
}
int upload_Y(hmx_ctx* ctx) {  // host Y[k*d+j] -> device Ycur, from it (k_y_images) Yt[j*K+k], the MFMA B-operand images and ||y||^2
  CHK(h2d(ctx, ctx->D.Ycur, ctx->Y.data(), ctx->Y.size()));
  l_y_images(ctx->L, ctx->D, nullptr, 0); KCHK();
  return 0;
}

// objective snapshot obj[2..4] -> the four series (src/harmony.cpp:165-168).  The copy is enqueued into a pinned slot;
// flush_objectives() waits for the last copy only (an event, not the stream: later kernels keep running) and appends.
int record_objectives(hmx_ctx* ctx) {      // obj_event behind every slot written so far
  if (!ctx->obj_unrecorded) return 0;
  HIPCHK(hipEventRecord(ctx->obj_event, ctx->L.stream)); ctx->n_event_records++;
  ctx->obj_unrecorded = false;
  return 0;
}
int flush_objectives(hmx_ctx* ctx) {
  if (!ctx->obj_pending) return 0;
  CHK(record_objectives(ctx));
  HIPCHK(hipEventSynchronize(ctx->obj_event));
  const float norm_const = 2000 / ((float)ctx->N_global);
  for (int i = 0; i < ctx->obj_pending; i++) {
    const double* o = ctx->h_obj + 4 * i;
    const int chain_err = (int)o[3] & 15, solve_err = (int)o[3] >> 4;
    if (solve_err) { ctx->obj_pending = 0; return fail(ctx, HMX_ERR_SOLVE, "singular ridge system (moe_correct_ridge_cpp; reported with the objective of the clustering round that followed it)"); }
    if (chain_err) { ctx->obj_pending = 0; return fail(ctx, HMX_ERR_DEVICE, "persistent block chain: a workgroup timed out waiting for its peers (code " + std::to_string(chain_err) + ")"); }
    if (ctx->obj_arith) {   // the three sums are the reference's fp32 accumulators: combined in fp32 as well (:165-168)
      const float a = (float)o[0], b = (float)o[1], c = (float)o[2];
      ctx->obj_kmeans.push_back(((a + b) + c) * norm_const);
      ctx->obj_dist.push_back(a * norm_const); ctx->obj_entropy.push_back(b * norm_const); ctx->obj_cross.push_back(c * norm_const);
      continue;
    }
    ctx->obj_kmeans.push_back((float)((o[0] + o[1] + o[2]) * norm_const));
    ctx->obj_dist.push_back((float)(o[0] * norm_const));
    ctx->obj_entropy.push_back((float)(o[1] * norm_const));
    ctx->obj_cross.push_back((float)(o[2] * norm_const));
  }
  ctx->obj_pending = 0;
  if (ctx->obj_harmony_pending) { ctx->obj_harmony.push_back(ctx->obj_kmeans.back()); ctx->obj_harmony_pending = false; }
  return 0;
}
int objective_slot(hmx_ctx* ctx, double** slot) {     // next pinned host slot of the objective series (4 doubles)
  if (!ctx->h_obj) {
    ctx->obj_cap = 64;
    HIPCHK(hipHostMalloc((void**)&ctx->h_obj, sizeof(double) * 4 * ctx->obj_cap, hipHostMallocDefault));
    std::memset(ctx->h_obj, 0, sizeof(double) * 4 * ctx->obj_cap);
    HIPCHK(hipEventCreateWithFlags(&ctx->obj_event, hipEventDisableTiming));
  }
  if (ctx->obj_pending == ctx->obj_cap) CHK(flush_objectives(ctx));
  *slot = ctx->h_obj + 4 * ctx->obj_pending;
  return 0;
}
int push_objective(hmx_ctx* ctx) {
  double* slot = nullptr;
  CHK(objective_slot(ctx, &slot));
  HIPCHK(hipMemcpyAsync(slot, ctx->D.obj + 2, sizeof(double) * 4, hipMemcpyDeviceToHost, ctx->L.stream));   // dist, entropy, cross, chain error word
  HIPCHK(hipEventRecord(ctx->obj_event, ctx->L.stream)); ctx->n_event_records++;
  ctx->obj_unrecorded = false;      // (the stream orders the earlier slots in front of this one)
  ctx->obj_pending++;
  return 0;
}

// R, O, E from scratch (src/harmony.cpp:141-150, :221-227); leaves objective partials in obj[0..1]
int prepare_round(hmx_ctx* ctx, uint64_t round);
int oe_head(hmx_ctx* ctx);
int objective_snapshot(hmx_ctx* ctx, const Dev* Dterms = nullptr);
int head_pass(hmx_ctx* ctx, bool normalise = false) {   // normalise: Z_corr <- normalise(Z_corr) first (:220)
  HeadIn in;      // the decisions: plan_head (hmx_round.h)
  in.carry_ok = ctx->carry_ok; in.host_order = !ctx->injected.empty() || ctx->rng_mode != 0; in.normalise = normalise;
  in.NT4 = ctx->D.NT4; in.NCT = ctx->D.NCT; in.upd_wps = ctx->D.upd_wps; in.max_iter_kmeans = ctx->max_iter_kmeans;
  in.poll = ctx->poll != nullptr; in.r_store_always = ctx->r_store_always; in.seed = ctx->seed; in.round = (int64_t)ctx->round_counter;
  in.sharded = ctx->world > 1 || ctx->comm_force; in.ref_arith = ctx->oe_arith || ctx->obj_arith;
  if (head_gathers(in)) {
    PhaseScope ph(ctx, "randomize");
    CHK(prepare_round(ctx, ctx->round_counter));     // (update_R finds this round sorted)
  }
  Dev D = ctx->D;
  ctx->head_is_stale = false;      // (dist_mat is recomputed here)
  ctx->objf_continued = true;      // (R is rewritten from the corrected embedding: the objective's warm starts are stale, its next evaluation takes a pass more up front)
  ctx->ledger.r_rewritten();
  const HeadPlan hp = plan_head(in, ctx->ledger);
  if (normalise && !hp.fused_norm) { l_normalize(ctx->L, D.Zc, D.n, D.d, D.zs); KCHK(); }
  D.head_norm = hp.fused_norm ? 1 : 0;
  D.head_gather = hp.files ? 1 : 0; D.Sold_head = hp.files ? ctx->sold_buf[ctx->ledger.cur] : nullptr; D.r_store = hp.r_store;
  void* const zero_sold = hp.clear_first ? D.Sold_head : nullptr;      // (cleared with the three tables below: one launch)
  const size_t n_sold = hp.clear_first ? (size_t)D.nb * D.B * D.K : 0;
  if (hp.files) ctx->ledger.head_filed(in.round, in.seed);
  ctx->R_valid = false;
  // O, the contribution replicas, the objective slots (and a stale old-contribution table): ONE launch instead of three or four memsets -- of
  // those the plan still asks for (l_zero4 launches nothing when there is nothing to clear)
  l_zero4(ctx->L, D.O_fx, hp.clear_O ? (size_t)D.B * D.K : 0, D.Snew_fx, hp.clear_set ? (size_t)D.nrep * D.B * D.K : 0,
          D.objpart, hp.clear_objpart ? 2 * (size_t)D.objslots * D.nwmax : 0, zero_sold, n_sold); KCHK();
  D.head_noobj = hp.skip_obj ? 1 : 0;
  ctx->ledger.head_started();
  CHK(tile_ran(ctx, TileKind::Head, l_tile_static(ctx->L, D, TileKind::Head))); KCHK();      // MFMA tiles; O contributions land in the Snew replicas
  l_fold(ctx->L, D, -1, hp.clear_O ? 0 : 3); KCHK();         // O = sum of the replicas
  ctx->ledger.head_folded();
  if (!hp.skip_obj) { l_obj_reduce(ctx->L, D); KCHK(); }
  CHK(allreduce(ctx, D.O_fx, (int64_t)D.B * D.K, 0));
  if (!hp.skip_obj) CHK(allreduce(ctx, D.obj, 2, 1));
  if (ctx->oe_arith) CHK(oe_head(ctx));        // E = sum(R, 1) Pr_b^T, O = R Phi^T as the reference sums them (:149-150)
  ctx->R_valid = D.r_store != 0;
  return 0;
}

bool check_convergence_impl(hmx_ctx* c, int type) {  // src/harmony.cpp:173-205
  float obj_new, obj_old;
  if (type == 0) {
    obj_old = 0; obj_new = 0;
    for (int i = 0; i < c->window_size; i++) {
      obj_old += c->obj_kmeans[c->obj_kmeans.size() - 2 - i];
      obj_new += c->obj_kmeans[c->obj_kmeans.size() - 1 - i];
    }
    return std::fabs(obj_old - obj_new) / std::fabs(obj_old) < c->eps_k;
  } else if (type == 1) {
    obj_old = c->obj_harmony[c->obj_harmony.size() - 2];
    obj_new = c->obj_harmony[c->obj_harmony.size() - 1];
    return (obj_old - obj_new) / std::fabs(obj_old) < c->eps_h;
  }
  return true;
}

// Results of the last device-side correction that live on the host only on demand: flags (singular system -> error; subset /
// skipped counts), W of the last solved cluster, the centroids.
int sync_solve_results(hmx_ctx* ctx) {
  if (ctx->solve_pending) {
    ctx->solve_pending = false;
    const int K = ctx->K, d = ctx->d;
    std::vector<int> flags(K), mrows(K);
    CHK(d2h(ctx, flags.data(), ctx->sv_flags, (size_t)K)); CHK(d2h(ctx, mrows.data(), ctx->sv_mrows, (size_t)K));
    ctx->subset_clusters = ctx->skipped_clusters = 0;
    int last = -1;
    for (int k = 0; k < K; k++) {
      if (flags[k] & 4) return fail(ctx, HMX_ERR_SOLVE, "singular ridge system");
      if (flags[k] & 1) ctx->subset_clusters++;
      if (flags[k] & 2) ctx->skipped_clusters++; else last = k;
    }
    if (last >= 0) {   // the reference's W field holds the last cluster's coefficients (:592-611)
      const int m = mrows[last];
      ctx->W.resize((size_t)m * d); ctx->W_rows = m;
      CHK(d2h(ctx, ctx->W.data(), ctx->sv_Wall + (size_t)last * d * ((size_t)ctx->B + 1), (size_t)m * d));
    }
  }
  if (ctx->y_on_device) { ctx->y_on_device = false; CHK(d2h(ctx, ctx->Y.data(), ctx->D.Ycur, ctx->Y.size())); }
  return 0;
}

// R-compatible mode: the generator is seeded like set.seed(seed) once per run (hmx_restart re-arms it)
void ensure_rrng(hmx_ctx* ctx) {
  if (!ctx->rrng_seeded) { ctx->rrng.set_seed((uint32_t)ctx->seed); ctx->rrng_seeded = true; }
}

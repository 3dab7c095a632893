// hmx_api_setup.inc -- part of hmx_api.cpp (included there, ONE translation unit): hmx_setup / hmx_setup_ex (src/harmony.cpp:29-128): ingest, level codes, combination sort, HBM layout, launch shapes
// ---- pieces shared by hmx_setup_ex and hmx_map_query ----------------------------------------------------------------------------
// per-covariate level codes from the C-hot CSC design (src/harmony.cpp:49-65, R/ui.R:210-213): codes[c * N + i] = level of cell i in covariate c
static int phi_codes(hmx_ctx* ctx, int64_t N, const int32_t* phi_i, const int32_t* phi_p, const double* phi_x, int32_t B, int32_t C,
                     std::vector<int>& codes) {
  codes.assign((size_t)C * N, 0);
  for (int64_t i = 0; i < N; i++) {
    if (phi_p[i + 1] - phi_p[i] != C) return fail(ctx, HMX_ERR_PHI, "Phi column does not hold exactly one level per covariate");
    for (int c = 0; c < C; c++) {
      const int b = phi_i[phi_p[i] + c];
      if (b < 0 || b >= B || b >= ctx->cov_bounds[c] || (c > 0 && b < ctx->cov_bounds[c - 1]))
        return fail(ctx, HMX_ERR_PHI, "Phi rows are not grouped by covariate");
      if (phi_x && phi_x[phi_p[i] + c] != 1.0) return fail(ctx, HMX_ERR_PHI, "Phi must be a 0/1 design");
      codes[(size_t)c * N + i] = b;
    }
  }
  return 0;
}
// level combinations: dense mixed-radix key of every cell and the cells per key (identical on every rank)
static int combo_keys(hmx_ctx* ctx, int64_t N, int32_t C, const std::vector<int>& codes, std::vector<int>& key, std::vector<long long>& present) {
  double dense = 1; for (int c = 0; c < C; c++) dense *= ctx->B_vec[c];
  if (dense > 16777216.0) return fail(ctx, HMX_ERR_LIMIT, "product of covariate level counts exceeds 2^24");
  present.assign((size_t)dense, 0);
  key.assign((size_t)N, 0);
  for (int64_t i = 0; i < N; i++) {
    int64_t kk = 0, mul = 1;
    for (int c = 0; c < C; c++) { kk += mul * (codes[(size_t)c * N + i] - (c ? ctx->cov_bounds[c - 1] : 0)); mul *= ctx->B_vec[c]; }
    key[i] = (int)kk; present[(size_t)kk]++;
  }
  return 0;
}
// compact combination ids (ctx->Q, ctx->qlev) and the internal order: cells sorted (stably) by combination (ctx->perm, invperm,
// start[q] = first cell of combination q, combo_sorted = combination of every internal position)
static void combo_order(hmx_ctx* ctx, int64_t N, int32_t C, const std::vector<long long>& present, const std::vector<int>& key,
                        std::vector<int>& start, std::vector<int>& invperm, std::vector<int>& combo_sorted) {
  const int64_t P = (int64_t)present.size();
  std::vector<int> qid((size_t)P, -1);
  ctx->Q = 0; ctx->qlev.clear();
  for (int64_t kk = 0; kk < P; kk++) if (present[(size_t)kk] > 0) {
    qid[(size_t)kk] = ctx->Q++;
    int64_t rem = kk;
    for (int c = 0; c < C; c++) { ctx->qlev.push_back((int)(rem % ctx->B_vec[c]) + (c ? ctx->cov_bounds[c - 1] : 0)); rem /= ctx->B_vec[c]; }
  }
  const int Q = ctx->Q;
  std::vector<int> combo_of((size_t)N);
  start.assign((size_t)Q + 1, 0); invperm.assign((size_t)N, 0); combo_sorted.assign((size_t)N, 0);
  for (int64_t i = 0; i < N; i++) { combo_of[i] = qid[(size_t)key[i]]; start[(size_t)combo_of[i] + 1]++; }
  for (int q = 0; q < Q; q++) start[q + 1] += start[q];
  ctx->perm.assign((size_t)N, 0);
  { std::vector<int> cur(start.begin(), start.end() - 1);
    for (int64_t i = 0; i < N; i++) { const int p = cur[combo_of[i]]++; ctx->perm[p] = (int)i; invperm[i] = p; combo_sorted[p] = combo_of[i]; } }
}
// Z: d x N (cell-major) -> ctx->D.Zo (fp32 rows in internal order through ctx->D.invperm, stride D.zs); hmx_get("timer:ingest_Z")
static int ingest_Z(hmx_ctx* ctx, const void* Z, int32_t z_dtype, int32_t z_location, int64_t N, int32_t d) {
  Dev& D = ctx->D;
  // Z: d x N (cell-major), double (the R seam, conv_to :41) or float, on the host or already in HBM -> fp32 rows in internal
  // order.  Host input goes through two HBM staging slabs: the copy of slab s+1 (copy stream) overlaps the conversion of slab s.
  if (z_location != HMX_DEVICE && xfer_mode() == 2) (void)xfer_ring(ctx->device).ensure();    // (once per process: not part of a matrix's transfer time)
  // (the buffers' first touch by the clears above is allocate_buffers' time, and the first launch of a library kernel in a process loads the
  //  code object -- tens of ms once per process --: neither is the ingest's)
  l_copy(ctx->L, D.Zo, D.Zo, 0); KCHK();
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  {
    const double t_in = now_ms();
    const int f32 = z_dtype == HMX_F32;
    const size_t esz = f32 ? 4 : 8;
    if (z_location == HMX_DEVICE) {
      l_convert_in(ctx->L, Z, f32, D.Zo, D.invperm, (int)N, d, D.zs); KCHK();
      HIPCHK(hipStreamSynchronize(ctx->L.stream));
    } else if (xfer_mode() == 2 && xfer_ring(ctx->device).ensure()) {
      // ring of page-locked slots: host threads fill slot b while the DMA engine drains the earlier ones and the conversion kernel
      // consumes what has landed (two HBM staging slabs)
      XferRing& ring = xfer_ring(ctx->device);
      std::lock_guard<std::mutex> ring_lock(ring.mu);
      XferPool pool; pool.start(xfer_threads());
      const int64_t slab = std::max<int64_t>(1, (int64_t)XferRing::SLOT / ((int64_t)esz * d));
      hipStream_t cs = ring.cs;
      hipEvent_t* copied = ring.ev_a; hipEvent_t* used = ring.ev_b; hipEvent_t* left = ring.ev_slot;   // left[b]: slot b's bytes have left for the device
      ctx->timers["ingest_pinned"] = 2.0;
      hipError_t e = hipSuccess;
      int it = 0;
      for (int64_t s0 = 0; s0 < N && e == hipSuccess; s0 += slab, it++) {
        const int64_t cnt = std::min<int64_t>(slab, N - s0);
        const size_t nbytes = (size_t)cnt * d * esz;
        const int b = it & 1, rb = it % XferRing::NB;
        if (it >= XferRing::NB) e = hipEventSynchronize(left[rb]);
        if (e != hipSuccess) break;
        pool.copy(ring.slot[rb], (const char*)Z + (size_t)s0 * d * esz, nbytes);
        if (it >= 2) e = hipStreamWaitEvent(cs, used[b], 0);           // the slab's previous conversion has read it
        if (e == hipSuccess) e = hipMemcpyAsync(ring.stage[b], ring.slot[rb], nbytes, hipMemcpyHostToDevice, cs);
        if (e == hipSuccess) e = hipEventRecord(left[rb], cs);
        if (e == hipSuccess) e = hipEventRecord(copied[b], cs);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->L.stream, copied[b], 0);
        if (e == hipSuccess) { l_convert_in(ctx->L, ring.stage[b], f32, D.Zo, D.invperm + s0, (int)cnt, d, D.zs); e = hipGetLastError(); }
        if (e == hipSuccess) e = hipEventRecord(used[b], ctx->L.stream);
      }
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->L.stream);
      (void)hipStreamSynchronize(cs);
      if (e != hipSuccess) return fail(ctx, HMX_ERR_DEVICE, hipGetErrorString(e));
    } else {
      const int64_t slab = std::max<int64_t>(1, (int64_t)(128ll << 20) / ((int64_t)esz * d));
      const int64_t scnt = std::min<int64_t>(slab, N);
      void* stage[2] = {nullptr, nullptr}; hipStream_t cs = nullptr; hipEvent_t copied[2] = {nullptr, nullptr}, used[2] = {nullptr, nullptr};
      // The caller's matrix is pageable (R's heap): page-lock it for the duration of the ingest, so that the slab copies are real DMA
      // at PCIe speed instead of the runtime's staged pageable path (HMX_PIN=0 leaves it pageable; a failed registration is not an error).
      const bool pinned = xfer_mode() >= 1 && hipHostRegister(const_cast<void*>(Z), (size_t)N * d * esz, hipHostRegisterDefault) == hipSuccess;
      if (!pinned) (void)hipGetLastError();
      ctx->timers["ingest_pinned"] = pinned ? 1.0 : 0.0;
      hipError_t e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
      for (int i = 0; i < 2 && e == hipSuccess; i++) {
        e = hipMalloc(&stage[i], (size_t)scnt * d * esz);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&copied[i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&used[i], hipEventDisableTiming);
      }
      int it = 0;
      for (int64_t s0 = 0; s0 < N && e == hipSuccess; s0 += slab, it++) {
        const int64_t cnt = std::min<int64_t>(slab, N - s0);
        const int b = it & 1;
        if (it >= 2) e = hipStreamWaitEvent(cs, used[b], 0);           // the slab's previous conversion has read it
        if (e == hipSuccess) e = hipMemcpyAsync(stage[b], (const char*)Z + (size_t)s0 * d * esz, (size_t)cnt * d * esz, hipMemcpyHostToDevice, cs);
        if (e == hipSuccess) e = hipEventRecord(copied[b], cs);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->L.stream, copied[b], 0);
        if (e == hipSuccess) { l_convert_in(ctx->L, stage[b], f32, D.Zo, D.invperm + s0, (int)cnt, d, D.zs); e = hipGetLastError(); }
        if (e == hipSuccess) e = hipEventRecord(used[b], ctx->L.stream);
      }
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->L.stream);
      for (int i = 0; i < 2; i++) { if (stage[i]) (void)hipFree(stage[i]); if (copied[i]) (void)hipEventDestroy(copied[i]); if (used[i]) (void)hipEventDestroy(used[i]); }
      if (cs) (void)hipStreamDestroy(cs);
      if (pinned) (void)hipHostUnregister(const_cast<void*>(Z));
      if (e != hipSuccess) return fail(ctx, HMX_ERR_DEVICE, hipGetErrorString(e));
    }
    ctx->timers["ingest_Z"] = now_ms() - t_in;
  }
  return 0;
}

// ---- setup (src/harmony.cpp:29-128) -------------------------------------------------------------------
int hmx_setup(hmx_ctx* ctx, const double* Z, int64_t N, int32_t d, const int32_t* phi_i, const int32_t* phi_p,
              const double* phi_x, int32_t B, const double* sigma, const double* theta, const double* lambda,
              int32_t n_lambda, double alpha, int32_t max_iter_kmeans, double epsilon_kmeans, double epsilon_harmony,
              int32_t K, double block_size, const int32_t* B_vec, int32_t C, double cutoff, int32_t verbose) {
  return hmx_setup_ex(ctx, Z, HMX_F64, HMX_HOST, N, d, phi_i, phi_p, phi_x, B, sigma, theta, lambda, n_lambda, alpha, max_iter_kmeans,
                      epsilon_kmeans, epsilon_harmony, K, block_size, B_vec, C, cutoff, verbose);
}

int hmx_setup_ex(hmx_ctx* ctx, const void* Z, int32_t z_dtype, int32_t z_location, int64_t N, int32_t d, const int32_t* phi_i,
                 const int32_t* phi_p, const double* phi_x, int32_t B, const double* sigma, const double* theta,
                 const double* lambda, int32_t n_lambda, double alpha, int32_t max_iter_kmeans, double epsilon_kmeans,
                 double epsilon_harmony, int32_t K, double block_size, const int32_t* B_vec, int32_t C, double cutoff,
                 int32_t verbose) {
  if (!ctx) return HMX_ERR_ARG;
  if (ctx->query_done) return fail(ctx, HMX_ERR_STATE, "this handle mapped a query: create a new handle for a fit");
  if ((z_dtype != HMX_F64 && z_dtype != HMX_F32) || (z_location != HMX_HOST && z_location != HMX_DEVICE))
    return fail(ctx, HMX_ERR_ARG, "bad dtype / location of Z");
  ctx->err.clear(); ctx->warn.clear();
  if (!Z || !phi_i || !phi_p || !sigma || !theta || !lambda || !B_vec) return fail(ctx, HMX_ERR_ARG, "null argument");
  if (N <= 0 || d <= 0 || K <= 0 || B <= 0 || C <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (d > 128 || K > 256 || C > 15) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: d <= 128, K <= 256, covariates <= 15");
  if (N > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 cells per GPU shard");
  if ((ctx->ridge_arith || ctx->oe_arith || ctx->obj_arith || ctx->solve_arith) && (ctx->world > 1 || ctx->comm_force))
    return fail(ctx, HMX_ERR_ARG, "the reference-arithmetic modes (ridge_arith / oe_arith / obj_arith / solve_arith) run on one GPU");
  if (ctx->world <= 1) { ctx->N_global = N; ctx->goff = 0; }
  if (ctx->N_global > 4000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 4e9 cells in total");
  if (ctx->N_global < 6) return fail(ctx, HMX_ERR_TOO_FEW, "Refusing to run with less than 6 cells");
  if (n_lambda != 1 && n_lambda != B + 1) return fail(ctx, HMX_ERR_ARG, "lambda must have length B+1 (or be the single value -1)");

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(ctx, HMX_ERR_DEVICE, "no HIP device available: libharmony_mi355x has no CPU fallback");
  if (ctx->device < 0) { int cur = 0; (void)hipGetDevice(&cur); ctx->device = cur; }
  HIPCHK(hipSetDevice(ctx->device));
  free_all(ctx);
  if (!ctx->L.stream) { HIPCHK(hipStreamCreateWithFlags(&ctx->L.stream, hipStreamNonBlocking)); ctx->own_stream = true; }
  if (ctx->L.grid <= 0) {
    const char* e = getenv("HMX_GRID");
    ctx->L.grid = e ? atoi(e) : 2048;
  }

  ctx->N = N; ctx->d = d; ctx->K = K; ctx->B = B; ctx->C = C; ctx->verbose = verbose;
  ctx->B_vec.assign(B_vec, B_vec + C);
  ctx->cov_bounds.resize(C);
  std::partial_sum(ctx->B_vec.begin(), ctx->B_vec.end(), ctx->cov_bounds.begin());
  if (ctx->cov_bounds.back() != B) return fail(ctx, HMX_ERR_ARG, "sum(B_vec) != nrow(Phi)");
  ctx->sigma.resize(K); for (int k = 0; k < K; k++) ctx->sigma[k] = (float)sigma[k];
  ctx->theta.resize(B); for (int b = 0; b < B; b++) ctx->theta[b] = (float)theta[b];
  if (lambda[0] == -1) { ctx->lambda_estimation = true; ctx->lambda.clear(); }
  else {
    if (n_lambda != B + 1) return fail(ctx, HMX_ERR_ARG, "fixed lambda must have length B+1");
    ctx->lambda_estimation = false; ctx->lambda.resize(B + 1); for (int i = 0; i <= B; i++) ctx->lambda[i] = (float)lambda[i];
  }
  ctx->alpha = (float)alpha; ctx->max_iter_kmeans = max_iter_kmeans; ctx->eps_k = (float)epsilon_kmeans;
  ctx->eps_h = (float)epsilon_harmony; ctx->cutoff = (float)cutoff;
  if (ctx->N_global < 40) { ctx->warn = "Too few cells. Setting block_size to 0.2"; ctx->block_size = 0.2f; }  // :86-88
  else ctx->block_size = (float)block_size;
  ctx->nb = my_ceil(1.0 / ctx->block_size);                                         // :280
  ctx->cells_per_block = (uint64_t)(unsigned)((float)ctx->N_global * ctx->block_size);  // :281 (fp32 product, truncated)
  if (ctx->cells_per_block < 1) ctx->cells_per_block = 1;
  if (ctx->nb < 1) ctx->nb = 1;

  // ---- per-covariate level codes from the C-hot CSC design (src/harmony.cpp:49-65, R/ui.R:210-213)
  std::vector<int> codes, key;
  std::vector<long long> present;
  CHK(phi_codes(ctx, N, phi_i, phi_p, phi_x, B, C, codes));
  CHK(combo_keys(ctx, N, C, codes, key, present));
  const int64_t P = (int64_t)present.size();
  // global level sizes N_b and global presence (one all-reduce each when sharded)
  std::vector<long long> nbcount((size_t)B, 0);
  for (int c = 0; c < C; c++) for (int64_t i = 0; i < N; i++) nbcount[codes[(size_t)c * N + i]]++;
  if (ctx->world > 1 || ctx->comm_force) {
    long long* dtmp; const size_t cnt = (size_t)P + B;
    HIPCHK(hipMalloc((void**)&dtmp, cnt * sizeof(long long)));
    std::vector<long long> tmp(present); tmp.insert(tmp.end(), nbcount.begin(), nbcount.end());
    int st = h2d(ctx, dtmp, tmp.data(), cnt);
    if (!st) st = allreduce(ctx, dtmp, (int64_t)cnt, 0);
    if (!st) st = d2h(ctx, tmp.data(), dtmp, cnt);
    (void)hipFree(dtmp);
    if (st) return st;
    std::copy(tmp.begin(), tmp.begin() + P, present.begin());
    std::copy(tmp.begin() + P, tmp.end(), nbcount.begin());
  }
  std::vector<int> start, invperm, combo_sorted;
  combo_order(ctx, N, C, present, key, start, invperm, combo_sorted);
  const int Q = ctx->Q;
  ctx->sizes.resize(B); ctx->Pr_b.resize(B);
  for (int b = 0; b < B; b++) { ctx->sizes[b] = (float)nbcount[b]; ctx->Pr_b[b] = ctx->sizes[b] / (float)ctx->N_global; }  // :67
  std::vector<Item> items, aitems, titems;
  for (int q = 0; q < Q; q++) {
    for (int s = start[q]; s < start[q + 1]; s += ITEM_CELLS) items.push_back({q, s, std::min(ITEM_CELLS, start[q + 1] - s)});
    for (int s = start[q]; s < start[q + 1]; s += APPLY_CELLS) aitems.push_back({q, s, std::min(APPLY_CELLS, start[q + 1] - s)});
    for (int s = start[q]; s < start[q + 1]; s += 16) titems.push_back({q, s, std::min(16, start[q + 1] - s)});
  }

  // ---- device state
  Dev& D = ctx->D;
  D = Dev{};
  D.n = (int)N; D.d = d; D.K = K; D.B = B; D.C = C; D.Q = Q; D.B0 = ctx->B_vec[0];
  for (int c = 0; c < 4; c++) D.cov_end[c] = c < C ? ctx->cov_bounds[c] : B;
  D.KP = (K + 63) / 64 * 64; D.nb = ctx->nb;
  D.zs = (d + 3) / 4 * 4;
  // (rows padded to whole 128-byte lines -- 208 -> 256 B at d = 50 -- were measured in round 4: the block step stayed where it was for 23 % more memory; the switch is gone)
  { const char* e = getenv("HMX_NREP"); int want = e ? atoi(e) : 8; if (want > 8) want = 8; D.nrep = 1; while (D.nrep * 2 <= want && (size_t)D.nrep * 2 * B * K <= (1u << 20)) D.nrep *= 2; }
  { static const int sup[] = {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 13, 14, 16};     // (13: K = 200, BASELINE configs[4])
    const int need = (K + 15) / 16; D.NCT = 16; for (int v : sup) if (v >= need) { D.NCT = v; break; } }
  { const char* e = getenv("HMX_MOE_IMPL");
    D.moe_mfma = (K % 4 == 0 && d <= 64 && K <= 256 && !(e && std::string(e) == "v1")) ? 1 : 0;   // K > 128: split statistics kernel
    D.wNT4 = K / 16; D.wtail = (K - 16 * D.wNT4) / 4; D.wNS = 4 * D.wNT4 + D.wtail; D.wNQ = ((d + 15) / 16 + 3) / 4; }
  D.r_store = 1;
  { const char* rs = getenv("HMX_R_STORE"); ctx->r_store_always = rs && atoi(rs) == 1; }
  D.nwmax = 4 * ctx->L.grid; D.objslots = std::min(D.nb, 64);
  D.pen_lds = ((size_t)D.NQ * 0 + (size_t)B * K * 4 + (size_t)Q * C * 4 <= 24576) ? 1 : 0;
  D.rvec = (K % 4 == 0) ? 1 : 0;
  D.NQ = (D.NCT + 3) / 4; D.NT4 = D.zs / 16; D.tail = (D.zs - 16 * D.NT4) / 4; D.NS = 4 * D.NT4 + D.tail;
  // the static-tile launches (head, seeding race, Lloyd) stage this centroid image in LDS: across the envelope (d <= 128, K <= 256) it is at most
  // 4 quads x 32 PC steps x 1 KB = 128 KB, so they need no fallback (Lloyd's K x d sum table beside it may not fit: k_lloyd, hmx_api_kmeans.inc)
  if ((size_t)D.NQ * D.NS * 1024 > 128 * 1024) return fail(ctx, HMX_ERR_LIMIT, "centroid image exceeds 128 KB of LDS");
  // split-bf16 form of the tile kernels' distance GEMM (hmx_tile_bf.hip): offered where its register form covers the shapes the fp32
  // register form covers (rows of <= 64 PCs in four 16-byte groups); each launch takes it when its LDS image fits (l_update & co)
  D.NS2 = (D.zs + 31) / 32;
  { const char* e = getenv("HMX_DOT"); D.dot_bf = !(e && std::string(e) == "f32") && (D.NT4 > 4 || D.NS2 <= 2) && D.NS2 <= 4; }
  { const char* e = getenv("HMX_UPD_THREADS"); D.upd_threads = (e && atoi(e) == 256) ? 256 : 512; }
  { // uniform sigma (the reference's default): scalar-constant kernel variants; with K <= 64 they also fit the register
    // budget of 4 waves per SIMD (1024-thread workgroups) -- measured 16 % faster per launch than 2 waves at K = 64
    bool usig = true; for (int k = 1; k < K; k++) usig = usig && ctx->sigma[k] == ctx->sigma[0];
    { const char* e = getenv("HMX_USIG"); if (e && atoi(e) == 0) usig = false; }
    D.usig = usig ? 1 : 0;
    const char* e = getenv("HMX_UPD_WPS");
    int w = ctx->tun_wps > 0 ? ctx->tun_wps : (e ? atoi(e) : 4);
    if (w != 4 || !usig || D.NCT > 4) w = 2;
    D.upd_wps = w;
    if (w == 4) D.upd_threads = 1024; }
  { const char* e = getenv("HMX_UPD_MAXBLOCKS"); D.upd_maxblocks = e ? atoi(e) : (D.upd_threads >= 512 ? 256 : 512); if (D.upd_maxblocks < 1) D.upd_maxblocks = 1; }
  D.upd_debug = 0;
  // static-tile launches (head / Lloyd / seeding): one resident generation of 256-thread workgroups (2 per CU at the 2 waves
  // per SIMD the K > 64 kernels get) re-stages the centroid image once instead of four times: head 213 -> 200 us at 1M
  { const char* e = getenv("HMX_STATIC_MAXBLOCKS"); D.static_maxblocks = e ? atoi(e) : (D.NCT >= 5 ? 512 : D.NCT >= 3 ? 768 : 1024); }
  { const char* e = getenv("HMX_OLDSUM_IMPL"); D.oldsum_stream = (e && std::string(e) == "gather") ? 0 : (e && std::string(e) == "stream1") ? 2 : 1; }   // 1: 16-byte stream, 2: dword stream
  D.need_lorder = (D.oldsum_stream == 0 || (size_t)D.nb * K * 8 > 64 * 1024) ? 1 : 0;
  { const char* e = getenv("HMX_UPD_TPW"); D.upd_tpw = ctx->tun_tpw > 0 ? ctx->tun_tpw : (e ? atoi(e) : 1); if (D.upd_tpw < 1) D.upd_tpw = 1; }
  std::vector<Item> schunks; std::vector<int> qchunk((size_t)Q + 1, 0);
  for (int q = 0; q < Q; q++) {
    qchunk[q] = (int)schunks.size();
    for (int s = start[q]; s < start[q + 1]; s += SORT_CHUNK) schunks.push_back({q, s, std::min(SORT_CHUNK, start[q + 1] - s)});
  }
  qchunk[Q] = (int)schunks.size();
  D.nchunks = (int)schunks.size();
  { // Old contributions carried from round to round (update_R): tiles keyed by (block, combination, NEXT block) cost up to 16
    // padding slots per key -- worth it while the expected padding (8 per key) stays below 4 % (12 % with the chain) of the cells.  HMX_SOLD_CARRY=0|1.
    const char* e = getenv("HMX_SOLD_CARRY");
    const bool fits = D.nb <= 63 && Q < (1 << 19) &&
                      (int64_t)N + (int64_t)D.nb * D.nb * Q * 16 <= 2147483000ll;
    // (round 4: with the R stores of carried rounds gone as well -- Dev::r_store -- the carry saves ~200 us per round at 1M cells where the
    //  persistent chain runs (K <= 112): worth up to ~12 % of padding there; measured at 1.25M cells / 20 batches, 5.1 %: 15.5 -> 12.7 ms per run.
    //  On the launch-per-step path (configs[4] shape, 41 %: 63 -> 70 ms) the old bound stays.)
    //  Round 6: 12 % of padding for K > 112 as well -- configs[4] at its full 5M cells (8.2 %): 165.9 -> 140.5 ms per run (no pass over R for the old
    //  contributions: 21.8 ms, no R stores in 21 of 28 rounds); 2.5M cells (16 %): 95.3 / 94.0 ms, break-even.)
    const bool pays = (int64_t)D.nb * D.nb * Q * 8 * 8 <= (int64_t)N;
    ctx->carry_ok = fits && (e ? atoi(e) == 1 : pays) && !ctx->oe_arith;      // (oe_arith: the tables follow the reference, nothing is carried)
    D.nxt = 0; D.Sold_next = nullptr; D.Sold_head = nullptr; D.head_gather = 0; ctx->carried_rounds = 0;
    D.qmask = ctx->carry_ok ? 0x7FFFF : 0x7FFFFFFF; }
  const int nV = ctx->carry_ok ? D.nb * D.nb : D.nb;      // sort keys of a round
  if ((int64_t)N + (int64_t)nV * Q * 16 > 2147483000ll)
    return fail(ctx, HMX_ERR_LIMIT, "padded block order (N + n_blocks * combinations * 16) exceeds the int32 index range of one shard");
  D.npad = (int)((int64_t)N + (int64_t)nV * Q * 16);
  D.nitems = (int)items.size(); D.naitems = (int)aitems.size(); D.ntitems = (int)titems.size();
  CHK(dalloc(ctx, &D.Zo, (size_t)N * D.zs)); CHK(dalloc(ctx, &D.Zc, (size_t)N * D.zs)); CHK(dalloc(ctx, &D.R, ((size_t)N + 1) * K));   // + one dummy row (target of masked stores)
  CHK(dalloc(ctx, &D.perm, (size_t)N)); CHK(dalloc(ctx, &D.invperm, (size_t)N)); CHK(dalloc(ctx, &D.combo, (size_t)N));
  CHK(dalloc(ctx, &D.qlev, (size_t)Q * C));
  CHK(dalloc(ctx, &D.Yt, (size_t)d * K)); CHK(dalloc(ctx, &D.Ycur, (size_t)d * K)); CHK(dalloc(ctx, &D.Yimg, (size_t)D.NQ * D.NS * 256)); HIPCHK(hipMemsetAsync(D.Yimg, 0, (size_t)D.NQ * D.NS * 1024, ctx->L.stream)); CHK(dalloc(ctx, &D.Yimg3, (size_t)D.NCT * D.NS2 * 3 * 512)); HIPCHK(hipMemsetAsync(D.Yimg3, 0, (size_t)D.NCT * D.NS2 * 3 * 1024, ctx->L.stream)); CHK(dalloc(ctx, &D.sigma, (size_t)K)); CHK(dalloc(ctx, &D.theta, (size_t)B)); CHK(dalloc(ctx, &D.Pr_b, (size_t)B));
  CHK(dalloc(ctx, &D.O_fx, (size_t)B * K)); CHK(dalloc(ctx, &D.Snew_fx, (size_t)D.nrep * B * K));
  // Sold_fx [nb][B][K] and the three rotating replica sets of the fused path share one buffer: one memset per round
  { long long* s3; CHK(dalloc(ctx, &s3, (size_t)2 * D.nb * B * K + (size_t)3 * D.nrep * B * K)); D.Sold_fx = s3;
    ctx->sold_buf[0] = s3; ctx->sold_buf[1] = s3 + (size_t)D.nb * B * K; ctx->sold_cur = 0; ctx->sold_state[0] = ctx->sold_state[1] = 1; ctx->sets_clean = false;
    for (int i = 0; i < 3; i++) D.Snew_set[i] = s3 + (size_t)2 * D.nb * B * K + (size_t)i * D.nrep * B * K; }
  CHK(dalloc(ctx, &D.O_alt, (size_t)B * K)); CHK(dalloc(ctx, &D.Snew_alt, (size_t)D.nrep * B * K)); CHK(dalloc(ctx, &D.objpart, (size_t)2 * D.objslots * D.nwmax)); CHK(dalloc(ctx, &D.objrow, (size_t)2 * D.objslots));
  D.trace = nullptr;
  if (const char* e = getenv("HMX_TRACE")) if (atoi(e)) { CHK(dalloc(ctx, &D.trace, (size_t)16 * D.nwmax)); HIPCHK(hipMemsetAsync(D.trace, 0, sizeof(unsigned long long) * 16 * (size_t)D.nwmax, ctx->L.stream)); }
  CHK(dalloc(ctx, &D.pen, (size_t)B * K)); CHK(dalloc(ctx, &D.obj, (size_t)8));
  CHK(dalloc(ctx, &D.blk, (size_t)N)); CHK(dalloc(ctx, &D.lorder, (size_t)3 * D.npad + 2)); D.lpair = reinterpret_cast<int2*>(D.lorder + (((size_t)D.npad + 1) & ~(size_t)1)); /* lorder + lpair: one 0xFF memset per round */ CHK(dalloc(ctx, &D.lcombo, (size_t)D.npad));
  CHK(dalloc(ctx, &D.binoff, (size_t)nV * Q + 1)); CHK(dalloc(ctx, &D.schunks, schunks.size())); CHK(dalloc(ctx, &D.qchunk, (size_t)Q + 1));
  CHK(dalloc(ctx, &D.blkv, (size_t)N)); CHK(dalloc(ctx, &D.bincnt, (size_t)nV * Q));
  CHK(dalloc(ctx, &D.ce, (size_t)K)); CHK(dalloc(ctx, &D.cl, (size_t)K)); CHK(dalloc(ctx, &D.boff, (size_t)D.nb + 1));
  CHK(dalloc(ctx, &D.counts, (size_t)nV * D.nchunks)); CHK(dalloc(ctx, &D.offs, (size_t)nV * D.nchunks));
  { // second buffer set + side stream for the overlapped shuffle of the next round 
    ctx->sets[0] = {D.blk, D.lorder, D.lpair, D.lcombo, D.boff, D.binoff, D.counts, D.offs, D.blkv, D.bincnt};
    hmx_ctx::SortSet& t = ctx->sets[1];
    CHK(dalloc(ctx, &t.blk, (size_t)N)); CHK(dalloc(ctx, &t.lorder, (size_t)3 * D.npad + 2)); t.lpair = reinterpret_cast<int2*>(t.lorder + (((size_t)D.npad + 1) & ~(size_t)1));
    CHK(dalloc(ctx, &t.lcombo, (size_t)D.npad)); CHK(dalloc(ctx, &t.binoff, (size_t)nV * Q + 1)); CHK(dalloc(ctx, &t.boff, (size_t)D.nb + 1));
    CHK(dalloc(ctx, &t.counts, (size_t)nV * D.nchunks)); CHK(dalloc(ctx, &t.offs, (size_t)nV * D.nchunks)); CHK(dalloc(ctx, &t.blkv, (size_t)N)); CHK(dalloc(ctx, &t.bincnt, (size_t)nV * Q));
    ctx->sort_overlap = true;
    { int lo = 0, hi = 0; (void)hipDeviceGetStreamPriorityRange(&lo, &hi);      // lowest priority: the shuffle only fills gaps
      HIPCHK(hipStreamCreateWithPriority(&ctx->side, hipStreamNonBlocking, lo)); }
    for (int i = 0; i < 2; i++) { HIPCHK(hipEventCreateWithFlags(&ctx->ev_sorted[i], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&ctx->ev_free[i], hipEventDisableTiming)); }
    ctx->sort_sched = 3;      // (the per-round schedule, sort_sched = 1, lost round 4 to the batched shuffle; its switches are gone)
    ctx->oset_mask = ctx->sort_sched == 3 ? 3 : 1;
    { const char* si = getenv("HMX_SHUFFLE_INV"); const int v = si ? atoi(si) : 1;      // 0: counting sort always; 2: sort-free form on sharded runs too
      ctx->shuf_inv = ctx->sort_sched == 3 && v != 0 && (ctx->world == 1 || v == 2) && ctx->carry_ok &&      /* (without the carry every round needs D.blk: the counting sort has it for free) */
                      D.nb < 64 && Q < 2048 && ctx->N_global < ((int64_t)1 << 31) &&
                      ((size_t)D.nb * Q + (size_t)Q + 1) * sizeof(int) + 5 * 4096 <= 64 * 1024; }     // (lpair packs the combination in 19 bits and the blocks in 6; posr the combination in 11)
    if (ctx->shuf_inv) {
      const int P = shuffle_parts((uint64_t)ctx->N_global, D.nb, ctx->cells_per_block);
      for (int i = 0; i < 4; i++) { CHK(dalloc(ctx, &ctx->posr[i], (size_t)ctx->N_global)); CHK(dalloc(ctx, &ctx->shuf_partcnt[i], (size_t)nV * Q * P));
        CHK(dalloc(ctx, &ctx->shuf_binacc[i], (size_t)nV * Q)); HIPCHK(hipMemsetAsync(ctx->shuf_binacc[i], 0, sizeof(int) * (size_t)nV * Q, ctx->L.stream)); }
    }
    if (ctx->sort_sched == 3) for (int i = 2; i < 4; i++) {
      hmx_ctx::SortSet& u = ctx->sets[i];
      CHK(dalloc(ctx, &u.blk, (size_t)N)); CHK(dalloc(ctx, &u.lorder, (size_t)3 * D.npad + 2)); u.lpair = reinterpret_cast<int2*>(u.lorder + (((size_t)D.npad + 1) & ~(size_t)1));
      CHK(dalloc(ctx, &u.lcombo, (size_t)D.npad)); CHK(dalloc(ctx, &u.binoff, (size_t)nV * Q + 1)); CHK(dalloc(ctx, &u.boff, (size_t)D.nb + 1));
      CHK(dalloc(ctx, &u.counts, (size_t)nV * D.nchunks)); CHK(dalloc(ctx, &u.offs, (size_t)nV * D.nchunks)); CHK(dalloc(ctx, &u.blkv, (size_t)N)); CHK(dalloc(ctx, &u.bincnt, (size_t)nV * Q));
    }
  }
  CHK(dalloc(ctx, &D.items, items.size())); CHK(dalloc(ctx, &D.aitems, aitems.size())); CHK(dalloc(ctx, &D.titems, titems.size()));
  CHK(dalloc(ctx, &D.Sq, (size_t)Q * d * K)); CHK(dalloc(ctx, &D.nq, (size_t)Q * K));
  { const char* e = getenv("HMX_MOE_SOLVE"); ctx->solve_on_device = !(e && std::string(e) == "host") && (size_t)(B + 1) * 16 * 8 + (size_t)(4 * B + 8 + C) * 4 <= 158 * 1024; }   // (LDS panel of the device Cholesky)
  ctx->y_on_device = false; ctx->solve_pending = false;
  if (ctx->solve_on_device) {
    const size_t M = (size_t)B + 1;
    CHK(dalloc(ctx, &ctx->sv_cov, (size_t)K * M * M)); CHK(dalloc(ctx, &ctx->sv_rhs, (size_t)K * d * M)); CHK(dalloc(ctx, &ctx->sv_Wall, (size_t)K * d * M));
    CHK(dalloc(ctx, &ctx->sv_mrows, (size_t)K)); CHK(dalloc(ctx, &ctx->sv_flags, (size_t)K)); CHK(dalloc(ctx, &ctx->sv_lambda, M)); CHK(dalloc(ctx, &ctx->sv_cov_bounds, (size_t)C));
    if (!ctx->lambda_estimation) CHK(h2d(ctx, ctx->sv_lambda, ctx->lambda.data(), M));
    CHK(h2d(ctx, ctx->sv_cov_bounds, ctx->cov_bounds.data(), (size_t)C));
    HIPCHK(hipMemsetAsync(ctx->sv_flags, 0, sizeof(int) * (size_t)K, ctx->L.stream));
    HIPCHK(hipMemsetAsync(ctx->sv_mrows, 0, sizeof(int) * (size_t)K, ctx->L.stream));
  }
  CHK(dalloc(ctx, &D.solve_err, (size_t)1)); HIPCHK(hipMemsetAsync(D.solve_err, 0, sizeof(int), ctx->L.stream));
  CHK(dalloc(ctx, &D.S0, (size_t)K * d)); CHK(dalloc(ctx, &D.n0, (size_t)K)); CHK(dalloc(ctx, &D.qstart, (size_t)Q + 1)); CHK(dalloc(ctx, &D.sizes, (size_t)B));
  CHK(h2d(ctx, D.qstart, start.data(), (size_t)Q + 1)); CHK(h2d(ctx, D.sizes, ctx->sizes.data(), (size_t)B)); CHK(dalloc(ctx, &D.Wq, (size_t)Q * K * d)); CHK(dalloc(ctx, &D.Wimg, D.moe_mfma ? (size_t)Q * D.wNQ * D.wNS * 256 : 1));
  { // deterministic statistics pass (k_moe_stats_q): static split of the 16-cell tiles over ~2 workgroups per CU; one partial
    // slot per (workgroup, combination met) -- known here because the tiles are listed by combination
    const char* e = getenv("HMX_MOE_STATS");
    // (round 6: K in (128, 224] -- configs[4]'s 200 -- as two halves of <= 8 cluster tiles each, by the same kernel: deterministic there too, and 0.26 ms per
    //  correction faster than the fp64-atomic kernel at 1M cells)
    D.st_KH = ((K + 1) / 2 + 3) & ~3;
    D.st_halves = (D.NCT > 8 && K % 4 == 0 && (D.st_KH + 15) / 16 <= 8 && K - D.st_KH >= 4 && K - D.st_KH <= 16 * ((D.st_KH + 15) / 16)) ? 2 : 1;
    D.st_dma = (D.moe_mfma && (D.NCT <= 8 || D.st_halves == 2) && !(e && std::string(e) == "atomic")) ? 1 : 0;
    if (D.st_dma) {
      const int nt = (int)titems.size();
      int tpw = (nt + 2 * 256 - 1) / (2 * 256); if (tpw < 16) tpw = 16;
      D.st_cpw = tpw; D.st_nwg = (nt + tpw - 1) / tpw;
      std::vector<int> slot0((size_t)D.st_nwg), qptr((size_t)Q + 1, 0);
      std::vector<std::vector<int>> byq((size_t)Q);
      int nslots = 0;
      for (int w = 0; w < D.st_nwg; w++) {
        slot0[w] = nslots;
        int last = -1;
        for (int t = w * tpw; t < std::min(nt, (w + 1) * tpw); t++) if (titems[t].q != last) { last = titems[t].q; byq[(size_t)last].push_back(nslots++); }
      }
      std::vector<int> qslots; qslots.reserve((size_t)nslots);
      for (int q = 0; q < Q; q++) { qptr[q] = (int)qslots.size(); qslots.insert(qslots.end(), byq[q].begin(), byq[q].end()); }
      qptr[Q] = (int)qslots.size();
      CHK(dalloc(ctx, &D.st_part, (size_t)std::max(nslots, 1) * ((size_t)K * d + K))); CHK(dalloc(ctx, &D.st_slot0, slot0.size()));
      CHK(dalloc(ctx, &D.st_qptr, qptr.size())); CHK(dalloc(ctx, &D.st_qslots, std::max<size_t>(qslots.size(), 1)));
      CHK(h2d(ctx, D.st_slot0, slot0.data(), slot0.size())); CHK(h2d(ctx, D.st_qptr, qptr.data(), qptr.size()));
      if (!qslots.empty()) CHK(h2d(ctx, D.st_qslots, qslots.data(), qslots.size()));
    }
  }
  CHK(dalloc(ctx, &D.km_gcells, (size_t)K)); CHK(dalloc(ctx, &D.km_rows, (size_t)K * d)); CHK(dalloc(ctx, &D.km_excl, (size_t)K));
  CHK(dalloc(ctx, &D.seedmin, (size_t)K)); CHK(dalloc(ctx, &D.lsum, (size_t)K * d + K)); D.lcnt = reinterpret_cast<unsigned long long*>(D.lsum + (size_t)K * d); CHK(dalloc(ctx, &D.ynorm, (size_t)K));
  CHK(h2d(ctx, D.perm, ctx->perm.data(), (size_t)N)); CHK(h2d(ctx, D.invperm, invperm.data(), (size_t)N));
  CHK(h2d(ctx, D.combo, combo_sorted.data(), (size_t)N)); CHK(h2d(ctx, D.qlev, ctx->qlev.data(), ctx->qlev.size()));
  CHK(h2d(ctx, D.sigma, ctx->sigma.data(), (size_t)K)); CHK(h2d(ctx, D.theta, ctx->theta.data(), (size_t)B)); CHK(h2d(ctx, D.Pr_b, ctx->Pr_b.data(), (size_t)B));
  CHK(h2d(ctx, D.schunks, schunks.data(), schunks.size())); CHK(h2d(ctx, D.qchunk, qchunk.data(), qchunk.size()));
  { std::vector<float> ce(K), cl(K);
    for (int k = 0; k < K; k++) { ce[k] = -1.44269504088896341f / ctx->sigma[k]; cl[k] = ctx->sigma[k] * 0.693147180559945309f; }
    CHK(h2d(ctx, D.ce, ce.data(), (size_t)K)); CHK(h2d(ctx, D.cl, cl.data(), (size_t)K)); }
  CHK(h2d(ctx, D.items, items.data(), items.size())); CHK(h2d(ctx, D.aitems, aitems.data(), aitems.size())); CHK(h2d(ctx, D.titems, titems.data(), titems.size()));
  HIPCHK(hipMemsetAsync(D.O_fx, 0, sizeof(long long) * B * K, ctx->L.stream));
  HIPCHK(hipMemsetAsync(D.Snew_fx, 0, sizeof(long long) * (size_t)D.nrep * B * K, ctx->L.stream));
  HIPCHK(hipMemsetAsync(D.Snew_alt, 0, sizeof(long long) * (size_t)D.nrep * B * K, ctx->L.stream));
  HIPCHK(hipMemsetAsync(D.O_alt, 0, sizeof(long long) * B * K, ctx->L.stream));
  HIPCHK(hipMemsetAsync(D.objpart, 0, sizeof(double) * 2 * (size_t)D.objslots * D.nwmax, ctx->L.stream));
  HIPCHK(hipMemsetAsync(D.obj, 0, sizeof(double) * 8, ctx->L.stream));
  HIPCHK(hipMemsetAsync(D.R, 0, sizeof(float) * (size_t)N * K, ctx->L.stream));
  HIPCHK(hipMemsetAsync(D.Zo, 0, sizeof(float) * (size_t)N * D.zs, ctx->L.stream));
  HIPCHK(hipMemsetAsync(D.Zc, 0, sizeof(float) * (size_t)N * D.zs, ctx->L.stream));
  HIPCHK(hipMemsetAsync(D.Wq, 0, sizeof(float) * (size_t)Q * K * d, ctx->L.stream));
  CHK(ingest_Z(ctx, Z, z_dtype, z_location, N, d));
  ctx->W.assign((size_t)(B + 1) * d, 0.f); ctx->W_rows = B + 1;  // allocate_buffers :127
  ctx->Y.assign((size_t)d * K, 0.f);
  { const char* e = getenv("HMX_FUSED_FOLD");
    ctx->fused_ok = !(e && std::string(e) == "0") &&
                    (size_t)D.NQ * D.NS * 1024 + (size_t)B * K * 12 + (size_t)Q * C * 4 + 64 <= 150 * 1024; }
  { // persistent block chain: one workgroup per CU must be resident at once (they synchronise inside the launch)
    const char* e = getenv("HMX_CHAIN");
    int cus = 0; (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
    ctx->chain_wgs = cus;
    if (const char* w = getenv("HMX_CHAIN_WGS")) ctx->chain_wgs = std::max(8, std::min(cus, atoi(w)));   // (tests: two ranks sharing one GPU)
    // The chain pays off while a block step is latency-bound: a few 16-cell tiles per resident wave (1.5 at 1M cells).  Round 3 measured the per-step launches
    // 6 % faster at 10M cells per GPU (15 tiles per wave) and drew the line at 6 tiles; re-measured in round 6 on the chain as it is now (K = 100, 20 batches, to
    // convergence): 5M cells 37.5 -> 33.8 ms, 7.5M 52.5 -> 49.2, 10M 65.9 -> 61.7 ON the chain, 15M (23 tiles per wave) 97.4 / 98.0: the line is at 20 tiles.
    const double tiles_per_wave = (double)N / std::max(D.nb, 1) / 16.0 / (8.0 * std::max(cus - 1, 1));
    double max_tpw = 20.0; if (const char* m = getenv("HMX_CHAIN_MAX_TPW")) max_tpw = atof(m);       // (tests: move the threshold between two shards)
    const bool chain_fits = (e && std::string(e) == "1") || tiles_per_wave <= max_tpw;
    ctx->chain_ok = !(e && std::string(e) == "0") && chain_fits && ctx->fused_ok && cus >= 8 && D.NCT <= 7 && D.NT4 <= 4 && D.nb <= 64 &&
                    (size_t)D.NQ * D.NS * 1024 + (size_t)B * K * 12 + (size_t)Q * C * 4 + 64 <= 150 * 1024;
    if (ctx->world > 1 || ctx->comm_force) {
      // The flags pick the inter-rank PROTOCOL of update_R (in-launch exchange of the persistent chain / one all-reduce per block
      // step): every rank must take the same path, but chain_ok depends on the LOCAL cell count and CU count.  Agree on the minimum
      // -- before anything is derived from the flags (the replica count below sizes a per-block all-reduce).
      long long* dflag; long long hf[2] = {ctx->chain_ok ? 1 : 0, ctx->fused_ok ? 1 : 0};
      CHK(dalloc(ctx, &dflag, (size_t)2));
      CHK(h2d(ctx, dflag, hf, 2)); CHK(allreduce(ctx, dflag, 2, 2)); CHK(d2h(ctx, hf, dflag, 2));
      ctx->chain_ok = hf[0] != 0; ctx->fused_ok = hf[1] != 0;
    }
    CHK(dalloc(ctx, &D.tail_ticket, (size_t)1)); HIPCHK(hipMemsetAsync(D.tail_ticket, 0, sizeof(int), ctx->L.stream));
    CHK(dalloc(ctx, &D.pen_g, (size_t)B * K)); CHK(dalloc(ctx, &D.chain_ctl, (size_t)8 * D.nb + 24)); CHK(dalloc(ctx, &D.chain_dbg, (size_t)64));
    HIPCHK(hipMemsetAsync(D.chain_dbg, 0, sizeof(unsigned long long) * 64, ctx->L.stream));
    HIPCHK(hipMemsetAsync(D.pen_g, 0, sizeof(unsigned long long) * (size_t)B * K, ctx->L.stream));
    HIPCHK(hipMemsetAsync(D.chain_ctl, 0, sizeof(int) * ((size_t)8 * D.nb + 24), ctx->L.stream));
    D.chain_wps = 2;      // (the 3- / 4-waves-per-SIMD chain variants and the in-chain gathering of the old contributions lost rounds 2 and 3: removed in round 5)
    // the folder reads AND resets every replica of the contribution table inside a block step (atomic exchanges on its critical
    // path): 4 replicas measured 0.4 us per step faster than 8 there (2: the workers' atomics start to queue, +2 us)
    if (ctx->chain_ok && !getenv("HMX_NREP") && D.nrep > 4) {
      D.nrep = 4;
      for (int i = 0; i < 3; i++) D.Snew_set[i] = ctx->sold_buf[0] + (size_t)2 * D.nb * B * K + (size_t)i * D.nrep * B * K;   // keep the three sets contiguous
    }
    // wave-pair chain (k_tile MODE 6) for 112 < K <= 224 -- BASELINE configs[4]: K = 200 -- where no single wave holds a row's clusters and no LDS holds the
    // K x B table: two halves of the clusters on the two waves of a SIMD, several folder workgroups, the penalty rows from memory.  HMX_CHAIN_PAIR=0|1.
    { const char* pe = getenv("HMX_CHAIN_PAIR");
      const int KH = ((K + 1) / 2 + 3) & ~3, nctp = (KH + 15) / 16;
      int kw = ((K + 11) / 12 + 3) & ~3;                                  // clusters per folder workgroup (a multiple of 4): ~12 folders
      if (const char* fe = getenv("HMX_CHAIN_FOLDERS")) { const int want = std::max(1, atoi(fe)); kw = ((K + want - 1) / want + 3) & ~3; }
      const int F = (K + kw - 1) / kw;
      const double tiles_per_stream = (double)N / std::max(D.nb, 1) / 16.0 / (4.0 * std::max(ctx->chain_wgs - F, 1));
      // (measured at configs[4]'s shape: 8 tiles per pair and block -- 2.5M cells -- 94.2 -> 79.1 ms on the chain; 16 -- 5M cells, old contributions carried on both
      //  paths -- 137.8 / 139.0: the launch-per-step path from 12 on)
      const double max_tpw_pair = getenv("HMX_CHAIN_MAX_TPW") ? max_tpw : 12.0;
      const size_t lds_w = (size_t)2 * nctp * D.NS2 * 3 * 1024 + (size_t)((Q * C + 3) & ~3) * 4 + 4 * 2 * 2 * 16 * 8 + (size_t)8 * 4 * 16 * nctp * 4;      // + [8 waves][4 tiles][16 nctp] log2 penalties
      const size_t lds_f = ((size_t)2 * B * kw + kw) * 8;      // folders: [ O slice | cluster masses | this rank's deltas (sharded) ]
      const bool want = !(e && std::string(e) == "0") && !(pe && std::string(pe) == "0") && ((pe && std::string(pe) == "1") || (e && std::string(e) == "1") || tiles_per_stream <= max_tpw_pair);
      D.chain_pair = (want && !ctx->chain_ok && D.NCT > 7 && nctp >= 4 && nctp <= 7 && K % 4 == 0 && K - KH <= 16 * nctp && K - KH >= 4 && D.usig && D.dot_bf && D.NS2 <= 2 && D.NT4 <= 4 &&
                      D.nb <= 64 && cus >= 64 && F < ctx->chain_wgs / 4 && !ctx->oe_arith && !ctx->obj_arith &&
                      std::max(lds_w, lds_f) + 64 <= 150 * 1024) ? 1 : 0;
      if (ctx->world > 1 || ctx->comm_force) {      // (the flag picks the inter-rank protocol of update_R: every rank takes the same path -- the minimum, as for chain_ok above)
        long long* dflag; long long hf = D.chain_pair;
        CHK(dalloc(ctx, &dflag, (size_t)1));
        CHK(h2d(ctx, dflag, &hf, 1)); CHK(allreduce(ctx, dflag, 1, 2)); CHK(d2h(ctx, &hf, dflag, 1));
        D.chain_pair = hf != 0 ? 1 : 0;
      }
      D.KH = KH; D.chain_folders = F; D.chain_kw = kw; D.Yimg3p = nullptr;
      if (D.chain_pair) {
        CHK(dalloc(ctx, &D.Yimg3p, (size_t)2 * nctp * D.NS2 * 3 * 512));
        HIPCHK(hipMemsetAsync(D.Yimg3p, 0, (size_t)2 * nctp * D.NS2 * 3 * 1024, ctx->L.stream));
        if (!getenv("HMX_NREP")) {      // 40 000 table entries spread the workers' atomics by themselves; the folders read AND reset every replica on the chain's critical path
          D.nrep = 1;
          for (int i = 0; i < 3; i++) D.Snew_set[i] = ctx->sold_buf[0] + (size_t)2 * D.nb * B * K + (size_t)i * D.nrep * B * K;
        }
      } }
    D.upd_contig = (!ctx->chain_ok && !D.chain_pair && tiles_per_wave >= 4.0) ? 1 : 0;     // launch-per-step path: contiguous tile ranges once a wave has several tiles per block
    ctx->chain_rounds = 0;
    D.p2p_world = 0; D.p2p_rank = ctx->p2p_rank;
    for (int g = 0; g < 8; g++) D.p2p_inbox[g] = ctx->p2p_peer[g]; }
  ctx->invperm_h = invperm; ctx->combo_h = combo_sorted;
  ctx->Zc_head = nullptr; ctx->Yt_head = nullptr; ctx->head_is_stale = false;
  if (ctx->stale_dist) { CHK(dalloc(ctx, &ctx->Zc_head, (size_t)N * D.zs)); CHK(dalloc(ctx, &ctx->Yt_head, (size_t)d * K)); }
  CHK(seq_setup_static(ctx));
  ctx->ran_setup = true;
  return hmx_restart(ctx);
}


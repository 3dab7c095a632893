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
  // order.  Host input goes through the slab pipeline of hmx_api_xfer.inc.
  if (z_location != HMX_DEVICE && xfer_mode() == 2) (void)xfer_ring(ctx->device).ensure();    // (once per process: not part of a matrix's transfer time)
  // (the buffers' first touch by the clears above is allocate_buffers' time, and the first launch of a library kernel in a process loads the
  //  code object -- tens of ms once per process --: neither is the ingest's)
  l_copy(ctx->L, D.Zo, D.Zo, 0); KCHK();
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  const double t_in = now_ms();
  const int f32 = z_dtype == HMX_F32;
  if (z_location == HMX_DEVICE) {
    l_convert_in(ctx->L, Z, f32, D.Zo, D.invperm, (int)N, d, D.zs); KCHK();
    HIPCHK(hipStreamSynchronize(ctx->L.stream));
  } else {
    const size_t cell = (size_t)d * (f32 ? 4 : 8);
    XferPipe pipe;
    hipError_t e = pipe.open(ctx->device, const_cast<void*>(Z), N, cell, ctx->xfer_slab_bytes);
    ctx->timers["ingest_pinned"] = (double)pipe.pinned;
    if (e == hipSuccess) e = xfer_ingest(pipe, ctx->L.stream, Z, N, cell, [&](const void* stage, int64_t s0, int64_t cnt) {
      l_convert_in(ctx->L, stage, f32, D.Zo, D.invperm + s0, (int)cnt, d, D.zs); return hipGetLastError(); });
    if (e != hipSuccess) return fail(ctx, HMX_ERR_DEVICE, hipGetErrorString(e));
  }
  ctx->timers["ingest_Z"] = now_ms() - t_in;
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

// the design of a fit on the host: internal order (cells sorted by level combination) and the static work lists over it
struct Design {
  std::vector<int> start, invperm, combo_sorted;      // first cell of every combination; original -> internal; combination of every internal position
  std::vector<Item> items, aitems, titems, schunks;   // <= ITEM_CELLS / APPLY_CELLS / 16 / SORT_CHUNK cells of one combination each
  std::vector<int> qchunk;                            // [Q + 1] first sort chunk of every combination
};

// level codes, combinations (global presence and level sizes: one all-reduce when sharded), internal order, work lists
static int design_order(hmx_ctx* ctx, int64_t N, const int32_t* phi_i, const int32_t* phi_p, const double* phi_x, Design& G) {
  const int B = ctx->B, C = ctx->C;
  std::vector<int> codes, key;
  std::vector<long long> present;
  CHK(phi_codes(ctx, N, phi_i, phi_p, phi_x, B, C, codes));
  CHK(combo_keys(ctx, N, C, codes, key, present));
  const int64_t P = (int64_t)present.size();
  std::vector<long long> nbcount((size_t)B, 0);
  for (int c = 0; c < C; c++) for (int64_t i = 0; i < N; i++) nbcount[codes[(size_t)c * N + i]]++;
  if (ctx->world > 1 || ctx->comm_force) {
    CallBufs bufs; long long* dtmp; const size_t cnt = (size_t)P + B;
    HIPCHK(bufs.get(&dtmp, cnt));
    std::vector<long long> tmp(present); tmp.insert(tmp.end(), nbcount.begin(), nbcount.end());
    CHK(h2d(ctx, dtmp, tmp.data(), cnt)); CHK(allreduce(ctx, dtmp, (int64_t)cnt, 0)); CHK(d2h(ctx, tmp.data(), dtmp, cnt));
    std::copy(tmp.begin(), tmp.begin() + P, present.begin());
    std::copy(tmp.begin() + P, tmp.end(), nbcount.begin());
  }
  combo_order(ctx, N, C, present, key, G.start, G.invperm, G.combo_sorted);
  ctx->sizes.resize(B); ctx->Pr_b.resize(B);
  for (int b = 0; b < B; b++) { ctx->sizes[b] = (float)nbcount[b]; ctx->Pr_b[b] = ctx->sizes[b] / (float)ctx->N_global; }  // :67
  const auto runs = [&](int q, int cells, std::vector<Item>& out) {
    for (int s = G.start[q]; s < G.start[q + 1]; s += cells) out.push_back({q, s, std::min(cells, G.start[q + 1] - s)}); };
  G.qchunk.assign((size_t)ctx->Q + 1, 0);
  for (int q = 0; q < ctx->Q; q++) {
    runs(q, ITEM_CELLS, G.items); runs(q, APPLY_CELLS, G.aitems); runs(q, 16, G.titems);
    G.qchunk[q] = (int)G.schunks.size(); runs(q, SORT_CHUNK, G.schunks);
  }
  G.qchunk[ctx->Q] = (int)G.schunks.size();
  return 0;
}

// a flag every rank of a sharded run must share: the minimum over the ranks (one MIN all-reduce of `n` words)
static int agree_min(hmx_ctx* ctx, long long* flags, size_t n) {
  CallBufs bufs; long long* dflag;
  HIPCHK(bufs.get(&dflag, n));
  CHK(h2d(ctx, dflag, flags, n)); CHK(allreduce(ctx, dflag, (int64_t)n, 2)); CHK(d2h(ctx, flags, dflag, n));
  return 0;
}

// the launch plan (hmx_plan.h) of this handle's shape, agreed between the ranks, written into ctx->D / ctx
static int plan_device(hmx_ctx* ctx, const Design& G, Plan& P) {
  const Switches sw = read_switches();
  if (ctx->L.grid <= 0) ctx->L.grid = sw.grid;
  Dev& D = ctx->D;
  D = Dev{};
  Shape S;
  S.N = ctx->N; S.N_global = ctx->N_global; S.d = ctx->d; S.K = ctx->K; S.B = ctx->B; S.C = ctx->C; S.Q = ctx->Q;
  S.nb = ctx->nb; S.cells_per_block = ctx->cells_per_block; S.world = ctx->world; S.sharded = ctx->world > 1 || ctx->comm_force;
  (void)hipDeviceGetAttribute(&S.cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
  for (int k = 1; k < ctx->K; k++) S.usig = S.usig && ctx->sigma[k] == ctx->sigma[0];
  S.ridge_arith = ctx->ridge_arith; S.oe_arith = ctx->oe_arith; S.obj_arith = ctx->obj_arith; S.solve_arith = ctx->solve_arith;
  S.tun_wps = ctx->tun_wps; S.tun_tpw = ctx->tun_tpw; S.grid = ctx->L.grid; S.ntitems = (int)G.titems.size();
  P = plan_shape(sw, S);
  if (P.limit) return fail(ctx, HMX_ERR_LIMIT, P.limit);
  // The flags pick the inter-rank PROTOCOL of update_R (in-launch exchange of the persistent chain / one all-reduce per block
  // step): every rank must take the same path, but chain_ok depends on the LOCAL cell count and CU count.  Agree on the minimum
  // -- before anything is derived from the flags (the replica count sizes a per-block all-reduce) -- and then, the wave-pair chain
  // depending on the agreed chain_ok, on the minimum of chain_pair.
  if (S.sharded) { long long hf[2] = {P.chain_ok ? 1 : 0, P.fused_ok ? 1 : 0}; CHK(agree_min(ctx, hf, 2)); P.chain_ok = hf[0] != 0; P.fused_ok = hf[1] != 0; }
  plan_pair(sw, S, P);
  if (S.sharded) { long long hf = P.chain_pair; CHK(agree_min(ctx, &hf, 1)); P.chain_pair = hf != 0 ? 1 : 0; }
  plan_finish(sw, S, P);

  D.n = (int)ctx->N; D.d = ctx->d; D.K = ctx->K; D.B = ctx->B; D.C = ctx->C; D.Q = ctx->Q; D.B0 = ctx->B_vec[0]; D.nb = ctx->nb;
  for (int c = 0; c < 4; c++) D.cov_end[c] = c < ctx->C ? ctx->cov_bounds[c] : ctx->B;
  D.KP = P.KP; D.zs = P.zs; D.NCT = P.NCT; D.NQ = P.NQ; D.NT4 = P.NT4; D.tail = P.tail; D.NS = P.NS; D.NS2 = P.NS2;
  D.wNQ = P.wNQ; D.wNT4 = P.wNT4; D.wtail = P.wtail; D.wNS = P.wNS;
  D.moe_mfma = P.moe_mfma; D.dot_bf = P.dot_bf; D.usig = P.usig; D.rvec = P.rvec; D.pen_lds = P.pen_lds;
  D.upd_wps = P.upd_wps; D.upd_threads = P.upd_threads; D.upd_maxblocks = P.upd_maxblocks; D.upd_tpw = P.upd_tpw;
  D.static_maxblocks = P.static_maxblocks; D.oldsum_stream = P.oldsum_stream; D.need_lorder = P.need_lorder;
  D.nwmax = P.nwmax; D.objslots = P.objslots; D.qmask = P.qmask; D.npad = P.npad; D.nrep = P.nrep; D.upd_contig = P.upd_contig;
  D.st_KH = P.st_KH; D.st_halves = P.st_halves; D.st_dma = P.st_dma; D.st_cpw = P.st_cpw; D.st_nwg = P.st_nwg;
  D.chain_pair = P.chain_pair; D.KH = P.KH; D.chain_folders = P.chain_folders; D.chain_kw = P.chain_kw;
  D.r_store = 1;
  D.solve_lds = (!sw.solve_lds_off && !S.sharded && P.solve_on_device && !ctx->ridge_arith && !ctx->solve_arith) ? 1 : 0;
  ctx->n_launches = ctx->n_event_records = ctx->n_gate_records = 0; ctx->L.count = &ctx->n_launches;
  D.chain_wps = 2;      // (the 3- / 4-waves-per-SIMD chain variants and the in-chain gathering of the old contributions lost rounds 2 and 3: removed in round 5)
  D.nchunks = (int)G.schunks.size(); D.nitems = (int)G.items.size(); D.naitems = (int)G.aitems.size(); D.ntitems = (int)G.titems.size();
  D.p2p_world = 0; D.p2p_rank = ctx->p2p_rank;
  for (int g = 0; g < 8; g++) D.p2p_inbox[g] = ctx->p2p_peer[g];
  ctx->r_store_always = P.r_store_always; ctx->carry_ok = P.carry_ok; ctx->shuf_inv = P.shuf_inv; ctx->solve_on_device = P.solve_on_device;
  ctx->fused_ok = P.fused_ok; ctx->chain_ok = P.chain_ok; ctx->chain_wgs = P.chain_wgs;
  ctx->carried_rounds = 0; ctx->chain_rounds = 0; std::fill(ctx->tile_seen, ctx->tile_seen + 5, false); ctx->y_on_device = false; ctx->solve_pending = false;
  ctx->fold_impl = sw.fold_impl; ctx->ledger.reset(); ctx->round_seen = false;
  return 0;
}

// one order set of a round's shuffle (lorder + lpair share a buffer: one 0xFF memset per round)
static int alloc_sort_set(hmx_ctx* ctx, const Plan& P, hmx_ctx::SortSet& t) {
  const Dev& D = ctx->D;
  const size_t N = (size_t)D.n, bins = (size_t)P.nkeys * D.Q, hist = (size_t)P.nkeys * D.nchunks;
  CHK(dalloc(ctx, &t.blk, N)); CHK(dalloc(ctx, &t.lorder, (size_t)3 * D.npad + 2)); t.lpair = reinterpret_cast<int2*>(t.lorder + (((size_t)D.npad + 1) & ~(size_t)1));
  CHK(dalloc(ctx, &t.lcombo, (size_t)D.npad)); CHK(dalloc(ctx, &t.binoff, bins + 1)); CHK(dalloc(ctx, &t.boff, (size_t)D.nb + 1));
  CHK(dalloc(ctx, &t.counts, hist)); CHK(dalloc(ctx, &t.offs, hist)); CHK(dalloc(ctx, &t.blkv, N)); CHK(dalloc(ctx, &t.bincnt, bins));
  return 0;
}

// every device buffer of the handle, sized by the plan; buffers that must start zero are cleared here
static int alloc_device(hmx_ctx* ctx, const Plan& P, const Design& G) {
  Dev& D = ctx->D;
  hipStream_t st = ctx->L.stream;
  const size_t N = (size_t)D.n, BK = (size_t)D.B * D.K, M = (size_t)D.B + 1;
  const int d = D.d, K = D.K, B = D.B, C = D.C, Q = D.Q;
  // cells and small tables
  CHK(dalloc(ctx, &D.Zo, N * D.zs)); CHK(dalloc(ctx, &D.Zc, N * D.zs)); CHK(dalloc(ctx, &D.R, (N + 1) * K));   // + one dummy row (target of masked stores)
  CHK(dalloc(ctx, &D.perm, N)); CHK(dalloc(ctx, &D.invperm, N)); CHK(dalloc(ctx, &D.combo, N)); CHK(dalloc(ctx, &D.qlev, (size_t)Q * C));
  CHK(dalloc(ctx, &D.Yt, (size_t)d * K)); CHK(dalloc(ctx, &D.Ycur, (size_t)d * K));
  CHK(dalloc(ctx, &D.Yimg, (size_t)D.NQ * D.NS * 256)); HIPCHK(hipMemsetAsync(D.Yimg, 0, (size_t)D.NQ * D.NS * 1024, st));
  CHK(dalloc(ctx, &D.Yimg3, (size_t)D.NCT * D.NS2 * 3 * 512)); HIPCHK(hipMemsetAsync(D.Yimg3, 0, (size_t)D.NCT * D.NS2 * 3 * 1024, st));
  if (D.chain_pair) { const size_t n = (size_t)2 * ((D.KH + 15) / 16) * D.NS2 * 3 * 512; CHK(dalloc(ctx, &D.Yimg3p, n)); HIPCHK(hipMemsetAsync(D.Yimg3p, 0, 2 * n, st)); }
  CHK(dalloc(ctx, &D.sigma, (size_t)K)); CHK(dalloc(ctx, &D.ce, (size_t)K)); CHK(dalloc(ctx, &D.cl, (size_t)K));
  CHK(dalloc(ctx, &D.theta, (size_t)B)); CHK(dalloc(ctx, &D.Pr_b, (size_t)B)); CHK(dalloc(ctx, &D.sizes, (size_t)B));
  // update_R tables.  Sold_fx [nb][B][K] twice and the three rotating replica sets of the fused path share one buffer: one memset per round
  CHK(dalloc(ctx, &D.O_fx, BK)); CHK(dalloc(ctx, &D.Snew_fx, D.nrep * BK)); CHK(dalloc(ctx, &D.O_alt, BK)); CHK(dalloc(ctx, &D.Snew_alt, D.nrep * BK));
  { long long* s3; CHK(dalloc(ctx, &s3, 2 * D.nb * BK + 3 * D.nrep * BK)); D.Sold_fx = s3;
    ctx->sold_buf[0] = s3; ctx->sold_buf[1] = s3 + D.nb * BK;
    for (int i = 0; i < 3; i++) D.Snew_set[i] = s3 + 2 * D.nb * BK + i * D.nrep * BK; }
  CHK(dalloc(ctx, &D.objpart, (size_t)2 * D.objslots * D.nwmax)); CHK(dalloc(ctx, &D.objrow, (size_t)2 * D.objslots));
  if (const char* e = getenv("HMX_TRACE")) if (atoi(e)) { CHK(dalloc(ctx, &D.trace, (size_t)16 * D.nwmax)); HIPCHK(hipMemsetAsync(D.trace, 0, sizeof(unsigned long long) * 16 * (size_t)D.nwmax, st)); }
  CHK(dalloc(ctx, &D.pen, BK)); CHK(dalloc(ctx, &D.obj, (size_t)8));
  CHK(dalloc(ctx, &D.tail_ticket, (size_t)1)); CHK(dalloc(ctx, &D.pen_g, BK)); CHK(dalloc(ctx, &D.chain_ctl, (size_t)8 * D.nb + 24)); CHK(dalloc(ctx, &D.chain_dbg, (size_t)64));
  HIPCHK(hipMemsetAsync(D.tail_ticket, 0, sizeof(int), st)); HIPCHK(hipMemsetAsync(D.chain_dbg, 0, sizeof(unsigned long long) * 64, st));
  HIPCHK(hipMemsetAsync(D.pen_g, 0, sizeof(unsigned long long) * BK, st)); HIPCHK(hipMemsetAsync(D.chain_ctl, 0, sizeof(int) * ((size_t)8 * D.nb + 24), st));
  HIPCHK(hipMemsetAsync(D.O_fx, 0, sizeof(long long) * BK, st)); HIPCHK(hipMemsetAsync(D.Snew_fx, 0, sizeof(long long) * D.nrep * BK, st));
  HIPCHK(hipMemsetAsync(D.O_alt, 0, sizeof(long long) * BK, st)); HIPCHK(hipMemsetAsync(D.Snew_alt, 0, sizeof(long long) * D.nrep * BK, st));
  HIPCHK(hipMemsetAsync(D.objpart, 0, sizeof(double) * 2 * (size_t)D.objslots * D.nwmax, st)); HIPCHK(hipMemsetAsync(D.obj, 0, sizeof(double) * 8, st));
  // a round's shuffle: four order sets (set 0 is the one Dev starts on), static sort chunks
  for (int i = 0; i < 4; i++) CHK(alloc_sort_set(ctx, P, ctx->sets[i]));
  { const hmx_ctx::SortSet& t = ctx->sets[0];
    D.blk = t.blk; D.lorder = t.lorder; D.lpair = t.lpair; D.lcombo = t.lcombo; D.boff = t.boff; D.binoff = t.binoff; D.counts = t.counts; D.offs = t.offs; D.blkv = t.blkv; D.bincnt = t.bincnt; }
  CHK(dalloc(ctx, &D.schunks, G.schunks.size())); CHK(dalloc(ctx, &D.qchunk, (size_t)Q + 1));
  if (ctx->shuf_inv) {
    const size_t bins = (size_t)P.nkeys * Q, parts = (size_t)shuffle_parts((uint64_t)ctx->N_global, D.nb, ctx->cells_per_block);
    for (int i = 0; i < 4; i++) { CHK(dalloc(ctx, &ctx->posr[i], (size_t)ctx->N_global)); CHK(dalloc(ctx, &ctx->shuf_partcnt[i], bins * parts));
      CHK(dalloc(ctx, &ctx->shuf_binacc[i], bins)); HIPCHK(hipMemsetAsync(ctx->shuf_binacc[i], 0, sizeof(int) * bins, st)); }
  }
  // static work lists, ridge correction
  CHK(dalloc(ctx, &D.items, G.items.size())); CHK(dalloc(ctx, &D.aitems, G.aitems.size())); CHK(dalloc(ctx, &D.titems, G.titems.size())); CHK(dalloc(ctx, &D.qstart, (size_t)Q + 1));
  CHK(dalloc(ctx, &D.Sq, (size_t)Q * d * K)); CHK(dalloc(ctx, &D.nq, (size_t)Q * K)); CHK(dalloc(ctx, &D.S0, (size_t)K * d)); CHK(dalloc(ctx, &D.n0, (size_t)K));
  CHK(dalloc(ctx, &D.Wq, (size_t)Q * K * d)); CHK(dalloc(ctx, &D.Wimg, D.moe_mfma ? (size_t)Q * D.wNQ * D.wNS * 256 : 1));
  CHK(dalloc(ctx, &D.solve_err, (size_t)1)); HIPCHK(hipMemsetAsync(D.solve_err, 0, sizeof(int), st));
  if (ctx->solve_on_device) {
    CHK(dalloc(ctx, &ctx->sv_cov, (size_t)K * M * M)); CHK(dalloc(ctx, &ctx->sv_rhs, (size_t)K * d * M)); CHK(dalloc(ctx, &ctx->sv_Wall, (size_t)K * d * M));
    CHK(dalloc(ctx, &ctx->sv_mrows, (size_t)K)); CHK(dalloc(ctx, &ctx->sv_flags, (size_t)K)); CHK(dalloc(ctx, &ctx->sv_lambda, M)); CHK(dalloc(ctx, &ctx->sv_cov_bounds, (size_t)C));
    HIPCHK(hipMemsetAsync(ctx->sv_flags, 0, sizeof(int) * (size_t)K, st)); HIPCHK(hipMemsetAsync(ctx->sv_mrows, 0, sizeof(int) * (size_t)K, st));
  }
  // kmeans init
  CHK(dalloc(ctx, &D.km_gcells, (size_t)K)); CHK(dalloc(ctx, &D.km_rows, (size_t)K * d)); CHK(dalloc(ctx, &D.km_excl, (size_t)K));
  CHK(dalloc(ctx, &D.seedmin, (size_t)K)); CHK(dalloc(ctx, &D.lsum, (size_t)K * d + K)); D.lcnt = reinterpret_cast<unsigned long long*>(D.lsum + (size_t)K * d); CHK(dalloc(ctx, &D.ynorm, (size_t)K));
  ctx->Zc_head = nullptr; ctx->Yt_head = nullptr; ctx->head_is_stale = false;
  if (ctx->stale_dist) { CHK(dalloc(ctx, &ctx->Zc_head, N * D.zs)); CHK(dalloc(ctx, &ctx->Yt_head, (size_t)d * K)); }
  HIPCHK(hipMemsetAsync(D.R, 0, sizeof(float) * N * K, st)); HIPCHK(hipMemsetAsync(D.Zo, 0, sizeof(float) * N * D.zs, st));
  HIPCHK(hipMemsetAsync(D.Zc, 0, sizeof(float) * N * D.zs, st)); HIPCHK(hipMemsetAsync(D.Wq, 0, sizeof(float) * (size_t)Q * K * d, st));
  return 0;
}

// deterministic statistics pass (k_moe_stats_q): one partial slot per (workgroup, combination met) -- known here because the tiles are
// listed by combination -- and, per combination, its slots in ascending (= cell) order
static int upload_stats_slots(hmx_ctx* ctx, const Design& G) {
  Dev& D = ctx->D;
  const int nt = D.ntitems, Q = D.Q;
  std::vector<int> slot0((size_t)D.st_nwg), qptr((size_t)Q + 1, 0), qslots;
  std::vector<std::vector<int>> byq((size_t)Q);
  int nslots = 0;
  for (int w = 0; w < D.st_nwg; w++) {
    slot0[w] = nslots;
    int last = -1;
    for (int t = w * D.st_cpw; t < std::min(nt, (w + 1) * D.st_cpw); t++) if (G.titems[t].q != last) { last = G.titems[t].q; byq[(size_t)last].push_back(nslots++); }
  }
  qslots.reserve((size_t)nslots);
  for (int q = 0; q < Q; q++) { qptr[q] = (int)qslots.size(); qslots.insert(qslots.end(), byq[q].begin(), byq[q].end()); }
  qptr[Q] = (int)qslots.size();
  CHK(dalloc(ctx, &D.st_part, (size_t)std::max(nslots, 1) * ((size_t)D.K * D.d + D.K))); CHK(dalloc(ctx, &D.st_slot0, slot0.size()));
  CHK(dalloc(ctx, &D.st_qptr, qptr.size())); CHK(dalloc(ctx, &D.st_qslots, std::max<size_t>(qslots.size(), 1)));
  CHK(h2d(ctx, D.st_slot0, slot0.data(), slot0.size())); CHK(h2d(ctx, D.st_qptr, qptr.data(), qptr.size()));
  if (!qslots.empty()) CHK(h2d(ctx, D.st_qslots, qslots.data(), qslots.size()));
  return 0;
}

// the tables that do not change during a fit: order, design, parameters, work lists
static int upload_static(hmx_ctx* ctx, const Design& G) {
  Dev& D = ctx->D;
  const size_t N = (size_t)D.n, K = (size_t)D.K, B = (size_t)D.B;
  CHK(h2d(ctx, D.perm, ctx->perm.data(), N)); CHK(h2d(ctx, D.invperm, G.invperm.data(), N));
  CHK(h2d(ctx, D.combo, G.combo_sorted.data(), N)); CHK(h2d(ctx, D.qlev, ctx->qlev.data(), ctx->qlev.size()));
  CHK(h2d(ctx, D.qstart, G.start.data(), (size_t)D.Q + 1)); CHK(h2d(ctx, D.sizes, ctx->sizes.data(), B));
  CHK(h2d(ctx, D.sigma, ctx->sigma.data(), K)); CHK(h2d(ctx, D.theta, ctx->theta.data(), B)); CHK(h2d(ctx, D.Pr_b, ctx->Pr_b.data(), B));
  { std::vector<float> ce(K), cl(K);
    for (size_t k = 0; k < K; k++) { ce[k] = -1.44269504088896341f / ctx->sigma[k]; cl[k] = ctx->sigma[k] * 0.693147180559945309f; }
    CHK(h2d(ctx, D.ce, ce.data(), K)); CHK(h2d(ctx, D.cl, cl.data(), K)); }
  CHK(h2d(ctx, D.schunks, G.schunks.data(), G.schunks.size())); CHK(h2d(ctx, D.qchunk, G.qchunk.data(), G.qchunk.size()));
  CHK(h2d(ctx, D.items, G.items.data(), G.items.size())); CHK(h2d(ctx, D.aitems, G.aitems.data(), G.aitems.size())); CHK(h2d(ctx, D.titems, G.titems.data(), G.titems.size()));
  if (ctx->solve_on_device) {
    if (!ctx->lambda_estimation) CHK(h2d(ctx, ctx->sv_lambda, ctx->lambda.data(), B + 1));
    CHK(h2d(ctx, ctx->sv_cov_bounds, ctx->cov_bounds.data(), (size_t)D.C));
  }
  if (D.st_dma) CHK(upload_stats_slots(ctx, G));
  return 0;
}

// argument checks of hmx_setup_ex, in the order their errors are documented
static int check_setup_args(hmx_ctx* ctx, const void* Z, int32_t z_dtype, int32_t z_location, int64_t N, int32_t d, bool null_arg, int32_t B,
                            int32_t n_lambda, int32_t K, int32_t C) {
  if (!ctx) return HMX_ERR_ARG;
  if (ctx->query_done) return fail(ctx, HMX_ERR_STATE, "this handle mapped a query: create a new handle for a fit");
  if ((z_dtype != HMX_F64 && z_dtype != HMX_F32) || (z_location != HMX_HOST && z_location != HMX_DEVICE))
    return fail(ctx, HMX_ERR_ARG, "bad dtype / location of Z");
  ctx->err.clear(); ctx->warn.clear();
  if (!Z || null_arg) return fail(ctx, HMX_ERR_ARG, "null argument");
  if (N <= 0 || d <= 0 || K <= 0 || B <= 0 || C <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (d > 128 || K > 256 || C > 15) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: d <= 128, K <= 256, covariates <= 15");
  if (N > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 cells per GPU shard");
  if ((ctx->ridge_arith || ctx->oe_arith || ctx->obj_arith || ctx->solve_arith) && (ctx->world > 1 || ctx->comm_force))
    return fail(ctx, HMX_ERR_ARG, "the reference-arithmetic modes (ridge_arith / oe_arith / obj_arith / solve_arith) run on one GPU");
  if (ctx->world <= 1) { ctx->N_global = N; ctx->goff = 0; }
  if (ctx->N_global > 4000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 4e9 cells in total");
  if (ctx->N_global < 6) return fail(ctx, HMX_ERR_TOO_FEW, "Refusing to run with less than 6 cells");
  if (n_lambda != 1 && n_lambda != B + 1) return fail(ctx, HMX_ERR_ARG, "lambda must have length B+1 (or be the single value -1)");
  return 0;
}

// the device of the handle, its stream; whatever an earlier setup of the handle left is released
static int open_device(hmx_ctx* ctx) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(ctx, HMX_ERR_DEVICE, "no HIP device available: libharmony_mi355x has no CPU fallback");
  if (ctx->device < 0) { int cur = 0; (void)hipGetDevice(&cur); ctx->device = cur; }
  HIPCHK(hipSetDevice(ctx->device));
  free_all(ctx);
  if (!ctx->L.stream) { HIPCHK(hipStreamCreateWithFlags(&ctx->L.stream, hipStreamNonBlocking)); ctx->own_stream = true; }
  return 0;
}

int hmx_setup_ex(hmx_ctx* ctx, const void* Z, int32_t z_dtype, int32_t z_location, int64_t N, int32_t d, const int32_t* phi_i,
                 const int32_t* phi_p, const double* phi_x, int32_t B, const double* sigma, const double* theta,
                 const double* lambda, int32_t n_lambda, double alpha, int32_t max_iter_kmeans, double epsilon_kmeans,
                 double epsilon_harmony, int32_t K, double block_size, const int32_t* B_vec, int32_t C, double cutoff,
                 int32_t verbose) {
  CHK(check_setup_args(ctx, Z, z_dtype, z_location, N, d, !phi_i || !phi_p || !sigma || !theta || !lambda || !B_vec, B, n_lambda, K, C));
  CHK(open_device(ctx));
  // the problem as the reference's setup stores it
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

  Design G; Plan P;
  CHK(design_order(ctx, N, phi_i, phi_p, phi_x, G));
  CHK(plan_device(ctx, G, P));
  CHK(alloc_device(ctx, P, G));
  CHK(upload_static(ctx, G));
  CHK(ingest_Z(ctx, Z, z_dtype, z_location, N, d));
  ctx->W.assign((size_t)(B + 1) * d, 0.f); ctx->W_rows = B + 1;  // allocate_buffers :127
  ctx->Y.assign((size_t)d * K, 0.f);
  ctx->invperm_h = std::move(G.invperm); ctx->combo_h = std::move(G.combo_sorted);
  CHK(seq_setup_static(ctx));
  ctx->ran_setup = true;
  return hmx_restart(ctx);
}

// hmx_api_p2p.inc -- part of hmx_api.cpp (included there, ONE translation unit): peer-to-peer block chain: inbox export / connect / self-test / enable
// ---- peer-to-peer block chain ------------------------------------------------------------------------------------------
int hmx_p2p_export(hmx_ctx* ctx, uint8_t* handle_out) {
  if (!ctx || !handle_out) return ctx ? fail(ctx, HMX_ERR_ARG, "null handle buffer") : HMX_ERR_ARG;
  static_assert(sizeof(hipIpcMemHandle_t) == HMX_P2P_HANDLE_BYTES, "HIP IPC handle size");
  if (ctx->device < 0) { int cur = 0; (void)hipGetDevice(&cur); ctx->device = cur; }
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx->p2p_self) {
    // fine-grained device memory: peers write it over xGMI while this GPU's folder polls it (coarse-grained memory is only
    // coherent at kernel boundaries).  HMX_P2P_MEM=uncached selects hipDeviceMallocUncached instead.
    const char* m = getenv("HMX_P2P_MEM");
    const unsigned flags = (m && std::string(m) == "uncached") ? hipDeviceMallocUncached : hipDeviceMallocFinegrained;
    void* p = nullptr;
    HIPCHK(hipExtMallocWithFlags(&p, P2P_INBOX_GRANULES * sizeof(unsigned long long), flags));
    HIPCHK(hipMemset(p, 0, P2P_INBOX_GRANULES * sizeof(unsigned long long)));
    HIPCHK(hipDeviceSynchronize());
    ctx->p2p_self = (unsigned long long*)p;
  }
  hipIpcMemHandle_t h;
  HIPCHK(hipIpcGetMemHandle(&h, ctx->p2p_self));
  std::memcpy(handle_out, &h, sizeof(h));
  return 0;
}
int hmx_p2p_connect(hmx_ctx* ctx, int32_t rank, int32_t world, const uint8_t* handles) {
  if (!ctx || !handles) return ctx ? fail(ctx, HMX_ERR_ARG, "null handle table") : HMX_ERR_ARG;
  if (world < 2 || world > 8 || rank < 0 || rank >= world) return fail(ctx, HMX_ERR_ARG, "the peer-to-peer chain takes 2..8 ranks");
  if (!ctx->p2p_self) return fail(ctx, HMX_ERR_STATE, "hmx_p2p_export first");
  HIPCHK(hipSetDevice(ctx->device));
  for (int g = 0; g < world; g++) {
    if (g == rank) { ctx->p2p_peer[g] = ctx->p2p_self; continue; }
    if (ctx->p2p_peer[g]) continue;
    hipIpcMemHandle_t h; std::memcpy(&h, handles + (size_t)g * HMX_P2P_HANDLE_BYTES, sizeof(h));
    void* p = nullptr;
    hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) { (void)hipGetLastError(); ctx->p2p_note = std::string("hipIpcOpenMemHandle: ") + hipGetErrorString(e); return fail(ctx, HMX_ERR_COMM, ctx->p2p_note); }
    ctx->p2p_peer[g] = (unsigned long long*)p;
  }
  ctx->p2p_rank = rank; ctx->p2p_world = world; ctx->p2p_note = "connected, not tested";
  return 0;
}
int hmx_p2p_selftest(hmx_ctx* ctx) {
  if (!ctx || ctx->p2p_world < 2) return ctx ? fail(ctx, HMX_ERR_STATE, "hmx_p2p_connect first") : HMX_ERR_ARG;
  HIPCHK(hipSetDevice(ctx->device));
  if (!ctx->L.stream) { HIPCHK(hipStreamCreateWithFlags(&ctx->L.stream, hipStreamNonBlocking)); ctx->own_stream = true; }
  if (!ctx->p2p_result) HIPCHK(hipMalloc((void**)&ctx->p2p_result, 2 * sizeof(int)));
  Dev T{};
  T.p2p_world = ctx->p2p_world; T.p2p_rank = ctx->p2p_rank;
  for (int g = 0; g < 8; g++) T.p2p_inbox[g] = ctx->p2p_peer[g];
  // tags of the test live above 2^31 (the chain's stay below 2^30 + 64), 128 per test
  l_p2p_selftest(ctx->L, T, 0x80000000u + ((++ctx->p2p_tests) & 0xffffffu) * 128u, ctx->p2p_result); KCHK();
  int res[2] = {-1, 0};
  HIPCHK(hipMemcpyAsync(res, ctx->p2p_result, sizeof(res), hipMemcpyDeviceToHost, ctx->L.stream));
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  if (res[0] != 0) {
    ctx->p2p_note = "self-test: " + std::to_string(res[0]) + " wrong or missing values";
    return fail(ctx, HMX_ERR_COMM, "peer-to-peer " + ctx->p2p_note);
  }
  ctx->p2p_exchange_us = (double)res[1] / 100.0 / 63.0;    // 100 MHz ticks over the 63 steps after the first
  char buf[96]; snprintf(buf, sizeof(buf), "self-test passed (%.2f us per exchange step)", ctx->p2p_exchange_us);
  ctx->p2p_note = buf;
  return 0;
}
int hmx_p2p_enable(hmx_ctx* ctx, int32_t on) {
  if (!ctx) return HMX_ERR_ARG;
  if (on && ctx->p2p_world < 2) return fail(ctx, HMX_ERR_STATE, "hmx_p2p_connect first");
  ctx->p2p_on = on != 0;
  if (on && ctx->p2p_note.find("passed") == std::string::npos) ctx->p2p_note = "on (self-test not run)";
  return 0;
}
// with the built-in communicator the whole bootstrap is automatic; every failure just leaves the per-block collectives in place
static void p2p_auto(hmx_ctx* ctx, RcclApi* api, int rank, int world) {
  const char* e = getenv("HMX_P2P");
  if ((e && std::string(e) == "0") || world < 2 || world > 8 || !api->AllGather) { ctx->p2p_note = "off"; return; }
  auto give_up = [&](const std::string& why) { ctx->p2p_note = why; ctx->p2p_on = false; ctx->err.clear(); };
  if (!ctx->L.stream) { if (hipStreamCreateWithFlags(&ctx->L.stream, hipStreamNonBlocking) != hipSuccess) return give_up("no stream"); ctx->own_stream = true; }
  uint8_t mine[HMX_P2P_HANDLE_BYTES] = {};
  long long ok = hmx_p2p_export(ctx, mine) == 0 ? 1 : 0;    // (a rank that cannot export still takes part in the collectives)
  CallBufs bufs; uint8_t* dev = nullptr; long long* flag = nullptr;
  std::vector<uint8_t> all((size_t)world * HMX_P2P_HANDLE_BYTES);
  if (bufs.get(&dev, all.size()) != hipSuccess || bufs.get(&flag, 1) != hipSuccess) return give_up("hipMalloc");
  bool comm_ok = hipMemcpyAsync(dev + (size_t)rank * HMX_P2P_HANDLE_BYTES, mine, sizeof(mine), hipMemcpyHostToDevice, ctx->L.stream) == hipSuccess &&
                 api->AllGather(dev + (size_t)rank * HMX_P2P_HANDLE_BYTES, dev, HMX_P2P_HANDLE_BYTES, ncclInt8, ctx->comm, ctx->L.stream) == ncclSuccess &&
                 hipMemcpyAsync(all.data(), dev, all.size(), hipMemcpyDeviceToHost, ctx->L.stream) == hipSuccess &&
                 hipStreamSynchronize(ctx->L.stream) == hipSuccess;
  auto agree = [&]() {     // min over the ranks of `ok`
    if (!comm_ok) return;
    comm_ok = hipMemcpyAsync(flag, &ok, 8, hipMemcpyHostToDevice, ctx->L.stream) == hipSuccess &&
              api->AllReduce(flag, flag, 1, ncclInt64, ncclMin, ctx->comm, ctx->L.stream) == ncclSuccess &&
              hipMemcpyAsync(&ok, flag, 8, hipMemcpyDeviceToHost, ctx->L.stream) == hipSuccess &&
              hipStreamSynchronize(ctx->L.stream) == hipSuccess;
  };
  agree();                                                                       // everyone exported (also a barrier)
  if (comm_ok && ok) { ok = hmx_p2p_connect(ctx, rank, world, all.data()) == 0 ? 1 : 0; agree(); }     // everyone connected
  if (comm_ok && ok) { ok = hmx_p2p_selftest(ctx) == 0 ? 1 : 0; agree(); }                             // everyone heard everyone
  if (!comm_ok) return give_up("bootstrap collectives failed");
  if (!ok) return give_up(ctx->p2p_note.empty() ? "a rank failed" : ctx->p2p_note + " (on some rank)");
  (void)hmx_p2p_enable(ctx, 1);
}
int hmx_set_stream(hmx_ctx* ctx, void* s) {
  if (!ctx) return HMX_ERR_ARG;
  if ((hipStream_t)s == ctx->L.stream) return 0;
  if (ctx->obj_unrecorded && ctx->obj_event && ctx->L.stream) { (void)hipEventRecord(ctx->obj_event, ctx->L.stream); ctx->n_event_records++; ctx->obj_unrecorded = false; }      // (the slots were written on the old stream)
  chain_gate_release(ctx);
  if (ctx->own_stream && ctx->L.stream) (void)hipStreamDestroy(ctx->L.stream);
  ctx->L.stream = (hipStream_t)s; ctx->own_stream = false;
  return 0;
}
int hmx_set_abort_poll(hmx_ctx* ctx, int (*poll)(void*), void* user) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->poll = poll; ctx->poll_user = user;
  return 0;
}
// probes of the R-compatible stream (no device needed): n uniforms after set.seed(seed); arma::shuffle(0..N-1) after set.seed(seed)
void hmx_r_runif(uint32_t seed, int32_t n, double* out) { hmx::RRng r; r.set_seed(seed); for (int i = 0; i < n; i++) out[i] = r.unif_rand(); }
void hmx_r_shuffle(uint32_t seed, int64_t N, int64_t* out) {
  hmx::RRng r; r.set_seed(seed);
  std::vector<int64_t> o; r.arma_shuffle(N, o);
  std::copy(o.begin(), o.end(), out);
}
void hmx_mt19937_by_array(const uint32_t* key, int32_t len, int32_t n, uint32_t* out) {   // MT19937's published known-answer vector
  hmx::RRng r; r.mt_init_by_array(key, len);
  for (int i = 0; i < n; i++) out[i] = r.genrand_int32();
}
int hmx_set_uniform_source(hmx_ctx* ctx, double (*unif_rand)(void*), void* user) {
  if (!ctx) return HMX_ERR_ARG;
  ctx->rrng.set_source(unif_rand, user);
  return 0;
}
int hmx_push_update_order(hmx_ctx* ctx, const int64_t* order) {
  if (!ctx || !ctx->ran_setup) return ctx ? fail(ctx, HMX_ERR_STATE, "setup first") : HMX_ERR_ARG;
  if (!order) return fail(ctx, HMX_ERR_ARG, "null update_order");
  {  // must be a permutation of 0..N_global-1: prepare_round indexes a position table with these values
    std::vector<bool> seen((size_t)ctx->N_global, false);
    for (int64_t p = 0; p < ctx->N_global; p++) {
      const int64_t v = order[p];
      if (v < 0 || v >= ctx->N_global || seen[(size_t)v]) return fail(ctx, HMX_ERR_ARG, "update_order is not a permutation of 0..N-1");
      seen[(size_t)v] = true;
    }
  }
  ctx->injected.emplace_back(order, order + ctx->N_global);
  return 0;
}

int hmx_set_int(hmx_ctx* ctx, const char* field, int64_t v) {
  if (!ctx || !field) return HMX_ERR_ARG;
  const std::string f(field);
  if (f == "max_iter_kmeans") ctx->max_iter_kmeans = (int)v;
  else if (f == "seed") { ctx->seed = (uint64_t)v; ctx->rrng_seeded = false; }
  else if (f == "rng") { if (v != 0 && v != 1) return fail(ctx, HMX_ERR_ARG, "rng: 0 (counter-based) or 1 (R-compatible)"); ctx->rng_mode = (int)v; ctx->rrng_seeded = false; }
  else if (f == "ridge_arith" || f == "oe_arith" || f == "obj_arith" || f == "solve_arith" || f == "ref_arith") {
    // "ref_arith" = 2 (round 6): the reference's accumulators where they MOVE the result -- the objective's my_accu sums (they decide the iteration counts), the
    // ridge statistics and the inverse -- with exact O / E tables: 4e-5 .. 6e-5 from the all-groups mode at 1M .. 2M cells (inside north_star's 1e-4), at a bit over
    // half its time, because update_R then runs in the persistent block chain (DESIGN 2.2)
    if (v != 0 && v != 1 && !(f == "ref_arith" && v == 2)) return fail(ctx, HMX_ERR_ARG, f + ": 0 (exact accumulators) or 1 (the reference's fp32 operation order); ref_arith: also 2 (all groups but the O / E tables)");
    if (ctx->ran_setup) return fail(ctx, HMX_ERR_STATE, f + " must be set before setup");
    if (f == "ridge_arith" || f == "ref_arith") ctx->ridge_arith = v ? 1 : 0;
    if (f == "oe_arith" || f == "ref_arith") ctx->oe_arith = (v == 1) ? 1 : 0;
    if (f == "obj_arith" || f == "ref_arith") ctx->obj_arith = v ? 1 : 0;
    if (f == "solve_arith" || f == "ref_arith") ctx->solve_arith = v ? 1 : 0;
  }
  else if (f == "stale_dist") { if (ctx->ran_setup) return fail(ctx, HMX_ERR_STATE, "stale_dist must be set before setup"); ctx->stale_dist = v != 0; }
  else if (f == "seq_passes") { if (v < 2 || v > 64) return fail(ctx, HMX_ERR_ARG, "seq_passes: 2..64"); ctx->seq_passes = (int)v; if (ctx->seq_max_passes < (int)v) ctx->seq_max_passes = (int)v; }
  else if (f == "seq_warm_passes") { if (v < 1 || v > 64) return fail(ctx, HMX_ERR_ARG, "seq_warm_passes: 1..64"); ctx->seq_warm_passes = (int)v; }
  else if (f == "seq_stats") ctx->seq_stats = v != 0;
  else if (f == "seq_fused") { ctx->obj_fused = (int)(v & 1); ctx->ridge_kl = (int)((v >> 2) & 1); ctx->obj_dist_cache = (int)((v >> 3) & 1); }      // round-6 forms, default all on (13): bit 0 the objective's chains in one launch; bit 2 the ridge pass with lane = cluster (0: the round-5 kernels); bit 3 dist_mat kept over the rounds of a cluster_cpp call
  else if (f == "seq_tol_ppb") { if (v < 0 || v > 100000000) return fail(ctx, HMX_ERR_ARG, "seq_tol_ppb: 0 .. 1e8 (parts per billion)"); ctx->seq_tol = 1e-9 * (double)v; }
  else if (f == "seq_strict") { ctx->seq_strict = v != 0; if (v && ctx->seq_max_passes < 64) ctx->seq_max_passes = 64; }
  else if (f == "seq_max_passes") { if (v < 2 || v > 256) return fail(ctx, HMX_ERR_ARG, "seq_max_passes: 2..256"); ctx->seq_max_passes = (int)v; }
  else if (f == "project_slab_bytes") { if (v < 0) return fail(ctx, HMX_ERR_ARG, "project_slab_bytes: 0 (the default) or a positive byte count"); ctx->project_slab_bytes = v; }
  else if (f == "xfer_slab_bytes") { if (v < 0) return fail(ctx, HMX_ERR_ARG, "xfer_slab_bytes: 0 (the default) or a positive byte count"); ctx->xfer_slab_bytes = v; }
  else if (f == "ranksum_list_bytes") { if (v < 0) return fail(ctx, HMX_ERR_ARG, "ranksum_list_bytes: 0 (the default) or a positive byte count"); ctx->ranksum_list_bytes = v; }
  else if (f == "louvain_short_cap") { if (v < -1) return fail(ctx, HMX_ERR_ARG, "louvain_short_cap: -1 (the default) or an entry count"); ctx->louvain_short_cap = v; }
  else if (f == "umap_short_cap") { if (v < -1 || v > 2147483647ll) return fail(ctx, HMX_ERR_ARG, "umap_short_cap: -1 (the default) or an entry count"); ctx->umap_short_cap = v; }
  else if (f == "device") ctx->device = (int)v;
  else if (f == "profile") { ctx->profile = (int)(v < 0 ? 0 : v > 2 ? 2 : v); ctx->prof_update_ms = 0; ctx->prof_update_launches = 0; ctx->prof_update_cells = 0; ctx->prof_update_steps = 0; ctx->ev_used = 0;
                             ctx->ph_used = 0; ctx->gpu_timers.clear(); }
  else if (f == "grid") { if (ctx->ran_setup) return fail(ctx, HMX_ERR_STATE, "grid must be set before setup"); ctx->L.grid = (int)v; }
  else if (f == "comm_force") ctx->comm_force = v != 0;
  else if (f == "upd_wps") { if (ctx->ran_setup) return fail(ctx, HMX_ERR_STATE, "upd_wps must be set before setup"); ctx->tun_wps = (int)v; }
  else if (f == "upd_debug") { if (ctx->ran_setup) ctx->D.upd_debug = (int)v; }
  else if (f == "upd_tpw") { ctx->tun_tpw = (int)v; if (ctx->ran_setup) ctx->D.upd_tpw = (int)(v < 1 ? 1 : v); }
  else return fail(ctx, HMX_ERR_ARG, "unknown or read-only field: " + f);
  return 0;
}

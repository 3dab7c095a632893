// hmx_api_diag.inc -- part of hmx_api.cpp (included there, ONE translation unit): diagnostics of the restarted sequential sums + tail of the C ABI
// ---- diagnostics of the restarted sequential sums (tests/test_gpu_seq.py): the machinery alone, on caller-provided data -----------
// totals[c][0][k] = the fp32 value of   s = 0; for i in chain c: s += R[list[off_c + i]][k]   (one add after the other);
// totals[c][1 + b][k] = the same loop over the chain's cells of level b only
int hmx_debug_seq_oe(const float* R, int64_t n, int32_t K, const int32_t* level, int32_t B, const int32_t* list, int64_t nlist,
                     const int32_t* chain_off, const int32_t* chain_cnt, int32_t nchains, int32_t seg_cells, int32_t passes, float* totals,
                     int64_t* mismatch, double* residual) {
  if (!R || !list || !level || !chain_off || !chain_cnt || !totals || n <= 0 || K <= 0 || B <= 0 || nchains <= 0 || seg_cells <= 0 || passes < 2) return HMX_ERR_ARG;
  // (a probe, but an exported one: every index the kernels will use is checked here -- cells inside R, levels inside the LDS rows, chains
  //  inside the list, the level rows inside the LDS budget of a workgroup)
  if (nlist <= 0 || n > 2000000000ll || nlist > 2000000000ll || (size_t)B * 256 > 60 * 1024) return HMX_ERR_ARG;
  for (int64_t i = 0; i < nlist; i++) if (list[i] < 0 || list[i] >= n) return HMX_ERR_ARG;
  for (int64_t i = 0; i < n; i++) if (level[i] < 0 || level[i] >= B) return HMX_ERR_ARG;
  for (int c = 0; c < nchains; c++) if (chain_off[c] < 0 || chain_cnt[c] < 0 || (int64_t)chain_off[c] + chain_cnt[c] > nlist) return HMX_ERR_ARG;
  hmx_ctx* ctx = hmx_create();
  auto run = [&]() -> int {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(ctx, HMX_ERR_DEVICE, "no HIP device");
    HIPCHK(hipStreamCreateWithFlags(&ctx->L.stream, hipStreamNonBlocking)); ctx->own_stream = true;
    CallBufs bufs; float* dR; int* dl; int* dlev; int* dq;
    HIPCHK(bufs.get(&dR, (size_t)n * K)); HIPCHK(bufs.get(&dl, (size_t)nlist));
    HIPCHK(bufs.get(&dlev, (size_t)n)); HIPCHK(bufs.get(&dq, (size_t)B));
    std::vector<int> ident(B); std::iota(ident.begin(), ident.end(), 0);
    CHK(h2d(ctx, dR, R, (size_t)n * K)); CHK(h2d(ctx, dl, list, (size_t)nlist)); CHK(h2d(ctx, dlev, level, (size_t)n)); CHK(h2d(ctx, dq, ident.data(), (size_t)B));
    ctx->K = K; ctx->B = B; ctx->seq_passes = passes; ctx->seq_stats = true;
    ctx->D.R = dR; ctx->D.K = K; ctx->D.B = B; ctx->D.C = 1; ctx->D.combo = dlev; ctx->D.qlev = dq;      // one covariate: combination == level
    for (int c = 0; c < 4; c++) ctx->D.cov_end[c] = B;
    std::vector<std::pair<int, int>> ch;
    for (int c = 0; c < nchains; c++) ch.push_back({chain_off[c], chain_cnt[c]});
    CHK(seq_plan_build(ctx, ctx->plan_round, ch, seg_cells));
    CHK(seq_run_oe(ctx, ctx->plan_round, dl, nullptr, 0, nchains));
    CHK(d2h(ctx, totals, ctx->sq_total, (size_t)nchains * (1 + B) * K));
    unsigned mm[2] = {0, 0}; CHK(d2h(ctx, mm, ctx->sq_conv, 2));
    if (mismatch) *mismatch = (int64_t)mm[0];
    if (residual) { float r; std::memcpy(&r, &mm[1], 4); *residual = (double)r; }
    return 0;
  };
  const int st = run();
  hmx_destroy(ctx);
  return st;
}
// total[a] = the fp32 value of   s = 0; for i < n: s += T[a * n + i]
int hmx_debug_seq_arr(const float* T, int64_t n, int32_t narr, int32_t seg_terms, int32_t passes, float* total, int64_t* mismatch, double* residual) {
  if (!T || !total || n <= 0 || narr <= 0 || narr > 64 || seg_terms < 0 || passes < 2) return HMX_ERR_ARG;
  if (seg_terms == 0 && (narr != 3 || n < 4)) return HMX_ERR_ARG;
  hmx_ctx* ctx = hmx_create();
  auto run = [&]() -> int {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(ctx, HMX_ERR_DEVICE, "no HIP device");
    HIPCHK(hipStreamCreateWithFlags(&ctx->L.stream, hipStreamNonBlocking)); ctx->own_stream = true;
    CallBufs bufs; float* dT;
    HIPCHK(bufs.get(&dT, (size_t)n * narr));
    CHK(h2d(ctx, dT, T, (size_t)n * narr));
    if (seg_terms == 0) {
      // the one-launch form (k_seq_obj_fused, round 6): segments of 32 terms in registers, `passes` passes inside launches of at most 8, the scans between
      // them through the in-launch exchange; later launches restart from the starts the one before left (exactly what the adaptive objective does)
      const int nsegs = seq_obj_fused_nsegs(n);
      const size_t words = seq_obj_fused_slot_words(n);
      CHK(seq_grow(ctx, ctx->obj_start, ctx->obj_start_cap, (size_t)3 * nsegs));
      CHK(seq_grow(ctx, ctx->objf_slots, ctx->objf_slots_cap, words));
      HIPCHK(hipMemsetAsync(ctx->objf_slots, 0, words * sizeof(unsigned long long), ctx->L.stream));
      { size_t c = 0; CHK(seq_grow(ctx, ctx->objf_stats, c, 16)); }
      CHK(seq_workspace(ctx, 1, 3));
      for (int p = 0; p < passes; p += 8) {
        if (!l_seq_obj_fused(ctx->L, ctx->D, 0, dT, n, nullptr, nullptr, n, std::min(8, passes - p), p == 0, ctx->obj_start, ctx->sq_total, ctx->objf_stats, ctx->objf_slots,
                             ++ctx->objf_epoch)) return fail(ctx, HMX_ERR_LIMIT, "fused launch refused");
        KCHK();
      }
      CHK(d2h(ctx, total, ctx->sq_total, (size_t)3));
      unsigned w[16]; CHK(d2h(ctx, w, ctx->objf_stats, 16));
      if (w[7]) return fail(ctx, HMX_ERR_DEVICE, "in-launch exchange timed out");
      if (mismatch) *mismatch = (int64_t)w[0];
      if (residual) { double r = 0.0; for (int c = 0; c < 3; c++) { float dm, tt; std::memcpy(&dm, &w[1 + c], 4); std::memcpy(&tt, &w[4 + c], 4); if (dm > 0.0f) r = std::max(r, (double)dm / std::max((double)std::fabs(tt), 1e-30)); } *residual = r; }
      return 0;
    }
    const int nsegs = (int)((n + seg_terms - 1) / seg_terms);
    CHK(seq_workspace(ctx, (size_t)narr * nsegs, (size_t)narr));
    CHK(seq_grow(ctx, ctx->obj_partial, ctx->obj_partial_cap, (size_t)narr * ((nsegs + 255) / 256)));
    for (int p = 0; p < passes; p++) {
      l_seq_arr_pass(ctx->L, dT, n, n, narr, seg_terms, nsegs, ctx->sq_start, ctx->sq_end, p == 0, ctx->obj_partial, p == passes - 1 ? ctx->sq_mismatch : nullptr); KCHK();
      l_seq_scan1(ctx->L, narr, nsegs, ctx->sq_start, ctx->sq_end, ctx->sq_start, ctx->sq_total, p == passes - 1 ? ctx->sq_mismatch : nullptr, p == 0, ctx->obj_partial); KCHK();
    }
    CHK(d2h(ctx, total, ctx->sq_total, (size_t)narr));
    unsigned mm[2] = {0, 0}; CHK(d2h(ctx, mm, ctx->sq_mismatch, 2));
    if (mismatch) *mismatch = (int64_t)mm[0];
    if (residual) { float r; std::memcpy(&r, &mm[1], 4); *residual = (double)r; }
    return 0;
  };
  const int st = run();
  hmx_destroy(ctx);
  return st;
}

// host-only micro-benchmark of the ridge solves (no device needed): returns microseconds per call of the full K-cluster loop
double hmx_debug_solve_bench(int K, int B, int d, int reps) {
  hmx_ctx c; c.K = K; c.B = B; c.C = 1; c.d = d; c.Q = B; c.B_vec = {B}; c.cov_bounds = {B};
  c.sizes.assign(B, 1000.f); c.lambda_estimation = true; c.alpha = 0.2f; c.cutoff = 1e-5f;
  c.qlev.resize(B); for (int b = 0; b < B; b++) c.qlev[b] = b;
  std::vector<float> O((size_t)K * B, 50.f), E((size_t)K * B, 40.f);
  std::vector<double> Sq((size_t)B * K * d, 0.3), nq((size_t)B * K, 50.0);
  for (size_t i = 0; i < Sq.size(); i++) Sq[i] = 0.1 + 1e-3 * (double)(i % 97);
  std::vector<float> Wq((size_t)B * K * d), Ynew((size_t)K * d);
  std::vector<SolveOut> outs(K);
  const double t0 = now_ms();
  for (int r = 0; r < reps; r++) for (int k = 0; k < K; k++) solve_cluster(&c, k, O, E, Sq, nq, Wq, Ynew, outs[k]);
  return 1e3 * (now_ms() - t0) / reps;
}

int64_t hmx_get(hmx_ctx* ctx, const char* field, double* out, int64_t cap) {
  if (!ctx || !field) return -1;
  const std::string f(field);
  if (f.rfind("objective_", 0) == 0 || f == "kmeans_rounds") { if (flush_objectives(ctx)) return -1; }
  // (-1 with hmx_last_error = "singular ridge system": the deferred verdict of the last device-side correction, not an unknown field)
  if (f == "Y" || f == "W" || f == "W_rows" || f == "subset_clusters" || f == "skipped_clusters") { if (sync_solve_results(ctx)) return -1; }
  auto scalar = [&](double v) -> int64_t { if (out && cap >= 1) out[0] = v; return 1; };
  auto vec = [&](const auto& v) -> int64_t {
    if (out) for (size_t i = 0; i < v.size() && (int64_t)i < cap; i++) out[i] = (double)v[i];
    return (int64_t)v.size();
  };
  if (f == "N") return scalar((double)ctx->N_global);
  if (f == "N_local") return scalar((double)ctx->N);
  if (f == "B") return scalar(ctx->B);
  if (f == "K") return scalar(ctx->K);
  if (f == "d") return scalar(ctx->d);
  if (f == "alpha") return scalar(ctx->alpha);
  if (f == "max_iter_kmeans") return scalar(ctx->max_iter_kmeans);
  if (f == "block_size") return scalar(ctx->block_size);
  if (f == "n_blocks") return scalar(ctx->nb);
  if (f == "cells_per_block") return scalar((double)ctx->cells_per_block);
  if (f == "W_rows") return scalar(ctx->W_rows);
  if (f == "n_combos") return scalar(ctx->Q);
  if (f == "subset_clusters") return scalar((double)ctx->subset_clusters);
  if (f == "skipped_clusters") return scalar((double)ctx->skipped_clusters);
  if (f == "comm:calls") return scalar((double)ctx->comm_calls);
  if (f == "comm:bytes") return scalar((double)ctx->comm_bytes);
  if (f == "trace") {   // HMX_TRACE=1: raw per-wave stamps of the last block-update launch
    if (!ctx->D.trace) return -1;
    const int64_t n = (int64_t)ctx->D.nwmax * 16;
    if (out) {
      std::vector<unsigned long long> h((size_t)n);
      (void)hipStreamSynchronize(ctx->L.stream);
      (void)hipMemcpy(h.data(), ctx->D.trace, sizeof(unsigned long long) * (size_t)n, hipMemcpyDeviceToHost);
      for (int64_t i = 0; i < std::min(n, cap); i++) out[i] = (double)(h[(size_t)i] & ((1ull << 52) - 1));
    }
    return n;
  }
  if (f == "usig") return scalar((double)ctx->D.usig);
  if (f == "upd_wps") return scalar((double)ctx->D.upd_wps);
  if (f.rfind("prof:", 0) == 0 && ctx->ev_used) {   // resolve the pending event pairs (one sync, outside any timed region)
    (void)hipStreamSynchronize(ctx->L.stream);
    for (size_t i = 0; i < ctx->ev_used; i++) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ctx->ev_pool[i].first, ctx->ev_pool[i].second) == hipSuccess) ctx->prof_update_ms += ms;
    }
    ctx->prof_update_launches += (int64_t)ctx->ev_used; ctx->ev_used = 0;
  }
  if (f == "seq:oe_cell_passes") return scalar(ctx->seq_oe_cell_passes);
  if (f == "prof:update_ms") return scalar(ctx->prof_update_ms);
  if (f == "prof:update_launches") return scalar((double)ctx->prof_update_launches);
  if (f == "prof:update_cells") return scalar((double)ctx->prof_update_cells);
  if (f == "prof:update_steps") return scalar((double)ctx->prof_update_steps);
  if (f == "sync") {        // everything queued on the handle's stream has completed (hosts without a HIP runtime of their own: bench.py --bootstrap file)
    if (ctx->L.stream && hipStreamSynchronize(ctx->L.stream) != hipSuccess) return -1;
    return scalar(1.0);
  }
  if (f == "chain") return scalar((ctx->chain_ok || ctx->D.chain_pair) ? 1.0 : 0.0);
  if (f == "chain_wgs") return scalar((double)ctx->chain_wgs);      // workgroups of the chain: the device's compute units unless HMX_CHAIN_WGS says otherwise
  if (f == "chain_pair") return scalar(ctx->D.chain_pair ? 1.0 : 0.0);      // the wave-pair chain (k_tile MODE 6: 112 < K <= 224)
  if (f == "dot_bf") return scalar(ctx->D.dot_bf ? 1.0 : 0.0);     // split-bf16 tile kernels offered (each launch still checks its LDS budget)
  if (f == "sold_carry") return scalar(ctx->carry_ok ? 1.0 : 0.0);
  if (f == "project_slabs") return scalar((double)ctx->project_slabs);
  if (f == "pca_entries") return scalar((double)ctx->pca_entries);
  if (f == "ranksum_blocks") return scalar((double)ctx->ranksum_blocks);      // the gene blocks (fill sweeps) of the last hmx_rank_sums
  if (f == "ranksum_sort_lds") return scalar((double)RS_SORT_LDS);            // ... the longest list it sorts in LDS, the chunk of its radix sort and rank scans
  if (f == "ranksum_chunk") return scalar((double)RS_CHUNK);
  if (f == "graph:cc_rounds") return scalar((double)ctx->graph_cc_rounds);      // the hook-and-jump rounds of the last hmx_graph_components
  if (f == "snn:s_min") return scalar((double)ctx->snn_s_min);      // the last SNN call: an entry was kept iff its shared count reached this
  if (f == "snn:long_rows") return scalar((double)ctx->snn_long_rows);      // ... and the rows that took the windowed path
  if (f == "snn:short_cap") return scalar((double)SNN_SHORT_CAP);      // the largest candidate count one wave sorts in LDS; the cells of the long path's window
  if (f == "snn:window") return scalar((double)SNN_WINDOW);
  if (f == "louvain:levels") return scalar((double)ctx->louvain_levels);      // the last hmx_louvain: recorded levels, the level returned (0: the singletons), sweeps of all levels, clusters
  if (f == "louvain:best_level") return scalar((double)ctx->louvain_best_level);
  if (f == "louvain:sweeps") return scalar((double)ctx->louvain_sweeps);
  if (f == "louvain:clusters") return scalar((double)ctx->louvain_clusters);
  if (f == "louvain:long_rows") return scalar((double)ctx->louvain_long_rows);      // ... and the rows of level 0 above the short path's cap
  if (f == "leiden:levels") return scalar((double)ctx->leiden_levels);      // the last hmx_leiden: recorded levels, sweeps of local moves and of refinement over all levels, clusters
  if (f == "leiden:sweeps") return scalar((double)ctx->leiden_sweeps);
  if (f == "leiden:refine_sweeps") return scalar((double)ctx->leiden_refine_sweeps);
  if (f == "leiden:clusters") return scalar((double)ctx->leiden_clusters);
  if (f == "leiden:converged") return scalar((double)ctx->leiden_converged);
  if (f == "leiden:long_rows") return scalar((double)ctx->leiden_long_rows);      // ... and the rows of level 0 (edges only) above the short path's cap
  if (f == "louvain:short_cap") return scalar((double)(ctx->louvain_short_cap >= 0 ? std::min<int64_t>(ctx->louvain_short_cap, LV_SHORT_CAP) : LV_SHORT_CAP));
  if (f == "umap:fired") return scalar((double)ctx->umap_fired);      // the last hmx_umap_layout: directed firings of its epochs, the epochs run, the rows above the short path's cap
  if (f == "umap:epochs") return scalar((double)ctx->umap_epochs);
  if (f == "umap:long_rows") return scalar((double)ctx->umap_long_rows);
  if (f == "umap:short_cap") return scalar((double)(ctx->umap_short_cap >= 0 ? ctx->umap_short_cap : UM_SHORT_CAP));
  if (f == "umap_transform:fired") return scalar((double)ctx->umap_transform_fired);      // the last hmx_umap_transform: firings of its epochs over all cells, the epochs run
  if (f == "umap_transform:epochs") return scalar((double)ctx->umap_transform_epochs);
  if (f == "diag:launches") return scalar((double)ctx->n_launches);      // since setup: kernel launches of the clustering / correction launchers (hmx_k_launch.inc; copies and memsets are not kernels of ours)
  if (f == "diag:event_records") return scalar((double)ctx->n_event_records);      // ... and events recorded (objective slots, the chain gate across streams, profile mode's phases)
  if (f == "diag:gate_records") return scalar((double)ctx->n_gate_records);      // ... those of them that were the chain gate's: they depend on which stream of the PROCESS launched a chain last
  if (f == "carried_rounds") return scalar((double)ctx->carried_rounds);
  if (f == "rounds_without_R") return scalar((double)ctx->rounds_without_R);
  if (f == "chain_rounds") return scalar((double)ctx->chain_rounds);
  if (f.rfind("launch:", 0) == 0) {      // the last k_tile launch of a kind as it ran: valid, bf, nct, mode, wps, usig, threads, blocks, lds
    for (int k = 0; k < 5; k++) if (f.substr(7) == TILE_KIND_NAME[k] && ctx->tile_seen[k]) {
      const TileLaunch& t = ctx->last_tile[k];
      return vec(std::vector<double>{(double)t.valid, (double)t.bf, (double)t.nct, (double)t.mode, (double)t.wps, (double)t.usig, (double)t.threads, (double)t.blocks, (double)t.lds});
    }
    // ... and of the ridge correction (plan_ridge_launch): valid, mfma, p0, p1, grid x, y, z, threads, lds, the solve's lds_b_bytes, lds_body_bytes, lds_mask_off, the reduce launch's grid x, y
    for (int k = 0; k < 3; k++) if (f.substr(7) == RIDGE_KIND_NAME[k] && ctx->ridge_seen[k]) {
      const RidgeLaunch& t = ctx->last_ridge[k];
      return vec(std::vector<double>{(double)t.valid, (double)t.mfma, (double)t.p0, (double)t.p1, (double)t.gx, (double)t.gy, (double)t.gz, (double)t.threads, (double)t.lds,
                                     (double)t.lds_b_bytes, (double)t.lds_body_bytes, (double)t.lds_mask_off, (double)t.rgx, (double)t.rgy,
                                     (double)t.lds_sys_off, (double)t.lds_total});      // (the solve's systems in LDS: their offset, 0: global scratch; the launch's LDS in all)
    }
    return -1;      // (no such kind, or no launch of it on this handle yet)
  }
  if (f == "round:last") {      // the plan of the last round of update_R (hmx_round.h): path, merged, chain_tail, carried, write_next, r_store, closing form, exchanges
    if (!ctx->round_seen) return -1;
    const RoundPlan& r = ctx->last_round;
    return vec(std::vector<double>{(double)r.path, (double)r.merged, (double)r.chain_tail, (double)r.carried, (double)r.write_next, (double)r.r_store, (double)r.close, (double)r.exchanges});
  }
  // further values of the launch plan (hmx_plan.h) as hmx_setup took them, for tests that claim a path
  if (f == "need_lorder") return scalar((double)ctx->D.need_lorder);     // the shuffle also writes lorder / lcombo (k_oldsum's gather variant reads them)
  if (f == "objslots") return scalar((double)ctx->D.objslots);           // slot rows of a round's objective partials: min(n_blocks, 64)
  if (f == "upd_contig") return scalar((double)ctx->D.upd_contig);       // launch-per-step path: a wave owns a contiguous range of a block's tiles
  if (f == "moe_mfma") return scalar((double)ctx->D.moe_mfma);           // MFMA ridge kernels (0: the first-generation ones)
  if (f == "shuffle_inv") return scalar(ctx->shuf_inv ? 1.0 : 0.0);
  if (f == "p2p:exchange_us") return scalar(ctx->p2p_exchange_us);
  if (f == "p2p:allreduce_calls") return scalar((double)ctx->p2p_ar_calls);
  if (f == "p2p:allreduce_big_windows") return scalar((double)ctx->p2p_ar_big_windows);
  if (f == "p2p") return scalar(ctx->p2p_on && ctx->p2p_world == ctx->world ? 1.0 : 0.0);
  if (f == "chain_dbg") {   // accumulated 100 MHz ticks of the persistent chain's phases (see hmx_internal.h); reading resets them
    if (!ctx->ran_setup) return -1;
    if (!out) return 64;      // [0..12] folder / workgroup 0 wave 0 phases, [16..31] workgroup 0 and [32..47] workgroup 100: per wave busy ticks, tiles; [48..55] / [56..63]: wave 4 / 5 of workgroup 0, the phases of [4..11]
    std::vector<unsigned long long> h(64);
    if (d2h(ctx, h.data(), ctx->D.chain_dbg, 64)) return -1;
    (void)hipMemsetAsync(ctx->D.chain_dbg, 0, sizeof(unsigned long long) * 64, ctx->L.stream);
    return vec(h);
  }
  if (f.rfind("gputimer:", 0) == 0) {   // GPU time of a phase (profile mode), ms; "gputimer:Rcells_update" == "prof:update_ms"
    resolve_phases(ctx);
    const std::string nm = f.substr(9);
    if (nm == "Rcells_update") return hmx_get(ctx, "prof:update_ms", out, cap);
    auto it = ctx->gpu_timers.find(nm); return scalar(it == ctx->gpu_timers.end() ? 0.0 : it->second);
  }
  if (f.rfind("timer:", 0) == 0) { auto it = ctx->timers.find(f.substr(6)); return scalar(it == ctx->timers.end() ? 0.0 : it->second); }
  if (f == "seed_cells") return vec(ctx->seed_cells);
  if (f == "Y") return vec(ctx->Y);
  if (f == "W") return vec(ctx->W);
  if (f == "Pr_b") return vec(ctx->Pr_b);
  if (f == "theta") return vec(ctx->theta);
  if (f == "sigma") return vec(ctx->sigma);
  if (f == "lambda") return vec(ctx->lambda);
  if (f == "B_vec") return vec(ctx->B_vec);
  if (f == "objective_kmeans") return vec(ctx->obj_kmeans);
  if (f == "objective_kmeans_dist") return vec(ctx->obj_dist);
  if (f == "objective_kmeans_entropy") return vec(ctx->obj_entropy);
  if (f == "objective_kmeans_cross") return vec(ctx->obj_cross);
  if (f == "objective_harmony") return vec(ctx->obj_harmony);
  if (f == "kmeans_rounds") return vec(ctx->kmeans_rounds);
  if (ctx->query_done && (f == "Z_corr" || f == "Z_orig" || f == "R")) return hmx_get_matrix(ctx, field, out, HMX_F64, HMX_HOST, cap);
  if (!ctx->ran_setup) return -1;
  if (hipSetDevice(ctx->device) != hipSuccess) return -1;
  if (f == "ref_Nr" || f == "ref_C") {       // reference summary for hmx_map_query, from the current R and Z_corr (sharded: collective)
    if (ctx->ran_init && !ctx->R_valid) { ctx->err = "R is not available: the clustering call that would have stored it did not complete"; return -1; }
    if (sync_solve_results(ctx)) return -1;
    const int K = ctx->K, d = ctx->d;
    const int64_t cnt = f == "ref_Nr" ? K : (int64_t)K * d;
    if (!out) return cnt;
    std::vector<double> res;
    if (ref_summary(ctx, res)) return -1;
    std::vector<double> v((size_t)cnt);
    for (int k = 0; k < K; k++) {
      if (f == "ref_Nr") v[k] = res[(size_t)k * (d + 1) + d];
      else for (int j = 0; j < d; j++) v[k + (size_t)K * j] = res[(size_t)k * (d + 1) + j];
    }
    return vec(v);
  }
  if (f == "seq:mismatch" || f == "seq:residual") {      // last scans of the restarted sequential sums: segment starts that still moved / the largest move relative to its chain's largest start
    if (!ctx->sq_mismatch) return scalar(0.0);
    bool dummy = false;
    if (seq_settled(ctx, &dummy)) return -1;          // (folds the last unchecked scan's words in)
    (void)hipMemsetAsync(ctx->sq_conv, 0, 2 * sizeof(unsigned), ctx->L.stream);
    return scalar(f == "seq:mismatch" ? (double)ctx->seq_mismatch_sum : ctx->seq_resid_max);
  }
  if (f == "seq:extra_passes") return scalar((double)ctx->seq_extra_passes);
  if (f == "seq:unsettled") return scalar((double)ctx->seq_unsettled);
  if (f == "seq:group_passes" || f == "seq:group_runs") {
    if (!out) return 4;
    for (int g = 0; g < 4; g++) out[g] = (double)(f == "seq:group_passes" ? ctx->seq_group_passes[g] : ctx->seq_group_runs[g]);
    return 4;
  }
  if (f == "seq:runs") return scalar((double)ctx->seq_runs);
  if (f == "O" || f == "E" || f == "Lambda") {
    const int K = ctx->K, B = ctx->B;
    const int64_t cnt = (f == "Lambda") ? (int64_t)K * (B + 1) : (int64_t)K * B;
    if (!out) return cnt;
    std::vector<long long> ofx((size_t)B * K);
    if (d2h(ctx, ofx.data(), ctx->D.O_fx, ofx.size())) return -1;
    std::vector<float> Of_h, Ef_h;
    if (ctx->oe_arith) {       // the tables ARE fp32 in this mode
      Of_h.resize((size_t)B * K); Ef_h.resize((size_t)B * K);
      if (d2h(ctx, Of_h.data(), ctx->Of, Of_h.size()) || d2h(ctx, Ef_h.data(), ctx->Ef, Ef_h.size())) return -1;
    }
    if (f == "O") return vec(ctx->oe_arith ? Of_h : table_O(ctx, ofx));
    const std::vector<float> E = ctx->oe_arith ? Ef_h : table_E(ctx, ofx);
    if (f == "E") return vec(E);
    std::vector<double> L((size_t)K * (B + 1), 0.0);  // getLambda :657-669
    // (estimated: find_lambda_cpp's [0, alpha * E[k,:]], src/utils.cpp:159-163; fixed: the caller's whole vector, its entry 0 included)
    for (int k = 0; k < K; k++) {
      if (!ctx->lambda_estimation) L[k] = (double)ctx->lambda[0];
      for (int b = 0; b < B; b++)
        L[(size_t)(b + 1) * K + k] = ctx->lambda_estimation ? (double)(E[(size_t)b * K + k] * ctx->alpha) : (double)ctx->lambda[b + 1];
    }
    return vec(L);
  }
  if (f == "Z_corr" || f == "Z_orig" || f == "R") return hmx_get_matrix(ctx, field, out, HMX_F64, HMX_HOST, cap);
  ctx->err = "hmx_get: unknown field '" + f + "'";
  return -1;
}

// getZcorr / getZorig / getR (src/harmony.cpp:640-655) with a choice of element type and destination: double on the host is the
// R seam; float and/or a device pointer avoid the fp64 blow-up and the PCIe trip for hosts that keep working on the GPU.
// Host destinations are filled slab by slab through two HBM staging buffers (conversion of slab s+1 overlaps the copy of slab s).
int64_t hmx_get_matrix(hmx_ctx* ctx, const char* field, void* out, int32_t dtype, int32_t location, int64_t cap) {
  if (!ctx || !field || !(ctx->ran_setup || ctx->query_done)) return -1;
  const std::string f(field);
  if (f != "Z_corr" && f != "Z_orig" && f != "R") { ctx->err = "hmx_get_matrix: unknown field " + f; return -1; }
  if ((dtype != HMX_F64 && dtype != HMX_F32) || (location != HMX_HOST && location != HMX_DEVICE)) { ctx->err = "bad dtype / location"; return -1; }
  if (hipSetDevice(ctx->device) != hipSuccess) return -1;
  if (out && f == "Z_corr" && sync_solve_results(ctx)) return -1;      // a singular system of the last correction surfaces here (hmx_last_error says so)
  if (f == "R" && ctx->ran_init && !ctx->R_valid) { ctx->err = "R is not available: the clustering call that would have stored it did not complete"; return -1; }
  const int w = (f == "R") ? ctx->K : ctx->d;
  const int64_t cnt = ctx->N * w;
  if (!out || cap < cnt) return cnt;
  const float* src = (f == "R") ? ctx->D.R : (f == "Z_corr" ? ctx->D.Zc : ctx->D.Zo);
  // a mapped query keeps no R: its rows are recomputed from Z_orig into a buffer that lives for this call only
  CallBufs tmp;
  if (ctx->query_done && f == "R") {
    float* rows;
    if (tmp.get(&rows, (size_t)cnt) != hipSuccess) { (void)hipGetLastError(); ctx->err = "out of device memory for R"; return -1; }
    if (query_R_rows(ctx, rows)) return -1;
    src = rows;
  }
  const int ws = (f == "R") ? w : ctx->D.zs;
  const int f32 = dtype == HMX_F32;
  const double t0 = now_ms();
  hipError_t e;
  if (location == HMX_DEVICE) {
    l_convert_out(ctx->L, src, out, f32, ctx->D.invperm, ctx->D.n, w, ws);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->L.stream);
  } else {
    const size_t cell = (size_t)w * (f32 ? 4 : 8);
    XferPipe pipe;
    e = pipe.open(ctx->device, out, ctx->N, cell, ctx->xfer_slab_bytes);
    if (e == hipSuccess) e = xfer_egress(pipe, ctx->L.stream, out, ctx->N, cell, [&](void* stage, int64_t s0, int64_t c) {
      l_convert_out(ctx->L, src, stage, f32, ctx->D.invperm + s0, (int)c, w, ws); return hipGetLastError(); });
  }
  if (e != hipSuccess) { ctx->err = hipGetErrorString(e); return -1; }
  ctx->timers["egress_" + f] = now_ms() - t0;
  return cnt;
}

}  // extern "C"

// hmx_api_refarith.inc -- part of hmx_api.cpp (included there, ONE translation unit): reference arithmetic: the restarted sequential sums' host side (hmx_seq.hip launches, pass control)
// ================================================================================================================================
// Reference arithmetic: the reference's sequential fp32 accumulators as restarted sequential sums (hmx_seq.hip, DESIGN 2.2)
// ================================================================================================================================
template <class T> int seq_grow(hmx_ctx* ctx, T*& p, size_t& cap, size_t need) {
  if (need <= cap && p) return 0;
  if (p) { HIPCHK(hipStreamSynchronize(ctx->L.stream)); (void)hipFree(p); p = nullptr; cap = 0; }
  void* q = nullptr;
  HIPCHK(hipMalloc(&q, std::max<size_t>(need, 1) * sizeof(T)));
  p = (T*)q; cap = need;
  return 0;
}
// chains = (first entry of the list, number of cells); every chain is cut into segments of L cells
int seq_plan_build(hmx_ctx* ctx, hmx_ctx::SeqPlan& P, const std::vector<std::pair<int, int>>& chains, int L) {
  std::vector<SeqSeg> segs; std::vector<SeqChain> ch(chains.size());
  P.seg0.assign(chains.size() + 1, 0); P.cells.assign(chains.size(), 0);
  for (size_t c = 0; c < chains.size(); c++) P.cells[c] = chains[c].second;
  for (size_t c = 0; c < chains.size(); c++) {
    ch[c].seg0 = (int)segs.size(); P.seg0[c] = (int)segs.size();
    for (int o = 0; o < chains[c].second; o += L) segs.push_back({chains[c].first + o, std::min(L, chains[c].second - o)});
    ch[c].nseg = (int)segs.size() - ch[c].seg0;
  }
  P.seg0[chains.size()] = (int)segs.size();
  P.nsegs = (int)segs.size(); P.nchains = (int)chains.size(); P.seg_cells = L;
  CHK(seq_grow(ctx, P.d_segs, P.cap_segs, segs.size())); CHK(seq_grow(ctx, P.d_chains, P.cap_chains, ch.size()));
  CHK(h2d(ctx, P.d_segs, segs.data(), segs.size())); CHK(h2d(ctx, P.d_chains, ch.data(), ch.size()));
  return 0;
}
int seq_workspace(hmx_ctx* ctx, size_t seg_floats, size_t total_floats) {
  if (seg_floats > ctx->sq_cap) { size_t c1 = ctx->sq_cap, c2 = ctx->sq_cap; CHK(seq_grow(ctx, ctx->sq_start, c1, seg_floats)); CHK(seq_grow(ctx, ctx->sq_end, c2, seg_floats)); ctx->sq_cap = seg_floats; }
  CHK(seq_grow(ctx, ctx->sq_total, ctx->sq_total_cap, total_floats));
  if (!ctx->sq_mismatch) { size_t c = 0; CHK(seq_grow(ctx, ctx->sq_mismatch, c, 4)); HIPCHK(hipMemsetAsync(ctx->sq_mismatch, 0, 4 * sizeof(unsigned), ctx->L.stream)); ctx->sq_conv = ctx->sq_mismatch + 2; }
  return 0;
}
// after a checked scan (the scan wrote {segments that moved, largest chain-relative move} into sq_conv): did the starts settle?
int seq_settled(hmx_ctx* ctx, bool* settled) {
  unsigned w[2] = {0, 0};
  CHK(d2h(ctx, w, ctx->sq_conv, 2));
  float r; std::memcpy(&r, &w[1], 4);
  *settled = w[0] == 0 || (!ctx->seq_strict && (double)r <= ctx->seq_tol);
  ctx->seq_last_mismatch = w[0];
  ctx->seq_mismatch_sum += w[0]; if ((double)r > ctx->seq_resid_max) ctx->seq_resid_max = (double)r;
  return 0;
}
// one restarted-sum iteration scheme for all users: `pass(p, zero_start)` runs the segments, `scan(p, zero_start, conv)` the scan.  The first
// `seq_passes` passes always run (warm: one less); long chains continue until the starts settled.
template <class PASS, class SCAN> int seq_iterate(hmx_ctx* ctx, int group, bool warm, bool adaptive, PASS pass, SCAN scan) {
  // cold: seq_passes passes from zero starts.  warm: seq_warm_passes passes from the starts the workspace still holds -- NOT one pass less by
  // default: a warm start of a block's put-back sums is as far from the truth as R moved in the block update, and ONE pass from it carries a
  // first-order error (100k cells: Z_corr 5.8e-6 from the oracle instead of 2.2e-6, tools/strict_probe.py); two passes from zero are second order.
  int p = warm ? std::max(0, ctx->seq_passes - ctx->seq_warm_passes) : 0;
  const int p_first = p;
  ctx->seq_group_runs[group]++;
  if (ctx->seq_strict) adaptive = true;
  struct Count { hmx_ctx* c; int g; const int& p; int p0; ~Count() { c->seq_group_passes[g] += p - p0; } } count{ctx, group, p, p_first};
  for (; p < ctx->seq_passes; p++) {
    const bool last = p == ctx->seq_passes - 1 && (adaptive || ctx->seq_stats);     // (short chains: statistics only on request, "seq_stats")
    CHK(pass(p == 0 && !warm, last ? ctx->sq_conv : nullptr));       // (the pass zeroes the statistics words its scan adds to)
    ctx->seq_scan_final = (p == ctx->seq_passes - 1) && !adaptive && !last;      // nobody reads the starts this scan would write: totals only
    CHK(scan(p == 0 && !warm, last ? ctx->sq_conv : nullptr));
    ctx->seq_scan_final = false;
  }
  if (!adaptive) {      // (short chains: three passes are far inside fp32 noise; their last scan's statistics are read when a getter asks)
    return 0;
  }
  bool ok = false;
  CHK(seq_settled(ctx, &ok));
  for (; !ok && p < ctx->seq_max_passes; p++) {
    CHK(pass(false, ctx->sq_conv));
    CHK(scan(false, ctx->sq_conv));
    CHK(seq_settled(ctx, &ok));
    ctx->seq_extra_passes++;
  }
  if (!ok) ctx->seq_unsettled++;       // (seq_max_passes reached with starts still moving: reported, "seq:unsettled")
  return 0;
}
// O / E sums of the chain sets [chain0, chain0 + nchains) of plan P over `list`: per chain set (1 + B) * K sequential fp32 sums
// (row 0: all its cells, row 1 + b: its cells of level b) -> ctx->sq_total[chain][1 + B][K].  passes x (segments in parallel, then the
// scan that hands every segment its start).
// warm: the workspace still holds these segments' starts from a run over (nearly) the same terms -- the first pass starts from them
// instead of from zero, which is worth one pass.
int seq_run_oe(hmx_ctx* ctx, const hmx_ctx::SeqPlan& P, const int* list, const int* poslev, int chain0, int nchains, bool warm = false) {
  const int W = (1 + ctx->B) * ctx->K, lo = P.seg0[chain0], n = P.seg0[chain0 + nchains] - lo;
  CHK(seq_workspace(ctx, (size_t)P.nsegs * W, (size_t)P.nchains * W));
  int longest = 0;
  for (int c = chain0; c < chain0 + nchains; c++) longest = std::max(longest, P.seg0[c + 1] - P.seg0[c]);
  const bool adaptive = (int64_t)longest * P.seg_cells >= ctx->seq_adaptive_cells;
  const int64_t passes_before = ctx->seq_group_passes[0];
  struct Walked { hmx_ctx* c; const hmx_ctx::SeqPlan& P; int c0, nc; int64_t p0; ~Walked() { double cells = 0; for (int i = c0; i < c0 + nc; i++) cells += P.cells[i]; c->seq_oe_cell_passes += cells * (double)(c->seq_group_passes[0] - p0); } } walked{ctx, P, chain0, nchains, passes_before};
  CHK(seq_iterate(ctx, 0, warm, adaptive,
                  [&](bool zero, unsigned* cz) -> int { l_seq_oe_pass(ctx->L, ctx->D, list, poslev, (int)ctx->N, P.d_segs, lo, n, ctx->sq_start, ctx->sq_end, zero ? 1 : 0, cz); KCHK(); return 0; },
                  [&](bool zero, unsigned* conv) -> int { l_seq_scan(ctx->L, P.d_chains, chain0, nchains, W, ctx->sq_start, ctx->sq_end, ctx->sq_start, ctx->sq_total, conv, zero ? 1 : 0, ctx->seq_scan_final ? 1 : 0); KCHK(); return 0; }));
  ctx->seq_runs++;
  return 0;
}
// static lists and plans of a handle that runs (part of) the reference's arithmetic; called at the end of hmx_setup
int seq_setup_static(hmx_ctx* ctx) {
  const int n = (int)ctx->N, C = ctx->C, B = ctx->B, K = ctx->K, Q = ctx->Q;
  const bool any = ctx->ridge_arith || ctx->oe_arith || ctx->obj_arith || ctx->solve_arith;
  if (!any) return 0;
  if (ctx->world > 1 || ctx->comm_force) return fail(ctx, HMX_ERR_ARG, "the reference-arithmetic modes (ridge_arith / oe_arith / obj_arith / solve_arith) run on one GPU");
  // headlist: [ cells in original order | for every covariate: cells by (level, original order) ]  (internal cell ids)
  std::vector<int> hl((size_t)(1 + C) * n);
  for (int i = 0; i < n; i++) hl[i] = ctx->invperm_h[i];
  ctx->lev_off.assign(B, 0); ctx->lev_cnt.assign(B, 0);
  for (int c = 0; c < C; c++) {
    const int b0 = c ? ctx->cov_bounds[c - 1] : 0, nl = ctx->B_vec[c];
    std::vector<int> cnt(nl + 1, 0);
    for (int i = 0; i < n; i++) cnt[ctx->qlev[(size_t)ctx->combo_h[ctx->invperm_h[i]] * C + c] - b0 + 1]++;
    for (int l = 0; l < nl; l++) { ctx->lev_cnt[b0 + l] = cnt[l + 1]; cnt[l + 1] += cnt[l]; ctx->lev_off[b0 + l] = (1 + c) * n + cnt[l]; }
    std::vector<int> cur(cnt.begin(), cnt.end() - 1);
    for (int i = 0; i < n; i++) { const int cell = ctx->invperm_h[i]; const int l = ctx->qlev[(size_t)ctx->combo_h[cell] * C + c] - b0; hl[(size_t)(1 + c) * n + cur[l]++] = cell; }
  }
  { size_t cap = 0; CHK(seq_grow(ctx, ctx->headlist, cap, hl.size())); CHK(h2d(ctx, ctx->headlist, hl.data(), hl.size())); }
  if (ctx->ridge_arith) {      // the list's combinations (static): the ridge pass fetches (cell, combination) with two independent loads
    std::vector<int> hq(hl.size());
    for (size_t i = 0; i < hl.size(); i++) hq[i] = ctx->combo_h[hl[i]];
    size_t cap = 0; CHK(seq_grow(ctx, ctx->headq, cap, hq.size())); CHK(h2d(ctx, ctx->headq, hq.data(), hq.size()));
  }
  { size_t c1 = 0, c2 = 0, c3 = 0; CHK(seq_grow(ctx, ctx->Of, c1, (size_t)B * K)); CHK(seq_grow(ctx, ctx->Ef, c2, (size_t)B * K)); CHK(seq_grow(ctx, ctx->Mtab, c3, (size_t)B * K));
    HIPCHK(hipMemsetAsync(ctx->Of, 0, sizeof(float) * (size_t)B * K, ctx->L.stream)); HIPCHK(hipMemsetAsync(ctx->Ef, 0, sizeof(float) * (size_t)B * K, ctx->L.stream)); }
  if (ctx->oe_arith || ctx->obj_arith) {      // level codes in ORIGINAL cell order, [min(C, 4)][n]: the head's O / E pass and the objective's fused launch read them
    const int Cl = std::min(C, 4); size_t c2 = 0; CHK(seq_grow(ctx, ctx->headlev, c2, (size_t)Cl * n));
    std::vector<int> hv((size_t)Cl * n);
    for (int i = 0; i < n; i++) for (int c = 0; c < Cl; c++) hv[(size_t)c * n + i] = ctx->qlev[(size_t)ctx->combo_h[ctx->invperm_h[i]] * C + c];
    CHK(h2d(ctx, ctx->headlev, hv.data(), hv.size()));
  }
  if (ctx->oe_arith) {
    // head: E = sum(R, 1) Pr_b^T, O = R Phi^T (:149-150): one chain set over all cells in original order
    CHK(seq_plan_build(ctx, ctx->plan_head, {{0, n}}, B > 32 ? 2048 : 1024));      // (many levels: (1 + B) K lane-chains per segment -- long segments keep the workspace below the R rows)
    // rounds: one chain set per block over the round's shuffled order; block j = positions [j cpb, (j + 1) cpb), the last takes the rest (:296-300)
    std::vector<std::pair<int, int>> ch;
    for (int j = 0; j < ctx->nb; j++) {
      const int lo = (int)std::min<uint64_t>((uint64_t)n, (uint64_t)j * ctx->cells_per_block);
      const int hi = (j == ctx->nb - 1) ? n : (int)std::min<uint64_t>((uint64_t)n, (uint64_t)(j + 1) * ctx->cells_per_block);
      ch.push_back({lo, hi - lo});
    }
    // (many levels: long segments -- (1 + B) K lane-chains per segment make the workspace traffic, a wave of k_seq_oe_pass_lg only adds the cells of its own 32 levels)
    CHK(seq_plan_build(ctx, ctx->plan_round, ch, B > 32 ? 1024 : 128));      // (measured at the configs[4] shape, 1M cells: 128 / 256 / 512 / 1024 / 2048 cells per segment -> O/E 553 / 475 / 437 / 420 / 596 ms per run)
    size_t cap = 0; CHK(seq_grow(ctx, ctx->roundlist, cap, (size_t)n));
    { const int Cl = std::min(C, 4); size_t c1 = 0; CHK(seq_grow(ctx, ctx->roundlev, c1, (size_t)Cl * n)); }
  }
  if (ctx->ridge_arith) {
    if (ctx->d > 62) return fail(ctx, HMX_ERR_LIMIT, "ridge_arith = 1 supports d <= 62");
    if (!ctx->solve_on_device) return fail(ctx, HMX_ERR_ARG, "ridge_arith = 1 needs the device-side ridge solve");
    std::vector<std::pair<int, int>> ch; ch.push_back({0, n});      // the intercept row's chain: all (kept) cells in original order
    if (C == 1) { for (int q = 0; q < Q; q++) { const int b = ctx->qlev[q]; ch.push_back({ctx->lev_off[b], ctx->lev_cnt[b]}); } }    // a level's cells, ascending
    else for (int b = 0; b < B; b++) ch.push_back({ctx->lev_off[b], ctx->lev_cnt[b]});      // several covariates: one chain per LEVEL (chain 1 + b)
    CHK(seq_plan_build(ctx, ctx->plan_ridge, ch, 1024));      // (measured with k_seq_ridge_pass_kl at 1M cells: 256 / 384 / 512 / 640 / 1024 cells per segment -> ridge statistics 20.3 / 19.1 / 19.3 / 20.1 / 16.6 ms per run)
    size_t cap = 0; CHK(seq_grow(ctx, ctx->inset, cap, (size_t)Q * ((K + 7) / 8 * 8) + 8));
    if (C > 1) {
      // level pairs across covariates: cells stably sorted by (level of c, level of c2), original order inside a pair
      std::vector<int> pl; std::vector<int> pidx((size_t)B * B, -1); std::vector<std::pair<int, int>> pch;
      for (int c = 0; c < C; c++) for (int c2 = c + 1; c2 < C; c2++) {
        std::map<std::pair<int, int>, std::vector<int>> by;
        for (int i = 0; i < n; i++) { const int cell = ctx->invperm_h[i]; const int* lv = &ctx->qlev[(size_t)ctx->combo_h[cell] * C]; by[{lv[c], lv[c2]}].push_back(cell); }
        for (auto& kv : by) {
          pidx[(size_t)kv.first.first * B + kv.first.second] = (int)pch.size();
          pch.push_back({(int)pl.size(), (int)kv.second.size()});
          pl.insert(pl.end(), kv.second.begin(), kv.second.end());
        }
      }
      ctx->npairs = (int)pch.size();
      { size_t c1 = 0, c2 = 0; CHK(seq_grow(ctx, ctx->pairlist, c1, pl.size())); CHK(seq_grow(ctx, ctx->pair_idx, c2, pidx.size()));
        CHK(h2d(ctx, ctx->pairlist, pl.data(), pl.size())); CHK(h2d(ctx, ctx->pair_idx, pidx.data(), pidx.size())); }
      CHK(seq_plan_build(ctx, ctx->plan_pair, pch, 256));
      { size_t c1 = 0, c2 = 0, c3 = 0; CHK(seq_grow(ctx, ctx->rg_tot, c1, (size_t)(1 + B) * K * 64)); CHK(seq_grow(ctx, ctx->rp_tot, c2, (size_t)std::max(ctx->npairs, 1) * K));
        CHK(seq_grow(ctx, ctx->rp_start, c3, (size_t)std::max(ctx->plan_pair.nsegs, 1) * K)); }
    }
  }
  if ((ctx->solve_arith || ctx->oe_arith) && !ctx->solve_on_device) return fail(ctx, HMX_ERR_ARG, "solve_arith / oe_arith need the device-side ridge solve");
  return 0;
}
// E, O of the head in the reference's arithmetic: R has just been rewritten
int oe_head(hmx_ctx* ctx) {
  CHK(seq_run_oe(ctx, ctx->plan_head, ctx->headlist, ctx->headlev, 0, 1));
  l_oe_fold(ctx->L, ctx->D, ctx->Of, ctx->Ef, nullptr, ctx->sq_total, nullptr, 1); KCHK();
  return 0;
}
// compute_objective's three my_accu sums (src/harmony.cpp:160-162) as sequential fp32 chains over K*N terms each -> obj[2..4]
// Dterms: the state the k-means term's distances are taken from (default: the current Z_corr / Y; stale_dist: the snapshot of the last head,
// i.e. the reference's stored dist_mat, src/harmony.cpp:160)
// the three chains in ONE launch: segments of 32 terms in registers, the passes of the fixed-point iteration and the scans between them inside the
// launch (k_seq_obj_fused).  Two halves: objf_begin enqueues the first launch on the run's stream; objf_settle waits for it, continues while the starts
// still move (the host reads the statistics words), and stores the three totals.  seq_objective_fused = both, back to back, on the library's stream.
// objf_begin returns 1 when the shape is outside the kernel's envelope (the caller then takes the pass / scan launches).
int objf_launch(hmx_ctx* ctx, hmx_ctx::ObjfRun& r, int passes, bool zero);
int objf_begin(hmx_ctx* ctx, hmx_ctx::ObjfRun& r) {
  const Dev& D = r.D; const long long nt = r.nt; const int mat = r.mat;
  const int nsegs = seq_obj_fused_nsegs(nt);
  if (mat >= 1 && mat != 3 && (D.K % 4 != 0 || D.C > 4 || !ctx->headlev)) return 1;
  if (ctx->objf_segs != nsegs) { ctx->obj_warm = false; ctx->objf_segs = nsegs; }
  if ((size_t)3 * nsegs > ctx->obj_start_cap) { CHK(seq_grow(ctx, ctx->obj_start, ctx->obj_start_cap, (size_t)3 * nsegs)); ctx->obj_warm = false; }
  const size_t words = seq_obj_fused_slot_words(nt);
  if (words > ctx->objf_slots_cap) {
    CHK(seq_grow(ctx, ctx->objf_slots, ctx->objf_slots_cap, words));
    HIPCHK(hipMemsetAsync(ctx->objf_slots, 0, words * sizeof(unsigned long long), r.L.stream));       // (once: a tag never repeats afterwards)
  }
  if (!ctx->objf_stats) { size_t c = 0; CHK(seq_grow(ctx, ctx->objf_stats, c, 16)); }
  r.adaptive = nt >= ctx->seq_adaptive_cells || ctx->seq_strict;
  const bool warm = ctx->obj_warm;
  int np = warm ? std::max(1, std::min(ctx->seq_warm_passes, ctx->seq_passes)) : ctx->seq_passes;
  // a further pass inside the launch costs one exchange (~0.09 ms at 1M cells), a further LAUNCH reloads the terms (0.4 ms): when the evaluation before
  // this one had to be continued -- the first rounds behind a correction, whose warm starts are stale -- this one takes a third pass up front
  if (r.adaptive && ctx->objf_continued) np++;
  r.np = std::min(np, 8);
  ctx->seq_group_runs[1]++;
  r.done = 0;
  CHK(objf_launch(ctx, r, r.np, !warm));
  return 0;
}
int objf_launch(hmx_ctx* ctx, hmx_ctx::ObjfRun& r, int passes, bool zero) {
  if (!l_seq_obj_fused(r.L, r.D, r.mat == 2 ? 2 : (r.mat == 1 ? 1 : 0), r.T, r.nt, ctx->Mtab, ctx->headlev, r.nt, passes, zero ? 1 : 0, ctx->obj_start, r.tot, ctx->objf_stats,
                       ctx->objf_slots, ++ctx->objf_epoch)) return fail(ctx, HMX_ERR_LIMIT, "objective: fused launch refused");
  KCHK();
  r.done += passes; ctx->seq_group_passes[1] += passes;
  return 0;
}
int objf_settle(hmx_ctx* ctx, hmx_ctx::ObjfRun& r) {
  if (r.adaptive) {
    // What the closing kernel reports: how far the workgroups' starts would still move after the last pass (r_last) and how far they moved one pass
    // earlier (r_prev), relative to the chain totals.  The iteration contracts by about the relative size of the rounding bias per pass (1e-2 at 1M
    // cells, 0.25 where the accumulators saturate at 10M), so what the TOTALS of the last pass are still off by is about r_last * (r_last / r_prev):
    // that product is held below seq_tol / 100 -- the round-5 rule (r_last <= seq_tol) left the same 1e-7 at 1M cells and 25 times more at 10M.
    auto settled = [&](bool* ok) -> int {
      unsigned w[12];
      HIPCHK(hipMemcpyAsync(w, ctx->objf_stats, sizeof(w), hipMemcpyDeviceToHost, r.L.stream));
      HIPCHK(hipStreamSynchronize(r.L.stream));
      if (w[7]) return fail(ctx, HMX_ERR_DEVICE, "objective: the in-launch exchange timed out (code " + std::to_string(w[7]) + ")");
      double rr = 0.0, rp = 0.0;
      for (int c = 0; c < 3; c++) {
        float dm, dp, tt; std::memcpy(&dm, &w[1 + c], 4); std::memcpy(&dp, &w[9 + c], 4); std::memcpy(&tt, &w[4 + c], 4);
        const double den = std::max((double)std::fabs(tt), 1e-30);
        rr = std::max(rr, (double)dm / den); rp = std::max(rp, (double)dp / den);
      }
      const double left = (rp > 0.0) ? rr * std::min(1.0, rr / rp) : rr;
      *ok = w[0] == 0 || (!ctx->seq_strict && (left <= 0.01 * ctx->seq_tol || rr <= ctx->seq_tol));      // (... or the round-5 rule: where the accumulators saturate -- 10M cells -- it is the weaker one)
      ctx->seq_last_mismatch = w[0]; ctx->seq_mismatch_sum += w[0]; if (rr > ctx->seq_resid_max) ctx->seq_resid_max = rr;
      return 0;
    };
    bool ok = false;
    CHK(settled(&ok));
    ctx->objf_continued = !ok;
    while (!ok && r.done < ctx->seq_max_passes) {
      const int before = r.done;
      CHK(objf_launch(ctx, r, std::min(std::max(r.np, 2), std::max(2, ctx->seq_max_passes - r.done)), false));      // (its first pass repeats the last one of the launch before: the starts it left are the ones that pass ran from)
      ctx->seq_extra_passes += r.done - before;
      CHK(settled(&ok));
    }
    if (!ok) ctx->seq_unsettled++;
  }
  ctx->obj_warm = true;
  l_obj_store(r.L, r.tot, r.objv, ctx->objf_stats + 7); KCHK();
  ctx->seq_runs++;
  return 0;
}
int seq_objective_fused(hmx_ctx* ctx, const Dev& D, int mat, long long nt) {
  CHK(seq_workspace(ctx, 1, 3));
  hmx_ctx::ObjfRun r; r.L = ctx->L; r.D = D; r.mat = mat; r.nt = nt; r.T = mat == 2 ? ctx->objD : ctx->objT; r.tot = ctx->sq_total; r.objv = D.obj;
  const int st = objf_begin(ctx, r);
  if (st != 0) return st;
  return objf_settle(ctx, r);
}
int seq_objective(hmx_ctx* ctx, const Dev& D) {
  const long long nt = (long long)ctx->N * ctx->K;
  constexpr int LSEG = 512;      // (round 5: 2048 -> 512 terms per segment: four times the threads for the thread-per-segment passes, which are latency-bound; measured 256 / 512 / 1024: objective 29.6 / 25.9 / 30.4 ms per run)
  const int nsegs = (int)((nt + LSEG - 1) / LSEG);
  CHK(seq_grow(ctx, ctx->objT, ctx->objT_cap, (size_t)3 * (size_t)nt));
  CHK(seq_workspace(ctx, (size_t)3 * nsegs, 3));
  if ((size_t)3 * nsegs > ctx->obj_start_cap) { CHK(seq_grow(ctx, ctx->obj_start, ctx->obj_start_cap, (size_t)3 * nsegs)); ctx->obj_warm = false; }
  CHK(seq_grow(ctx, ctx->obj_partial, ctx->obj_partial_cap, (size_t)3 * ((nsegs + 255) / 256)));
  // (round 6) inside hmx_cluster's round loop dist_mat is computed by the call's FIRST evaluation and kept: the later ones skip the terms kernel (0.25 ms of 0.75 per
  // evaluation at 1M cells) and form R % dist inside the fused launch, with the same single rounding
  const bool cache = ctx->obj_fused && ctx->obj_dist_cache && ctx->in_cluster_rounds && &D == &ctx->D && !D.obj_stale && D.K % 4 == 0 && D.C <= 4 && ctx->headlev;
  int mat = 0;
  if (cache) {
    CHK(seq_grow(ctx, ctx->objD, ctx->objD_cap, (size_t)nt));
    mat = l_obj_terms(ctx->L, D, ctx->oe_arith ? ctx->Of : nullptr, ctx->oe_arith ? ctx->Ef : nullptr, ctx->Mtab, ctx->objD, nt, ctx->objD_valid ? 2 : 1); KCHK();
    if (mat == 2) {
      ctx->objD_valid = true;
      const int st = seq_objective_fused(ctx, D, 2, nt);
      if (st != 1) return st;
    }
    ctx->objD_valid = false;        // (the MFMA terms kernel or the fused launch does not take this shape: the ordinary forms below)
  }
  mat = l_obj_terms(ctx->L, D, ctx->oe_arith ? ctx->Of : nullptr, ctx->oe_arith ? ctx->Ef : nullptr, ctx->Mtab, ctx->objT, nt); KCHK();
  // mat == 1: only R % dist is materialised; the entropy / cross-entropy chains are summed straight from R (k_seq_obj_fused, k_seq_objr_pass)
  if (ctx->obj_fused) { const int st = seq_objective_fused(ctx, D, mat, nt); if (st != 1) return st; }
  if (ctx->objf_segs) { ctx->obj_warm = false; ctx->objf_segs = 0; }      // (the starts the buffer holds belong to the fused launch's segments)
  CHK(seq_iterate(ctx, 1, ctx->obj_warm, nt >= ctx->seq_adaptive_cells,
                  [&](bool zero, unsigned* cz) -> int {
                    l_seq_arr_pass(ctx->L, ctx->objT, nt, nt, mat, LSEG, nsegs, ctx->obj_start, ctx->sq_end, zero ? 1 : 0, ctx->obj_partial, cz); KCHK();
                    if (mat == 1) { l_seq_objr_pass(ctx->L, D, ctx->Mtab, nt, LSEG, nsegs, ctx->obj_start, ctx->sq_end, zero ? 1 : 0, ctx->obj_partial); KCHK(); }
                    return 0; },
                  [&](bool zero, unsigned* conv) -> int { l_seq_scan1(ctx->L, 3, nsegs, ctx->obj_start, ctx->sq_end, ctx->obj_start, ctx->sq_total, conv, zero ? 1 : 0, ctx->obj_partial); KCHK(); return 0; }));
  ctx->obj_warm = true;
  l_obj_store(ctx->L, ctx->sq_total, D.obj); KCHK();
  ctx->seq_runs++;
  return 0;
}
// the objective snapshot obj[2..4] from what the last pass over the cells left behind (obj[0..1]: exact per-cell sums)
int objective_snapshot(hmx_ctx* ctx, const Dev* Dterms) {
  l_objective_tables(ctx->L, ctx->D); KCHK();      // (also resets the block chain's control words)
  if (ctx->obj_arith) return seq_objective(ctx, Dterms ? *Dterms : ctx->D);
  if (ctx->oe_arith) { l_obj_cross_f32(ctx->L, ctx->D, ctx->Of, ctx->Ef, ctx->Mtab); KCHK(); }
  return 0;
}
// ridge statistics in the reference's arithmetic (ridge_arith = 1, one covariate): per cluster the intercept row's chain over all kept
// cells in original order (sum(Z_tmp, 1), :599) and a chain per level over its cells (sum(Z_tmp.cols(index[b]), 1), :605-608;
// Phi_Rk * Phi_moe_t, :567) -> S0 / n0, Sq / nq
int seq_ridge_stats(hmx_ctx* ctx) {
  const Dev& D = ctx->D;
  const hmx_ctx::SeqPlan& P = ctx->plan_ridge;
  // round 6: lane = cluster (k_seq_ridge_pass_kl): the segments' starts / ends hold [d + 1][K] per segment instead of [K][64]; the chain totals are handed
  // to the consumers (k_seq_ridge_store, k_moe_solve) in the old [chain][K][64] layout by a small kernel
  const bool kl = ctx->ridge_kl && D.zs <= 64 && D.zs % 4 == 0;
  const int W = kl ? (ctx->d + 1) * ctx->K : ctx->K * 64;
  const bool multi = ctx->C > 1;
  CHK(seq_workspace(ctx, (size_t)P.nsegs * W, (size_t)P.nchains * ctx->K * 64));
  float* const tot = multi ? ctx->rg_tot : ctx->sq_total;          // (after the workspace call: it may have re-allocated sq_total)
  if (kl) { size_t c = ctx->rg_totkl_cap; CHK(seq_grow(ctx, ctx->rg_totkl, c, (size_t)P.nchains * W)); ctx->rg_totkl_cap = c; }
  if ((size_t)P.nsegs * W > ctx->rg_start_cap || ctx->rg_start_kl != (kl ? 1 : 0)) {
    if ((size_t)P.nsegs * W > ctx->rg_start_cap) CHK(seq_grow(ctx, ctx->rg_start, ctx->rg_start_cap, (size_t)P.nsegs * W));
    ctx->rg_warm = false; ctx->rg_start_kl = kl ? 1 : 0; }
  l_seq_inset(ctx->L, D, ctx->oe_arith ? ctx->Of : nullptr, ctx->sv_cov_bounds, ctx->cutoff, ctx->inset); KCHK();
  CHK(seq_iterate(ctx, 2, ctx->rg_warm, ctx->N >= ctx->seq_adaptive_cells,
                  [&](bool zero, unsigned* cz) -> int {
                    if (kl) { if (!l_seq_ridge_pass_kl(ctx->L, D, ctx->headlist, P.d_segs, 0, P.nsegs, ctx->inset, ctx->rg_start, ctx->sq_end, zero ? 1 : 0, cz)) return fail(ctx, HMX_ERR_LIMIT, "ridge pass: shape refused"); }
                    else l_seq_ridge_pass(ctx->L, D, ctx->headlist, ctx->headq, P.d_segs, 0, P.nsegs, ctx->inset, ctx->rg_start, ctx->sq_end, zero ? 1 : 0, cz);
                    KCHK(); return 0; },
                  [&](bool zero, unsigned* conv) -> int { l_seq_scan(ctx->L, P.d_chains, 0, P.nchains, W, ctx->rg_start, ctx->sq_end, ctx->rg_start, kl ? ctx->rg_totkl : tot, conv, zero ? 1 : 0); KCHK(); return 0; }));
  if (kl) { l_seq_ridge_rows2lanes(ctx->L, ctx->rg_totkl, tot, P.nchains, ctx->K, ctx->d); KCHK(); }
  ctx->rg_warm = true;
  ctx->seq_runs++;
  if (!multi) { l_seq_ridge_store(ctx->L, D, ctx->sq_total); KCHK(); return 0; }
  // several covariates: the level-pair entries of Phi_Rk * Phi_moe_t (:561-568): plain sequential sums of R_k over each pair's cells
  const hmx_ctx::SeqPlan& PP = ctx->plan_pair;
  if (PP.nchains > 0) {
    CHK(seq_workspace(ctx, (size_t)PP.nsegs * ctx->K, 1));
    int longest = 0;
    for (int c = 0; c < PP.nchains; c++) longest = std::max(longest, PP.seg0[c + 1] - PP.seg0[c]);
    CHK(seq_iterate(ctx, 3, ctx->rp_warm, (int64_t)longest * PP.seg_cells >= ctx->seq_adaptive_cells,
                    [&](bool zero, unsigned* cz) -> int { l_seq_sum_pass(ctx->L, D, ctx->pairlist, PP.d_segs, 0, PP.nsegs, ctx->rp_start, ctx->sq_end, zero ? 1 : 0, cz); KCHK(); return 0; },
                    [&](bool zero, unsigned* conv) -> int { l_seq_scan(ctx->L, PP.d_chains, 0, PP.nchains, ctx->K, ctx->rp_start, ctx->sq_end, ctx->rp_start, ctx->rp_tot, conv, zero ? 1 : 0); KCHK(); return 0; }));
    ctx->rp_warm = true;
    ctx->seq_runs++;
  }
  return 0;
}

// update_R with the reference's O / E arithmetic (oe_arith): the tables are fp32 and every block removes / puts back its cells'
// sums exactly as src/harmony.cpp:312-313,329-330 -- sequential fp32 sums in the round's shuffled order, formed first, then one
// subtraction / addition per table entry.  One launch of the tile kernel per block (penalty table from memory), the block chain's
// persistent launch does not apply.  Host-visible shuffle: the order is materialised on the host whatever its source.
int update_R_ref(hmx_ctx* ctx) {
  Dev& D = ctx->D;
  const double t0 = now_ms();
  const int n = (int)ctx->N, B = ctx->B, K = ctx->K, nb = ctx->nb;
  const hmx_ctx::SeqPlan& P = ctx->plan_round;
  ctx->R_valid = false; D.r_store = 1;
  { PhaseScope ph(ctx, "randomize");
    if (!ctx->injected.empty() || ctx->rng_mode == 1) {       // the host owns the shuffle: its order goes to the device as it is
      if (ctx->injected.empty()) { ensure_rrng(ctx); std::vector<int64_t> o; ctx->rrng.arma_shuffle(ctx->N_global, o); ctx->injected.push_back(std::move(o)); }
      const std::vector<int64_t>& order = ctx->injected.front();
      std::vector<int> po((size_t)n);
      for (int p = 0; p < n; p++) po[p] = ctx->invperm_h[(size_t)order[p]];
      CHK(h2d(ctx, ctx->roundlist, po.data(), po.size()));
      { const int Cl = std::min(ctx->C, 4); std::vector<int> lv((size_t)Cl * n);
        for (int p = 0; p < n; p++) for (int c = 0; c < Cl; c++) lv[(size_t)c * n + p] = ctx->qlev[(size_t)ctx->combo_h[po[p]] * ctx->C + c];
        CHK(h2d(ctx, ctx->roundlev, lv.data(), lv.size())); }
    } else { l_ref_posord(ctx->L, D, ctx->seed, ctx->round_counter, (uint64_t)ctx->N_global, ctx->roundlist, ctx->roundlev); KCHK(); }
    CHK(prepare_round(ctx, ctx->round_counter)); }             // the tile kernels' padded block order, from the same shuffle
  ctx->round_counter++;
  HIPCHK(hipMemsetAsync(D.Snew_fx, 0, sizeof(long long) * (size_t)D.nrep * B * K, ctx->L.stream));   // (the kernel's fixed-point sums are not used here)
  const int W = (1 + B) * K;
  { PhaseScope ph(ctx, "EO_update");     // every block's cells are still untouched at this point: the sums each block will remove (:312-313), all at once
    CHK(seq_run_oe(ctx, P, ctx->roundlist, ctx->roundlev, 0, nb)); }
  D.fused_fold = 0; D.Sold_next = nullptr;
  const float* put_back = nullptr;                                   // the sums of the block updated last, still to be added back (:329-330)
  for (int j = 0; j < nb; j++) {
    if (P.seg0[j + 1] == P.seg0[j]) continue;                      // N * block_size rounding can leave trailing empty blocks
    float* tot = ctx->sq_total + (size_t)j * W;
    // one launch: the previous block goes back in, this block comes out, this block's penalty table (:329-330, :312-313, :322)
    { PhaseScope ph(ctx, "EO_update"); l_oe_fold(ctx->L, D, ctx->Of, ctx->Ef, put_back, tot, D.pen, 0); KCHK(); }
    { Launch Le; CHK(launch_with_events(ctx, Le)); CHK(tile_ran(ctx, TileKind::Update, l_update(Le, D, j))); KCHK(); if (ctx->profile) ctx->prof_update_steps++; }
    { PhaseScope ph(ctx, "EO_update");
      // the same cells in the same order as the sums removed above, their R rows updated: that run's segment starts are this run's first guess
      CHK(seq_run_oe(ctx, P, ctx->roundlist, ctx->roundlev, j, 1, true)); }
    put_back = tot;
  }
  if (put_back) { PhaseScope ph(ctx, "EO_update"); l_oe_fold(ctx->L, D, ctx->Of, ctx->Ef, put_back, nullptr, nullptr, 0); KCHK(); }
  { PhaseScope ph(ctx, "objective");
    l_obj_reduce(ctx->L, D); KCHK();
    // (measured in round 6 and removed: this evaluation on a side stream beside the NEXT round's block steps -- nothing needs the value before -- on a snapshot of R.
    //  Bit-identical, and no gain: the one large launch and the chain of small dependent ones do not overlap, the block steps took exactly the 10 ms longer that the
    //  objective left the library's stream, with the library's stream at the highest priority as well: 71.9 / 72.6 ms against 70.5 / 71.4 in line.)
    CHK(objective_snapshot(ctx)); }
  CHK(push_objective(ctx));
  ctx->ledger.sets_used(); ctx->ledger.r_rewritten();
  if (ctx->profile) ctx->prof_update_cells += ctx->N;
  ctx->R_valid = true;
  ctx->timers["update_R"] += now_ms() - t0;
  return 0;
}

// hmx_api_update.inc -- part of hmx_api.cpp (included there, ONE translation unit): update_R: the rounds of a cluster_cpp call (chain / launch-per-step, carry, R-store elision)
// ---- update_R (src/harmony.cpp:269-342) ---------------------------------------------------------
int update_R(hmx_ctx* ctx) {
  if (ctx->oe_arith) return update_R_ref(ctx);
  Dev& D = ctx->D;
  const bool sharded = ctx->world > 1 || ctx->comm_force;
  const char* fold_env = getenv("HMX_FOLD_IMPL");   // "split": force the two-kernel fold + penalty fallback (tests)
  // k_foldpen (one launch, K/16 workgroups, every thread walks B/16 levels x the replicas) suits small tables; with thousands of
  // entries (configs[4]: 200 levels x 200 clusters) one thread per entry in two launches is faster, unless the fused / chain paths apply
  const bool merged = (size_t)D.B * 128 <= 64 * 1024 && !(fold_env && std::string(fold_env) == "split") &&
                      (ctx->fused_ok || (size_t)D.B * D.K <= 8192 || (fold_env && std::string(fold_env) == "merged"));   // LDS budget of k_foldpen
  const double t0 = now_ms();
  ctx->R_valid = false;
  { PhaseScope ph(ctx, "randomize");      // the round's shuffle (:272-291, timers "randomize")
    CHK(prepare_round(ctx, ctx->round_counter)); }
  ctx->round_counter++;
  // sharded: the chain needs the in-launch exchange over the peers' inboxes (hmx_p2p_*); without it, one launch + one collective per block
  const bool p2p = sharded && ctx->p2p_on && ctx->p2p_world == ctx->world && !ctx->comm_force && (size_t)D.B * D.K <= (size_t)P2P_CAP;
  const bool chain_path = (merged && ctx->fused_ok && ctx->chain_ok && (!sharded || p2p)) || (D.chain_pair && (!sharded || p2p));      // (the wave-pair chain, K = 200)
  D.p2p_world = p2p ? ctx->p2p_world : 0; D.p2p_rank = ctx->p2p_rank;
  for (int g = 0; g < 8; g++) D.p2p_inbox[g] = ctx->p2p_peer[g];
  { PhaseScope ph(ctx, "EO_update");      // removal of every block's old contribution (:312-313)
    D.r_store = 1;
    {
      const size_t nBKs = (size_t)D.B * D.K, nSold = (size_t)D.nb * nBKs, nSets = 3 * (size_t)D.nrep * nBKs;
      const int cur = ctx->sold_cur, oth = cur ^ 1;
      const int64_t rnd = (int64_t)ctx->round_counter - 1;          // this round
      D.Sold_fx = ctx->sold_buf[cur];
      if (!ctx->sets_clean) { HIPCHK(hipMemsetAsync(D.Snew_set[0], 0, sizeof(long long) * nSets, ctx->L.stream)); ctx->sets_clean = true; }
      const bool carried = ctx->sold_state[cur] == 2 && ctx->sold_round[cur] == rnd && ctx->sold_seed[cur] == ctx->seed &&
                           ctx->sorted_round[rnd & ctx->oset_mask] == rnd && ctx->sorted_seed[rnd & ctx->oset_mask] == ctx->seed;   // (same Feistel permutation as the sort's)
      if (carried) ctx->carried_rounds++;     // filled by the previous round's tile kernels: no pass over R
      else {             // all blocks in one pass over R
        if (ctx->sold_state[cur] != 0) HIPCHK(hipMemsetAsync(D.Sold_fx, 0, sizeof(long long) * nSold, ctx->L.stream));
        if (ctx->shuf_inv && ctx->injected_round != rnd) {      // (the sort-free shuffle leaves D.blk alone: block ids of this round's cells, on demand)
          l_shuffle_blocks(ctx->L, D, ctx->seed, (uint64_t)rnd, (uint64_t)ctx->N_global, (uint64_t)ctx->goff, ctx->cells_per_block); KCHK(); }
        l_oldsum(ctx->L, D); KCHK();
      }
      ctx->sold_state[cur] = 1;
      if (!(chain_path && p2p)) CHK(allreduce(ctx, D.Sold_fx, (int64_t)nSold, 0));      // (p2p chain: the folder exchanges new(j - 1) - old_local(j), the ranks' old sums meet there)
      // this round's tile kernels collect the next round's old contributions if this round's tiles are keyed by the next block
      const bool write_next = ctx->carry_ok && ctx->sorted_nxt[rnd & ctx->oset_mask] && !ctx->last_round_hint;
      D.Sold_next = nullptr;
      if (write_next) {
        if (ctx->sold_state[oth] != 0) HIPCHK(hipMemsetAsync(ctx->sold_buf[oth], 0, sizeof(long long) * nSold, ctx->L.stream));
        D.Sold_next = ctx->sold_buf[oth];
        ctx->sold_state[oth] = 2; ctx->sold_round[oth] = rnd + 1; ctx->sold_seed[oth] = ctx->seed;
      }
      ctx->sets_clean = false;
      // R rows nobody reads are not written: this round's rows are dead if the NEXT round takes its old contributions from the carried sums
      // (write_next) and this round cannot be the call's last (round_may_be_last, set by hmx_cluster) -- moe_correct_ridge_cpp, the getters
      // and a stand-alone compute_objective only ever see the last round's R.  (A host with an abort poll may leave the call early: it
      // always gets its rows.  HMX_R_STORE=1: always store.  obj_arith: the round's objective is summed from R itself -- k_obj_terms_mfma and
      // every pass of k_seq_objr_pass read the rows -- so every round stores them.)
      D.r_store = (write_next && !ctx->round_may_be_last && !ctx->poll && !ctx->r_store_always && !ctx->obj_arith) ? 0 : 1;
      if (!D.r_store) ctx->rounds_without_R++;
    } }
  // (objpart needs no memset here: k_obj_reduce zeroes every slot it reads, setup / head_pass zero it initially)
  bool round_done = false;   // set by the fused path: all block steps done, skip the step loop below
  bool chain_tail = false;   // the persistent chain closed the round by itself
  const bool fused = merged && ctx->fused_ok;
  if (chain_path) {
    // default on one GPU: the whole block chain in ONE persistent launch (k_tile MODE 4)
    // (chain_ctl was reset by the launch that closed the previous round: k_round_tail / k_objective_tables.  The shuffle kernels must
    //  not touch chain_ctl, pen_g or the Sold buffers: prefetch_next() runs them on the side stream while a chain may be in flight)
    D.chain_tag = (unsigned)(1 + (ctx->chain_rounds++ % (1u << 24)) * 64);
    D.chain_xseq = ctx->p2p_xseq;
    long long* const keep_snew = D.Snew_fx;
    D.Snew_fx = D.Snew_set[0];     // one replica set: the folder resets it by exchange (zeroed by the round's memset)
    // one GPU: the chain's folder also closes the round (objective snapshot, table clears, control reset): no k_round_tail launch
    // (sharded runs with the in-launch exchange too: the ranks' objective sums travel through the inboxes, entries nBK and nBK + 1)
    chain_tail = (!sharded || (p2p && (size_t)D.B * D.K + 2 <= (size_t)P2P_CAP && D.nb <= 62)) && !ctx->obj_arith && !D.chain_pair;      // (several folders, a slice of the table each: k_round_tail closes the round)
    D.chain_tail = chain_tail ? 1 : 0;
    if (p2p) ctx->p2p_xseq += (unsigned)D.nb + 1u + (chain_tail ? 1u : 0u);      // exchanges of this round: nb + 1 block steps (+ the objective's)
    if (chain_tail) {
      double* slot = nullptr;
      CHK(objective_slot(ctx, &slot));
      const size_t nBKs = (size_t)D.B * D.K;
      D.tail_host_slot = slot; D.tail_z0 = D.Sold_fx; D.tail_n0 = (unsigned long long)D.nb * nBKs;
      D.tail_z1 = D.Snew_set[0]; D.tail_n1 = 3ull * (unsigned long long)D.nrep * nBKs;
    }
    {
      ChainGate& gate = chain_gate();
      std::lock_guard<std::mutex> lk(gate.mu);
      hipEvent_t& ev = gate.last[ctx->device];
      const void*& owner = gate.owner[ctx->device];
      if (!ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      else if (owner != (const void*)ctx->L.stream) HIPCHK(hipStreamWaitEvent(ctx->L.stream, ev, 0));   // (the same stream orders its own launches: no event, ~20 us of barrier packet less per round)
      { Launch Le; CHK(launch_with_events(ctx, Le)); CHK(tile_ran(ctx, TileKind::Chain, l_chain(Le, D, ctx->chain_wgs))); KCHK(); }
      HIPCHK(hipEventRecord(ev, ctx->L.stream));
      owner = (const void*)ctx->L.stream;
    }
    D.chain_tail = 0;
    if (ctx->profile) ctx->prof_update_steps += D.nb;
    D.Snew_fx = keep_snew;
    ctx->chain_check = true;
    round_done = true;
  } else if (fused) {
    // default: the fold + penalty of step j happens in the prologue of its own update launch.  Sharded: the replica set a
    // launch has filled is all-reduced IN PLACE (nrep*B*K int64, 64 KB at C4: latency-bound like the 8 KB of one table), so
    // the next launch's prologue sums global replicas exactly as it sums local ones -- one kernel + one collective per block
    // step instead of three kernels + one collective.
    long long* const keep_snew = D.Snew_fx;
    D.fused_fold = 1;
    for (int j = 0; j < D.nb; j++) {
      D.fold_prev = D.Snew_set[(j + 2) % 3]; D.Snew_fx = D.Snew_set[j % 3]; D.fold_zero = D.Snew_set[(j + 1) % 3];
      { Launch Le; CHK(launch_with_events(ctx, Le)); CHK(tile_ran(ctx, TileKind::Update, l_update(Le, D, j))); KCHK(); }
      if (ctx->profile) ctx->prof_update_steps++;
      if (sharded) CHK(allreduce(ctx, D.Snew_fx, (int64_t)D.nrep * D.B * D.K, 0));   // this block's new contribution, all ranks
      std::swap(D.O_fx, D.O_alt);   // workgroup 0 published O' into O_alt
    }
    D.fused_fold = 0;
    // O += new(last block): fold-only launch; the set it zeroes is one of the three (re-zeroed next round anyway)
    l_foldpen(ctx->L, D, -1, D.O_fx, D.O_alt, D.Snew_set[(D.nb - 1) % 3], D.Snew_set[D.nb % 3]); KCHK();
    std::swap(D.O_fx, D.O_alt);
    D.Snew_fx = keep_snew;
    round_done = true;
  }
  for (int j = 0; j <= D.nb && !round_done; j++) {
    // fold the previous block's new contribution into O, remove block j's old one (src/harmony.cpp:312-313,329-330)
    if (sharded) {  // shard-local replicas -> one table, summed over the ranks (the only collective of a block step)
      l_fold(ctx->L, D, j, 1); KCHK();
      CHK(allreduce(ctx, D.Snew_fx, (int64_t)D.B * D.K, 0));
    }
    if (merged) {
      // one launch: O' = O + new(prev) - old(j) and the penalty table; ping-pong so nothing is read while written
      l_foldpen(ctx->L, D, j < D.nb ? j : -1, D.O_fx, D.O_alt, D.Snew_fx, D.Snew_alt); KCHK();
      std::swap(D.O_fx, D.O_alt); std::swap(D.Snew_fx, D.Snew_alt);
    } else {
      l_fold(ctx->L, D, j < D.nb ? j : -1, sharded ? 2 : 0); KCHK();
      if (j < D.nb) { l_penalty(ctx->L, D); KCHK(); }
    }
    if (j == D.nb) break;
    { Launch Le; CHK(launch_with_events(ctx, Le)); CHK(tile_ran(ctx, TileKind::Update, l_update(Le, D, j))); KCHK(); if (ctx->profile) ctx->prof_update_steps++; }
  }
  if (chain_tail) {
    ctx->sold_state[ctx->sold_cur] = 0;
    ctx->sets_clean = true;
    HIPCHK(hipEventRecord(ctx->obj_event, ctx->L.stream));
    ctx->obj_pending++;
  } else if (!sharded && !ctx->obj_arith) {
    // one launch: slot rows -> objective terms -> snapshot written STRAIGHT into the pinned host slot (no copy engine, no
    // second launch), chain control reset.  Resolved by flush_objectives (event) when a value is needed.
    double* slot = nullptr;
    CHK(objective_slot(ctx, &slot));
    {   // the table this round consumed and the replica sets are cleared by the same launch
      const size_t nBKs = (size_t)D.B * D.K;
      const size_t n0 = (size_t)D.nb * nBKs, n1 = 3 * (size_t)D.nrep * nBKs;
      if (n0 + n1 > ((size_t)1 << 18)) {
        // many-level designs (configs[4]: 7.4 MB of tables): the tail's few workgroups -- one per slot row -- needed 88 us for the clears (rocprofv3, round 6: 2.5 ms
        // of a 52 ms run); a wide clearing launch in front of it instead
        l_zero4(ctx->L, D.Sold_fx, n0, D.Snew_set[0], n1, nullptr, 0, nullptr, 0); KCHK();
        l_round_tail(ctx->L, D, slot, D.Sold_fx, 0, D.Snew_set[0], 0); KCHK();
      } else { l_round_tail(ctx->L, D, slot, D.Sold_fx, n0, D.Snew_set[0], n1); KCHK(); }
      ctx->sold_state[ctx->sold_cur] = 0;
      ctx->sets_clean = true;
    }
    HIPCHK(hipEventRecord(ctx->obj_event, ctx->L.stream));
    ctx->obj_pending++;
  } else {
    l_obj_reduce(ctx->L, D); KCHK();
    CHK(allreduce(ctx, D.obj, 2, 1));
    CHK(objective_snapshot(ctx));
    CHK(push_objective(ctx));  // asynchronous: resolved by flush_objectives when a value is needed
  }
  ctx->sold_cur ^= 1;      // next round subtracts what this round's tile kernels collected (or a fresh k_oldsum pass)
  D.Sold_next = nullptr;
  ctx->R_valid = D.r_store != 0;
  if (ctx->profile) { ctx->prof_update_cells += ctx->N; }   // the event pairs are resolved when a "prof:*" field is read
  ctx->timers["update_R"] += now_ms() - t0;
  return 0;
}

// hmx_api_update.inc -- part of hmx_api.cpp (included there, ONE translation unit): update_R: the rounds of a cluster_cpp call (chain / launch-per-step, carry, R-store elision)
// ---- the chain gate (ChainGate, hmx_api.cpp): the stream of the last chain launch OWNS the device's gate; its own launches are ordered by the stream, with
// no event at all.  A launch from another stream records the gate's event on the owner's stream -- under the gate's mutex, so behind the owner's last chain
// launch -- and waits for it: the exclusion between two handles' persistent launches is what an event per launch gave.  An owner that goes away (hmx_destroy,
// hmx_set_stream) records once and leaves the event armed for whoever launches next.  A caller's stream must therefore outlive its handle (or be replaced through
// hmx_set_stream first); if the record on an owner's stream fails all the same, ownership is dropped and the launch waits for the whole device instead.
int chain_gate_enter(hmx_ctx* ctx, ChainGate& gate) {      // gate.mu held
  ChainGate::PerDevice& g = gate.dev[ctx->device];
  const bool mine = g.owned && g.owner == ctx->L.stream;
  if (g.owned && !mine) {
    hipError_t e = g.ev ? hipSuccess : hipEventCreateWithFlags(&g.ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(g.ev, g.owner);
    g.owned = false; g.owner = nullptr;
    if (e == hipSuccess) { ctx->n_event_records++; ctx->n_gate_records++; g.armed = true; }
    else {      // the owner's stream is gone (a caller's stream destroyed without hmx_set_stream): nothing can be recorded behind its launches -- wait for the device
      (void)hipGetLastError(); g.armed = false;
      HIPCHK(hipDeviceSynchronize());
    }
  }
  if (g.armed && !mine) HIPCHK(hipStreamWaitEvent(ctx->L.stream, g.ev, 0));
  g.armed = false;
  return 0;
}
void chain_gate_own(hmx_ctx* ctx, ChainGate& gate) { ChainGate::PerDevice& g = gate.dev[ctx->device]; g.owned = true; g.owner = ctx->L.stream; }      // gate.mu held, behind the launch
void chain_gate_release(hmx_ctx* ctx) {      // the handle's stream is about to go away (or to be replaced)
  if (ctx->device < 0) return;
  ChainGate& gate = chain_gate();
  std::lock_guard<std::mutex> lk(gate.mu);
  auto it = gate.dev.find(ctx->device);
  if (it == gate.dev.end() || !it->second.owned || it->second.owner != ctx->L.stream) return;
  ChainGate::PerDevice& g = it->second;
  (void)hipSetDevice(ctx->device);
  if (!g.ev && hipEventCreateWithFlags(&g.ev, hipEventDisableTiming) != hipSuccess) g.ev = nullptr;
  if (g.ev && hipEventRecord(g.ev, ctx->L.stream) == hipSuccess) { ctx->n_event_records++; ctx->n_gate_records++; g.armed = true; }
  else { (void)hipGetLastError(); (void)hipStreamSynchronize(ctx->L.stream); }      // (no event: the launches end before the stream goes)
  g.owned = false; g.owner = nullptr;
}
// ---- update_R (src/harmony.cpp:269-342) ---------------------------------------------------------
int update_R(hmx_ctx* ctx) {
  if (ctx->oe_arith) return update_R_ref(ctx);
  const bool sharded = ctx->world > 1 || ctx->comm_force;
  const double t0 = now_ms();
  ctx->R_valid = false;
  { PhaseScope ph(ctx, "randomize");      // the round's shuffle (:272-291, timers "randomize")
    CHK(prepare_round(ctx, ctx->round_counter)); }
  const int64_t rnd = (int64_t)ctx->round_counter++;          // this round
  RoundLedger& lg = ctx->ledger;
  RoundIn in;      // every decision of the round: plan_round (hmx_round.h); below, only dispatch
  in.sharded = sharded; in.inbox_ok = ctx->p2p_on && ctx->p2p_world == ctx->world && !ctx->comm_force;
  in.B = ctx->D.B; in.K = ctx->D.K; in.nb = ctx->D.nb; in.nrep = ctx->D.nrep; in.p2p_cap = P2P_CAP;
  in.fused_ok = ctx->fused_ok; in.chain_ok = ctx->chain_ok; in.chain_pair = ctx->D.chain_pair != 0; in.carry_ok = ctx->carry_ok; in.shuf_inv = ctx->shuf_inv;
  in.obj_arith = ctx->obj_arith != 0; in.poll = ctx->poll != nullptr; in.r_store_always = ctx->r_store_always; in.last_round_hint = ctx->last_round_hint; in.round_may_be_last = ctx->round_may_be_last;
  in.seed = ctx->seed; in.round = rnd; in.injected_round = ctx->injected_round; in.fold_impl = ctx->fold_impl;
  const RoundPlan rp = plan_round(in, lg);
  ctx->last_round = rp; ctx->round_seen = true;
  Dev D = ctx->D;      // the round's own copy: what is set per launch does not outlive the round
  const size_t nBK = (size_t)D.B * D.K, nSold = (size_t)D.nb * nBK, nSets = 3 * (size_t)D.nrep * nBK;
  D.p2p_world = rp.p2p ? ctx->p2p_world : 0; D.p2p_rank = ctx->p2p_rank;
  for (int g = 0; g < 8; g++) D.p2p_inbox[g] = ctx->p2p_peer[g];
  D.Sold_fx = ctx->sold_buf[lg.cur]; D.Sold_next = rp.write_next ? ctx->sold_buf[lg.cur ^ 1] : nullptr; D.r_store = rp.r_store;
  { PhaseScope ph(ctx, "EO_update");      // removal of every block's old contribution (:312-313)
    if (rp.clear_sets) HIPCHK(hipMemsetAsync(D.Snew_set[0], 0, sizeof(long long) * nSets, ctx->L.stream));
    if (rp.carried) ctx->carried_rounds++;     // filled by the previous round's tile kernels: no pass over R
    else {             // all blocks in one pass over R
      if (rp.clear_cur) HIPCHK(hipMemsetAsync(D.Sold_fx, 0, sizeof(long long) * nSold, ctx->L.stream));
      if (rp.gen_blocks) { l_shuffle_blocks(ctx->L, D, ctx->seed, (uint64_t)rnd, (uint64_t)ctx->N_global, (uint64_t)ctx->goff, ctx->cells_per_block); KCHK(); }      // block ids of this round's cells, on demand
      l_oldsum(ctx->L, D); KCHK();
    }
    lg.round_started();
    if (rp.path == PATH_STEP_LOOP) lg.step_loop_used();
    if (rp.reduce_old) CHK(allreduce(ctx, D.Sold_fx, (int64_t)nSold, 0));      // (p2p chain: the folder exchanges new(j - 1) - old_local(j), the ranks' old sums meet there)
    if (rp.clear_next) HIPCHK(hipMemsetAsync(D.Sold_next, 0, sizeof(long long) * nSold, ctx->L.stream));
    if (rp.write_next) lg.round_filed_next(rnd, ctx->seed);
    if (!rp.r_store) ctx->rounds_without_R++;
  }
  // (objpart needs no memset here: k_obj_reduce zeroes every slot it reads, setup / head_pass zero it initially)
  if (rp.path == PATH_CHAIN) {
    // default on one GPU: the whole block chain in ONE persistent launch (k_tile MODE 4)
    // (chain_ctl was reset by the launch that closed the previous round: k_round_tail / k_objective_tables)
    D.chain_tag = (unsigned)(1 + (ctx->chain_rounds++ % (1u << 24)) * 64); D.chain_xseq = ctx->p2p_xseq;
    D.Snew_fx = D.Snew_set[0];     // one replica set: the folder resets it by exchange (zeroed by the round's memset)
    D.chain_tail = rp.chain_tail ? 1 : 0; ctx->p2p_xseq += rp.exchanges;
    if (rp.chain_tail) {      // the chain's folder also closes the round: no k_round_tail launch
      CHK(objective_slot(ctx, &D.tail_host_slot));
      D.tail_z0 = D.Sold_fx; D.tail_n0 = (unsigned long long)nSold;
      D.tail_z1 = D.Snew_set[0]; D.tail_n1 = (unsigned long long)nSets;
    }
    {
      ChainGate& gate = chain_gate();
      std::lock_guard<std::mutex> lk(gate.mu);
      CHK(chain_gate_enter(ctx, gate));      // (the same stream orders its own launches: no event recorded, none waited for)
      { Launch Le; CHK(launch_with_events(ctx, Le)); CHK(tile_ran(ctx, TileKind::Chain, l_chain(Le, D, ctx->chain_wgs))); KCHK(); }
      chain_gate_own(ctx, gate);
    }
    if (ctx->profile) ctx->prof_update_steps += D.nb;
    ctx->chain_check = true;
  } else if (rp.path == PATH_FOLD_PROLOGUE) {
    // default: the fold + penalty of step j happens in the prologue of its own update launch.  Sharded: the replica set a
    // launch has filled is all-reduced IN PLACE (nrep*B*K int64, 64 KB at C4: latency-bound like the 8 KB of one table), so
    // the next launch's prologue sums global replicas exactly as it sums local ones -- one kernel + one collective per block
    // step instead of three kernels + one collective.
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
  } else for (int j = 0; j <= D.nb; j++) {
    // fold the previous block's new contribution into O, remove block j's old one (src/harmony.cpp:312-313,329-330)
    if (sharded) {  // shard-local replicas -> one table, summed over the ranks (the only collective of a block step)
      l_fold(ctx->L, D, j, 1); KCHK();
      CHK(allreduce(ctx, D.Snew_fx, (int64_t)D.B * D.K, 0));
    }
    if (rp.merged) {
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
  // what persists of the round's copy: the ping-pong partners as the folds left them
  ctx->D.O_fx = D.O_fx; ctx->D.O_alt = D.O_alt;
  if (rp.path == PATH_STEP_LOOP) { ctx->D.Snew_fx = D.Snew_fx; ctx->D.Snew_alt = D.Snew_alt; }
  else D.Snew_fx = ctx->D.Snew_fx;
  if (rp.close == CLOSE_REDUCE_SNAPSHOT) {
    l_obj_reduce(ctx->L, D); KCHK();
    CHK(allreduce(ctx, D.obj, 2, 1));
    CHK(objective_snapshot(ctx));
    CHK(push_objective(ctx));  // asynchronous: resolved by flush_objectives when a value is needed
  } else {
    // one launch (the chain's folder, or k_round_tail): slot rows -> objective terms -> snapshot written STRAIGHT into the pinned host slot (no
    // copy engine, no second launch), chain control reset, the table this round consumed and the replica sets cleared.  Resolved by
    // flush_objectives (event) when a value is needed.
    double* slot = nullptr;
    if (rp.close != CLOSE_CHAIN_TAIL) CHK(objective_slot(ctx, &slot));
    if (rp.close == CLOSE_WIDE_CLEAR_TAIL) {      // many-level designs: a wide clearing launch in front of the tail (TAIL_CLEAR_MAX_ENTRIES)
      l_zero4(ctx->L, D.Sold_fx, nSold, D.Snew_set[0], nSets, nullptr, 0, nullptr, 0); KCHK();
      l_round_tail(ctx->L, D, slot, D.Sold_fx, 0, D.Snew_set[0], 0); KCHK();
    } else if (rp.close == CLOSE_TAIL) { l_round_tail(ctx->L, D, slot, D.Sold_fx, nSold, D.Snew_set[0], nSets); KCHK(); }
    lg.tail_cleared();
    ctx->obj_unrecorded = true;      // (obj_event: once at the end of hmx_cluster, or in front of a flush that is really taken -- record_objectives)
    ctx->obj_pending++;
  }
  lg.flip();      // next round subtracts what this round's tile kernels collected (or a fresh k_oldsum pass)
  ctx->R_valid = rp.r_store != 0;
  if (ctx->profile) { ctx->prof_update_cells += ctx->N; }   // the event pairs are resolved when a "prof:*" field is read
  ctx->timers["update_R"] += now_ms() - t0;
  return 0;
}

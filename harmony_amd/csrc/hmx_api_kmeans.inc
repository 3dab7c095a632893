// hmx_api_kmeans.inc -- part of hmx_api.cpp (included there, ONE translation unit): kmeans_centers (seeding race + Lloyd) and the batched shuffle schedule
// ---- kmeans_centers (src/utils.cpp:10-64) ---------------------------------------------------
int gather_centres(hmx_ctx* ctx, const std::vector<long long>& gcells, long long* d_gcells, double* d_rows) {
  const int K = ctx->K, d = ctx->d;
  CHK(h2d(ctx, d_gcells, gcells.data(), (size_t)K));
  l_gather_rows(ctx->L, ctx->D, d_gcells, (uint64_t)ctx->goff, d_rows); KCHK();
  CHK(allreduce(ctx, d_rows, (int64_t)K * d, 1));
  l_y_images(ctx->L, ctx->D, d_rows, 0); KCHK();       // rows -> Ycur, Yt, the MFMA images, ||y||^2: no trip to the host
  ctx->y_on_device = true;                              // (the host copy is fetched when somebody asks for it)
  return 0;
}

int kmeans_centers(hmx_ctx* ctx) {
  const int K = ctx->K, d = ctx->d;
  const Dev& D = ctx->D;
  ctx->Y.assign((size_t)d * K, 0.f);
  long long* const d_gcells = D.km_gcells; double* const d_rows = D.km_rows; unsigned* const d_excl = D.km_excl;   // allocated once in hmx_setup
  // random anchors (:12-15): indices = floor(randu * (N-1))
  std::vector<long long> gcells(K);
  const float Nm1 = (float)((uint64_t)ctx->N_global - 1);
  const bool rmode = ctx->rng_mode == 1;
  if (rmode) ensure_rrng(ctx);
  for (int i = 0; i < K; i++) gcells[i] = (long long)std::floor((rmode ? ctx->rrng.arma_randu() : hmx_u01(ctx->seed, 0, (uint64_t)i)) * Nm1);
  CHK(gather_centres(ctx, gcells, d_gcells, d_rows));
  std::vector<unsigned long long> win(K), sentinel(K, SEED_SENTINEL);
  std::set<unsigned> sup;
  if (rmode) {
    // R-compatible stream: anchor i consumes N_global uniforms in cell order (VECTYPE random_numbers(size(distances), randu), :29).
    // The host draws them (MT19937 or the host's unif_rand callback), a batch of anchors at a time; the race itself
    // (-log(u) / |2(1 - y_i.x)|, index_min) runs on the device over this shard's cells.
    const int64_t n = ctx->N;
    int A = (int)std::max<int64_t>(1, std::min<int64_t>(K, (int64_t)(64ll << 20) / (4 * std::max<int64_t>(n, 1))));
    A = std::max(1, std::min(A, 12288 / d));   // anchor rows of a batch live in LDS (<= 48 KB)
    CallBufs bufs; float* d_u; HIPCHK(bufs.get(&d_u, (size_t)A * (size_t)n));
    std::vector<float> hu((size_t)A * (size_t)n);
    const auto race = [&](int a0, int na, int first, const unsigned* excl, int nexcl) {
      l_seed_race_u(ctx->L, D, d_u, a0, na, first, (uint64_t)ctx->goff, excl, nexcl);
      return hipGetLastError() == hipSuccess ? 0 : fail(ctx, HMX_ERR_DEVICE, "seed race launch failed");
    };
    for (int a0 = 0; a0 < K; a0 += A) {
      const int na = std::min(A, K - a0);
      for (int a = 0; a < na; a++)
        for (int64_t g = 0; g < ctx->N_global; g++) {
          const float u = ctx->rrng.arma_randu();
          if (g >= ctx->goff && g < ctx->goff + n) hu[(size_t)a * n + (size_t)(g - ctx->goff)] = u;
        }
      CHK(h2d(ctx, d_u, hu.data(), (size_t)na * (size_t)n));
      CHK(h2d(ctx, D.seedmin, sentinel.data(), (size_t)K));
      CHK(race(a0, na, 0, nullptr, 0));
      CHK(allreduce(ctx, D.seedmin, K, 2));
      CHK(d2h(ctx, win.data(), D.seedmin, (size_t)K));
      for (int i = a0; i < a0 + na; i++) {   // duplicates in cluster order (:38-43)
        if (win[i] == SEED_SENTINEL) return fail(ctx, HMX_ERR_STATE, "centroid seeding found no candidate cell");
        unsigned g = (unsigned)(win[i] & 0xffffffffu);
        if (sup.count(g)) {
          std::vector<unsigned> ex(sup.begin(), sup.end());
          CHK(h2d(ctx, d_excl, ex.data(), ex.size()));
          CHK(h2d(ctx, D.seedmin, sentinel.data(), (size_t)K));
          CHK(race(a0, na, i - a0, d_excl, (int)ex.size()));
          CHK(allreduce(ctx, D.seedmin, K, 2));
          std::vector<unsigned long long> w2(K);
          CHK(d2h(ctx, w2.data(), D.seedmin, (size_t)K));
          if (w2[i] == SEED_SENTINEL) return fail(ctx, HMX_ERR_STATE, "centroid seeding ran out of distinct cells");
          g = (unsigned)(w2[i] & 0xffffffffu);
        }
        sup.insert(g);
        gcells[i] = (long long)g;
      }
    }
  } else {
  // exponential race for every anchor in one pass (:24-34)
  CHK(h2d(ctx, D.seedmin, sentinel.data(), (size_t)K));
  // the race on the matrix cores (k_tile mode 3)
  auto seed_probe = [&](const unsigned* excl, int nexcl) -> int {
    ctx->D.seed_key = ctx->seed; ctx->D.seed_goff = (unsigned long long)ctx->goff; ctx->D.seed_excl = excl; ctx->D.seed_nexcl = nexcl;
    CHK(tile_ran(ctx, TileKind::Seed, l_tile_static(ctx->L, ctx->D, TileKind::Seed))); KCHK();
    return 0;
  };
  CHK(seed_probe(nullptr, 0));
  CHK(allreduce(ctx, D.seedmin, K, 2));
  CHK(d2h(ctx, win.data(), D.seedmin, (size_t)K));
  // duplicates are resolved in cluster order (:38-43): re-sample cluster i among cells not yet chosen
  for (int i = 0; i < K; i++) {
    unsigned g = (unsigned)(win[i] & 0xffffffffu);
    if (win[i] == SEED_SENTINEL) return fail(ctx, HMX_ERR_STATE, "centroid seeding found no candidate cell");
    if (sup.count(g)) {
      std::vector<unsigned> ex(sup.begin(), sup.end());
      CHK(h2d(ctx, d_excl, ex.data(), ex.size()));
      CHK(h2d(ctx, D.seedmin, sentinel.data(), (size_t)K));
      CHK(seed_probe(d_excl, (int)ex.size()));
      CHK(allreduce(ctx, D.seedmin, K, 2));
      std::vector<unsigned long long> w2(K);
      CHK(d2h(ctx, w2.data(), D.seedmin, (size_t)K));
      if (w2[i] == SEED_SENTINEL) return fail(ctx, HMX_ERR_STATE, "centroid seeding ran out of distinct cells");
      g = (unsigned)(w2[i] & 0xffffffffu);
    }
    sup.insert(g);
    gcells[i] = (long long)g;
  }
  }
  ctx->seed_cells.assign(gcells.begin(), gcells.end());   // diagnostics: hmx_get("seed_cells")
  CHK(gather_centres(ctx, gcells, d_gcells, d_rows));
  // 10 x one Lloyd iteration (:53-64); the centre update runs on the device, no host round trip per iteration
  // (the tile kernel stages the centroid image next to the K x d sum table; where both do not fit, k_lloyd sums into memory)
  const bool tile_ok = lloyd_tile_fits(D.NQ, D.NS, K, d);
  for (int it = 0; it < 10; it++) {
    if (it == 0) HIPCHK(hipMemsetAsync(D.lsum, 0, sizeof(long long) * ((size_t)K * d + K), ctx->L.stream));   // sums + counts: one buffer (k_lloyd_finish leaves it zeroed for the next iteration)
    if (tile_ok) { CHK(tile_ran(ctx, TileKind::Lloyd, l_tile_static(ctx->L, D, TileKind::Lloyd))); KCHK(); }
    else { l_lloyd(ctx->L, D); KCHK(); }
    CHK(allreduce(ctx, D.lsum, (int64_t)K * d + K, 0));   // sums and counts in one collective
    l_lloyd_finish(ctx->L, D); KCHK();
  }
  ctx->y_on_device = true;       // (Ycur holds the centres; the host copy follows on demand)
  return 0;
}

// The round's block order: block id per cell (Feistel bijection of (seed, round), or a host-injected shuffle) + the padded
// counting sort.  Touches no algorithmic state (only blk / lorder / lcombo / lpair / boff).  (Enqueuing it speculatively
// for the NEXT round before the host waits for this round's objective was measured: no gain, 26.1 vs 25.9 ms per step.)
void apply_set(Dev& D, const hmx_ctx::SortSet& s) {
  D.blk = s.blk; D.lorder = s.lorder; D.lpair = s.lpair; D.lcombo = s.lcombo; D.boff = s.boff; D.binoff = s.binoff; D.counts = s.counts; D.offs = s.offs; D.blkv = s.blkv; D.bincnt = s.bincnt;
}
// rounds first..(first | 3) in one batch of launches on the main stream, into sets round & 3.
// (Sorting a group AHEAD on a side stream was measured twice and lost twice: next to the persistent block chain every block step got
//  1 us slower (14.2 vs 14.1 ms per run); in the shadow of the correction's statistics pass that pass went from 1.47 to 2.25 ms per run for
//  0.5 ms of sort taken off the main stream.  The sort's thousands of one-wave workgroups get in the way of whatever runs beside them.)
int sort_group(hmx_ctx* ctx, uint64_t first) {
  const int nr = 4 - (int)(first & 3);
  SortBatch Sb{};
  Dev Dt = ctx->D; Dt.nxt = ctx->carry_ok ? 1 : 0;
  if (ctx->shuf_inv) {
    ShufSets T{};
    for (int r = 0; r < nr; r++) {
      const int os = (int)((first + (uint64_t)r) & 3);
      const hmx_ctx::SortSet& t = ctx->sets[os];
      T.posr[r] = ctx->posr[os]; T.lpair[r] = t.lpair; T.lorder[r] = t.lorder; T.lcombo[r] = t.lcombo; T.boff[r] = t.boff; T.partcnt[r] = ctx->shuf_partcnt[os]; T.binbase[r] = t.binoff; T.bincnt[r] = t.bincnt; T.binacc[r] = ctx->shuf_binacc[os];
    }
    l_shuffle_inv(ctx->L, Dt, T, nr, ctx->seed, first, (uint64_t)ctx->N_global, (uint64_t)ctx->goff, ctx->cells_per_block); KCHK();
  } else {
  for (int r = 0; r < nr; r++) {
    const hmx_ctx::SortSet& t = ctx->sets[(first + (uint64_t)r) & 3];
    Sb.p[r] = SortPtrs{t.blk, t.blkv, t.counts, t.offs, t.binoff, t.bincnt, t.boff, t.lorder, t.lcombo, t.lpair};
  }
  l_sort_batch(ctx->L, Dt, Sb, nr, ctx->seed, first, (uint64_t)ctx->N_global, (uint64_t)ctx->goff, ctx->cells_per_block); KCHK();
  }
  for (int r = 0; r < nr; r++) ctx->ledger.sorted(first + (uint64_t)r, ctx->seed, Dt.nxt != 0);
  return 0;
}
int prepare_round(hmx_ctx* ctx, uint64_t round) {
  Dev& D = ctx->D;
  apply_set(D, ctx->sets[round & 3]);
  if (ctx->injected.empty() && ctx->rng_mode != 1) {
    if (!ctx->ledger.is_order(round, ctx->seed)) CHK(sort_group(ctx, round));    // this round and the rest of its group
    D.nxt = ctx->ledger.keyed_by_next(round) ? 1 : 0;
    return 0;
  }
  ctx->ledger.lost(round);      // the host owns this round's shuffle: its order goes into the round's set, keyed by the block alone
  if (ctx->injected.empty()) {   // update_order = shuffle(linspace(0, N-1, N)) from R's stream (:272-273)
    ensure_rrng(ctx);
    std::vector<int64_t> order;
    ctx->rrng.arma_shuffle(ctx->N_global, order);
    ctx->injected.push_back(std::move(order));
  }
  std::vector<int64_t> order = std::move(ctx->injected.front());      // block(g) from its position
  ctx->injected.pop_front();
  std::vector<int> pos_blk((size_t)ctx->N);
  std::vector<int64_t> pos((size_t)ctx->N_global);
  for (int64_t p = 0; p < ctx->N_global; p++) pos[(size_t)order[p]] = p;
  for (int64_t i = 0; i < ctx->N; i++) {
    uint64_t b = (uint64_t)pos[(size_t)(ctx->goff + ctx->perm[i])] / ctx->cells_per_block;
    pos_blk[i] = (int)std::min<uint64_t>(b, (uint64_t)(ctx->nb - 1));
  }
  CHK(h2d(ctx, D.blk, pos_blk.data(), pos_blk.size()));
  ctx->injected_round = (int64_t)round;
  D.nxt = 0;
  l_sort_blocks(ctx->L, D); KCHK();
  return 0;
}

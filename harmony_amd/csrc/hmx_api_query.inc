// hmx_api_query.inc -- part of hmx_api.cpp (included there, ONE translation unit): hmx_map_query (mapping query cells onto a fitted
// reference, Symphony's mapQuery restated in DESIGN "Query mapping") and the reference summary behind hmx_get "ref_Nr" / "ref_C".
// Kernels: hmx_query.hip.

// chunks of <= cells (a multiple of 16) contiguous cells that never straddle a combination; qchunk[q] = first chunk of combination q
static void query_chunks(const std::vector<int>& start, int64_t n, int target, std::vector<Item>& chunks, std::vector<int>& qchunk) {
  int64_t per = (n + target - 1) / target;
  per = std::max<int64_t>(16, (per + 15) / 16 * 16);
  const int Q = (int)start.size() - 1;
  chunks.clear(); qchunk.assign((size_t)Q + 1, 0);
  for (int q = 0; q < Q; q++) {
    qchunk[q] = (int)chunks.size();
    for (int64_t s = start[q]; s < start[q + 1]; s += per) chunks.push_back({q, (int)s, (int)std::min<int64_t>(per, start[q + 1] - s)});
  }
  qchunk[Q] = (int)chunks.size();
}

// statistics pass + fixed-order fold: out[q][k][0..d) = sum over combination q's cells of R_k z, out[q][k][d] = sum R_k (fp64, on the host);
// summary 2 (pass A of the reference moments, hmx_api_confidence.inc): one more entry per cluster, out[q][k][d + 1] = sum R_k^2
static int query_sums(hmx_ctx* ctx, QueryDev Q, int summary, const std::vector<Item>& chunks, const std::vector<int>& qchunk, std::vector<double>& out) {
  const int total = Q.K * query_stats_width(Q.d, summary), nq = (int)qchunk.size() - 1;
  const int nsl = (total + QUERY_SLICE - 1) / QUERY_SLICE;
  Q.slice = (total + nsl - 1) / nsl;
  Q.nchunks = (int)chunks.size();
  const auto dev = [&](hipError_t e) { return e == hipSuccess ? 0 : fail(ctx, HMX_ERR_DEVICE, std::string("query statistics: ") + hipGetErrorString(e)); };
  hipStream_t st = ctx->L.stream; CallBufs bufs; Item* dch; int* dqc; double* dres;
  out.assign((size_t)nq * total, 0.0);
  CHK(dev(bufs.get(&dch, chunks.size()))); CHK(dev(bufs.get(&dqc, qchunk.size())));
  CHK(dev(bufs.get(&Q.part, (size_t)Q.nchunks * total))); CHK(dev(bufs.get(&dres, out.size())));
  CHK(dev(upload(dch, chunks.data(), chunks.size(), st))); CHK(dev(upload(dqc, qchunk.data(), qchunk.size(), st)));
  Q.chunks = dch;
  if (Q.nchunks) { l_query_stats(ctx->L, Q, summary); CHK(dev(hipGetLastError())); }
  l_query_fold(ctx->L, Q.part, dqc, nq, total, dres); CHK(dev(hipGetLastError()));
  if (summary) CHK(allreduce(ctx, dres, (int64_t)nq * total, 1));      // sharded handle: the global summary on every rank
  CHK(dev(download(out.data(), dres, out.size(), st)));
  return dev(hipStreamSynchronize(st));
}

// the reference summary of a fitted handle: res[k][0..d) = sum_i R[k,i] Z_corr[:,i], res[k][d] = sum_i R[k,i] over the current rows
static int ref_summary(hmx_ctx* ctx, std::vector<double>& res) {
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, HMX_ERR_DEVICE, "hipSetDevice");
  QueryDev Q{};
  Q.n = (int)ctx->N; Q.d = ctx->d; Q.K = ctx->K; Q.zs = ctx->D.zs; Q.KP16 = (ctx->K + 15) / 16 * 16;
  Q.Zsum = ctx->D.Zc; Q.Rsum = ctx->D.R;
  std::vector<int> start = {0, (int)ctx->N};
  std::vector<Item> chunks; std::vector<int> qchunk;
  query_chunks(start, ctx->N, 512, chunks, qchunk);
  return query_sums(ctx, Q, 1, chunks, qchunk, res);
}

// R rows of a mapped query, recomputed on request into dst ([n][K], internal order)
static int query_R_rows(hmx_ctx* ctx, float* dst) {
  QueryDev Q = ctx->qd;
  Q.out = nullptr; Q.Rout = dst;
  l_query_apply(ctx->L, Q);
  HIPCHK(hipGetLastError());
  return 0;
}

int hmx_map_query(hmx_ctx* ctx, const void* Zq, int32_t z_dtype, int32_t z_location, int64_t Nq, int32_t d,
                  const int32_t* phi_i, const int32_t* phi_p, int32_t B, const int32_t* B_vec, int32_t C,
                  const double* lambda, int32_t n_lambda, double alpha, double cutoff,
                  const double* Nr, const double* Cref, const double* sigma, int32_t K) {
  if (!ctx) return HMX_ERR_ARG;
  if (ctx->ran_setup || ctx->query_done) return fail(ctx, HMX_ERR_STATE, "hmx_map_query needs a fresh handle");
  ctx->err.clear(); ctx->warn.clear();
  if (ctx->world > 1) return fail(ctx, HMX_ERR_ARG, "a query handle is single-GPU: no hmx_set_shard");
  if ((z_dtype != HMX_F64 && z_dtype != HMX_F32) || (z_location != HMX_HOST && z_location != HMX_DEVICE))
    return fail(ctx, HMX_ERR_ARG, "bad dtype / location of Zq");
  if (!Zq || !phi_i || !phi_p || !B_vec || !lambda || !Nr || !Cref || !sigma) return fail(ctx, HMX_ERR_ARG, "null argument");
  if (Nq <= 0 || d <= 0 || K <= 0 || B <= 0 || C <= 0) return fail(ctx, HMX_ERR_ARG, "non-positive dimension");
  if (d > 128 || K > 256 || C > 15) return fail(ctx, HMX_ERR_LIMIT, "supported envelope: d <= 128, K <= 256, covariates <= 15");
  if (Nq > 2000000000ll) return fail(ctx, HMX_ERR_LIMIT, "at most 2e9 query cells");
  if (n_lambda != 1 && n_lambda != B + 1) return fail(ctx, HMX_ERR_ARG, "lambda must have length B+1 (or be the single value -1)");
  const bool est = lambda[0] == -1 && n_lambda == 1;
  if (!est && n_lambda != B + 1) return fail(ctx, HMX_ERR_ARG, "fixed lambda must have length B+1");
  if (!est) for (int b = 1; b <= B; b++) if (!(lambda[b] > 0)) return fail(ctx, HMX_ERR_ARG, "lambda must be positive");
  if (est && !(alpha > 0)) return fail(ctx, HMX_ERR_ARG, "alpha must be positive");
  for (int k = 0; k < K; k++) {
    if (!(sigma[k] > 0)) return fail(ctx, HMX_ERR_ARG, "sigma must be positive");
    if (!(Nr[k] >= 0) || !std::isfinite(Nr[k])) return fail(ctx, HMX_ERR_ARG, "Nr must be finite and non-negative");
  }
  for (int64_t i = 0; i < (int64_t)K * d; i++) if (!std::isfinite(Cref[i])) return fail(ctx, HMX_ERR_ARG, "Cref must be finite");
  ctx->B_vec.assign(B_vec, B_vec + C);
  for (int c = 0; c < C; c++) if (B_vec[c] <= 0) return fail(ctx, HMX_ERR_ARG, "B_vec entries must be positive");
  ctx->cov_bounds.resize(C);
  std::partial_sum(ctx->B_vec.begin(), ctx->B_vec.end(), ctx->cov_bounds.begin());
  if (ctx->cov_bounds.back() != B) return fail(ctx, HMX_ERR_ARG, "sum(B_vec) != nrow(Phi)");
  std::vector<int> codes, key, start, invperm, combo_sorted;
  std::vector<long long> present;
  CHK(phi_codes(ctx, Nq, phi_i, phi_p, nullptr, B, C, codes));
  CHK(combo_keys(ctx, Nq, C, codes, key, present));

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(ctx, HMX_ERR_DEVICE, "no HIP device available: libharmony_mi355x has no CPU fallback");
  if (ctx->device < 0) { int cur = 0; (void)hipGetDevice(&cur); ctx->device = cur; }
  HIPCHK(hipSetDevice(ctx->device));
  const double t0 = now_ms();
  free_all(ctx);
  if (!ctx->L.stream) { HIPCHK(hipStreamCreateWithFlags(&ctx->L.stream, hipStreamNonBlocking)); ctx->own_stream = true; }
  combo_order(ctx, Nq, C, present, key, start, invperm, combo_sorted);
  const int Q = ctx->Q;
  std::vector<double> Nb((size_t)B, 0.0);
  for (size_t i = 0; i < codes.size(); i++) Nb[(size_t)codes[i]] += 1.0;
  ctx->N = ctx->N_global = Nq; ctx->goff = 0; ctx->d = d; ctx->K = K; ctx->B = B; ctx->C = C;
  ctx->sigma.assign(sigma, sigma + K);
  ctx->lambda_estimation = est; ctx->alpha = (float)alpha; ctx->cutoff = (float)cutoff;
  if (est) ctx->lambda.clear(); else ctx->lambda.assign(lambda, lambda + B + 1);
  ctx->sizes.assign(Nb.begin(), Nb.end());

  // ---- device state: the query rows (internal order), the normalised centroid image, 2 / sigma
  Dev& D = ctx->D;
  D = Dev{};
  D.n = (int)Nq; D.d = d; D.K = K; D.B = B; D.C = C; D.Q = Q; D.zs = (d + 3) / 4 * 4;
  const int KP16 = (K + 15) / 16 * 16;
  CHK(dalloc(ctx, &D.Zo, (size_t)Nq * D.zs)); CHK(dalloc(ctx, &D.Zc, (size_t)Nq * D.zs));
  CHK(dalloc(ctx, &D.perm, (size_t)Nq)); CHK(dalloc(ctx, &D.invperm, (size_t)Nq));
  HIPCHK(hipMemsetAsync(D.Zo, 0, sizeof(float) * (size_t)Nq * D.zs, ctx->L.stream));
  CHK(h2d(ctx, D.perm, ctx->perm.data(), (size_t)Nq)); CHK(h2d(ctx, D.invperm, invperm.data(), (size_t)Nq));
  QueryDev& Qd = ctx->qd;
  Qd = QueryDev{};
  Qd.n = (int)Nq; Qd.d = d; Qd.K = K; Qd.zs = D.zs; Qd.KP16 = KP16; Qd.Z = D.Zo;
  {
    std::vector<float> yhat((size_t)KP16 * D.zs, 0.f), sig2((size_t)K);
    for (int k = 0; k < K; k++) {
      double nn = 0; for (int j = 0; j < d; j++) nn += Cref[k + (size_t)K * j] * Cref[k + (size_t)K * j];
      const double iv = nn > 0 ? 1.0 / std::sqrt(nn) : 0.0;
      for (int j = 0; j < d; j++) yhat[(size_t)k * D.zs + j] = (float)(Cref[k + (size_t)K * j] * iv);
      sig2[k] = (float)(2.0 / sigma[k]);
    }
    float* dy; float* ds;
    CHK(dalloc(ctx, &dy, yhat.size())); CHK(dalloc(ctx, &ds, sig2.size()));
    CHK(h2d(ctx, dy, yhat.data(), yhat.size())); CHK(h2d(ctx, ds, sig2.data(), sig2.size()));
    Qd.yhat = dy; Qd.sig2 = ds;
  }
  CHK(ingest_Z(ctx, Zq, z_dtype, z_location, Nq, d));
  const double t_dev = now_ms();

  // ---- pass 1: per-combination sums n[q][k] = sum R, S[q][k][:] = sum R z (R never leaves the registers / LDS)
  std::vector<Item> schunks, achunks; std::vector<int> sq, aq;
  query_chunks(start, Nq, 512, schunks, sq);
  std::vector<double> st;
  CHK(query_sums(ctx, Qd, 0, schunks, sq, st));
  const double t_stats = now_ms();

  // ---- K ridge systems in fp64 (DESIGN "Query mapping"): the reference's mass enters the intercept, its centroid the right-hand side
  const int W1 = d + 1;
  std::vector<float> Wq((size_t)Q * K * d, 0.f);
  std::vector<int> status((size_t)K, 0);
  auto solve = [&](int k) {
    std::vector<double> nb((size_t)B, 0.0);
    double tot = 0.0;
    for (int q = 0; q < Q; q++) {
      const double nqk = st[((size_t)q * K + k) * W1 + d];
      tot += nqk;
      for (int c = 0; c < C; c++) nb[(size_t)ctx->qlev[(size_t)q * C + c]] += nqk;
    }
    std::vector<int> pos((size_t)B, -1), lev;
    for (int b = 0; b < B; b++) if (nb[b] / Nb[b] > cutoff) { pos[b] = 1 + (int)lev.size(); lev.push_back(b); }
    const int m = 1 + (int)lev.size();
    std::vector<double> A((size_t)m * m, 0.0), G((size_t)m * d, 0.0);
    for (int q = 0; q < Q; q++) {
      const double nqk = st[((size_t)q * K + k) * W1 + d];
      const double* sqk = &st[((size_t)q * K + k) * W1];
      int rows[16]; int nr = 0;
      rows[nr++] = 0;
      for (int c = 0; c < C; c++) { const int p = pos[(size_t)ctx->qlev[(size_t)q * C + c]]; if (p > 0) rows[nr++] = p; }
      for (int a = 0; a < nr; a++) {
        for (int b2 = 0; b2 < nr; b2++) A[(size_t)rows[a] * m + rows[b2]] += nqk;
        for (int j = 0; j < d; j++) G[(size_t)rows[a] * d + j] += sqk[j];
      }
    }
    A[0] += Nr[k];
    for (int j = 0; j < d; j++) G[j] += Cref[k + (size_t)K * j];
    for (int i = 1; i < m; i++) {
      const int b = lev[(size_t)i - 1];
      A[(size_t)i * m + i] += est ? alpha * (tot * Nb[b] / (double)Nq) : lambda[1 + b];
    }
    // Cholesky A = L L^T (lower triangle in place), then W = A^-1 G
    for (int j = 0; j < m; j++) {
      double s = A[(size_t)j * m + j];
      for (int p = 0; p < j; p++) s -= A[(size_t)j * m + p] * A[(size_t)j * m + p];
      if (!(s > 0)) { status[k] = HMX_ERR_SOLVE; return; }
      const double ljj = std::sqrt(s);
      A[(size_t)j * m + j] = ljj;
      for (int i = j + 1; i < m; i++) {
        double t = A[(size_t)i * m + j];
        for (int p = 0; p < j; p++) t -= A[(size_t)i * m + p] * A[(size_t)j * m + p];
        A[(size_t)i * m + j] = t / ljj;
      }
    }
    for (int j = 0; j < d; j++) {
      for (int i = 0; i < m; i++) {
        double t = G[(size_t)i * d + j];
        for (int p = 0; p < i; p++) t -= A[(size_t)i * m + p] * G[(size_t)p * d + j];
        G[(size_t)i * d + j] = t / A[(size_t)i * m + i];
      }
      for (int i = m - 1; i >= 0; i--) {
        double t = G[(size_t)i * d + j];
        for (int p = i + 1; p < m; p++) t -= A[(size_t)p * m + i] * G[(size_t)p * d + j];
        G[(size_t)i * d + j] = t / A[(size_t)i * m + i];
      }
    }
    // row 0 (the intercept) is not applied: Wq[q][k] = sum of the rows of q's kept levels
    for (int q = 0; q < Q; q++)
      for (int c = 0; c < C; c++) {
        const int p = pos[(size_t)ctx->qlev[(size_t)q * C + c]];
        if (p > 0) for (int j = 0; j < d; j++) Wq[((size_t)q * K + k) * d + j] += (float)G[(size_t)p * d + j];
      }
  };
  {
    unsigned nt = std::thread::hardware_concurrency(); if (nt < 1) nt = 1; if (nt > 16) nt = 16; if ((int)nt > K) nt = K;
    if ((size_t)K * (B + 1) * (B + 1) * (B + 1) < 2000000) nt = 1;
    if (nt == 1) for (int k = 0; k < K; k++) solve(k);
    else {
      std::vector<std::thread> th;
      for (unsigned t = 0; t < nt; t++) th.emplace_back([&, t] { for (int k = (int)t; k < K; k += (int)nt) solve(k); });
      for (auto& x : th) x.join();
    }
  }
  for (int k = 0; k < K; k++) if (status[k]) return fail(ctx, HMX_ERR_SOLVE, "singular ridge system of the query (cluster " + std::to_string(k) + ")");
  const double t_solve = now_ms();

  // ---- pass 2: Z_corr = Zq - sum_k R_k Wq[q][k] (R recomputed in registers / LDS)
  float* dW;
  CHK(dalloc(ctx, &dW, Wq.size()));
  CHK(h2d(ctx, dW, Wq.data(), Wq.size()));
  query_chunks(start, Nq, 2048, achunks, aq);
  Item* dch;
  CHK(dalloc(ctx, &dch, achunks.size()));
  CHK(h2d(ctx, dch, achunks.data(), achunks.size()));
  Qd.Wq = dW; Qd.w_lds = (size_t)K * d * sizeof(float) <= 32768 ? 1 : 0;
  Qd.chunks = dch; Qd.nchunks = (int)achunks.size();
  Qd.out = D.Zc; Qd.Rout = nullptr;
  l_query_apply(ctx->L, Qd); KCHK();
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  const double t1 = now_ms();
  ctx->timers["map_query"] = t1 - t0;
  ctx->timers["map_query_stats"] = t_stats - t_dev;
  ctx->timers["map_query_solve"] = t_solve - t_stats;
  ctx->timers["map_query_apply"] = t1 - t_solve;
  ctx->query_done = true;
  return 0;
}

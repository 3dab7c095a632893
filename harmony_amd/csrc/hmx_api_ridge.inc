// hmx_api_ridge.inc -- part of hmx_api.cpp (included there, ONE translation unit): ridge solves on the host (HMX_MOE_SOLVE=host) and moe_correct_ridge's orchestration (at the end)
// ---- ridge solves (src/harmony.cpp:358-611), fp64, one cluster at a time --------------------------
bool chol_solve(std::vector<double>& A, int n, std::vector<double>& Bm, int m) {  // column-major, in place
  for (int c = 0; c < n; c++) {
    double s = A[(size_t)c * n + c];
    for (int k = 0; k < c; k++) s -= A[(size_t)k * n + c] * A[(size_t)k * n + c];
    if (!(s > 0)) return false;
    const double l = std::sqrt(s);
    A[(size_t)c * n + c] = l;
    for (int r = c + 1; r < n; r++) {
      double t = A[(size_t)c * n + r];
      for (int k = 0; k < c; k++) t -= A[(size_t)k * n + r] * A[(size_t)k * n + c];
      A[(size_t)c * n + r] = t / l;
    }
  }
  for (int j = 0; j < m; j++) {
    double* b = &Bm[(size_t)j * n];
    for (int r = 0; r < n; r++) { double t = b[r]; for (int k = 0; k < r; k++) t -= A[(size_t)k * n + r] * b[k]; b[r] = t / A[(size_t)r * n + r]; }
    for (int r = n - 1; r >= 0; r--) { double t = b[r]; for (int k = r + 1; k < n; k++) t -= A[(size_t)r * n + k] * b[k]; b[r] = t / A[(size_t)r * n + r]; }
  }
  return true;
}
bool lu_solve(std::vector<double>& A, int n, std::vector<double>& Bm, int m) {
  for (int c = 0; c < n; c++) {
    int p = c; double best = std::fabs(A[(size_t)c * n + c]);
    for (int r = c + 1; r < n; r++) if (std::fabs(A[(size_t)c * n + r]) > best) { best = std::fabs(A[(size_t)c * n + r]); p = r; }
    if (best == 0) return false;
    if (p != c) {
      for (int j = 0; j < n; j++) std::swap(A[(size_t)j * n + c], A[(size_t)j * n + p]);
      for (int j = 0; j < m; j++) std::swap(Bm[(size_t)j * n + c], Bm[(size_t)j * n + p]);
    }
    const double inv = 1 / A[(size_t)c * n + c];
    for (int r = c + 1; r < n; r++) {
      const double f = A[(size_t)c * n + r] * inv; if (f == 0) continue;
      for (int j = c + 1; j < n; j++) A[(size_t)j * n + r] -= f * A[(size_t)j * n + c];
      for (int j = 0; j < m; j++) Bm[(size_t)j * n + r] -= f * Bm[(size_t)j * n + c];
    }
  }
  for (int j = 0; j < m; j++)
    for (int r = n - 1; r >= 0; r--) {
      double s = Bm[(size_t)j * n + r];
      for (int c = r + 1; c < n; c++) s -= A[(size_t)c * n + r] * Bm[(size_t)j * n + c];
      Bm[(size_t)j * n + r] = s / A[(size_t)r * n + r];
    }
  return true;
}

struct SolveOut { int status = 0; bool skipped = false, subset = false; std::vector<float> W; int m = 0; };

// O, E: K x B column-major floats; Sq [Q][K][d], nq [Q][K] doubles; Wq [Q][K][d] floats (output)
void solve_cluster(const hmx_ctx* ctx, int k, const std::vector<float>& O, const std::vector<float>& E,
                   const std::vector<double>& Sq, const std::vector<double>& nq, std::vector<float>& Wq,
                   std::vector<float>& Ynew, SolveOut& out, const double* S0 = nullptr, const double* n0 = nullptr) {
  const int K = ctx->K, B = ctx->B, C = ctx->C, d = ctx->d, Q = ctx->Q;
  std::vector<int> cov_levels(C, 0);
  for (int b = 0, cov = 0; b < B; b++) {  // :368-380
    if (!(b < ctx->cov_bounds[cov])) cov++;
    const float rep = O[(size_t)b * K + k] / ctx->sizes[b];
    if (rep > ctx->cutoff) cov_levels[cov]++;
  }
  std::vector<int> keep;
  for (int b = 0, cov = 0; b < B; b++) {  // :389-402
    if (cov < C && !(b < ctx->cov_bounds[cov])) cov++;
    const float rep = O[(size_t)b * K + k] / ctx->sizes[b];
    if (rep > ctx->cutoff && cov_levels[cov] > 1) keep.push_back(b);
  }
  int active = 0; for (int l : cov_levels) if (l > 1) active++;
  const bool full = ((int)keep.size() == B);
  out.subset = !full;
  for (int q = 0; q < Q; q++) std::fill_n(&Wq[((size_t)q * K + k) * d], d, 0.f);
  if (!full && active == 0) { out.skipped = true; return; }  // :449-452
  const int m = (int)keep.size() + 1;
  if (C == 1) {
    // One covariate: Phi* diag(R_k) Phi*^T + Lambda is an arrowhead matrix; solve it in closed form in fp64
    // (the reference inverts it in closed form too, src/harmony.cpp:575-586).  Combinations == levels here.
    thread_local std::vector<double> w0, coef;
    thread_local std::vector<int> qof;
    w0.assign(d, 0.0); coef.assign(B, 0.0); qof.assign(B, -1);
    for (int q = 0; q < Q; q++) qof[ctx->qlev[q]] = q;
    double N = 0.0, u = 0.0;
    bool ok = true;
    for (int b : keep) {
      const int q = qof[b];
      const double n = (q >= 0) ? nq[(size_t)q * K + k] : 0.0;
      const float lam = ctx->lambda_estimation ? E[(size_t)b * K + k] * ctx->alpha : ctx->lambda[b + 1];
      const double den = n + (double)lam;
      if (!(den > 0.0)) { ok = false; break; }
      coef[b] = n / den;                       // n_b / (n_b + lambda_b)
      N += n; u += n * coef[b];
      if (q >= 0) { const double* sq = &Sq[((size_t)q * K + k) * d]; for (int j = 0; j < d; j++) w0[j] += (S0 ? -coef[b] : (1.0 - coef[b])) * sq[j]; }
    }
    // the arrowhead system's first row: (sum_i R_ki) w0 + sum_b n_b w_b = sum_i R_ki z_i.  Exact statistics: both totals are
    // the sums of the level rows.  ridge_arith = 1: the reference's OWN sequential fp32 totals (separate chains, :567,:599).
    if (S0) { N = *n0; for (int j = 0; j < d; j++) w0[j] += S0[j]; }
    u = N - u;
    if (ok && u > 0.0 && std::isfinite(u)) {
      for (int j = 0; j < d; j++) { w0[j] /= u; Ynew[(size_t)k * d + j] = (float)w0[j]; }          // intercept row :610
      out.m = m; out.W.assign((size_t)m * d, 0.f);
      int a = 1;
      for (int b : keep) {
        const int q = qof[b];
        const double n = (q >= 0) ? nq[(size_t)q * K + k] : 0.0;
        const float lam = ctx->lambda_estimation ? E[(size_t)b * K + k] * ctx->alpha : ctx->lambda[b + 1];
        const double inv = 1.0 / (n + (double)lam);
        float* wq = (q >= 0) ? &Wq[((size_t)q * K + k) * d] : nullptr;
        for (int j = 0; j < d; j++) {
          const double s = (q >= 0) ? Sq[((size_t)q * K + k) * d + j] : 0.0;
          const float w = (float)((s - n * w0[j]) * inv);
          out.W[(size_t)j * m + a] = w;
          if (wq) wq[j] = w;
        }
        a++;
      }
      return;
    }
  }
  std::vector<int> row_of(B, -1);
  for (int a = 0; a < (int)keep.size(); a++) row_of[keep[a]] = a + 1;
  std::vector<double> cov((size_t)m * m, 0.0), rhs((size_t)m * d, 0.0);
  std::vector<int> rows(C + 1);
  for (int q = 0; q < Q; q++) {
    int nr = 0; rows[nr++] = 0;
    for (int c = 0; c < C; c++) { const int ro = row_of[ctx->qlev[(size_t)q * C + c]]; if (ro >= 0) rows[nr++] = ro; }
    if (nr == 1) continue;  // none of this combination's levels is kept: its cells do not enter (:400,456-460)
    const double n = nq[(size_t)q * K + k];
    for (int a = 0; a < nr; a++) for (int b2 = 0; b2 < nr; b2++) cov[(size_t)rows[b2] * m + rows[a]] += n;
    const double* sq = &Sq[((size_t)q * K + k) * d];
    for (int j = 0; j < d; j++) { const double s = sq[j]; for (int a = 0; a < nr; a++) rhs[(size_t)j * m + rows[a]] += s; }
  }
  for (int a = 1; a < m; a++) {  // :434-439, :533-544
    const float lam = ctx->lambda_estimation ? E[(size_t)keep[a - 1] * K + k] * ctx->alpha : ctx->lambda[keep[a - 1] + 1];
    cov[(size_t)a * m + a] += (double)lam;
  }
  std::vector<double> A = cov, X = rhs;
  if (!chol_solve(A, m, X, d)) { A = cov; X = rhs; if (!lu_solve(A, m, X, d)) { out.status = HMX_ERR_SOLVE; return; } }
  for (int j = 0; j < d; j++) { Ynew[(size_t)k * d + j] = (float)X[(size_t)j * m]; X[(size_t)j * m] = 0.0; }  // :610-611
  out.m = m; out.W.resize((size_t)m * d);
  for (size_t i = 0; i < out.W.size(); i++) out.W[i] = (float)X[i];
  for (int q = 0; q < Q; q++) {  // correction of a cell of combination q from cluster k: sum of its kept levels' rows
    float* w = &Wq[((size_t)q * K + k) * d];
    for (int c = 0; c < C; c++) { const int ro = row_of[ctx->qlev[(size_t)q * C + c]]; if (ro < 0) continue;
      for (int j = 0; j < d; j++) w[j] += out.W[(size_t)j * m + ro]; }
  }
}

std::vector<float> table_O(const hmx_ctx* ctx, const std::vector<long long>& ofx) {
  std::vector<float> O(ofx.size());
  for (size_t i = 0; i < ofx.size(); i++) O[i] = (float)((double)ofx[i] * FX_INV);
  return O;
}
std::vector<float> table_E(const hmx_ctx* ctx, const std::vector<long long>& ofx) {
  const int K = ctx->K, B = ctx->B;
  std::vector<float> E((size_t)K * B);
  for (int k = 0; k < K; k++) {
    long long rs = 0; for (int b = 0; b < ctx->B_vec[0]; b++) rs += ofx[(size_t)b * K + k];
    const double rsd = (double)rs * FX_INV;
    for (int b = 0; b < B; b++) E[(size_t)b * K + k] = (float)(rsd * (double)ctx->Pr_b[b]);
  }
  return E;
}

// ---- moe_correct_ridge (src/harmony.cpp:345-638): statistics, then the device tail or the host tail ------------------------------------------------
// a launch of the correction as its launcher returned it: kept for hmx_get("launch:stats" | "launch:solve" | "launch:apply"); one that could not be made is a limit of the shape
int ridge_ran(hmx_ctx* ctx, RidgeKind kind, const RidgeLaunch& t) {
  ctx->last_ridge[(int)kind] = t; ctx->ridge_seen[(int)kind] = true;
  return t.valid ? 0 : fail(ctx, HMX_ERR_LIMIT, std::string("no ridge launch for kind ") + RIDGE_KIND_NAME[(int)kind] + ": " + (t.mfma ? "MFMA" : "first-generation") + " form, parameters " +
                                                    std::to_string(t.p0) + ", " + std::to_string(t.p1) + ", " + std::to_string(t.lds) + " bytes of LDS (over the limit, or no such instantiation)");
}
// reference timers Phi_Rk + Phi_cov + Z_tmp + Z_intercept + batch_exprod: ONE pass here (the reference's sequential sums / the slot form / the first generation), all-reduced
int ridge_statistics(hmx_ctx* ctx) {
  const Dev& D = ctx->D;
  PhaseScope ph(ctx, "ridge_statistics");
  // the slot form overwrites every entry of Sq and nq with plain stores (k_moe_stats_reduce): only the first-generation kernels' atomics and the
  // sequential sums start from zero
  const bool slot_form = ctx->ridge_arith != 1 && D.moe_mfma && D.st_dma;
  if (!slot_form) { l_zero4(ctx->L, D.Sq, (size_t)D.Q * D.d * D.K, D.nq, (size_t)D.Q * D.K, nullptr, 0, nullptr, 0); KCHK(); }      // (one launch instead of two memsets)
  if (ctx->ridge_arith == 1) CHK(seq_ridge_stats(ctx));
  else { CHK(ridge_ran(ctx, RidgeKind::Stats, l_moe_stats(ctx->L, D))); KCHK(); }
  CHK(allreduce(ctx, D.Sq, (int64_t)D.Q * D.d * D.K, 1));
  return allreduce(ctx, D.nq, (int64_t)D.Q * D.K, 1);
}
// the whole correction stays on the device: statistics -> K fp64 solves (one workgroup per cluster) -> apply -> Y;
// no host synchronisation (a singular system is reported by the next call that waits for the device)
int ridge_device_tail(hmx_ctx* ctx) {
  const Dev& D = ctx->D;
  const bool seq = ctx->ridge_arith == 1;
  const RidgeLaunch s = plan_ridge_launch(ridge_geom(D, ctx->L), RidgeKind::Solve);
  SolveArgs A;
  A.cov = ctx->sv_cov; A.rhs = ctx->sv_rhs; A.Wall = ctx->sv_Wall; A.mrows = ctx->sv_mrows; A.flags = ctx->sv_flags;
  A.lambda = ctx->lambda_estimation ? nullptr : ctx->sv_lambda; A.cov_bounds = ctx->sv_cov_bounds;
  A.alpha = ctx->alpha; A.cutoff = ctx->cutoff; A.use_s0 = seq ? 1 : 0; A.err = ctx->D.solve_err;
  A.Of = ctx->oe_arith ? ctx->Of : nullptr; A.Ef = ctx->oe_arith ? ctx->Ef : nullptr; A.solve_f32 = ctx->solve_arith;
  A.ref_tot = (seq && ctx->C > 1) ? ctx->rg_tot : nullptr; A.pair_tot = ctx->rp_tot; A.pair_idx = ctx->pair_idx;
  A.lds_b_bytes = s.lds_b_bytes; A.lds_body_bytes = s.lds_body_bytes; A.lds_mask_off = s.lds_mask_off;
  A.lds_sys_off = s.lds_sys_off;
  { PhaseScope ph(ctx, "arma_inv"); CHK(ridge_ran(ctx, RidgeKind::Solve, l_moe_solve(ctx->L, D, A))); KCHK(); }
  { PhaseScope ph(ctx, "update_Zcorr"); CHK(ridge_ran(ctx, RidgeKind::Apply, l_moe_apply(ctx->L, D))); KCHK(); }
  ctx->y_on_device = true; ctx->solve_pending = true;
  return 0;
}
// HMX_MOE_SOLVE=host, or more levels than the device solve's LDS takes: statistics to the host, K threaded fp64 solves, table (or its MFMA image) and centroids back
int ridge_host_tail(hmx_ctx* ctx) {
  const Dev& D = ctx->D;
  const int K = ctx->K, B = ctx->B, d = ctx->d, Q = ctx->Q;
  const bool seq = ctx->ridge_arith == 1;
  std::vector<double> Sq((size_t)Q * d * K), nq((size_t)Q * K);
  std::vector<long long> ofx((size_t)B * K);
  CHK(d2h(ctx, Sq.data(), D.Sq, Sq.size())); CHK(d2h(ctx, nq.data(), D.nq, nq.size())); CHK(d2h(ctx, ofx.data(), D.O_fx, ofx.size()));
  std::vector<double> S0, n0;
  if (seq) { S0.resize((size_t)K * d); n0.resize((size_t)K); CHK(d2h(ctx, S0.data(), D.S0, S0.size())); CHK(d2h(ctx, n0.data(), D.n0, n0.size())); }
  const double t1 = now_ms();
  const std::vector<float> O = table_O(ctx, ofx), E = table_E(ctx, ofx);
  CHK(sync_solve_results(ctx));        // (host solve path: the centroids may still live on the device only)
  std::vector<float> Wq((size_t)Q * K * d), Ynew = ctx->Y;
  std::vector<SolveOut> outs(K);
  {
    unsigned nt = std::thread::hardware_concurrency(); if (nt < 1) nt = 1; if (nt > 16) nt = 16; if ((int)nt > K) nt = K;
    if ((size_t)K * (B + 1) * (B + 1) < 200000) nt = 1;
    std::vector<std::thread> th;
    auto work = [&](int t) { for (int k = t; k < K; k += (int)nt) solve_cluster(ctx, k, O, E, Sq, nq, Wq, Ynew, outs[k], seq ? &S0[(size_t)k * d] : nullptr, seq ? &n0[k] : nullptr); };
    if (nt == 1) work(0);
    else { for (unsigned t = 0; t < nt; t++) th.emplace_back(work, (int)t); for (auto& x : th) x.join(); }
  }
  ctx->subset_clusters = ctx->skipped_clusters = 0;
  for (int k = 0; k < K; k++) {
    if (outs[k].status) return fail(ctx, outs[k].status, "singular ridge system");
    if (outs[k].subset) ctx->subset_clusters++;
    if (outs[k].skipped) ctx->skipped_clusters++;
    else { ctx->W = outs[k].W; ctx->W_rows = outs[k].m; }
  }
  ctx->timers["moe_solve_host"] += now_ms() - t1;
  if (D.moe_mfma) {      // the table as k_moe_apply_mfma's B-operand image (entries of clusters and PCs beyond K, d stay 0)
    std::vector<float> img((size_t)Q * D.wNQ * D.wNS * 256, 0.f);
    for (int q = 0; q < Q; q++) for (int k = 0; k < K; k++) for (int j = 0; j < d; j++) img[wimg_index(D, q, k, j)] = Wq[((size_t)q * K + k) * d + j];
    CHK(h2d(ctx, D.Wimg, img.data(), img.size()));
  } else CHK(h2d(ctx, D.Wq, Wq.data(), Wq.size()));
  CHK(ridge_ran(ctx, RidgeKind::Apply, l_moe_apply(ctx->L, D))); KCHK();   // Z_corr = Z_orig - sum_k R_k W_k[levels]   :347,:615
  ctx->Y = Ynew;
  normalise_cols(ctx->Y, d, K);     // :633
  CHK(upload_Y(ctx));
  HIPCHK(hipStreamSynchronize(ctx->L.stream));
  return 0;
}
int moe_correct_ridge(hmx_ctx* ctx) {
  { PhaseScope pall(ctx, "correct_ridge_loop");
    CHK(ridge_statistics(ctx));
    if (ctx->solve_on_device) return ridge_device_tail(ctx); }
  return ridge_host_tail(ctx);
}
